// opts.cpp -- process-wide switch table (opts.h).
#include "opts.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <map>
#include <mutex>

#ifndef MAMG_DIAG
#define MAMG_DIAG 0
#endif

namespace mamg {
namespace {

constexpr const char* kNames[] = {
#define X(name, field, type, def) #name,
    MAMG_SWITCHES(X)
#undef X
};

struct Table {
  std::mutex m;
  std::map<std::string, size_t> set;   // name -> index into vals
  std::deque<std::string> vals;        // never shrinks: returned pointers stay valid
  std::string names;
  int64_t rd_min_rows = -1;            // set_rowdict_hook (negative: default)
  int rd_max_types = -1, rd_hash_bits = -1;
  int mf_mode = -1;                    // set_post_mf_hook (negative: default)
  int64_t mf_min_rows = -1;
  int vmb_mode = 1;                    // set_vmb_hook
  int64_t vmb_max_rounds = -1;
};
Table& table() {
  static Table t;
  return t;
}
bool known(const char* name) {
  for (const char* k : kNames)
    if (std::strcmp(k, name) == 0) return true;
  return false;
}
// with t.m held
const char* find(Table& t, const char* name) {
  auto it = t.set.find(name);
  if (it != t.set.end()) return t.vals[it->second].c_str();
#if MAMG_DIAG
  return std::getenv(name);
#else
  return nullptr;
#endif
}

// one parser and one printer per field type (e != nullptr)
void parse(const char* e, int* v) { *v = std::atoi(e); }
void parse(const char* e, int64_t* v) { *v = std::atoll(e); }
void parse(const char* e, double* v) { *v = std::atof(e); }
void parse(const char* e, bool* v) { *v = std::atoi(e) != 0; }
void parse(const char* e, std::string* v) { *v = e; }
void parse(const char* e, AutoCount* v) { *v = {true, std::atoll(e)}; }

std::string show(int v) { return std::to_string(v); }
std::string show(int64_t v) { return std::to_string(v); }
std::string show(bool v) { return v ? "1" : "0"; }
std::string show(const std::string& v) { return v; }
std::string show(const AutoCount& v) { return v.set ? std::to_string(v.v) : "auto"; }
std::string show(double v) {
  char b[32];
  std::snprintf(b, sizeof b, "%g", v);
  return b;
}

}  // namespace

const char* opt(const char* name) {
  Table& t = table();
  std::lock_guard<std::mutex> g(t.m);
  return find(t, name);
}

bool set_opt(const char* name, const char* value) {
  if (!name || !known(name)) return false;
  Table& t = table();
  std::lock_guard<std::mutex> g(t.m);
  if (!value) {
    t.set.erase(name);
    return true;
  }
  t.vals.emplace_back(value);
  t.set[name] = t.vals.size() - 1;
  return true;
}

const char* opt_names() {
  Table& t = table();
  std::lock_guard<std::mutex> g(t.m);
  if (t.names.empty())
    for (const char* k : kNames) {
      if (!t.names.empty()) t.names += ',';
      t.names += k;
    }
  return t.names.c_str();
}

Switches read_switches() {
  Switches s;
  {
    Table& t = table();
    std::lock_guard<std::mutex> g(t.m);
#define X(name, field, type, def) \
    if (const char* e = find(t, #name)) parse(e, &s.field);
    MAMG_SWITCHES(X)
#undef X
    if (t.rd_min_rows >= 0) s.rowdict_min_rows = t.rd_min_rows;
    if (t.rd_max_types >= 0) s.rowdict_max_types = std::max(1, std::min(2048, t.rd_max_types));
    if (t.rd_hash_bits >= 0) s.rowdict_hash_bits = std::max(1, std::min(62, t.rd_hash_bits));
    if (t.mf_mode >= 0) s.post_mf_mode = t.mf_mode;
    if (t.mf_min_rows >= 0) s.post_mf_min_rows = t.mf_min_rows;
    s.vmb_mode = t.vmb_mode;
    s.vmb_max_rounds = t.vmb_max_rounds;
  }
  s.tail_vl = std::max(1, std::min(64, s.tail_vl));
  s.upload_threads = std::max(1, std::min(16, s.upload_threads));
  if (s.patch_inv < 1 || s.patch_inv > (MAMG_DIAG ? 5 : 3)) s.patch_inv = 3;   // 4, 5: diagnosis variants
#if MAMG_DIAG
  if (const char* e = std::getenv("MAMG_K_VARIANT")) s.k_variant = std::atoi(e);
#endif
  return s;
}

void set_rowdict_hook(int64_t min_rows, int max_types, int hash_bits) {
  Table& t = table();
  std::lock_guard<std::mutex> g(t.m);
  t.rd_min_rows = min_rows;
  t.rd_max_types = max_types;
  t.rd_hash_bits = hash_bits;
}

void set_post_mf_hook(int mode, int64_t min_rows) {
  Table& t = table();
  std::lock_guard<std::mutex> g(t.m);
  t.mf_mode = mode;
  t.mf_min_rows = min_rows;
}

void set_vmb_hook(int mode, int64_t max_rounds) {
  Table& t = table();
  std::lock_guard<std::mutex> g(t.m);
  t.vmb_mode = mode;
  t.vmb_max_rounds = max_rounds < 0 ? -1 : max_rounds;
}

std::string format_switches(const Switches& s) {
  std::string out;
#define X(name, field, type, def) out += (out.empty() ? "" : ",") + std::string(#name "=") + show(s.field);
  MAMG_SWITCHES(X)
#undef X
  return out;
}

}  // namespace mamg
