// opts.h -- the library's internal switches: layout choices kept selectable
// for A/B measurements and tests.
//
// The product library reads no environment.  A switch changes only through
// mamg_set_option (include/mamg.h: a test and tuning hook, not part of the
// preconditioner's parameters), for the whole process.  Every setup takes one
// typed snapshot of the table at its entry (read_switches), and the handle it
// returns keeps that snapshot for life: a later mamg_set_option reaches only
// handles set up after it.  The diagnosis build
// (make diag, -DMAMG_DIAG=1) also reads the MAMG_* environment variable of a
// switch the call has not set, so A/B scripts and child-process tests can set
// switches before the library loads; its diagnosis-only switches
// (MAMG_K_VARIANT, MAMG_DEBUG_SUMS, ...) are compiled out of the product.
#pragma once
#include <cstdint>
#include <string>

namespace mamg {

// a count that is chosen automatically while the switch is unset
struct AutoCount {
  bool set = false;
  int64_t v = 0;
};

// Every switch of the product library, in mamg_option_names() order: name,
// Switches field, type (bool: given and nonzero), default (DESIGN.md section
// 4 gives the measurements behind each default)
#define MAMG_SWITCHES(X) \
  X(MAMG_POST_K, post_k, int, 1) /* 1: K = P - W A P after the coarse correction; 0: [P | AP]; 2: split K */ \
  X(MAMG_SELL_MIN_ROWS, sell_min_rows, int64_t, 1 << 20) /* node rows from which level 0 is SELL-64 / half-symmetric */ \
  X(MAMG_MSELL_MIN_ROWS, msell_min_rows, int64_t, (int64_t)1 << 40) /* ... coarse levels are multi-lane SELL-64 (never) */ \
  X(MAMG_TAIL_NODES, tail_nodes, AutoCount, {}) /* coarse tail from the first level of <= this many nodes (unset: GS 1024, else off) */ \
  X(MAMG_TAIL_VL, tail_vl, int, 4) /* coarse tail: lanes per row cap, clamped to [1, 64] (1/2/4/8/64 measured) */ \
  X(MAMG_TAIL_LDS, tail_lds, bool, true) /* 0: the coarse tail's work vectors stay in global memory */ \
  X(MAMG_TAIL_PROG_LDS, tail_prog_lds, bool, false) /* 1: coarse tail's op descriptors copied into LDS; 0: scalar loads */ \
  X(MAMG_TAIL_RES, tail_res, bool, true) /* 1: coarse tail's operators held in registers, one row per thread */ \
  X(MAMG_HALF, half, bool, true) /* 1: half-symmetric ELL-64 level-0 A; 0: SELL-64 */ \
  X(MAMG_HALF_BANDS, half_bands, int, 1) /* band schedule of the half-symmetric kernel: sub-bands per XCD (0: row order) */ \
  X(MAMG_R_BANDS, r_bands, int, 1) /* band schedule of the level-0 restriction: sub-bands per XCD (0: XCD-contiguous rows) */ \
  X(MAMG_K_SORT, k_sort, int, 1) /* 1: level-0 K's rows sorted by length inside SELL slices (sort_sell_slices) */ \
  X(MAMG_K_COL16, k_col16, int, 1) /* 1: level-0 K's columns as 16-bit offsets from a per-slice base */ \
  X(MAMG_FUSE_RBD, fuse_rbd, int, 2) /* restrictions writing the next first sweep: 2 those below level 0, 1 all, 0 none */ \
  X(MAMG_CSR2BSR_FILL, csr2bsr_fill, bool, true) /* 1: column-only LDS fill of CSR -> BSR2 / the node graph; 0: staged merge */ \
  X(MAMG_KREGION_TRIES, kregion_tries, int, 4) /* K value regions timed at upload (select_k_region) */ \
  X(MAMG_KREGION_BUDGET_MS, kregion_budget_ms, double, 200.0) /* time budget of that search */ \
  X(MAMG_REHOME, rehome, bool, true) /* 1: operators re-homed after the setup */ \
  X(MAMG_PRERESERVE_B_PER_NNZ, prereserve_b_per_nnz, double, 20.0) /* layout reservation, bytes per A0 entry (0: off) */ \
  X(MAMG_POISON, poison, bool, false) /* 1: new double arrays start as NaN bytes (tests) */ \
  X(MAMG_OVERLAP, overlap, bool, true) /* multi-GPU: interior rows during the forward halo */ \
  X(MAMG_DIST_TEST, dist_test, std::string, {}) /* virtual ranks: "dry" skips exchanges (timing); "full" / "rows": host plan */ \
  X(MAMG_SPGEMM_PAIR, spgemm_pair, bool, true) /* 1: staged SpGEMM count pass over node row pairs */ \
  X(MAMG_SPGEMM_STAGE_GB, spgemm_stage_gb, double, 16.0) /* SpGEMM staging block cap (<= 0: unstaged products) */ \
  X(MAMG_SPGEMM_STAGE_STRIDE, spgemm_stage_stride, int64_t, 128) /* SpGEMM staging stride cap */ \
  X(MAMG_MIS_STAGED, mis_staged, bool, true) /* 1: MIS-2 maxima over staged rows */ \
  X(MAMG_UPLOAD_THREADS, upload_threads, int, 2) /* host threads copying A0, clamped to [1, 16] */ \
  X(MAMG_PATCH_INV, patch_inv, int, 3) /* node-patch inverses: 1 one patch per wave, 2 two per wave, else 3 matrix cores */

// Row-pattern dictionary of a level-0 A: tried from
// ROWDICT_MIN_ROWS node rows.  The bound stays above 3-D n=128 (2,146,689
// rows), where one plane band of the half layout's upper values still fits an
// XCD's L2 and the mirrors cost no HBM traffic.
constexpr int64_t ROWDICT_MIN_ROWS = (int64_t)1 << 22;
constexpr int ROWDICT_MAX_TYPES = 256;    // row types at most (64 KB of table / ~9 blocks of 28 B per type)
constexpr int ROWDICT_MAX_LEN = 32;       // blocks in a row at most
constexpr int ROWDICT_HASH_BITS = 62;     // bits kept of a row's hash
constexpr int64_t ROWDICT_MAX_TABLE = 64 << 10;   // bytes of the type table at most

// Matrix-free level-0 prolongation + first post pass through the dictionary
// (DESIGN.md section 4.9): taken from POST_MF_MIN_ROWS node rows.  A bound of
// its own, so that a test which lowers only the dictionary's keeps the K path.
constexpr int64_t POST_MF_MIN_ROWS = ROWDICT_MIN_ROWS;

struct Switches {
#define X(name, field, type, def) type field = def;
  MAMG_SWITCHES(X)
#undef X
  // diagnosis build only (the environment's MAMG_K_VARIANT; always 0 in the
  // product): the level-0 K kernel, see launch_kvariant
  int k_variant = 0;
  // the row-pattern dictionary's thresholds (mamg_test.h mamg_test_set_rowdict;
  // not switches: a test hook, defaults in the product): node rows from which
  // a level-0 A is tried, the cap on row types, the bits kept of a row's hash
  int64_t rowdict_min_rows = ROWDICT_MIN_ROWS;
  int rowdict_max_types = ROWDICT_MAX_TYPES;
  int rowdict_hash_bits = ROWDICT_HASH_BITS;
  // the matrix-free level-0 post step (mamg_test.h mamg_test_set_post_mf; a
  // test hook as the three above): 0 never, else from post_mf_min_rows node rows
  int post_mf_mode = 1;
  int64_t post_mf_min_rows = POST_MF_MIN_ROWS;
  // where the GPU setup runs the VMB aggregation (mamg_test.h
  // mamg_test_set_vmb; a test hook as the three above): 1 on the device from
  // VMB_MIN_NODES nodes up and on the host below, 2 on the device whatever the
  // size, 0 on the host; the cap on the device rounds of one level (negative:
  // the default rule, gsetup.hip vmb_round_cap)
  int vmb_mode = 1;
  int64_t vmb_max_rounds = -1;
};

// process-wide thresholds of the row-pattern dictionary, read by the next
// read_switches() (a negative value: the default)
void set_rowdict_hook(int64_t min_rows, int max_types, int hash_bits);
// process-wide mode (0: never; negative: default) and threshold (negative:
// default) of the matrix-free level-0 post step, read likewise
void set_post_mf_hook(int mode, int64_t min_rows);
// process-wide path and round cap of the GPU setup's VMB aggregation, read
// likewise
void set_vmb_hook(int mode, int64_t max_rounds);

// the switch's value (nullptr: unset, the built-in default applies)
const char* opt(const char* name);

// set (value != nullptr) or reset (nullptr) a switch; false for an unknown name
bool set_opt(const char* name, const char* value);

// the switch names, comma-separated
const char* opt_names();

// the table as it stands, parsed and clamped, read under one lock
Switches read_switches();

// "NAME=value,..." in opt_names() order with the defaults spelled out
// ("auto" / empty where unset is a state of its own)
std::string format_switches(const Switches& s);

}  // namespace mamg
