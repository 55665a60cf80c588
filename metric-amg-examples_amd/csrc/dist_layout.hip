// dist_layout.hip -- the rank-local operators of the multi-GPU path: the rank
// layout kernels, the device-side row slices, patches, rings and colour halos
// of a rank, dist_check and dist_upload.  Plan: dist.cpp.
#include "device_int.h"

namespace mamg {

namespace {

// loads this file's code object (device_warm)
__global__ void dist_layout_warm_kernel() {}

}  // namespace

void dist_layout_warm(hipStream_t s) { dist_layout_warm_kernel<<<1, 64, 0, s>>>(); }

namespace {

// ---------------------------------------------------------------------------
// Rank-local operators built in HBM from the GPU hierarchy (mamg_setup_dist's
// default): the device restatement of build_dist_plan's conversions, so no
// matrix of the hierarchy crosses PCIe.  Row slices are gathered from the
// field-major CSRs, converted by the single-GPU csr2bsr kernel, and their
// columns renumbered [owned | ghost] (owned first, each part in global order:
// dist.cpp remap_cols); K by kmerge_kernel, the partial restriction from R's
// rows (R = P^T exactly, so its blocks are transpose_bsr's).  Bitwise the
// host plan's operators (tests/test_gpu_dist.py::test_rank_slice_download_bitwise).
// ---------------------------------------------------------------------------

// rows f m + i of the gathered CSR = rows f nvr + row(i) of M, row(i) =
// rows[i] or r0 + i
__global__ __launch_bounds__(256) void rowlen_gather_kernel(int64_t m, int64_t nvr, const int64_t* __restrict__ rows,
                                                            int64_t r0, const int64_t* __restrict__ ptr,
                                                            int64_t* __restrict__ len) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= 2 * m) return;
  const int64_t f = i / m, k = i - f * m;
  const int64_t src = f * nvr + (rows ? rows[k] : r0 + k);
  len[i + 1] = ptr[src + 1] - ptr[src];
}

__global__ __launch_bounds__(256) void rowcopy_gather_kernel(int64_t m, int64_t nvr, const int64_t* __restrict__ rows,
                                                             int64_t r0, const int64_t* __restrict__ ptr,
                                                             const int32_t* __restrict__ col,
                                                             const double* __restrict__ val,
                                                             const int64_t* __restrict__ optr,
                                                             int32_t* __restrict__ ocol, double* __restrict__ oval) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= 2 * m) return;
  const int64_t f = i / m, k = i - f * m;
  const int64_t src = f * nvr + (rows ? rows[k] : r0 + k);
  int64_t o = optr[i];
  for (int64_t q = ptr[src]; q < ptr[src + 1]; ++q, ++o) {
    ocol[o] = col[q];
    oval[o] = val[q];
  }
}

// node columns -> local [owned | ghost] numbering: owned blocks first, then
// ghosts, each in the row's (global) order
__global__ __launch_bounds__(256) void map_part_kernel(int64_t nr, const int64_t* __restrict__ ptr,
                                                       const int32_t* __restrict__ col, const dv4* __restrict__ val,
                                                       const int32_t* __restrict__ map, int32_t nown,
                                                       int32_t* __restrict__ ocol, dv4* __restrict__ oval) {
  const int64_t I = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (I >= nr) return;
  int64_t o = ptr[I];
  for (int part = 0; part < 2; ++part)
    for (int64_t k = ptr[I]; k < ptr[I + 1]; ++k) {
      const int32_t c = map[col[k]];
      if ((c < nown) == (part == 0)) { ocol[o] = c; oval[o] = val[k]; ++o; }
    }
}

// keep the blocks whose column lies in [w0, w1), renumbered from w0
__global__ __launch_bounds__(256) void window_len_kernel(int64_t nr, const int64_t* __restrict__ ptr,
                                                         const int32_t* __restrict__ col, int64_t w0, int64_t w1,
                                                         int64_t* __restrict__ len) {
  const int64_t I = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (I >= nr) return;
  int64_t c = 0;
  for (int64_t k = ptr[I]; k < ptr[I + 1]; ++k) c += col[k] >= w0 && col[k] < w1;
  len[I + 1] = c;
}

__global__ __launch_bounds__(256) void window_fill_kernel(int64_t nr, const int64_t* __restrict__ ptr,
                                                          const int32_t* __restrict__ col,
                                                          const dv4* __restrict__ val, int64_t w0, int64_t w1,
                                                          const int64_t* __restrict__ optr,
                                                          int32_t* __restrict__ ocol, dv4* __restrict__ oval) {
  const int64_t I = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (I >= nr) return;
  int64_t o = optr[I];
  for (int64_t k = ptr[I]; k < ptr[I + 1]; ++k)
    if (col[k] >= w0 && col[k] < w1) { ocol[o] = (int32_t)(col[k] - w0); oval[o] = val[k]; ++o; }
}

__global__ __launch_bounds__(256) void map_fill_kernel(int64_t n, int64_t first, int32_t base,
                                                       const int64_t* __restrict__ ids, int32_t* __restrict__ map) {
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (k >= n) return;
  map[ids ? ids[k] : first + k] = base + (int32_t)k;
}

__global__ __launch_bounds__(256) void ghost_row_kernel(int64_t nr, const int64_t* __restrict__ ptr,
                                                        const int32_t* __restrict__ col, int32_t nown,
                                                        uint8_t* __restrict__ flag) {
  const int64_t I = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (I >= nr) return;
  uint8_t g = 0;
  for (int64_t k = ptr[I]; k < ptr[I + 1]; ++k) g |= col[k] >= nown;
  flag[I] = g;
}

// a node split by seed blocks keeps the two diagonal entries of its block
__global__ __launch_bounds__(256) void unjoin_kernel(int64_t n, const uint8_t* __restrict__ joined, dv4* W) {
  const int64_t I = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (I < n && !joined[I]) { W[I].y = 0.0; W[I].z = 0.0; }
}

// rows of a field-major CSR (node rows r0 + i, or rows[i]) as a BSR2 with
// global node columns
int dev_rows_to_bsr(TmpPool* T, const DevMat& M, int64_t nvr, int64_t nvc, int64_t m, const int64_t* rows,
                    int64_t r0, TBsr* B, std::string* err) {
  int rc;
  DevMat S;
  S.n = 2 * m;
  S.m = M.m;
  if ((rc = T->alloc(&S.ptr, 2 * m + 1, err))) return rc;
  HIPCHK(dev_memset(S.ptr, 0, sizeof(int64_t)));
  if (m) rowlen_gather_kernel<<<nblocks(2 * m), 256>>>(m, nvr, rows, r0, M.ptr, S.ptr);
  HIPCHK(hipGetLastError());
  if ((rc = dscan_incl_i64(S.ptr, S.ptr, 2 * m + 1, nullptr, err))) return rc;
  HIPCHK(hipMemcpy(&S.nnz, S.ptr + 2 * m, sizeof(int64_t), hipMemcpyDeviceToHost));
  if ((rc = T->alloc(&S.col, S.nnz, err))) return rc;
  if ((rc = T->alloc(&S.val, S.nnz, err))) return rc;
  if (m) rowcopy_gather_kernel<<<nblocks(2 * m), 256>>>(m, nvr, rows, r0, M.ptr, M.col, M.val, S.ptr, S.col, S.val);
  HIPCHK(hipGetLastError());
  return dev_csr_to_bsr(T, S, m, nvc, B, err);
}

// column map of a distributed level: owned J -> J - o0, ghost g_k -> nloc + k
int dev_col_map(TmpPool* T, const DistLevel& L, int32_t** map, std::string* err) {
  int rc;
  if ((rc = T->alloc(map, L.nv, err))) return rc;
  HIPCHK(dev_memset(*map, 0xff, L.nv * sizeof(int32_t)));
  if (L.nloc) map_fill_kernel<<<nblocks(L.nloc), 256>>>(L.nloc, L.o0, 0, nullptr, *map);
  const int64_t ng = (int64_t)L.ghosts.size();
  if (ng) {
    int64_t* g = nullptr;
    if ((rc = T->alloc(&g, ng, err))) return rc;
    HIPCHK(hipMemcpy(g, L.ghosts.data(), ng * sizeof(int64_t), hipMemcpyHostToDevice));
    map_fill_kernel<<<nblocks(ng), 256>>>(ng, 0, (int32_t)L.nloc, g, *map);
  }
  HIPCHK(hipGetLastError());
  return MAMG_OK;
}

// BSR2 columns renumbered by map, [owned | ghost] order; nc = local columns
int dev_map_cols(TmpPool* T, const TBsr& B, const int32_t* map, int64_t nown, int64_t nc, TBsr* O,
                 std::string* err) {
  int rc;
  *O = B;
  O->nc = nc;
  if ((rc = T->alloc(&O->col, B.nb, err))) return rc;
  if ((rc = T->alloc(&O->val, B.nb, err))) return rc;
  if (B.nr) map_part_kernel<<<nblocks(B.nr), 256>>>(B.nr, B.ptr, B.col, B.val, map, (int32_t)nown, O->col, O->val);
  HIPCHK(hipGetLastError());
  return MAMG_OK;
}

int dev_window_cols(TmpPool* T, const TBsr& B, int64_t w0, int64_t w1, TBsr* O, std::string* err) {
  int rc;
  O->nr = B.nr; O->nc = w1 - w0; O->merged = false;
  if ((rc = T->alloc(&O->ptr, B.nr + 1, err))) return rc;
  HIPCHK(dev_memset(O->ptr, 0, sizeof(int64_t)));
  if (B.nr) window_len_kernel<<<nblocks(B.nr), 256>>>(B.nr, B.ptr, B.col, w0, w1, O->ptr);
  HIPCHK(hipGetLastError());
  if ((rc = dscan_incl_i64(O->ptr, O->ptr, B.nr + 1, nullptr, err))) return rc;
  HIPCHK(hipMemcpy(&O->nb, O->ptr + B.nr, sizeof(int64_t), hipMemcpyDeviceToHost));
  if ((rc = T->alloc(&O->col, O->nb, err))) return rc;
  if ((rc = T->alloc(&O->val, O->nb, err))) return rc;
  if (B.nr) window_fill_kernel<<<nblocks(B.nr), 256>>>(B.nr, B.ptr, B.col, B.val, w0, w1, O->ptr, O->col, O->val);
  HIPCHK(hipGetLastError());
  return MAMG_OK;
}

// ---- node patches on N ranks (dist_patches) --------------------------------
// hop distance of every node from the owned range (0 owned, 1..3, 127 beyond)
__global__ __launch_bounds__(256) void hop_init_kernel(int64_t nv, int64_t o0, int64_t o1, int8_t* __restrict__ d) {
  const int64_t I = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (I < nv) d[I] = (I >= o0 && I < o1) ? 0 : 127;
}
__global__ __launch_bounds__(256) void hop_step_kernel(int64_t nv, const int64_t* __restrict__ ptr,
                                                       const int32_t* __restrict__ col, const int8_t* __restrict__ din,
                                                       int8_t* __restrict__ dout, int k) {
  const int64_t I = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (I >= nv) return;
  int8_t v = din[I];
  if (v == 127)
    for (int64_t q = ptr[I]; q < ptr[I + 1]; ++q)
      if (din[col[q]] == k - 1) { v = (int8_t)k; break; }
  dout[I] = v;
}
// global id of local node li ([owned | ghost])
__device__ __forceinline__ int64_t local_gid(int64_t li, int64_t nloc, int64_t o0, const int64_t* gh) {
  return li < nloc ? o0 + li : gh[li - nloc];
}
// the rank's patch / ring-block rows: local row li = B's row of its global
// node when that node is within hmax hops of the owned range, else empty
// (len[li + 1])
__global__ __launch_bounds__(256) void srow_len_kernel(int64_t nl, int64_t nloc, int64_t o0, const int64_t* __restrict__ gh,
                                                       const int8_t* __restrict__ hop, const int64_t* __restrict__ bptr,
                                                       int64_t* __restrict__ len, int hmax) {
  const int64_t li = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (li >= nl) return;
  const int64_t g = local_gid(li, nloc, o0, gh);
  len[li + 1] = hop[g] <= hmax ? bptr[g + 1] - bptr[g] : 0;
}
// ... its blocks in B's (global) column order: local columns (map) and the
// global ids (the inverse kernel's search keys)
__global__ __launch_bounds__(256) void srow_fill_kernel(int64_t nl, int64_t nloc, int64_t o0, const int64_t* __restrict__ gh,
                                                        const int64_t* __restrict__ bptr, const int32_t* __restrict__ bcol,
                                                        const dv4* __restrict__ bval, const int32_t* __restrict__ map,
                                                        const int64_t* __restrict__ sptr, int32_t* __restrict__ scol,
                                                        int32_t* __restrict__ sgcol, dv4* __restrict__ sval) {
  const int64_t li = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (li >= nl || sptr[li + 1] == sptr[li]) return;
  const int64_t g = local_gid(li, nloc, o0, gh);
  int64_t o = sptr[li];
  for (int64_t k = bptr[g]; k < bptr[g + 1]; ++k, ++o) {
    scol[o] = map[bcol[k]];
    sgcol[o] = bcol[k];
    sval[o] = bval[k];
  }
}
// per local node: its hop distance and colour (for the centre list)
__global__ __launch_bounds__(256) void local_hop_colour_kernel(int64_t nl, int64_t nloc, int64_t o0,
                                                               const int64_t* __restrict__ gh,
                                                               const int8_t* __restrict__ hop,
                                                               const int16_t* __restrict__ c, int8_t* __restrict__ lh,
                                                               int16_t* __restrict__ lc) {
  const int64_t li = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (li >= nl) return;
  const int64_t g = local_gid(li, nloc, o0, gh);
  lh[li] = hop[g];
  lc[li] = c[g];
}
// colours of the patches that write node J (the centres in J's closed
// neighbourhood), -1 padded: PATCH_MAX_NODES + 1 slots per node
__global__ __launch_bounds__(256) void cover_kernel(int64_t cnt, const int64_t* __restrict__ nodes,
                                                    const int64_t* __restrict__ bptr, const int32_t* __restrict__ bcol,
                                                    const int16_t* __restrict__ c, int16_t* __restrict__ out) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= cnt) return;
  const int64_t J = nodes[t];
  int16_t* o = out + t * (PATCH_MAX_NODES + 1);
  int k = 0;
  bool self = false;
  for (int64_t q = bptr[J]; q < bptr[J + 1] && k < PATCH_MAX_NODES + 1; ++q) {
    self |= bcol[q] == J;
    o[k++] = c[bcol[q]];
  }
  if (!self && k < PATCH_MAX_NODES + 1) o[k++] = c[J];
  for (; k < PATCH_MAX_NODES + 1; ++k) o[k] = -1;
}

// Level-0 node patches of a rank: the global distance-3
// colouring (every rank colours the whole level-0 graph, as the single-GPU
// build_patches, so all ranks hold the same colours); the centres within 1
// hop of the owned nodes (their patches write owned nodes; the owner of
// every written node computes the same patch from the same x, so its bits
// agree); their rows (nodes within 2 hops) with the global column order kept
// (the patch's local dof order, hence its Gauss-Jordan, equals the single
// GPU's); the inverses; and per colour the halo of the nodes its patches
// write (send: owned nodes in a peer's 3-hop region, receive: ghosts), so
// that the ghosts within 3 hops are current before the next colour.
int dist_patches(DistHandle* h, const DevMat& A0d, const DistLevel& P, DDLevel* D, std::string* err) {
  int rc;
  TmpPool T(h->sw);
  const int64_t nv = P.nv, nloc = P.nloc, ng = (int64_t)P.ghosts.size(), nl = nloc + ng;
  const int R = h->nranks;
  TBsr B;
  if ((rc = dev_csr_to_bsr(&T, A0d, nv, nv, &B, err))) return rc;
  int16_t* c = nullptr;
  int maxlen = 0;
  if ((rc = patch_colour(&T, B, &c, &maxlen, err))) return rc;
  int16_t hcol_max = 0;
  {
    std::vector<int16_t> hc(nv);
    HIPCHK(hipMemcpy(hc.data(), c, nv * sizeof(int16_t), hipMemcpyDeviceToHost));
    for (int16_t v : hc) hcol_max = std::max(hcol_max, v);
  }
  const int ncol = hcol_max + 1;
  int8_t *hop = nullptr, *hop2 = nullptr;
  if ((rc = T.alloc(&hop, nv, err)) || (rc = T.alloc(&hop2, nv, err))) return rc;
  hop_init_kernel<<<nblocks(nv), 256>>>(nv, P.o0, P.o1, hop);
  for (int k = 1; k <= 3; ++k) {
    hop_step_kernel<<<nblocks(nv), 256>>>(nv, B.ptr, B.col, hop, hop2, k);
    std::swap(hop, hop2);
  }
  HIPCHK(hipGetLastError());
  int64_t* gh = nullptr;
  if ((rc = T.alloc(&gh, std::max<int64_t>(ng, 1), err))) return rc;
  if (ng) HIPCHK(hipMemcpy(gh, P.ghosts.data(), ng * sizeof(int64_t), hipMemcpyHostToDevice));
  int32_t* map = nullptr;
  if ((rc = dev_col_map(&T, P, &map, err))) return rc;
  // the patch rows
  DLevel& L = D->pl;
  if ((rc = ddalloc(h, &L.Sptr, nl + 1, err))) return rc;
  if (nl) srow_len_kernel<<<nblocks(nl), 256>>>(nl, nloc, P.o0, gh, hop, B.ptr, L.Sptr, 2);
  HIPCHK(hipGetLastError());
  if ((rc = dscan_incl_i64(L.Sptr, L.Sptr, nl + 1, nullptr, err))) return rc;
  HIPCHK(hipMemcpy(&L.Snb, L.Sptr + nl, sizeof(int64_t), hipMemcpyDeviceToHost));
  if ((rc = ddalloc(h, &L.Scol, std::max<int64_t>(L.Snb, 1), err))) return rc;
  if ((rc = ddalloc(h, &D->Sgcol, std::max<int64_t>(L.Snb, 1), err))) return rc;
  if ((rc = ddalloc(h, &L.Sval, std::max<int64_t>(L.Snb, 1), err))) return rc;
  if (nl) srow_fill_kernel<<<nblocks(nl), 256>>>(nl, nloc, P.o0, gh, B.ptr, B.col, B.val, map, L.Sptr, L.Scol, D->Sgcol,
                                                 L.Sval);
  HIPCHK(hipGetLastError());
  // the centres (within 1 hop), colour by colour, ascending global id inside a colour
  std::vector<int8_t> lh(nl);
  std::vector<int16_t> lc(nl);
  {
    int8_t* dlh = nullptr;
    int16_t* dlc = nullptr;
    if ((rc = T.alloc(&dlh, std::max<int64_t>(nl, 1), err)) || (rc = T.alloc(&dlc, std::max<int64_t>(nl, 1), err)))
      return rc;
    if (nl) local_hop_colour_kernel<<<nblocks(nl), 256>>>(nl, nloc, P.o0, gh, hop, c, dlh, dlc);
    HIPCHK(hipGetLastError());
    if (nl) {
      HIPCHK(hipMemcpy(lh.data(), dlh, nl, hipMemcpyDeviceToHost));
      HIPCHK(hipMemcpy(lc.data(), dlc, nl * sizeof(int16_t), hipMemcpyDeviceToHost));
    }
  }
  std::vector<std::pair<int64_t, int64_t>> cen;   // (colour << 40 | global id, local id)
  for (int64_t li = 0; li < nl; ++li)
    if (lh[li] <= 1) {
      const int64_t g = li < nloc ? P.o0 + li : P.ghosts[li - nloc];
      cen.push_back({((int64_t)lc[li] << 40) | g, li});
    }
  std::sort(cen.begin(), cen.end());
  const int64_t np = (int64_t)cen.size();
  L.pcs.assign(ncol + 1, 0);
  std::vector<int32_t> perm(np);
  for (int64_t i = 0; i < np; ++i) {
    perm[i] = (int32_t)cen[i].second;
    ++L.pcs[(cen[i].first >> 40) + 1];
  }
  for (int k = 0; k < ncol; ++k) L.pcs[k + 1] += L.pcs[k];
  L.n = 2 * np;
  if ((rc = ddalloc(h, &L.pperm, std::max<int64_t>(np, 1), err))) return rc;
  if (np) HIPCHK(hipMemcpy(L.pperm, perm.data(), np * sizeof(int32_t), hipMemcpyHostToDevice));
  // inverses
  const int64_t dmax = 2 * (int64_t)maxlen;
  L.pus = dmax * (dmax + 1) / 2;
  if ((rc = ddalloc(h, &L.pu, std::max<int64_t>(np * L.pus, 1), err))) return rc;
  int* bad = nullptr;
  if ((rc = T.alloc(&bad, 1, err))) return rc;
  HIPCHK(dev_memset(bad, 0, sizeof(int)));
  launch_patch_inv(h->sw.patch_inv, np, L.pperm, L.Sptr, L.Scol, D->Sgcol, L.Sval, L.pus, L.pu, bad);
  HIPCHK(hipGetLastError());
  int hb = 0;
  HIPCHK(hipMemcpy(&hb, bad, sizeof(int), hipMemcpyDeviceToHost));
  if (hb) { *err = "node patches: a patch matrix is not SPD (non-positive Gauss-Jordan pivot)"; return MAMG_ERR_SETUP; }
  // each colour's halo: the listed nodes its patches write
  const int64_t ns = P.send_off.empty() ? 0 : P.send_off.back();
  std::vector<int64_t> lst(ns + ng);
  for (int64_t t = 0; t < ns; ++t) lst[t] = P.o0 + P.send_idx[t];
  for (int64_t g = 0; g < ng; ++g) lst[ns + g] = P.ghosts[g];
  constexpr int CW = PATCH_MAX_NODES + 1;
  std::vector<int16_t> cov((size_t)(ns + ng) * CW);
  if (ns + ng) {
    int64_t* dl = nullptr;
    int16_t* dc = nullptr;
    if ((rc = T.alloc(&dl, ns + ng, err)) || (rc = T.alloc(&dc, (ns + ng) * CW, err))) return rc;
    HIPCHK(hipMemcpy(dl, lst.data(), (ns + ng) * sizeof(int64_t), hipMemcpyHostToDevice));
    cover_kernel<<<nblocks(ns + ng), 256>>>(ns + ng, dl, B.ptr, B.col, c, dc);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpy(cov.data(), dc, cov.size() * sizeof(int16_t), hipMemcpyDeviceToHost));
  }
  auto covers = [&](int64_t t, int col) {
    for (int k = 0; k < CW; ++k)
      if (cov[(size_t)t * CW + k] == col) return true;
    return false;
  };
  std::vector<int64_t> cs, cg;
  D->cs_off.assign((size_t)ncol * (R + 1), 0);
  D->cg_off.assign((size_t)ncol * (R + 1), 0);
  for (int col = 0; col < ncol; ++col) {
    for (int q = 0; q < R; ++q) {
      D->cs_off[(size_t)col * (R + 1) + q] = (int64_t)cs.size();
      D->cg_off[(size_t)col * (R + 1) + q] = (int64_t)cg.size();
      for (int64_t t = P.send_off[q]; t < P.send_off[q + 1]; ++t)
        if (covers(t, col)) cs.push_back(P.send_idx[t]);
      for (int64_t g = P.ghost_off[q]; g < P.ghost_off[q + 1]; ++g)
        if (covers(ns + g, col)) cg.push_back(g);
    }
    D->cs_off[(size_t)col * (R + 1) + R] = (int64_t)cs.size();
    D->cg_off[(size_t)col * (R + 1) + R] = (int64_t)cg.size();
  }
  if (!cs.empty()) {
    if ((rc = ddalloc(h, &D->csend_idx, (int64_t)cs.size(), err))) return rc;
    HIPCHK(hipMemcpy(D->csend_idx, cs.data(), cs.size() * sizeof(int64_t), hipMemcpyHostToDevice));
  }
  if (!cg.empty()) {
    if ((rc = ddalloc(h, &D->cghost_idx, (int64_t)cg.size(), err))) return rc;
    HIPCHK(hipMemcpy(D->cghost_idx, cg.data(), cg.size() * sizeof(int64_t), hipMemcpyHostToDevice));
  }
  D->patches = true;
  if (h->p.print_level >= 2)
    std::fprintf(stderr, "[mamg] rank %d/%d node patches: %d colours, %lld centres (%lld owned), %lld ghost nodes "
                 "(3 hops), colour halos %lld sends / %lld receives in all\n", h->rank, R, ncol, (long long)np,
                 (long long)nloc, (long long)ng, (long long)cs.size(), (long long)cg.size());
  return MAMG_OK;
}

// Level-0 seed-ring Schwarz of a rank (SCHWARZ_RINGS on N GPUs, DESIGN.md
// 6.4): every rank builds the global blocks, inverses and
// conflict colouring (ring_blocks_dev + ring_colouring, the single-GPU
// build_rings' steps, so every rank holds the same blocks and colours) and
// keeps the blocks with a member node it owns -- the owner of every written
// node computes every block that writes it, from the same x, so its bits agree
// with one GPU's.  A block's members lie within 2 maxlvl hops of an owned node
// and its rows read x within 2 maxlvl + 1 hops: the ghost region.  The rest's
// multicolour GS runs on the owned rows with the covered dofs masked
// (dev_rank_ops, from *cov_owned).  One colour table serves both: ring colour
// c at index c (the nodes its blocks write), GS colour g at nrc + g (the nodes
// of that colour), each with the halo of those nodes in the send / ghost
// lists, so the exchange code is the multicolour GS's.
int dist_rings(DistHandle* h, const DevMat& A0d, const DistLevel& P, const std::vector<int32_t>& seeds,
               const int8_t* gcol, int ngc, DDLevel* D, uint8_t** cov_owned, std::string* err) {
  int rc;
  TmpPool T(h->sw);
  const mamg_params& p = h->p;
  const int64_t nv = P.nv, nloc = P.nloc, ng = (int64_t)P.ghosts.size(), nl = nloc + ng, n = A0d.n;
  const int R = h->nranks, L = p.Schwarz_maxlvl;
  const int64_t ns = (int64_t)seeds.size();
  if (ns <= 0) { *err = "seed rings: no seeds"; return MAMG_ERR_ARG; }
  // the global blocks and their conflict colouring (build_rings)
  RingBlocks RB;
  if ((rc = ring_blocks_dev(A0d, seeds.data(), ns, L, p.Schwarz_mmsize, &RB, err))) return rc;
  struct Guard { RingBlocks* r; ~Guard() { ring_blocks_free(r); } } guard{&RB};
  const int mm = RB.mm;
  std::vector<int32_t> blk((size_t)ns * mm);
  std::vector<int64_t> blen(ns);
  HIPCHK(hipMemcpy(blk.data(), RB.blk, blk.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(blen.data(), RB.blen, ns * sizeof(int64_t), hipMemcpyDeviceToHost));
  std::vector<int64_t> bptr(ns + 1, 0);
  for (int64_t k = 0; k < ns; ++k) bptr[k + 1] = bptr[k] + blen[k];
  std::vector<int32_t> mem(bptr[ns]);
  for (int64_t k = 0; k < ns; ++k) std::copy(blk.begin() + k * mm, blk.begin() + k * mm + blen[k], mem.begin() + bptr[k]);
  std::vector<int32_t>().swap(blk);
  std::vector<int32_t> colour;
  {
    std::vector<int64_t> aptr(n + 1);
    std::vector<int32_t> acol(A0d.nnz);
    HIPCHK(hipMemcpy(aptr.data(), A0d.ptr, (n + 1) * sizeof(int64_t), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(acol.data(), A0d.col, A0d.nnz * sizeof(int32_t), hipMemcpyDeviceToHost));
    CsrView Av;
    Av.n = Av.m = n; Av.ptr = aptr.data(); Av.col = acol.data();
    ring_colouring(Av, bptr, mem, &colour);
  }
  int nrc = 0;
  for (int32_t c : colour) nrc = std::max(nrc, c + 1);
  std::vector<int32_t> ord(ns);
  std::iota(ord.begin(), ord.end(), 0);
  std::stable_sort(ord.begin(), ord.end(), [&](int32_t a, int32_t b) { return colour[a] < colour[b]; });
  // local node ids (owned first, then ghosts), covered dofs, the colours
  // writing each node (one bit per ring colour)
  std::vector<int32_t> loc(nv, -1);
  for (int64_t i = 0; i < nloc; ++i) loc[P.o0 + i] = (int32_t)i;
  for (int64_t g = 0; g < ng; ++g) loc[P.ghosts[g]] = (int32_t)(nloc + g);
  const int CW = (nrc + 63) / 64;
  std::vector<uint64_t> wr((size_t)nv * std::max(CW, 1), 0);
  std::vector<uint8_t> cov(nv, 0);
  for (int64_t k = 0; k < ns; ++k)
    for (int64_t t = bptr[k]; t < bptr[k + 1]; ++t) {
      const int64_t gd = mem[t], I = gd % nv, f = gd / nv;
      cov[I] |= (uint8_t)(1u << f);
      wr[(size_t)I * CW + colour[k] / 64] |= 1ull << (colour[k] % 64);
    }
  // the rank's blocks: a member node owned, colour by colour (seed order inside)
  DLevel& RL = D->rl;
  RL.rcs.assign(nrc + 1, 0);
  std::vector<int32_t> mine;
  std::vector<int64_t> mo(1, 0), io(1, 0);
  std::vector<int32_t> rm;
  for (int64_t j = 0; j < ns; ++j) {
    const int32_t k = ord[j];
    bool own = false;
    for (int64_t t = bptr[k]; t < bptr[k + 1] && !own; ++t) {
      const int64_t I = mem[t] % nv;
      own = I >= P.o0 && I < P.o1;
    }
    if (!own) continue;
    for (int64_t t = bptr[k]; t < bptr[k + 1]; ++t) {
      const int64_t gd = mem[t], I = gd % nv, f = gd / nv;
      if (loc[I] < 0) {
        *err = "multi-GPU seed rings: a block member outside the rank's " + std::to_string(2 * L + 1) +
               "-hop ghost region";
        return MAMG_ERR_SETUP;
      }
      rm.push_back(2 * loc[I] + (int32_t)f);
    }
    mine.push_back(k);
    mo.push_back(mo.back() + blen[k]);
    io.push_back(io.back() + blen[k] * blen[k]);
    ++RL.rcs[colour[k] + 1];
  }
  for (int c = 0; c < nrc; ++c) RL.rcs[c + 1] += RL.rcs[c];
  const int64_t nb = (int64_t)mine.size();
  RL.n = 2 * nl;
  RL.rnm = mo.back();
  RL.rinv_n = (double)io.back();
  if ((rc = ddalloc(h, &RL.rmo, nb + 1, err)) || (rc = ddalloc(h, &RL.rio, nb + 1, err)) ||
      (rc = ddalloc(h, &RL.rmem, std::max<int64_t>(RL.rnm, 1), err)) ||
      (rc = ddalloc(h, &RL.rinv, std::max<int64_t>(io.back(), 1), err)))
    return rc;
  HIPCHK(hipMemcpy(RL.rmo, mo.data(), (nb + 1) * sizeof(int64_t), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(RL.rio, io.data(), (nb + 1) * sizeof(int64_t), hipMemcpyHostToDevice));
  if (RL.rnm) HIPCHK(hipMemcpy(RL.rmem, rm.data(), rm.size() * sizeof(int32_t), hipMemcpyHostToDevice));
  if (nb) {
    int32_t* dmine = nullptr;
    if ((rc = T.alloc(&dmine, nb, err))) return rc;
    HIPCHK(hipMemcpy(dmine, mine.data(), nb * sizeof(int32_t), hipMemcpyHostToDevice));
    ring_perm_inv(nb, dmine, RB.blen, RB.sq, RB.inv, RL.rio, RL.rinv);
    HIPCHK(hipGetLastError());
  }
  // the block rows: A_0's node rows of the local nodes within 2 L hops,
  // local columns (the ring kernel reads x through them)
  TBsr B;
  if ((rc = dev_csr_to_bsr(&T, A0d, nv, nv, &B, err))) return rc;
  int8_t *hop = nullptr, *hop2 = nullptr;
  if ((rc = T.alloc(&hop, nv, err)) || (rc = T.alloc(&hop2, nv, err))) return rc;
  hop_init_kernel<<<nblocks(nv), 256>>>(nv, P.o0, P.o1, hop);
  for (int k = 1; k <= 2 * L; ++k) {
    hop_step_kernel<<<nblocks(nv), 256>>>(nv, B.ptr, B.col, hop, hop2, k);
    std::swap(hop, hop2);
  }
  HIPCHK(hipGetLastError());
  int64_t* gh = nullptr;
  if ((rc = T.alloc(&gh, std::max<int64_t>(ng, 1), err))) return rc;
  if (ng) HIPCHK(hipMemcpy(gh, P.ghosts.data(), ng * sizeof(int64_t), hipMemcpyHostToDevice));
  int32_t* map = nullptr;
  if ((rc = dev_col_map(&T, P, &map, err))) return rc;
  if ((rc = ddalloc(h, &RL.Sptr, nl + 1, err))) return rc;
  if (nl) srow_len_kernel<<<nblocks(nl), 256>>>(nl, nloc, P.o0, gh, hop, B.ptr, RL.Sptr, 2 * L);
  HIPCHK(hipGetLastError());
  if ((rc = dscan_incl_i64(RL.Sptr, RL.Sptr, nl + 1, nullptr, err))) return rc;
  HIPCHK(hipMemcpy(&RL.Snb, RL.Sptr + nl, sizeof(int64_t), hipMemcpyDeviceToHost));
  int32_t* sg = nullptr;
  if ((rc = ddalloc(h, &RL.Scol, std::max<int64_t>(RL.Snb, 1), err)) ||
      (rc = T.alloc(&sg, std::max<int64_t>(RL.Snb, 1), err)) ||
      (rc = ddalloc(h, &RL.Sval, std::max<int64_t>(RL.Snb, 1), err)))
    return rc;
  if (nl) srow_fill_kernel<<<nblocks(nl), 256>>>(nl, nloc, P.o0, gh, B.ptr, B.col, B.val, map, RL.Sptr, RL.Scol, sg,
                                                 RL.Sval);
  HIPCHK(hipGetLastError());
  // the covered dofs of the owned nodes (the rest's GS masks them)
  if ((rc = ddalloc(h, cov_owned, std::max<int64_t>(nloc, 1), err))) return rc;
  if (nloc) HIPCHK(hipMemcpy(*cov_owned, cov.data() + P.o0, nloc, hipMemcpyHostToDevice));
  // the colour table: ring colours, then the rest GS's node colours
  std::vector<int8_t> hc(nv);
  if (nv) HIPCHK(hipMemcpy(hc.data(), gcol, nv, hipMemcpyDeviceToHost));
  auto in = [&](int64_t I, int idx) {
    return idx < nrc ? ((wr[(size_t)I * CW + idx / 64] >> (idx % 64)) & 1ull) != 0 : hc[I] == idx - nrc;
  };
  const int nct = nrc + ngc;
  std::vector<int64_t> cs, cg;
  D->cs_off.assign((size_t)nct * (R + 1), 0);
  D->cg_off.assign((size_t)nct * (R + 1), 0);
  for (int idx = 0; idx < nct; ++idx) {
    for (int q = 0; q < R; ++q) {
      D->cs_off[(size_t)idx * (R + 1) + q] = (int64_t)cs.size();
      D->cg_off[(size_t)idx * (R + 1) + q] = (int64_t)cg.size();
      for (int64_t t = P.send_off[q]; t < P.send_off[q + 1]; ++t)
        if (in(P.o0 + P.send_idx[t], idx)) cs.push_back(P.send_idx[t]);
      for (int64_t g = P.ghost_off[q]; g < P.ghost_off[q + 1]; ++g)
        if (in(P.ghosts[g], idx)) cg.push_back(g);
    }
    D->cs_off[(size_t)idx * (R + 1) + R] = (int64_t)cs.size();
    D->cg_off[(size_t)idx * (R + 1) + R] = (int64_t)cg.size();
  }
  if (!cs.empty()) {
    if ((rc = ddalloc(h, &D->csend_idx, (int64_t)cs.size(), err))) return rc;
    HIPCHK(hipMemcpy(D->csend_idx, cs.data(), cs.size() * sizeof(int64_t), hipMemcpyHostToDevice));
  }
  if (!cg.empty()) {
    if ((rc = ddalloc(h, &D->cghost_idx, (int64_t)cg.size(), err))) return rc;
    HIPCHK(hipMemcpy(D->cghost_idx, cg.data(), cg.size() * sizeof(int64_t), hipMemcpyHostToDevice));
  }
  D->rings = true;
  D->nrc = nrc;
  if (p.print_level >= 2)
    std::fprintf(stderr, "[mamg] rank %d/%d seed rings: %lld of %lld blocks, %d ring colours + %d GS colours, "
                 "%lld ghost nodes (%d hops), colour halos %lld sends / %lld receives in all\n", h->rank, R,
                 (long long)nb, (long long)ns, nrc, ngc, (long long)ng, 2 * L + 1, (long long)cs.size(),
                 (long long)cg.size());
  return MAMG_OK;
}

// each colour's halo of a distributed level: colour c's nodes in every send
// list and ghost list, in list order (so the sender's subset and the
// receiver's subset match), offsets per (colour, peer); gcol = the level's
// global colouring on the device
int colour_halo_lists(DistHandle* h, const DistLevel& P, const int8_t* gcol, int ncol, DDLevel* D,
                      std::string* err) {
  const int R = h->nranks;
  std::vector<int8_t> hc(P.nv);
  if (P.nv) HIPCHK(hipMemcpy(hc.data(), gcol, P.nv, hipMemcpyDeviceToHost));
  std::vector<int64_t> cs, cg;
  D->cs_off.assign((size_t)ncol * (R + 1), 0);
  D->cg_off.assign((size_t)ncol * (R + 1), 0);
  for (int c = 0; c < ncol; ++c) {
    for (int q = 0; q < R; ++q) {
      D->cs_off[(size_t)c * (R + 1) + q] = (int64_t)cs.size();
      D->cg_off[(size_t)c * (R + 1) + q] = (int64_t)cg.size();
      for (int64_t t = P.send_off[q]; t < P.send_off[q + 1]; ++t)
        if (hc[P.o0 + P.send_idx[t]] == c) cs.push_back(P.send_idx[t]);
      for (int64_t g = P.ghost_off[q]; g < P.ghost_off[q + 1]; ++g)
        if (hc[P.ghosts[g]] == c) cg.push_back(g);
    }
    D->cs_off[(size_t)c * (R + 1) + R] = (int64_t)cs.size();
    D->cg_off[(size_t)c * (R + 1) + R] = (int64_t)cg.size();
  }
  int rc;
  if (!cs.empty()) {
    if ((rc = ddalloc(h, &D->csend_idx, (int64_t)cs.size(), err))) return rc;
    HIPCHK(hipMemcpy(D->csend_idx, cs.data(), cs.size() * sizeof(int64_t), hipMemcpyHostToDevice));
  }
  if (!cg.empty()) {
    if ((rc = ddalloc(h, &D->cghost_idx, (int64_t)cg.size(), err))) return rc;
    HIPCHK(hipMemcpy(D->cghost_idx, cg.data(), cg.size() * sizeof(int64_t), hipMemcpyHostToDevice));
  }
  return MAMG_OK;
}

// the longest run [*r0, *r1) of M's rows whose columns are all < nown (owned:
// no ghost), for the launches during a halo
constexpr int64_t K_ROWS_ALIGN = 256;   // launch_msell row ranges: whole workgroups of every LPR
int ghost_free_run(TmpPool* T, const TBsr& M, int64_t nown, int64_t* r0, int64_t* r1, std::string* err) {
  int rc;
  const int64_t n = M.nr;
  uint8_t* fl = nullptr;
  if ((rc = T->alloc(&fl, n, err))) return rc;
  if (n) ghost_row_kernel<<<nblocks(n), 256>>>(n, M.ptr, M.col, (int32_t)nown, fl);
  HIPCHK(hipGetLastError());
  std::vector<uint8_t> hf(n);
  if (n) HIPCHK(hipMemcpy(hf.data(), fl, n, hipMemcpyDeviceToHost));
  int64_t best0 = 0, best1 = 0, run0 = 0;
  for (int64_t I = 0; I <= n; ++I)
    if (I == n || hf[I]) {
      if (I - run0 > best1 - best0) { best0 = run0; best1 = I; }
      run0 = I + 1;
    }
  *r0 = best0;
  *r1 = best1;
  return MAMG_OK;
}

// level l's A_loc (+ overlap window, band schedule), K / [P | AP] / P, R_loc
// and W from the GPU hierarchy (the operator block of dist_upload)
int dev_rank_ops(DistHandle* h, const GHier& G, const DevMat& A0d, const DistPlan& plan, int l, double kw,
                 const int8_t* gcol, int ncol, std::string* err) {
  int rc;
  const DistLevel& P = plan.levels[l];
  const GLevel& g = G.levels[l];
  DDLevel& D = h->L[l];
  const int64_t nv = P.nv, nloc = P.nloc, nc = nloc + (int64_t)P.ghosts.size();
  TmpPool T(h->sw);
  int32_t* map = nullptr;
  if (!P.replicated && (rc = dev_col_map(&T, P, &map, err))) return rc;
  // W (node blocks of the owned rows)
  if ((rc = ddalloc(h, &D.W, nloc, err))) return rc;
  if (nloc) {
    HIPCHK(dev_copy(D.W, reinterpret_cast<const dv4*>(g.W) + P.o0, nloc * sizeof(dv4)));
    if (g.joined) unjoin_kernel<<<nblocks(nloc), 256>>>(nloc, g.joined + P.o0, D.W);
    HIPCHK(hipGetLastError());
  }
  // A_loc (+ the multicolour GS layout of its rows, colours of the level's
  // global colouring gcol)
  {
    TBsr raw, tA;
    const DevMat& Am = l == 0 ? A0d : g.A;
    if ((rc = dev_rows_to_bsr(&T, Am, nv, nv, nloc, nullptr, P.o0, &raw, err))) return rc;
    if (P.replicated) tA = raw;
    else if ((rc = dev_map_cols(&T, raw, map, nloc, nc, &tA, err))) return rc;
    if (!P.replicated && (rc = ghost_free_run(&T, tA, nloc, &D.ib0, &D.ib1, err)))   // overlap window
      return rc;
    bool half = false;
    if (l == 0 && h->sw.half && tA.nr >= h->sw.sell_min_rows && tA.nb > 0) {   // upload_half_or_bsr
      int* bad = nullptr;
      if ((rc = T.alloc(&bad, 1, err))) return rc;
      HIPCHK(dev_memset(bad, 0, sizeof(int)));
      sym_check(tA.nb, tA.val, bad);
      int hb = 1;
      HIPCHK(hipMemcpy(&hb, bad, sizeof(int), hipMemcpyDeviceToHost));
      if (hb == 0) {
        D.A.nr = tA.nr; D.A.nc = tA.nc; D.A.nb = tA.nb;
        D.A.lanes = pick_lanes_bsr(tA.nr, tA.nb);
        D.A.sym = true;
        if ((rc = try_half(h, &T, tA, &D.A, err))) return rc;
        half = D.A.half;
      }
    }
    if (!half && (rc = finalize_bsr(h, &T, tA, &D.A, 0, true, err))) return rc;
    if (l == 0 && (rc = build_band_sched_range(h, &D.A, D.ib0, D.ib1, err))) return rc;
    if (gcol) {
      // seed rings: the rest's GS, covered dofs masked (build_rings' rest_w /
      // rest_mask on the owned rows)
      const double* Wg = reinterpret_cast<const double*>(D.W);
      if (D.rcov && nloc) {
        dv4* Wp = nullptr;
        if ((rc = T.alloc(&Wp, nloc, err))) return rc;
        rest_w(nloc, D.W, D.rcov, Wp);
        HIPCHK(hipGetLastError());
        Wg = reinterpret_cast<const double*>(Wp);
      }
      if ((rc = gs_layout(h, &T, tA, Wg, gcol + P.o0, ncol, l, &D.Gb, &D.gperm, &D.Gd, &D.gcs, &D.gbk, err)))
        return rc;
      const int64_t nrp = D.gcs.empty() ? 0 : D.gcs.back();
      if (D.rcov && nrp) rest_mask(nrp, D.gperm, D.rcov, D.Gd);
      HIPCHK(hipGetLastError());
    }
  }
  // prolongation side (level l+1 numbering)
  const DistLevel& C = plan.levels[l + 1];
  const int64_t cnc = C.replicated ? C.nv : C.nloc + (int64_t)C.ghosts.size();
  int32_t* cmap = nullptr;
  if (!C.replicated && (rc = dev_col_map(&T, C, &cmap, err))) return rc;
  auto rows_c = [&](const DevMat& M, TBsr* O) -> int {   // rows [o0, o1) of a fine x coarse CSR
    TBsr raw;
    int r = dev_rows_to_bsr(&T, M, nv, C.nv, nloc, nullptr, P.o0, &raw, err);
    if (r) return r;
    if (C.replicated) { *O = raw; return MAMG_OK; }
    return dev_map_cols(&T, raw, cmap, C.nloc, cnc, O, err);
  };
  TBsr tP;
  if ((rc = rows_c(g.P, &tP))) return rc;
  if (plan.fuse) {
    TBsr tAP, tK;
    if ((rc = rows_c(g.AP, &tAP))) return rc;
    if (plan.kpost) {
      const double* Wk = reinterpret_cast<const double*>(D.W);
      if (kw != 1.0 && nloc) {
        double* q = nullptr;
        if ((rc = T.alloc(&q, 4 * nloc, err))) return rc;
        wscale(4 * nloc, kw, Wk, q);
        HIPCHK(hipGetLastError());
        Wk = q;
      }
      if ((rc = dev_kmerge(&T, tP, tAP, Wk, &tK, err))) return rc;
      if ((rc = finalize_bsr(h, &T, tK, &D.K, 0, false, err))) return rc;
      D.K.kvar = h->sw.k_variant;
      if (l == 0 && h->sw.k_sort && D.K.sell && D.K.lpr <= 1)   // rows sorted inside slices (section 4.1)
        if ((rc = sort_sell_slices(h, &T, &D.K, err))) return rc;
      // K's rows without coarse ghost columns, run while the coarse-e halo is
      // in flight (level 0's SELL K: launch_msell takes row ranges)
      if (l == 0 && !P.replicated && !C.replicated) {
        int64_t k0 = 0, k1 = 0;
        if ((rc = ghost_free_run(&T, tK, C.nloc, &k0, &k1, err))) return rc;
        k0 = (k0 + K_ROWS_ALIGN - 1) / K_ROWS_ALIGN * K_ROWS_ALIGN;
        k1 = k1 == nloc ? nloc : k1 / K_ROWS_ALIGN * K_ROWS_ALIGN;
        if (k1 > k0) { D.kb0 = k0; D.kb1 = k1; }
      }
    } else {
      if ((rc = dev_merge_rows(&T, tP, tAP, &tK, err))) return rc;
      if ((rc = finalize_bsr(h, &T, tK, &D.PA, 0, false, err))) return rc;
    }
  } else if ((rc = finalize_bsr(h, &T, tP, &D.P, 0, false, err))) {
    return rc;
  }
  // partial restriction R_loc = P_loc^T: R's rows of the local coarse nodes
  // ([owned | ghost], or all when replicated), columns in [o0, o1)
  {
    std::vector<int64_t> rows;
    rows.reserve(cnc);
    if (C.replicated) {
      for (int64_t J = 0; J < C.nv; ++J) rows.push_back(J);
    } else {
      for (int64_t J = C.o0; J < C.o1; ++J) rows.push_back(J);
      rows.insert(rows.end(), C.ghosts.begin(), C.ghosts.end());
    }
    int64_t* drows = nullptr;
    if ((rc = T.alloc(&drows, cnc, err))) return rc;
    if (cnc) HIPCHK(hipMemcpy(drows, rows.data(), cnc * sizeof(int64_t), hipMemcpyHostToDevice));
    TBsr raw, tR;
    if ((rc = dev_rows_to_bsr(&T, g.R, C.nv, nv, cnc, drows, 0, &raw, err))) return rc;
    if ((rc = dev_window_cols(&T, raw, P.o0, P.o1, &tR, err))) return rc;
    if ((rc = finalize_bsr(h, &T, tR, &D.R, 0, false, err))) return rc;
  }
  return MAMG_OK;
}

int upload_dcsr(DistHandle* h, const Csr& M, DCsr* D, int lanes, std::string* err) {
  D->n = M.n;
  D->m = M.m;
  D->nnz = M.nnz();
  D->lanes = lanes > 0 ? lanes : pick_lanes(M.n, D->nnz);
  int rc;
  if ((rc = ddalloc(h, &D->ptr, M.n + 1, err))) return rc;
  if ((rc = ddalloc(h, &D->col, std::max<int64_t>(D->nnz, 1), err))) return rc;
  if ((rc = ddalloc(h, &D->val, std::max<int64_t>(D->nnz, 1), err))) return rc;
  if (M.ptr.size() == (size_t)M.n + 1)
    HIPCHK(hipMemcpy(D->ptr, M.ptr.data(), (M.n + 1) * sizeof(int64_t), hipMemcpyHostToDevice));
  if (D->nnz) {
    HIPCHK(hipMemcpy(D->col, M.col.data(), D->nnz * sizeof(int32_t), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(D->val, M.val.data(), D->nnz * sizeof(double), hipMemcpyHostToDevice));
  }
  return MAMG_OK;
}

// one level of a scalar (CSR) plan: A_loc / P_loc / Rp_loc, the WB rows or
// the winv slice, POLY's step smoothers (values only, as poly_scaled), the
// dense inverse in natural order, and the level-0 interior row run
int upload_scalar_level(DistHandle* h, const HostLevel& hl, const DistLevel& P, int l, int pm, const double* pw,
                        std::string* err) {
  DDLevel& D = h->L[l];
  int rc;
  if ((rc = upload_dcsr(h, P.cA, &D.cA, l == 0 ? h->p.spmv_lanes : 0, err))) return rc;
  if (D.coarsest) {
    const int64_t n = hl.n;
    if ((rc = ddalloc(h, &D.Ainv, n * n, err))) return rc;
    HIPCHK(hipMemcpy(D.Ainv, hl.Ainv.data(), n * n * sizeof(double), hipMemcpyHostToDevice));
    return MAMG_OK;
  }
  if ((rc = upload_dcsr(h, P.cP, &D.cP, 0, err))) return rc;
  if ((rc = upload_dcsr(h, P.cRp, &D.cR, 0, err))) return rc;
  const bool blk = P.cWB.n > 0;
  if (blk) {
    if ((rc = upload_dcsr(h, P.cWB, &D.cWB, 0, err))) return rc;
  } else {
    if ((int64_t)P.W.size() != D.nloc) { *err = "scalar plan: winv slice does not cover the owned rows"; return MAMG_ERR_ARG; }
    if ((rc = ddalloc(h, &D.winv, D.nloc, err))) return rc;
    if (D.nloc) HIPCHK(hipMemcpy(D.winv, P.W.data(), D.nloc * sizeof(double), hipMemcpyHostToDevice));
  }
  if (h->p.smoother == MAMG_SMOOTHER_POLY) {
    const int64_t n = blk ? D.cWB.nnz : D.nloc;
    const double* src = blk ? D.cWB.val : D.winv;
    for (int k = 0; k < pm; ++k) {
      double* q = nullptr;
      if ((rc = ddalloc(h, &q, std::max<int64_t>(n, 1), err))) return rc;
      if (n) wscale(n, pw[k], src, q);
      HIPCHK(hipGetLastError());
      if (blk) {
        DCsr c = D.cWB;
        c.val = q;
        D.cWBk.push_back(c);
      } else {
        D.winvk.push_back(q);
      }
    }
  }
  if (l == 0 && !P.replicated) {   // longest run of A_loc rows without ghost columns
    int64_t best0 = 0, best1 = 0, run0 = 0;
    for (int64_t i = 0; i <= P.cA.n; ++i) {
      // rows are sorted by local column: the last entry tells
      const bool ghost = i == P.cA.n || (P.cA.ptr[i + 1] > P.cA.ptr[i] && P.cA.col[P.cA.ptr[i + 1] - 1] >= P.nloc);
      if (ghost) {
        if (i - run0 > best1 - best0) { best0 = run0; best1 = i; }
        run0 = i + 1;
      }
    }
    D.ib0 = best0;
    D.ib1 = best1;
  }
  return MAMG_OK;
}

}  // namespace

int dist_check(const mamg_params& p, std::string* err) {
  if (p.maxit != 1) {
    *err = "multi-GPU apply supports maxit 1 (one cycle per application, src/amg_parameters.py:71)";
    return MAMG_ERR_UNSUPPORTED;
  }
  if (p.cycle_type == MAMG_NL_AMLI_CYCLE) {
    *err = "multi-GPU apply supports the V and W cycles: the nonlinear AMLI cycle (K-cycle) is single-GPU";
    return MAMG_ERR_UNSUPPORTED;
  }
  if (int rc = dist_layout_check(p, err)) return rc;   // scalar (CSR) or nodal (BSR2) hierarchies (dist.cpp)
  return MAMG_OK;
}

int dist_upload(const Hierarchy& H, const CsrView& A0, const mamg_params& p, const Switches& sw, int rank,
                int nranks, const void* comm_id, int64_t rep_nodes, DistHandle** out, std::string* err,
                const GhostLists* ghosts, const GHier* G, const DevMat* A0d) {
  if (int rc = dist_check(p, err)) return rc;
  const bool gs = gs_smoother(p);
  const bool patches = patch_schwarz(p);
  const bool rings = rings_schwarz(p);
  if ((patches || rings) && !(G && A0d && ghosts)) {
    *err = std::string("multi-GPU ") + (patches ? "node patches need the rank operators and the 3-hop" :
           "seed rings need the rank operators and the (2 Schwarz_maxlvl + 1)-hop") +
           " ghost lists built from the GPU hierarchy (mamg_setup_dist with a GPU-setup profile)";
    return MAMG_ERR_UNSUPPORTED;
  }
  if (gs && !G) {
    *err = "multi-GPU multicolour GS needs the rank operators built from the GPU hierarchy (mamg_setup_dist "
           "with a GPU-setup profile)";
    return MAMG_ERR_UNSUPPORTED;
  }
  double pw[MAMG_POLY_MAX];
  const int pm = poly_weights(p, pw);
  DistPlan plan;
  const auto tp0 = std::chrono::steady_clock::now();
  const double kw = p.smoother == MAMG_SMOOTHER_POLY ? pw[pm - 1] : 1.0;
  bool fuse = p.post_fusion != 0 && !gs && !patches && !rings;   // GS / patches / rings post-smooth after x += P e (as on one GPU)
  if (G)                   // operators from the GPU hierarchy: fusion needs its A P on every level
    for (size_t l = 0; l + 1 < G->levels.size() && fuse; ++l)
      if (!G->levels[l].coarsest && G->levels[l].AP.n != G->levels[l].n) fuse = false;
  int rc = build_dist_plan(H, A0, rank, nranks, rep_nodes, fuse, &plan, err, sw.post_k != 0, kw, ghosts,
                           G != nullptr);
  if (rc) return rc;
  if (p.print_level >= 2)
    std::fprintf(stderr, "[mamg] rank %d/%d setup:   of which host plan    %.3f s\n", rank, nranks,
                 std::chrono::duration<double>(std::chrono::steady_clock::now() - tp0).count());
  std::unique_ptr<DistHandle> h(new DistHandle(sw));
  h->p = p;
  h->rank = rank;
  h->nranks = nranks;
  h->w = plan.dofs;
  h->device = p.device;
  adopt_prereserve(h.get(), h->device);
  HIPCHK(hipSetDevice(p.device));
  if (comm_id) {                         // RCCL communicator; NULL = virtual (tests)
    ncclUniqueId uid;
    std::memcpy(&uid, comm_id, sizeof(uid));
    NCCLCHK(ncclCommInitRank(&h->comm, nranks, uid, rank));
  }
  h->dry = !comm_id && sw.dist_test == "dry";
  HIPCHK(hipStreamCreateWithFlags(&h->side, hipStreamNonBlocking));
  HIPCHK(hipEventCreateWithFlags(&h->ev_in, hipEventDisableTiming));
  HIPCHK(hipEventCreateWithFlags(&h->ev_out, hipEventDisableTiming));
  const int nl = (int)plan.levels.size();
  h->L.resize(nl);
  for (int l = 0; l < nl; ++l) {
    DistLevel& P = plan.levels[l];
    DDLevel& D = h->L[l];
    D.nv = P.nv;
    D.nloc = P.nloc;
    D.ng = (int64_t)P.ghosts.size();
    D.replicated = P.replicated;
    D.coarsest = P.coarsest;
    D.send_off = P.send_off;
    D.ghost_off = P.ghost_off;
    if (h->w == 1) {   // scalar level: the plan's CSR operators as they are
      if ((rc = upload_scalar_level(h.get(), H.levels[l], P, l, pm, pw, err))) return rc;
    } else if (D.coarsest) {
      const HostLevel& hl = H.levels[l];
      const int64_t n = hl.n, nv = n / 2;
      std::vector<double> Ap(n * n);
      auto pos = [nv](int64_t i) { return 2 * (i % nv) + i / nv; };
      for (int64_t i = 0; i < n; ++i)
        for (int64_t j = 0; j < n; ++j) Ap[pos(i) * n + pos(j)] = hl.Ainv[i * n + j];
      if ((rc = ddalloc(h.get(), &D.Ainv, n * n, err))) return rc;
      HIPCHK(hipMemcpy(D.Ainv, Ap.data(), n * n * sizeof(double), hipMemcpyHostToDevice));
    } else if (G) {
      // multicolour GS: the level's global colouring (every rank computes the
      // same one, as the single-GPU build_gs), then each colour's halo lists
      TmpPool TC(h->sw);
      int8_t* gcol = nullptr;
      int ncol = 0;
      const bool rl0 = l == 0 && rings && !G->seeds.empty();   // level-0 seed rings + the rest's GS
      if ((gs || rl0) && !(l == 0 && patches)) {
        TBsr B;
        if ((rc = dev_csr_to_bsr(&TC, l == 0 ? *A0d : G->levels[l].A, D.nv, D.nv, &B, err))) return rc;
        if ((rc = gs_colour(&TC, B, l, &gcol, &ncol, err))) return rc;
        TC.release(B.ptr); TC.release(B.col); TC.release(B.val);
        if (rl0) {
          if ((rc = dist_rings(h.get(), *A0d, P, G->seeds, gcol, ncol, &D, &D.rcov, err))) return rc;
        } else if (!D.replicated && (rc = colour_halo_lists(h.get(), P, gcol, ncol, &D, err))) {
          return rc;
        }
      }
      if ((rc = dev_rank_ops(h.get(), *G, *A0d, plan, l, kw, gcol, ncol, err))) return rc;
      if (l == 0 && patches && !D.coarsest && (rc = dist_patches(h.get(), *A0d, P, &D, err))) return rc;
    } else {
      // longest run of rows without ghost columns (columns < nown): the
      // overlap windows, as ghost_free_run on the device path
      auto run_of = [](const HBsr& M, int64_t nown, int64_t* r0, int64_t* r1) {
        int64_t best0 = 0, best1 = 0, run0 = 0;
        for (int64_t I = 0; I <= M.nr; ++I) {
          bool ghost = I == M.nr;
          for (int64_t k = I < M.nr ? M.ptr[I] : 0; !ghost && k < M.ptr[I + 1]; ++k)
            ghost = M.col[k] >= nown;
          if (ghost) {
            if (I - run0 > best1 - best0) { best0 = run0; best1 = I; }
            run0 = I + 1;
          }
        }
        *r0 = best0;
        *r1 = best1;
      };
      if (!P.replicated) run_of(P.A, P.A.nr, &D.ib0, &D.ib1);
      if (l == 0 && !P.replicated && !plan.levels[1].replicated && P.K.nr > 0) {
        int64_t k0 = 0, k1 = 0;
        run_of(P.K, plan.levels[1].nloc, &k0, &k1);
        k0 = (k0 + K_ROWS_ALIGN - 1) / K_ROWS_ALIGN * K_ROWS_ALIGN;
        k1 = k1 == P.K.nr ? P.K.nr : k1 / K_ROWS_ALIGN * K_ROWS_ALIGN;
        if (k1 > k0) { D.kb0 = k0; D.kb1 = k1; }
      }
      if (l == 0) {
        if ((rc = upload_half_or_bsr(h.get(), P.A, &D.A, err))) return rc;
        if ((rc = build_band_sched_range(h.get(), &D.A, D.ib0, D.ib1, err))) return rc;
      } else if ((rc = upload_bsr(h.get(), P.A, &D.A, 0, err, true))) {
        return rc;
      }
      if (P.K.nr > 0) {
        if ((rc = upload_bsr(h.get(), P.K, &D.K, 0, err))) return rc;
        D.K.kvar = h->sw.k_variant;
      } else if (P.PA.nr > 0) {
        if ((rc = upload_bsr(h.get(), P.PA, &D.PA, 0, err))) return rc;
      } else {
        if ((rc = upload_bsr(h.get(), P.P, &D.P, 0, err))) return rc;
      }
      if ((rc = upload_bsr(h.get(), P.Rp, &D.R, 0, err))) return rc;
      if ((rc = ddalloc(h.get(), &D.W, D.nloc, err))) return rc;
      HIPCHK(hipMemcpy(D.W, P.W.data(), 4 * D.nloc * sizeof(double), hipMemcpyHostToDevice));
    }
    if (!D.coarsest && h->w == 2) {
      if (p.smoother == MAMG_SMOOTHER_POLY) {   // w_k W as on one GPU (poly_scaled)
        for (int k = 0; k < pm; ++k) {
          dv4* q = nullptr;
          if ((rc = ddalloc(h.get(), &q, D.nloc, err))) return rc;
          if (D.nloc)
            wscale(4 * D.nloc, pw[k], reinterpret_cast<const double*>(D.W),
                                                         reinterpret_cast<double*>(q));
          HIPCHK(hipGetLastError());
          D.Wk.push_back(q);
        }
      }
    }
    const int64_t full = D.nloc + D.ng;
    const int w = h->w;
    if ((rc = ddalloc(h.get(), &D.b, w * full, err))) return rc;
    if ((rc = ddalloc(h.get(), &D.x, w * full, err))) return rc;
    if ((rc = ddalloc(h.get(), &D.t, w * full, err))) return rc;
    if ((rc = ddalloc(h.get(), &D.t2, w * full, err))) return rc;
    if ((rc = ddalloc(h.get(), &D.r, w * full, err))) return rc;
    if (l == 0 && !D.coarsest && (rc = ddalloc(h.get(), &D.spx, w * full, err))) return rc;
    if ((D.patches || D.rings) && (rc = ddalloc(h.get(), &D.pb, w * full, err))) return rc;
    if (D.cWB.n > 0 && (rc = ddalloc(h.get(), &D.gb, full, err))) return rc;
    if (l > 0 && p.cycle_type == MAMG_W_CYCLE) {
      if ((rc = ddalloc(h.get(), &D.c, w * full, err))) return rc;
      if ((rc = ddalloc(h.get(), &D.e, w * full, err))) return rc;
    }
    if (l > 0 && p.coarse_scaling) {
      if ((rc = ddalloc(h.get(), &D.q, w * full, err))) return rc;
      if ((rc = ddalloc(h.get(), &D.part2, 2 * SCALE_BLOCKS, err))) return rc;
    }
    const int64_t ns = P.send_idx.size();
    // colour halos: a node in the lists of every colour that writes it (node
    // patches), so their totals may exceed the plain lists
    const int64_t tcs = D.cs_off.empty() ? 0 : D.cs_off.back(), tcg = D.cg_off.empty() ? 0 : D.cg_off.back();
    if (ns) {
      if ((rc = ddalloc(h.get(), &D.send_idx, ns, err))) return rc;
      HIPCHK(hipMemcpy(D.send_idx, P.send_idx.data(), ns * sizeof(int64_t), hipMemcpyHostToDevice));
    }
    if (std::max(ns, tcs) > 0 && (rc = ddalloc(h.get(), &D.sendbuf, w * std::max(ns, tcs), err))) return rc;
    const int64_t nrcv = std::max(std::max(ns, D.ng), tcg);
    if (nrcv > 0 && (rc = ddalloc(h.get(), &D.recvbuf, w * nrcv, err))) return rc;
  }
  h->nv0 = plan.levels[0].nv;
  h->o0 = plan.levels[0].o0;
  h->o1 = plan.levels[0].o1;
  // the rank-local operators are not re-homed: they are plain allocations
  // made after the setup already, and a second copy measured 204-208 vs
  // 209-214 applies/s (2 ranks, one GPU, profiles/r02_bench_2rank_rehome_ab.txt)
  std::vector<DOp> ops;
  dapply_ops(h.get(), nullptr, nullptr, &ops);
  for (const DOp& d : ops) h->apply_bytes += d.bytes;
  HIPCHK(null_sync());
  *out = h.release();
  return MAMG_OK;
}

}  // namespace mamg
