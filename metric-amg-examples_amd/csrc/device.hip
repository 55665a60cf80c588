// device.hip -- CDNA4 (gfx950) apply path of the metric-AMG preconditioner.
//
// Replaces the HAZmath multigrid cycle behind `BB * r` (cbc.block operator,
// one cycle per call: `maxit: 1` /root/reference/src/amg_parameters.py:71,
// called by ConjGrad /root/reference/src/bidomain_3d.py:149-150) and the
// cbc.block PCG loop itself (mamg_pcg_device).
//
// Two device layouts of the same hierarchy (chosen at upload):
//  * CSR (general): every level as CSR {int64 rowptr, int32 col, fp64 val},
//    vectors in the caller's dof order.  Kernel: csr_kernel<VL,EPI,TAG>.
//  * BSR2 (nodal hierarchies, num_functions == 2, block-aligned smoother):
//    every level as 2x2 block CSR, node-major {int64 bptr, int32 node col,
//    4 fp64 per block}; internal vectors node-interleaved (x[2I+f]) so one
//    16-byte load gathers a node's pair; the level-0 block-Jacobi smoother is
//    kept as one 2x2 block per node and fused into the SpMV epilogue
//    (x' = x + W_I (b_I - (A x)_I)).  The caller's r / z stay field-major
//    ([u1; u2], src/bidomain_3d.py:124,138): level-0 kernels read/write them
//    with a field stride.  Index bytes drop from 4 per value to 1, gathers
//    halve; measured 2.2x faster level-0 SpMV than CSR (bench/spmv_micro.hip).
//
// Kernels (all HBM-bound, ~0.17 flop/B): VL lanes per
// row (node), VL a power of two chosen from the mean row length; lanes stride
// the row's contiguous block window (coalesced 32-byte block loads), x
// gathered through L2/MALL, partial sums reduced with wavefront shuffles, and
// a fused epilogue.  One apply = a fixed schedule of launches captured into a
// hipGraph; each launch carries its algorithmic bytes (roofline from the
// hierarchy, not from counters).
#include "device_int.h"

#include <pthread.h>

namespace mamg {

// hipGraphInstantiate on a thread whose stack fits the graph.  The runtime
// walks a captured graph recursively at instantiation, one 64-byte frame per
// node of its longest dependency chain (a stream capture is one chain): the
// 8 virtual ranks' lockstep apply of the reference preset at nrefs=5 overflowed
// the 8 MiB main-thread stack after 130,903 frames and crashed the process
// (SIGSEGV on the guard page inside hipGraphInstantiate; diagnosis-build tracer,
// profiles/r06_graph_segv.txt).  Graphs of up to
// GRAPH_INSTANTIATE_INLINE nodes instantiate on the caller's thread (at most
// 1 MiB of its stack); larger ones on a helper thread with 256 B of stack per
// node (4x the measured frame) + 16 MiB, reserved, touched only as deep as the
// walk goes.
constexpr size_t GRAPH_INSTANTIATE_INLINE = 16384;

// Held across every stream capture of the library and every setup (capi.cpp
// TmpTrim): the HIP runtime invalidates a capture when another host thread
// issues legacy null-stream work meanwhile (the setups' synchronous copies),
// and refuses that work ("would make the legacy stream depend on a capturing
// blocking stream"), thread-local capture mode notwithstanding (two threads
// setting up and applying at once, tests/test_gpu_setup.py).  Setups of one
// process therefore run one at a time.
std::recursive_mutex& capture_mutex() {
  static std::recursive_mutex m;
  return m;
}
static hipError_t graph_instantiate(hipGraphExec_t* ex, hipGraph_t g) {
  size_t nodes = 0;
  hipError_t e = hipGraphGetNodes(g, nullptr, &nodes);
  if (e != hipSuccess) return e;
  if (nodes <= GRAPH_INSTANTIATE_INLINE) return hipGraphInstantiate(ex, g, nullptr, nullptr, 0);
  struct Job {
    hipGraphExec_t* ex;
    hipGraph_t g;
    int dev;
    hipError_t e;
  } job{ex, g, 0, hipSuccess};
  if ((e = hipGetDevice(&job.dev)) != hipSuccess) return e;
  pthread_attr_t a;
  if (pthread_attr_init(&a) != 0) return hipErrorOutOfMemory;
  const size_t stack = ((nodes * 256 + ((size_t)16 << 20)) + 4095) & ~(size_t)4095;
  pthread_t t;
  int rc = pthread_attr_setstacksize(&a, stack);
  if (rc == 0)
    rc = pthread_create(&t, &a, [](void* p) -> void* {
      Job* j = static_cast<Job*>(p);
      j->e = hipSetDevice(j->dev);
      if (j->e == hipSuccess) j->e = hipGraphInstantiate(j->ex, j->g, nullptr, nullptr, 0);
      return nullptr;
    }, &job);
  pthread_attr_destroy(&a);
  if (rc != 0) return hipErrorOutOfMemory;
  pthread_join(t, nullptr);
  return job.e;
}

int capture_graph(hipStream_t* cap, const std::function<int()>& body, const char* what, CapturedGraph* out,
                  std::string* err) {
  *out = CapturedGraph();
  std::lock_guard<std::recursive_mutex> capture_lock(capture_mutex());
  hipGraph_t g = nullptr;
  hipGraphExec_t ex = nullptr;
  int rc = MAMG_OK;
  hipError_t e = *cap ? hipSuccess : hipStreamCreateWithFlags(cap, hipStreamNonBlocking);
  if (e == hipSuccess) e = hipStreamBeginCapture(*cap, hipStreamCaptureModeThreadLocal);
  if (e == hipSuccess) {
    rc = body();
    e = hipStreamEndCapture(*cap, &g);   // also after a failed body: the stream must leave capture mode
  }
  const char* stage = "stream capture of the ";
  if (!rc && e == hipSuccess) {
    e = graph_instantiate(&ex, g);
    stage = "hipGraphInstantiate of the ";
  }
  if (rc || e != hipSuccess) {
    if (g) (void)hipGraphDestroy(g);
    (void)hipGetLastError();
    if (!rc) *err = std::string(stage) + what + ": " + hipGetErrorString(e);
    return rc ? rc : MAMG_ERR_HIP;
  }
  out->graph = g;
  out->exec = ex;
  return MAMG_OK;
}

namespace {

// ---------------------------------------------------------------------------
// CSR kernels (general layout)
// ---------------------------------------------------------------------------
template <int VL, int EPI, int TAG>
__global__ __launch_bounds__(256) void csr_kernel(
    int64_t r0, int64_t n, const int64_t* __restrict__ ptr, const int32_t* __restrict__ col,
    const double* __restrict__ val, const double* __restrict__ x,
    const double* y, const double* __restrict__ b, const double* __restrict__ w,
    double* out) {
  // rows [r0, n): r0 > 0 for the multi-GPU rank-local A's row ranges (interior
  // rows during the halo); a row's sum does not depend on where the launch starts
  const int lane = threadIdx.x & (VL - 1);
  const int64_t row = r0 + ((int64_t)blockIdx.x * 256 + threadIdx.x) / VL;
  double s0 = 0.0, s1 = 0.0;
  if (row < n) {
    const int64_t p0 = ptr[row], p1 = ptr[row + 1];
    int64_t k = p0 + lane;
    for (; k + VL < p1; k += 2 * VL) {
      const int32_t c0 = col[k], c1 = col[k + VL];
      const double v0 = val[k], v1 = val[k + VL];
      s0 += v0 * x[c0];
      s1 += v1 * x[c1];
    }
    if (k < p1) s0 += val[k] * x[col[k]];
  }
  double s = s0 + s1;
#pragma unroll
  for (int off = VL / 2; off > 0; off >>= 1) s += __shfl_xor(s, off, VL);
  if (row < n && lane == 0) {
    if (EPI == EPI_Y) out[row] = s;
    else if (EPI == EPI_YADD) out[row] = y[row] + s;
    else if (EPI == EPI_RESID) out[row] = b[row] - s;
    else out[row] = y[row] + w[row] * (b[row] - s);
  }
}

// ---------------------------------------------------------------------------
// Point-wise multicolour Gauss-Seidel on the CSR layout (SMOOTHER_GS_POINT /
// SGS_POINT): the smoother of the reference's plain AMG (AMGhaz,
// src/utils.py:40, SGS of src/amg_parameters.py:72) in a parallel order.  The
// rows of the scalar A_l are coloured on its off-diagonal pattern
// (jp_round_kernel, as the node-block GS); G = A_l with its rows permuted
// colour by colour (build_gs_csr), so one colour is one contiguous row range
// [r0, r1):   x_I <- x_I + (b_I - sum_j a_Ij x_j) / a_II,   I = perm[i],
// in place (no row of a colour reads an x another row of that colour writes).
// dinv[i] = 1 / a_II in permuted order.  csr_gs_row is csr_kernel's lane-group
// row loop; every lane of the group returns the row's sum.
// ---------------------------------------------------------------------------
template <int VL>
__device__ __forceinline__ double csr_gs_row(bool on, int64_t i, int lane, const int64_t* __restrict__ ptr,
                                             const int32_t* __restrict__ col, const double* __restrict__ val,
                                             const double* x) {
  double s0 = 0.0, s1 = 0.0;
  if (on) {
    const int64_t p0 = ptr[i], p1 = ptr[i + 1];
    int64_t k = p0 + lane;
    for (; k + VL < p1; k += 2 * VL) {
      const int32_t c0 = col[k], c1 = col[k + VL];
      const double v0 = val[k], v1 = val[k + VL];
      s0 += v0 * x[c0];
      s1 += v1 * x[c1];
    }
    if (k < p1) s0 += val[k] * x[col[k]];
  }
  double s = s0 + s1;
#pragma unroll
  for (int off = VL / 2; off > 0; off >>= 1) s += __shfl_xor(s, off, VL);
  return s;
}

// one colour: the permuted rows [r0, r1), one launch
template <int VL>
__global__ __launch_bounds__(256) void csr_gs_kernel(
    int64_t r0, int64_t r1, const int32_t* __restrict__ perm, const int64_t* __restrict__ ptr,
    const int32_t* __restrict__ col, const double* __restrict__ val, const double* __restrict__ dinv,
    double* x, const double* __restrict__ b) {
  const int lane = threadIdx.x & (VL - 1);
  const int64_t i = r0 + ((int64_t)blockIdx.x * 256 + threadIdx.x) / VL;
  const bool on = i < r1;
  const double s = csr_gs_row<VL>(on, i, lane, ptr, col, val, x);
  if (on && lane == 0) {
    const int64_t I = perm[i];
    x[I] = x[I] + dinv[i] * (b[I] - s);
  }
}

// A whole smoothing call of a small level (n <= CSR_GS_SMALL_ROWS rows) in
// one launch of one workgroup: nu x (sweep d0, then sweep d1), a sweep being
// every colour in turn (d > 0 ascending, d < 0 descending, 0: no sweep).  x
// lives in LDS (xs[n]; from zero if `zero`, else read from global memory), b
// and the permuted operator are read from global memory, a workgroup barrier
// separates the colours, x is written back coalesced at the end.  Every loop
// is bounded by nu, the colour count and the row count.
constexpr int CSR_GS_SMALL_THREADS = 1024;
template <int VL>
__global__ __launch_bounds__(CSR_GS_SMALL_THREADS) void csr_gs_small_kernel(
    int64_t n, int ncol, const int64_t* __restrict__ cs, const int32_t* __restrict__ perm,
    const int64_t* __restrict__ ptr, const int32_t* __restrict__ col, const double* __restrict__ val,
    const double* __restrict__ dinv, double* x, const double* __restrict__ b, int zero, int nu, int d0, int d1) {
  extern __shared__ double csr_gs_xs[];
  double* xs = csr_gs_xs;
  const int tid = threadIdx.x, lane = tid & (VL - 1);
  constexpr int RPP = CSR_GS_SMALL_THREADS / VL;   // rows per pass
  for (int64_t i = tid; i < n; i += CSR_GS_SMALL_THREADS) xs[i] = zero ? 0.0 : x[i];
  __syncthreads();
  for (int rep = 0; rep < nu; ++rep)
    for (int leg = 0; leg < 2; ++leg) {
      const int d = leg ? d1 : d0;
      if (d == 0) continue;
      for (int k = 0; k < ncol; ++k) {
        const int c = d > 0 ? k : ncol - 1 - k;
        const int64_t r0 = cs[c], r1 = cs[c + 1];
        for (int64_t base = r0; base < r1; base += RPP) {
          const int64_t i = base + tid / VL;
          const bool on = i < r1;
          const double s = csr_gs_row<VL>(on, i, lane, ptr, col, val, xs);
          if (on && lane == 0) {
            const int64_t I = perm[i];
            xs[I] = xs[I] + dinv[i] * (b[I] - s);
          }
        }
        __syncthreads();
      }
    }
  for (int64_t i = tid; i < n; i += CSR_GS_SMALL_THREADS) x[i] = xs[i];
}

// permuted row i = row perm[i] of A: its columns and values copied in order,
// dinv[i] = 1 / a_II; *bad set where the diagonal entry is missing or <= 0
// (or not a number)
__global__ __launch_bounds__(256) void csr_gs_fill_kernel(int64_t n, const int32_t* __restrict__ perm,
                                                          const int64_t* __restrict__ ptr,
                                                          const int32_t* __restrict__ col,
                                                          const double* __restrict__ val,
                                                          const int64_t* __restrict__ gptr, int32_t* __restrict__ gcol,
                                                          double* __restrict__ gval, double* __restrict__ dinv,
                                                          int* bad) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int64_t I = perm[i];
  const int64_t a = ptr[I], e = ptr[I + 1], g = gptr[i];
  double d = 0.0;
  for (int64_t k = a; k < e; ++k) {
    const int32_t c = col[k];
    const double v = val[k];
    gcol[g + (k - a)] = c;
    gval[g + (k - a)] = v;
    if (c == I) d = v;
  }
  if (!(d > 0.0)) { *bad = 1; d = 1.0; }
  dinv[i] = 1.0 / d;
}

// ---------------------------------------------------------------------------
// BSR2 kernels (nodal layout).  Vector element (node I, field f):
//   node-major:  v[2I + f]          (stride argument 0)
//   field-major: v[f * stride + I]  (the caller's [u1; u2] order)
// ---------------------------------------------------------------------------
__device__ __forceinline__ double vget(const double* v, int64_t stride, int64_t I, int f) {
  return stride ? v[f * stride + I] : v[2 * I + f];
}
__device__ __forceinline__ void vset(double* v, int64_t stride, int64_t I, int f, double a) {
  if (stride) v[f * stride + I] = a; else v[2 * I + f] = a;
}

// XCD-aware row order: the dispatcher hands workgroup b to XCD b % 8, so
// consecutive workgroups (neighbouring rows, which gather the same x entries)
// would land in 8 different L2s.  Renumber so that every XCD walks one
// contiguous range of rows (bijective for any grid size).
// W_I b_I with the contraction spelled out (fma of the first product onto
// the second), so that bd2_kernel and the restriction's EPI_YBD epilogue,
// compiled in different contexts, produce the same bits
__device__ __forceinline__ double2 wmul(const dv4& w, double b0, double b1) {
  return double2{__builtin_fma(w.x, b0, w.y * b1), __builtin_fma(w.z, b0, w.w * b1)};
}

__device__ __forceinline__ int64_t row_block_of(uint32_t b, uint32_t G, int remap) {
  if (!remap) return b;
  const uint32_t q = G >> 3, r = G & 7, x = b & 7;
  return (int64_t)(x * q + (x < r ? x : r) + (b >> 3));
}
__device__ __forceinline__ int64_t row_block(int remap) { return row_block_of(blockIdx.x, gridDim.x, remap); }

// block k of a BSR2 value array: 4 doubles (0,0) (0,1) (1,0) (1,1) per block,
// or in the symmetric-block format (SYM) two aligned streams: the diagonal
// pairs {(0,0), (1,1)} (16 B per block) then the off-diagonals (0,1) = (1,0)
// (8 B per block) starting at v + 2 nb
// NT: non-temporal (streaming) loads, so the matrix stream does not evict
// the gathered vector from L2
template <bool NT, class T>
__device__ __forceinline__ T ldg(const T* p) {
  if (NT) return __builtin_nontemporal_load(p);
  return *p;
}

// VT: the stored value type.  double, or float for an operator narrowed by
// dev_set_cycle_storage: the same element layout at
// half the width (a general block is one 16-byte float4, a SYM block a float2
// diagonal pair plus one float, the split streams keep their proportions),
// converted to fp64 on load; every product and sum stays fp64.
typedef float fv4 __attribute__((ext_vector_type(4)));
typedef float fv2 __attribute__((ext_vector_type(2)));
template <class VT> struct vvec { typedef double s; typedef dv2 v2; typedef dv4 v4; };
template <> struct vvec<float> { typedef float s; typedef fv2 v2; typedef fv4 v4; };
template <class VT> __device__ __forceinline__ dv2 widen2(const typename vvec<VT>::v2& a) {
  if constexpr (sizeof(VT) == 8) return a;
  else return dv2{(double)a.x, (double)a.y};
}
template <class VT> __device__ __forceinline__ dv4 widen4(const typename vvec<VT>::v4& a) {
  if constexpr (sizeof(VT) == 8) return a;
  else return dv4{(double)a.x, (double)a.y, (double)a.z, (double)a.w};
}

template <bool SYM, bool NT = false, class VT = double>
__device__ __forceinline__ dv4 blk(const VT* __restrict__ v, const typename vvec<VT>::s* __restrict__ off,
                                   int64_t k) {
  typedef typename vvec<VT>::v2 V2;
  typedef typename vvec<VT>::v4 V4;
  if (SYM) {
    const dv2 d = widen2<VT>(ldg<NT>(reinterpret_cast<const V2*>(v) + k));
    const double b = (double)ldg<NT>(off + k);
    return dv4{d.x, b, b, d.y};
  }
  return widen4<VT>(ldg<NT>(reinterpret_cast<const V4*>(v) + k));
}

// x(node c) as a pair: node-interleaved (one 16-byte load) or field-major
template <bool XFM>
__device__ __forceinline__ double2 xget(const double* x, int64_t xs, int32_t c) {
  if (XFM) return double2{x[c], x[xs + c]};
  return reinterpret_cast<const double2*>(x)[c];
}

template <int VL, int EPI, bool XFM, bool SYM, int TAG, bool NT = false, class VT = double>
__global__ __launch_bounds__(256) void bsr2_kernel(
    int64_t nr, const int64_t* __restrict__ bptr, const int32_t* __restrict__ bcol,
    const VT* __restrict__ bval, const double* __restrict__ x, int64_t xs,
    const double* y, const double* __restrict__ b, int64_t bs,
    const dv4* __restrict__ W, double* out, int64_t os, int remap, const int32_t* __restrict__ sched,
    int64_t rb0 = 0) {
  const int lane = threadIdx.x & (VL - 1);
  // rb0: first workgroup of a row-range launch (rows from 256 rb0 / VL)
  const int64_t node = ((sched ? (int64_t)sched[blockIdx.x] : rb0 + row_block(remap)) * 256 + threadIdx.x) / VL;
  const VT* offd = SYM ? bval + 2 * bptr[nr] : nullptr;
  double s0 = 0.0, s1 = 0.0, t0 = 0.0, t1 = 0.0;
  // EPI_YBD's W block loaded with the row, not after the reduction (a
  // dependent load at the end of every row measured +36 us on level 0's R)
  const dv4 wy = (EPI == EPI_YBD && node < nr && lane == 0) ? W[node] : dv4{0.0, 0.0, 0.0, 0.0};
  if (node < nr) {
    // chunks of 2 VL blocks, branch-free: every lane issues both loads of a
    // chunk at once (index clamped into the row, contribution selected away),
    // so a row costs one load -> gather chain per chunk instead of a loop
    // chain followed by a divergent tail chain
    const int64_t p0 = bptr[node], p1 = bptr[node + 1];
    for (int64_t base = p0; base < p1; base += 2 * VL) {
      const int64_t ka = base + lane, kb = ka + VL;
      const bool ha = ka < p1, hb = kb < p1;
      const int64_t la = ha ? ka : p1 - 1, lb = hb ? kb : p1 - 1;
      const int32_t c0 = ldg<NT>(bcol + la), c1 = ldg<NT>(bcol + lb);
      const dv4 v0 = blk<SYM, NT, VT>(bval, offd, la), v1 = blk<SYM, NT, VT>(bval, offd, lb);
      const double2 a = xget<XFM>(x, xs, c0), e = xget<XFM>(x, xs, c1);
      s0 += ha ? v0.x * a.x + v0.y * a.y : 0.0;
      s1 += ha ? v0.z * a.x + v0.w * a.y : 0.0;
      t0 += hb ? v1.x * e.x + v1.y * e.y : 0.0;
      t1 += hb ? v1.z * e.x + v1.w * e.y : 0.0;
    }
  }
  s0 += t0;
  s1 += t1;
#pragma unroll
  for (int off = VL / 2; off > 0; off >>= 1) {
    s0 += __shfl_xor(s0, off, VL);
    s1 += __shfl_xor(s1, off, VL);
  }
  if (node < nr && lane == 0) {
    double o0, o1;
    if (EPI == EPI_Y) {
      o0 = s0; o1 = s1;
    } else if (EPI == EPI_YBD) {
      o0 = s0; o1 = s1;
      const double2 wb = wmul(wy, o0, o1);
      double* x1 = const_cast<double*>(y);
      x1[2 * node] = wb.x;
      x1[2 * node + 1] = wb.y;
    } else if (EPI == EPI_YADD) {
      o0 = y[2 * node] + s0; o1 = y[2 * node + 1] + s1;
    } else if (EPI == EPI_RESID) {
      o0 = vget(b, bs, node, 0) - s0; o1 = vget(b, bs, node, 1) - s1;
    } else if (EPI == EPI_KPOST) {
      const double r0 = vget(b, bs, node, 0), r1 = vget(b, bs, node, 1);
      const dv4 w = W[node];
      o0 = y[2 * node] + (w.x * r0 + w.y * r1) + s0;
      o1 = y[2 * node + 1] + (w.z * r0 + w.w * r1) + s1;
    } else {  // EPI_BJAC
      const double r0 = vget(b, bs, node, 0) - s0, r1 = vget(b, bs, node, 1) - s1;
      const dv4 w = W[node];
      o0 = y[2 * node] + (w.x * r0 + w.y * r1);
      o1 = y[2 * node + 1] + (w.z * r0 + w.w * r1);
    }
    vset(out, os, node, 0, o0);
    vset(out, os, node, 1, o1);
  }
}

// prolongation fused into the first post-smoothing sweep (post_fusion):
//   out(I) = x1(I) + (P e)(I) + W_I (r1(I) - (AP e)(I))
// which equals x2 + W (b - A x2) for x2 = x1 + P e, since r1 = b - A x1 and
// A x2 = A x1 + (AP) e.  Row I of the merged matrix holds P's blocks in
// [mptr[2I], mptr[2I+1]) then AP's in [mptr[2I+1], mptr[2I+2]): one contiguous
// window per node, both sums gathered from the same coarse vector e.
// The row's epilogue operands (x1, r1, W) are loaded by lane 0 before the
// block loop, so their latency overlaps the loop instead of following it.
template <int VL, bool NT, int TAG>
__global__ __launch_bounds__(256) void bsr2_post_kernel(
    int64_t nr, const int64_t* __restrict__ mptr, const int32_t* __restrict__ bcol,
    const double* __restrict__ bval, const double* __restrict__ e, const double* __restrict__ x1,
    const double* __restrict__ r1, const dv4* __restrict__ W, double* out, int64_t os, int remap) {
  const int lane = threadIdx.x & (VL - 1);
  const int64_t node = (row_block(remap) * 256 + threadIdx.x) / VL;
  const double2* e2 = reinterpret_cast<const double2*>(e);
  double p0 = 0.0, p1 = 0.0, q0 = 0.0, q1 = 0.0;
  dv4 w = {0.0, 0.0, 0.0, 0.0};
  double2 xx = {0.0, 0.0}, rr = {0.0, 0.0};
  if (node < nr && lane == 0) {
    w = W[node];
    xx = reinterpret_cast<const double2*>(x1)[node];
    rr = reinterpret_cast<const double2*>(r1)[node];
  }
  if (node < nr) {   // branch-free chunks of 2 VL blocks (see bsr2_kernel)
    const int64_t k0 = mptr[2 * node], km = mptr[2 * node + 1], k1 = mptr[2 * node + 2];
    for (int64_t base = k0; base < k1; base += 2 * VL) {
      const int64_t ka = base + lane, kb = ka + VL;
      const bool ha = ka < k1, hb = kb < k1;
      const int64_t la = ha ? ka : k1 - 1, lb = hb ? kb : k1 - 1;
      const int32_t c0 = ldg<NT>(bcol + la), c1 = ldg<NT>(bcol + lb);
      const dv4 v0 = blk<false, NT>(bval, nullptr, la), v1 = blk<false, NT>(bval, nullptr, lb);
      const double2 a = e2[c0], b = e2[c1];
      const double u0 = ha ? v0.x * a.x + v0.y * a.y : 0.0, u1 = ha ? v0.z * a.x + v0.w * a.y : 0.0;
      const double w0 = hb ? v1.x * b.x + v1.y * b.y : 0.0, w1 = hb ? v1.z * b.x + v1.w * b.y : 0.0;
      const bool pa = ka < km, pb = kb < km;
      p0 += pa ? u0 : 0.0; p1 += pa ? u1 : 0.0; q0 += pa ? 0.0 : u0; q1 += pa ? 0.0 : u1;
      p0 += pb ? w0 : 0.0; p1 += pb ? w1 : 0.0; q0 += pb ? 0.0 : w0; q1 += pb ? 0.0 : w1;
    }
  }
#pragma unroll
  for (int off = VL / 2; off > 0; off >>= 1) {
    p0 += __shfl_xor(p0, off, VL);
    p1 += __shfl_xor(p1, off, VL);
    q0 += __shfl_xor(q0, off, VL);
    q1 += __shfl_xor(q1, off, VL);
  }
  if (node < nr && lane == 0) {
    const double d0 = rr.x - q0, d1 = rr.y - q1;
    vset(out, os, node, 0, xx.x + p0 + (w.x * d0 + w.y * d1));
    vset(out, os, node, 1, xx.y + p1 + (w.z * d0 + w.w * d1));
  }
}

// ---------------------------------------------------------------------------
// Sliced-ELL variant of BSR2 (SELL-64) for the large short-row level-0
// operators (A_0: ~15 blocks per node, [P | AP]: ~13).  One lane per node;
// slice s = nodes [64 s, 64 s + 64) = one wavefront; block j of the slice's
// lane l sits at soff[s] + 64 j + l, so every load of the row loop is one
// fully coalesced 64-lane access (2 KB of blocks, 256 B of columns) with no
// cross-lane reduction.  meta[I] = row length | (P-part length << 16) (the
// split is used by the fused post kernel only).  Each lane loops only to its
// own length; padding is storage, never loaded.  Sums run in block order.
// ---------------------------------------------------------------------------
constexpr int SELL_C = 64;
constexpr int SELL_U = 4;     // blocks in flight per lane

// SPL: general blocks stored as two 16-byte streams per slot, the (0,0)(0,1)
// pairs at bval[2k] and the (1,0)(1,1) pairs at bval[2 nbs + 2k]: each load
// instruction reads 1 KB contiguous instead of 16 B of every 32 B over 2 KB
template <class VT>
__device__ __forceinline__ dv4 blk_split(const VT* __restrict__ v, int64_t nbs, int64_t k) {
  typedef typename vvec<VT>::v2 V2;
  const dv2 a = widen2<VT>(reinterpret_cast<const V2*>(v)[k]);
  const dv2 b = widen2<VT>(reinterpret_cast<const V2*>(v + 2 * nbs)[k]);
  return dv4{a.x, a.y, b.x, b.y};
}
// split inside each 64-slot SELL slot row: the row's 64 (0,0)(0,1) pairs
// (1 KB) then its 64 (1,0)(1,1) pairs, so a 16-byte-per-lane load of
// consecutive slots reads one contiguous piece and the slot row stays 2 KB
template <class VT>
__device__ __forceinline__ dv4 blk_split_local(const VT* __restrict__ v, int64_t k) {
  typedef typename vvec<VT>::v2 V2;
  const int64_t r = k & ~(int64_t)63, i = k & 63;
  const dv2 a = widen2<VT>(reinterpret_cast<const V2*>(v + 4 * r)[i]);
  const dv2 b = widen2<VT>(reinterpret_cast<const V2*>(v + 4 * r + 128)[i]);
  return dv4{a.x, a.y, b.x, b.y};
}
template <int SPL, class VT>
__device__ __forceinline__ dv4 blk_any(const VT* __restrict__ v, int64_t nbs, int64_t k) {
  typedef typename vvec<VT>::v4 V4;
  if (SPL == 1) return blk_split<VT>(v, nbs, k);
  if (SPL == 2) return blk_split_local<VT>(v, k);
  return widen4<VT>(reinterpret_cast<const V4*>(v)[k]);
}

template <int EPI, bool XFM, bool SYM, int U, bool SPL, int TAG, class VT = double>
__global__ __launch_bounds__(256) void sell2_kernel(
    int64_t nr, const int64_t* __restrict__ soff, const int32_t* __restrict__ meta,
    const int32_t* __restrict__ bcol, const VT* __restrict__ bval, int64_t nbs,
    const double* __restrict__ x, int64_t xs, const double* y, const double* __restrict__ b,
    int64_t bs, const dv4* __restrict__ W, double* out, int64_t os, int remap,
    const int32_t* __restrict__ sched, int lsort) {
  const int64_t slot = (sched ? (int64_t)sched[blockIdx.x] : row_block(remap)) * 256 + threadIdx.x;
  if (slot >= nr) return;
  const VT* offd = SYM ? bval + 2 * nbs : nullptr;
  const int m = meta[slot];
  const int len = m & 0xffff;
  int64_t k = soff[slot / SELL_C] + (slot & (SELL_C - 1));
  // the row this slot holds (DBsr::lsort: rows sorted by length in the slice)
  const int64_t node = lsort ? (slot & ~(int64_t)(SELL_C - 1)) | ((m >> 16) & (SELL_C - 1)) : slot;
  double s0 = 0.0, s1 = 0.0;
  // chunks of U blocks, branch-free (slot clamped into the row, contribution
  // selected away): one load -> gather chain per chunk
  for (int j = 0; j < len; j += U) {
    int32_t c[U];
    dv4 v[U];
    double2 a[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t kk = k + (int64_t)SELL_C * (j + u < len ? j + u : len - 1);
      c[u] = bcol[kk];
      v[u] = SPL ? blk_split<VT>(bval, nbs, kk) : blk<SYM, false, VT>(bval, offd, kk);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) a[u] = xget<XFM>(x, xs, c[u]);
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const bool ok = j + u < len;
      s0 += ok ? v[u].x * a[u].x + v[u].y * a[u].y : 0.0;
      s1 += ok ? v[u].z * a[u].x + v[u].w * a[u].y : 0.0;
    }
  }
  // epilogue operands after the loop (measured: loading them first is slower)
  double2 bb = {0.0, 0.0}, yy = {0.0, 0.0};
  dv4 w = {0.0, 0.0, 0.0, 0.0};
  if (EPI == EPI_RESID || EPI == EPI_BJAC || EPI == EPI_KPOST)
    bb = double2{vget(b, bs, node, 0), vget(b, bs, node, 1)};
  if (EPI == EPI_YADD || EPI == EPI_BJAC || EPI == EPI_KPOST) yy = reinterpret_cast<const double2*>(y)[node];
  if (EPI == EPI_BJAC || EPI == EPI_KPOST) w = W[node];
  double o0, o1;
  if (EPI == EPI_Y) {
    o0 = s0; o1 = s1;
  } else if (EPI == EPI_YADD) {
    o0 = yy.x + s0; o1 = yy.y + s1;
  } else if (EPI == EPI_RESID) {
    o0 = bb.x - s0; o1 = bb.y - s1;
  } else if (EPI == EPI_KPOST) {
    o0 = yy.x + (w.x * bb.x + w.y * bb.y) + s0;
    o1 = yy.y + (w.z * bb.x + w.w * bb.y) + s1;
  } else {  // EPI_BJAC
    const double r0 = bb.x - s0, r1 = bb.y - s1;
    o0 = yy.x + (w.x * r0 + w.y * r1);
    o1 = yy.y + (w.z * r0 + w.w * r1);
  }
  vset(out, os, node, 0, o0);
  vset(out, os, node, 1, o1);
}

// SELL-64 operator with LPR lanes per node row (multi-lane SELL).  A wavefront
// takes 64 / LPR rows of a 64-row slice; part q < LPR - 1 of a row takes its
// blocks [q U, (q + 1) U), the last part the rest in chunks of U, so a row of
// up to LPR U blocks is one load -> gather round trip per lane instead of a
// chain of chunks on one lane.  For a fixed chunk slot the lanes of one part
// read 64 / LPR consecutive slots.  The parts' sums meet by a __shfl_xor
// butterfly (addition commutes: every lane of a row ends with the same bits),
// then part f < 2 writes field f; its epilogue operands are loaded before
// the block loop.  Used for the level-0 fused post operator
// z = x1 + W r1 + K e (EPI_KPOST, LPR 2, U 5: K 1.69 -> 1.54 ms on one
// upload) and the SELL-stored coarse operators.
template <int LPR, int U, int EPI, bool XFM, bool SYM, int SPL, int TAG, int PROBE = 0, bool C16 = false,
          class VT = double>
__global__ __launch_bounds__(256) void msell_kernel(
    int64_t nr, const int64_t* __restrict__ soff, const int32_t* __restrict__ meta,
    const int32_t* __restrict__ bcol, const VT* __restrict__ bval, int64_t nbs,
    const double* __restrict__ x, int64_t xs, const double* y, const double* __restrict__ b, int64_t bs,
    const dv4* __restrict__ W, double* out, int64_t os, int remap, int lsort, int64_t rb0,
    const uint16_t* __restrict__ c16, const int32_t* __restrict__ cbase) {
  constexpr int RW = 64 / LPR;                          // rows per wavefront
  const int lane = threadIdx.x & 63, q = lane / RW;
  // rb0: first workgroup of a row-range launch (rows [256 rb0 / LPR, ...))
  const int64_t slot = (rb0 + row_block(remap)) * (4 * RW) + (threadIdx.x >> 6) * RW + (lane & (RW - 1));
  const bool live = slot < nr;
  const int64_t ns = live ? slot : nr - 1;            // dead lanes mirror the last slot, write nothing
  const int m = meta[ns];
  const int len = m & 0xffff;
  const int64_t k = soff[ns / SELL_C] + (ns & (SELL_C - 1));
  // the row this slot holds (DBsr::lsort: rows sorted by length in the slice)
  const int64_t node = lsort ? (ns & ~(int64_t)(SELL_C - 1)) | ((m >> 16) & (SELL_C - 1)) : ns;
  const int64_t nd = node;
  const VT* offd = SYM ? bval + 2 * nbs : nullptr;
  const int f = q & 1;
  const bool wr = q < 2;
  constexpr bool NB = EPI == EPI_RESID || EPI == EPI_BJAC || EPI == EPI_KPOST;
  constexpr bool NY = EPI == EPI_YADD || EPI == EPI_BJAC || EPI == EPI_KPOST;
  constexpr bool NW = EPI == EPI_BJAC || EPI == EPI_KPOST;
  const double yf = NY && wr ? y[2 * nd + f] : 0.0;
  const dv2 wf = NW && wr ? reinterpret_cast<const dv2*>(W + nd)[f] : dv2{0.0, 0.0};
  const double2 bb = NB && wr ? double2{vget(b, bs, nd, 0), vget(b, bs, nd, 1)} : double2{0.0, 0.0};
  double s0 = 0.0, s1 = 0.0;
  const int j0 = q * U, j1 = q == LPR - 1 ? len : (len < j0 + U ? len : j0 + U);
  const int32_t cb0 = C16 ? cbase[ns / SELL_C] : 0;
  for (int j = j0; j < j1; j += U) {
    int32_t c[U];
    dv4 v[U];
    double2 a[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t kk = k + (int64_t)SELL_C * (j + u < j1 ? j + u : j1 - 1);
      if constexpr (C16) c[u] = cb0 + (int32_t)c16[kk];
      else c[u] = PROBE == 2 ? __builtin_nontemporal_load(bcol + kk) : bcol[kk];
      v[u] = SPL ? blk_any<SPL, VT>(bval, nbs, kk) : blk<SYM, (PROBE >= 2), VT>(bval, offd, kk);
    }
#pragma unroll
    for (int u = 0; u < U; ++u)   // PROBE 1 (A/B only, wrong results): no gather, the column as the value
      a[u] = PROBE == 1 ? double2{(double)c[u], 1.0} : xget<XFM>(x, xs, c[u]);
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const bool ok = j + u < j1;
      s0 += ok ? v[u].x * a[u].x + v[u].y * a[u].y : 0.0;
      s1 += ok ? v[u].z * a[u].x + v[u].w * a[u].y : 0.0;
    }
  }
#pragma unroll
  for (int off = RW; off < 64; off <<= 1) {
    s0 += __shfl_xor(s0, off);
    s1 += __shfl_xor(s1, off);
  }
  if (!live || !wr) return;
  const double sf = f ? s1 : s0;
  double o;
  if (EPI == EPI_Y) {
    o = sf;
  } else if (EPI == EPI_YADD) {
    o = yf + sf;
  } else if (EPI == EPI_RESID) {
    o = (f ? bb.y : bb.x) - sf;
  } else if (EPI == EPI_KPOST) {
    o = yf + (wf.x * bb.x + wf.y * bb.y) + sf;
  } else {  // EPI_BJAC
    const double r0 = bb.x - s0, r1 = bb.y - s1;
    o = yf + (wf.x * r0 + wf.y * r1);
  }
  vset(out, os, node, f, o);
}

// ---------------------------------------------------------------------------
// Half-symmetric ELL-64 for a symmetric A0 (A_JI = A_IJ^T bitwise and every
// block symmetric, so A_JI = A_IJ): only the upper part J >= I is streamed
// (28 B per block with its column); a lower entry J < I is a 4-byte slot
// pointer to its mirror (J, I) in the upper part, whose row J the sweep
// streamed a few MB earlier, so the re-read is served by L2 / the 256 MB
// MALL instead of HBM.  The ELL slot p of upper block j of row J is
// (J / 64) 64 hwu + 64 j + J % 64, so J = 64 (p / (64 hwu)) + p % 64 needs no
// column.  For a translation-invariant stencil the 64 lanes' mirror slots
// are 64 consecutive rows of one slot: the gathers are coalesced too.
// Sums run lower part then upper part, each in column order: the full row's
// block order, so the result is bitwise that of sell2_kernel.
// ---------------------------------------------------------------------------
// streams of hsell2_kernel touched once: row meta, lower slot pointers and
// upper columns (level 1), and the b loads / output stores (level 2) are
// non-temporal, so that they do not displace from L2 the upper values the
// mirrors re-read.  Round 4 A/B at nrefs=6 (profiles/r04_hsell_nt.txt):
// residual L2-miss bytes 6.30 -> 6.03 (1) -> 5.87 GB (2) per launch,
// 1.077 -> 1.070 ms.  Build switch (0 = plain loads), default 2.
#ifndef MAMG_HSELL_NT
#define MAMG_HSELL_NT 2
#endif
template <class T>
__device__ __forceinline__ T ld_once(const T* p) {
  if constexpr (MAMG_HSELL_NT != 0) return __builtin_nontemporal_load(p);
  else return *p;
}

template <int EPI, bool XFM, int U, bool GH, int TAG, class VT = double>
__global__ __launch_bounds__(256) void hsell2_kernel(
    int64_t row0, int64_t nr, const int32_t* __restrict__ meta, const int32_t* __restrict__ ucol,
    const VT* __restrict__ uval, int64_t nbs, int hwu, const int32_t* __restrict__ lptr, int hwl,
    const int64_t* __restrict__ gsoff, const int32_t* __restrict__ gcol, const VT* __restrict__ gval,
    int64_t ngs, const double* __restrict__ x, int64_t xs, const double* y, const double* __restrict__ b,
    int64_t bs, const dv4* __restrict__ W, double* out, int64_t os, int remap,
    const int32_t* __restrict__ sched) {
  const int64_t blk0 = sched ? (int64_t)sched[blockIdx.x] : row_block(remap);
  const int64_t node = row0 + blk0 * 256 + threadIdx.x;   // rows [row0, nr)
  if (node >= nr) return;
  const VT* offd = uval + 2 * nbs;
  const int m = ld_once(meta + node);
  const int ulen = m & 0xff, llen = (m >> 8) & 0xff;
  const uint32_t urow = 64u * (uint32_t)hwu;
  double s0 = 0.0, s1 = 0.0;
  {
    const int64_t k = (node >> 6) * (int64_t)(64 * hwl) + (node & 63);
    for (int j = 0; j < llen; j += U) {
      uint32_t p[U];
      dv4 v[U];
      double2 a[U];
#pragma unroll
      for (int u = 0; u < U; ++u) p[u] = (uint32_t)ld_once(lptr + k + (int64_t)SELL_C * (j + u < llen ? j + u : llen - 1));
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int32_t c = (int32_t)((p[u] / urow) * 64u + (p[u] & 63u));
        v[u] = blk<true, false, VT>(uval, offd, p[u]);
        a[u] = xget<XFM>(x, xs, c);
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const bool ok = j + u < llen;
        s0 += ok ? v[u].x * a[u].x + v[u].y * a[u].y : 0.0;
        s1 += ok ? v[u].z * a[u].x + v[u].w * a[u].y : 0.0;
      }
    }
  }
  {
    const int64_t k = (node >> 6) * (int64_t)urow + (node & 63);
    for (int j = 0; j < ulen; j += U) {
      int32_t c[U];
      dv4 v[U];
      double2 a[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int64_t kk = k + (int64_t)SELL_C * (j + u < ulen ? j + u : ulen - 1);
        c[u] = ld_once(ucol + kk);
        v[u] = blk<true, false, VT>(uval, offd, kk);
      }
#pragma unroll
      for (int u = 0; u < U; ++u) a[u] = xget<XFM>(x, xs, c[u]);
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const bool ok = j + u < ulen;
        s0 += ok ? v[u].x * a[u].x + v[u].y * a[u].y : 0.0;
        s1 += ok ? v[u].z * a[u].x + v[u].w * a[u].y : 0.0;
      }
    }
  }
  if (GH) {   // ghost columns (after every owned column in the row's order)
    const int glen = m >> 16;
    const int64_t k = gsoff[node >> 6] + (node & 63);
    const VT* goff = gval + 2 * ngs;
    for (int j = 0; j < glen; j += U) {
      int32_t c[U];
      dv4 v[U];
      double2 a[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int64_t kk = k + (int64_t)SELL_C * (j + u < glen ? j + u : glen - 1);
        c[u] = gcol[kk];
        v[u] = blk<true, false, VT>(gval, goff, kk);
      }
#pragma unroll
      for (int u = 0; u < U; ++u) a[u] = xget<XFM>(x, xs, c[u]);
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const bool ok = j + u < glen;
        s0 += ok ? v[u].x * a[u].x + v[u].y * a[u].y : 0.0;
        s1 += ok ? v[u].z * a[u].x + v[u].w * a[u].y : 0.0;
      }
    }
  }
  double2 bb = {0.0, 0.0}, yy = {0.0, 0.0};
  dv4 w = {0.0, 0.0, 0.0, 0.0};
  if (EPI == EPI_RESID || EPI == EPI_BJAC)
    bb = MAMG_HSELL_NT >= 2 ? double2{ld_once(b + (bs ? node : 2 * node)), ld_once(b + (bs ? bs + node : 2 * node + 1))}
                            : double2{vget(b, bs, node, 0), vget(b, bs, node, 1)};
  if (EPI == EPI_YADD || EPI == EPI_BJAC) yy = reinterpret_cast<const double2*>(y)[node];
  if (EPI == EPI_BJAC) w = W[node];
  double o0, o1;
  if (EPI == EPI_Y) {
    o0 = s0; o1 = s1;
  } else if (EPI == EPI_YADD) {
    o0 = yy.x + s0; o1 = yy.y + s1;
  } else if (EPI == EPI_RESID) {
    o0 = bb.x - s0; o1 = bb.y - s1;
  } else {  // EPI_BJAC
    const double r0 = bb.x - s0, r1 = bb.y - s1;
    o0 = yy.x + (w.x * r0 + w.y * r1);
    o1 = yy.y + (w.z * r0 + w.w * r1);
  }
  if constexpr (MAMG_HSELL_NT >= 2) {
    __builtin_nontemporal_store(o0, out + (os ? node : 2 * node));
    __builtin_nontemporal_store(o1, out + (os ? os + node : 2 * node + 1));
  } else {
    vset(out, os, node, 0, o0);
    vset(out, os, node, 1, o1);
  }
}

// ---------------------------------------------------------------------------
// Row-pattern dictionary for an A0 whose node rows repeat (a constant-
// coefficient stencil: 28 distinct rows in 3-D, 10 in 2-D, whatever the mesh
// size).  The matrix is one 16-bit row-type code per node row plus a table
// of a few KB: type t has rlen[t] entries (column - row, block) in the row's
// stored column order at slots t rw + j.  No matrix stream is left: the
// kernel reads 2 B of code per row, gathers x and streams b / out.
// A wavefront whose 64 rows share one type (97 % of them at n = 256) takes
// the type through readfirstlane, so the table reads are scalar loads and
// x[node + delta] is 64 consecutive nodes, one coalesced 1 KB load; other
// wavefronts read the table per lane (it stays in L1 / L2).
// Each row is summed in its stored column order with hsell2_kernel's
// expression, so the result is bitwise that of the half and SELL layouts.
// ---------------------------------------------------------------------------
template <bool XFM, bool SYM, int U, class VT>
__device__ __forceinline__ void rowdict_row(int t, int64_t node, const int32_t* __restrict__ rlen,
                                            const int32_t* __restrict__ rdelta, const VT* __restrict__ rval,
                                            const VT* __restrict__ offd, int rw, const double* __restrict__ x,
                                            int64_t xs, double& s0, double& s1) {
  const int len = rlen[t];
  const int k0 = t * rw;
  for (int j = 0; j < len; j += U) {
    int32_t c[U];
    dv4 v[U];
    double2 a[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int kk = k0 + (j + u < len ? j + u : len - 1);
      c[u] = (int32_t)(node + rdelta[kk]);
      v[u] = blk<SYM, false, VT>(rval, offd, kk);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) a[u] = xget<XFM>(x, xs, c[u]);
#pragma unroll
    for (int u = 0; u < U; ++u) {
      // hsell2_kernel's and sell2_kernel's v.x * a.x + v.y * a.y as the
      // compiler contracts it there, spelled out: left to itself it turned
      // the products round for some entries of this kernel's fp32 side
      const bool ok = j + u < len;
      s0 += ok ? __builtin_fma(v[u].x, a[u].x, v[u].y * a[u].y) : 0.0;
      s1 += ok ? __builtin_fma(v[u].z, a[u].x, v[u].w * a[u].y) : 0.0;
    }
  }
}

// U: entries in flight per lane on the wave-uniform path (mixed waves take 4)
#ifndef MAMG_ROWDICT_LDS
#define MAMG_ROWDICT_LDS 0   // 1: mixed waves read the table from LDS (A/B: slower)
#endif
template <int EPI, bool XFM, bool SYM, int U, int TAG, class VT = double>
__global__ __launch_bounds__(256) void rowdict2_kernel(
    int64_t row0, int64_t nr, const uint16_t* __restrict__ rcode, const int32_t* __restrict__ rlen,
    const int32_t* __restrict__ rdelta, const VT* __restrict__ rval, int64_t nbs, int rw,
    const double* __restrict__ x, int64_t xs, const double* y, const double* __restrict__ b, int64_t bs,
    const dv4* __restrict__ W, double* out, int64_t os, int remap, const int32_t* __restrict__ sched) {
  const int64_t blk0 = sched ? (int64_t)sched[blockIdx.x] : row_block(remap);
  const int64_t node = row0 + blk0 * 256 + threadIdx.x;   // rows [row0, nr)
  if (node >= nr) return;
  const VT* offd = SYM ? rval + 2 * nbs : nullptr;
  const int code = (int)ld_once(rcode + node);
  const int first = __builtin_amdgcn_readfirstlane(code);
  double s0 = 0.0, s1 = 0.0;
  const bool mixed = __ballot(code != first) != 0;
#if MAMG_ROWDICT_LDS
  // A/B only: a workgroup with a mixed wave stages the
  // table in LDS and its mixed waves read it from there
  extern __shared__ double rowdict_lds[];
  if (__syncthreads_or(mixed)) {   // every thread of the workgroup is live here (full blocks) or none votes
    constexpr int PER = SYM ? 3 : 4;
    VT* lval = reinterpret_cast<VT*>(rowdict_lds);
    int32_t* ldel = reinterpret_cast<int32_t*>(lval + PER * nbs);
    for (int i = threadIdx.x; i < PER * (int)nbs; i += 256) lval[i] = rval[i];
    for (int i = threadIdx.x; i < (int)nbs; i += 256) ldel[i] = rdelta[i];
    __syncthreads();
    if (mixed) rowdict_row<XFM, SYM, 4, VT>(code, node, rlen, ldel, lval, SYM ? lval + 2 * nbs : nullptr, rw, x, xs, s0, s1);
  } else if (mixed) {
    rowdict_row<XFM, SYM, 4, VT>(code, node, rlen, rdelta, rval, offd, rw, x, xs, s0, s1);
  }
  if (!mixed) rowdict_row<XFM, SYM, U, VT>(first, node, rlen, rdelta, rval, offd, rw, x, xs, s0, s1);
#else
  if (!mixed) rowdict_row<XFM, SYM, U, VT>(first, node, rlen, rdelta, rval, offd, rw, x, xs, s0, s1);
  else rowdict_row<XFM, SYM, 4, VT>(code, node, rlen, rdelta, rval, offd, rw, x, xs, s0, s1);
#endif
  double2 bb = {0.0, 0.0}, yy = {0.0, 0.0};
  dv4 w = {0.0, 0.0, 0.0, 0.0};
  if (EPI == EPI_RESID || EPI == EPI_BJAC)
    bb = MAMG_HSELL_NT >= 2 ? double2{ld_once(b + (bs ? node : 2 * node)), ld_once(b + (bs ? bs + node : 2 * node + 1))}
                            : double2{vget(b, bs, node, 0), vget(b, bs, node, 1)};
  if (EPI == EPI_YADD || EPI == EPI_BJAC || EPI == EPI_PSM) yy = reinterpret_cast<const double2*>(y)[node];
  if (EPI == EPI_BJAC) w = W[node];
  if (EPI == EPI_PSM) {   // the row type's w D_B^-1: four scalars on the wave-uniform path
    if (!mixed) w = W[first];
    else w = W[code];
  }
  double o0, o1;
  if (EPI == EPI_Y) {
    o0 = s0; o1 = s1;
  } else if (EPI == EPI_YADD) {
    o0 = yy.x + s0; o1 = yy.y + s1;
  } else if (EPI == EPI_RESID) {
    o0 = bb.x - s0; o1 = bb.y - s1;
  } else if (EPI == EPI_PSM) {   // u = x1 + y - Wp (A y), y = T e the gathered vector itself
    const double2 ty = xget<XFM>(x, xs, (int32_t)node);
    o0 = (yy.x + ty.x) - (w.x * s0 + w.y * s1);
    o1 = (yy.y + ty.y) - (w.z * s0 + w.w * s1);
  } else {  // EPI_BJAC
    const double r0 = bb.x - s0, r1 = bb.y - s1;
    o0 = yy.x + (w.x * r0 + w.y * r1);
    o1 = yy.y + (w.z * r0 + w.w * r1);
  }
  if constexpr (MAMG_HSELL_NT >= 2) {
    __builtin_nontemporal_store(o0, out + (os ? node : 2 * node));
    __builtin_nontemporal_store(o1, out + (os ? os + node : 2 * node + 1));
  } else {
    vset(out, os, node, 0, o0);
    vset(out, os, node, 1, o1);
  }
}

// y = T e on level 0 (the matrix-free post step): T is
// the tentative prolongator, one 1 per aggregated node, so y(I) = e(agg[I]),
// both fields, and 0 for an isolated node.  e is the coarse level's
// node-interleaved correction (L2-resident), agg streams once.
__global__ __launch_bounds__(256) void tgather_kernel(int64_t nv, const int32_t* __restrict__ agg,
                                                      const double* __restrict__ e, double* __restrict__ y) {
  const int64_t I = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (I >= nv) return;
  const int32_t a = ld_once(agg + I);
  double2 v = {0.0, 0.0};
  if (a >= 0) v = reinterpret_cast<const double2*>(e)[a];
  reinterpret_cast<double2*>(y)[I] = v;
}

// fused prolongation + first post sweep on a SELL-64 [P | AP] (see
// bsr2_post_kernel).  Rows are sorted by length inside windows of
// SELL_SIGMA rows (slot i holds row perm[i]) so a wavefront's lanes have
// near-equal trip counts; blocks [0, plen) of a row are P's, [plen, len) AP's,
// selected per block (one loop, no divergence between the two parts).
constexpr int SELL_SIGMA = 4096;

template <int TAG>
__global__ __launch_bounds__(256) void sell2_post_kernel(
    int64_t nr, const int64_t* __restrict__ soff, const int32_t* __restrict__ meta,
    const int32_t* __restrict__ perm, const int32_t* __restrict__ bcol,
    const double* __restrict__ bval, const double* __restrict__ e, const double* __restrict__ x1,
    const double* __restrict__ r1, const dv4* __restrict__ W, double* out, int64_t os) {
  const int64_t slot = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (slot >= nr) return;
  const int64_t node = perm[slot];
  const int32_t m = meta[slot];
  const int len = m & 0xffff, plen = m >> 16;
  int64_t k = soff[slot / SELL_C] + (slot & (SELL_C - 1));
  double p0 = 0.0, p1 = 0.0, q0 = 0.0, q1 = 0.0;
  int j = 0;
  for (; j + SELL_U <= len; j += SELL_U, k += SELL_U * SELL_C) {
    int32_t c[SELL_U];
    dv4 v[SELL_U];
    double2 a[SELL_U];
#pragma unroll
    for (int u = 0; u < SELL_U; ++u) { c[u] = bcol[k + u * SELL_C]; v[u] = blk<false>(bval, nullptr, k + u * SELL_C); }
#pragma unroll
    for (int u = 0; u < SELL_U; ++u) a[u] = xget<false>(e, 0, c[u]);
#pragma unroll
    for (int u = 0; u < SELL_U; ++u) {
      const double u0 = v[u].x * a[u].x + v[u].y * a[u].y, u1 = v[u].z * a[u].x + v[u].w * a[u].y;
      const bool isp = j + u < plen;
      p0 += isp ? u0 : 0.0; p1 += isp ? u1 : 0.0; q0 += isp ? 0.0 : u0; q1 += isp ? 0.0 : u1;
    }
  }
  for (; j < len; ++j, k += SELL_C) {
    const dv4 v = blk<false>(bval, nullptr, k);
    const double2 a = xget<false>(e, 0, bcol[k]);
    const double u0 = v.x * a.x + v.y * a.y, u1 = v.z * a.x + v.w * a.y;
    const bool isp = j < plen;
    p0 += isp ? u0 : 0.0; p1 += isp ? u1 : 0.0; q0 += isp ? 0.0 : u0; q1 += isp ? 0.0 : u1;
  }
  const dv4 w = W[node];
  const double d0 = r1[2 * node] - q0, d1 = r1[2 * node + 1] - q1;
  vset(out, os, node, 0, x1[2 * node] + p0 + (w.x * d0 + w.y * d1));
  vset(out, os, node, 1, x1[2 * node + 1] + p1 + (w.z * d0 + w.w * d1));
}

// block-diagonal apply: out(I) = [y(I) +] W_I b(I)
template <bool ADD>
__global__ __launch_bounds__(256) void bd2_kernel(int64_t nv, const dv4* __restrict__ W,
                                                  const double* __restrict__ b, int64_t bs,
                                                  const double* y, double* out, int64_t os) {
  const int64_t I = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (I >= nv) return;
  const double b0 = vget(b, bs, I, 0), b1 = vget(b, bs, I, 1);
  const double2 wb = wmul(W[I], b0, b1);
  double o0 = wb.x, o1 = wb.y;
  if (ADD) { o0 += y[2 * I]; o1 += y[2 * I + 1]; }
  vset(out, os, I, 0, o0);
  vset(out, os, I, 1, o1);
}

__global__ __launch_bounds__(256) void scale_kernel(int64_t n, const double* __restrict__ w,
                                                    const double* __restrict__ b,
                                                    double* __restrict__ x) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) x[i] = w[i] * b[i];
}

// out = w * in (SMOOTHER_POLY step smoothers w_k W, built once at upload)
__global__ __launch_bounds__(256) void wscale_kernel(int64_t n, double w, const double* __restrict__ in,
                                                     double* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) out[i] = w * in[i];
}

}  // namespace

// the rank layout's launch of wscale_kernel (dist_layout.hip), on the null stream
void wscale(int64_t n, double w, const double* in, double* out) {
  wscale_kernel<<<nblocks(n), 256>>>(n, w, in, out);
}

namespace {

__global__ __launch_bounds__(256) void axpy_kernel(int64_t n, const double* __restrict__ e,
                                                   double* x) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) x[i] = x[i] + e[i];
}

// coarsest level: x = Ainv b, one wave per row
__global__ __launch_bounds__(256) void gemv_kernel(int64_t n, const double* __restrict__ Ainv,
                                                   const double* __restrict__ b,
                                                   double* __restrict__ x) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + wave;
  double s = 0.0;
  if (row < n) {
    const double* a = Ainv + row * n;
    for (int64_t j = lane; j < n; j += 64) s += a[j] * b[j];
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
  if (row < n && lane == 0) x[row] = s;
}

// ---- CG vector kernels ------------------------------------------------------

__global__ __launch_bounds__(256) void dot_partial_kernel(int64_t n, const double* __restrict__ a,
                                                          const double* __restrict__ b,
                                                          double* __restrict__ part) {
  __shared__ double red[4];
  double s = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
    s += a[i] * b[i];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) part[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

__device__ double block_sum256(double s) {   // 256 threads -> thread 0
  __shared__ double red[4];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

// rz = <r, z> (partials) -> residuals[0], tolerance, first active flag
__global__ __launch_bounds__(256) void pcg_init_kernel(int nb, const double* __restrict__ part, PcgState* st,
                                                       double tol, int relconv, int maxiter, double* res) {
  double s = 0.0;
  for (int i = threadIdx.x; i < nb; i += 256) s += part[i];
  s = block_sum256(s);
  if (threadIdx.x) return;
  st->it = 0; st->maxiter = maxiter; st->run = 0; st->alpha = 0.0; st->beta = 0.0; st->dq = 0.0;
  st->rz = s;
  if (s < 0.0) { st->active = 0; st->status = PCG_NOT_POS; st->tol = tol; res[0] = 0.0; return; }
  const double r0 = sqrt(s);
  res[0] = r0;
  st->tol = relconv ? tol * r0 : tol;
  st->active = (r0 > st->tol && maxiter > 0) ? 1 : 0;
  st->status = st->active ? PCG_RUNNING : PCG_STOPPED;
}

// dq = <d, A d>; alpha = rz / dq (the host loop's breakdown on dq == 0)
__global__ __launch_bounds__(256) void pcg_alpha_kernel(int nb, const double* __restrict__ part, PcgState* st) {
  double s = 0.0;
  for (int i = threadIdx.x; i < nb; i += 256) s += part[i];
  s = block_sum256(s);
  if (threadIdx.x) return;
  st->run = st->active;
  if (!st->active) return;
  st->dq = s;
  if (s == 0.0) { st->active = 0; st->status = PCG_DQ_ZERO; return; }
  st->alpha = st->rz / s;
}

__global__ __launch_bounds__(256) void pcg_xr_kernel(int64_t n, const PcgState* __restrict__ st,
                                                     const double* __restrict__ d, const double* __restrict__ q,
                                                     double* __restrict__ x, double* __restrict__ r) {
  if (!st->active) return;
  const double alpha = st->alpha;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) {
    x[i] = x[i] + alpha * d[i];
    r[i] = r[i] - alpha * q[i];
  }
}

// rz' = <r, B r>: beta, residuals[it + 1], stop test (tolerance / maxiter)
__global__ __launch_bounds__(256) void pcg_beta_kernel(int nb, const double* __restrict__ part, PcgState* st,
                                                       double* res, double* alphas, double* betas) {
  double s = 0.0;
  for (int i = threadIdx.x; i < nb; i += 256) s += part[i];
  s = block_sum256(s);
  if (threadIdx.x) return;
  if (!st->active) return;
  if (s < 0.0) { st->active = 0; st->status = PCG_RZ_NEG; return; }
  const double beta = s / st->rz;
  const int k = st->it;
  st->beta = beta;
  st->rz = s;
  res[k + 1] = sqrt(s);
  alphas[k] = st->alpha;
  betas[k] = beta;
  st->it = k + 1;
  if (!(res[k + 1] > st->tol) || k + 1 >= st->maxiter) { st->active = 0; st->status = PCG_STOPPED; }
}

// d = z + beta d; on <r, Br> < 0 this iteration's x update is undone instead
// (cbc.block restores x before breaking)
__global__ __launch_bounds__(256) void pcg_d_kernel(int64_t n, const PcgState* __restrict__ st,
                                                    const double* __restrict__ z, double* __restrict__ d,
                                                    double* __restrict__ x) {
  if (!st->run || st->status == PCG_DQ_ZERO) return;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  if (st->status == PCG_RZ_NEG) x[i] = x[i] - st->alpha * d[i];
  else d[i] = z[i] + st->beta * d[i];
}

__device__ __forceinline__ void block_part256(double s, double* __restrict__ out) {
  __shared__ double red[4];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) *out = (red[0] + red[1]) + (red[2] + red[3]);
  __syncthreads();
}

// part[block] = this block's share of <a, b> (DOT_BLOCKS blocks, grid stride)
__global__ __launch_bounds__(256) void dpcg_dot_kernel(int64_t n, const double* __restrict__ a,
                                                       const double* __restrict__ b, double* __restrict__ part) {
  double s = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
    s += a[i] * b[i];
  block_part256(s, part + blockIdx.x);
}

// the rank's nd dots: partials part[k * nb .. ) -> pv[k * P + rank], zeros in
// the other ranks' slots (one block)
__global__ __launch_bounds__(256) void dpcg_slot_kernel(int nb, int nd, const double* __restrict__ part,
                                                        double* __restrict__ pv, int P, int rank) {
  __shared__ double tot[3];
  for (int k = 0; k < nd; ++k) {
    double s = 0.0;
    for (int i = threadIdx.x; i < nb; i += 256) s += part[(int64_t)k * nb + i];
    block_part256(s, &tot[k]);
  }
  for (int i = threadIdx.x; i < nd * P; i += 256) pv[i] = (i % P == rank) ? tot[i / P] : 0.0;
}

__device__ __forceinline__ double dpcg_rank_sum(const double* __restrict__ pv, int P) {
  double s = 0.0;
  for (int q = 0; q < P; ++q) s += pv[q];   // rank order, on every rank
  return s;
}

// start-up: r = b - q (q = A x0), partials of ||r||^2 and ||b||^2 for stop_type 1
__global__ __launch_bounds__(256) void dpcg_r0_kernel(int64_t n, int stop, const double* __restrict__ b,
                                                      const double* __restrict__ q, double* __restrict__ r,
                                                      double* __restrict__ part, int nb) {
  double rr = 0.0, bb = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const double bi = b[i], ri = bi - q[i];
    r[i] = ri;
    rr += ri * ri;
    bb += bi * bi;
  }
  if (!stop) return;
  block_part256(rr, part + nb + blockIdx.x);
  block_part256(bb, part + 2 * nb + blockIdx.x);
}

// pv = [<r,z> | ||r||^2 | ||b||^2] (the last two with stop_type 1): first state
__global__ void dpcg_init_kernel(const double* __restrict__ pv, int P, DPcgState* st, double tol, int relconv,
                                 int maxiter, int stop, double* res, double* rn) {
  if (threadIdx.x || blockIdx.x) return;
  const double s = dpcg_rank_sum(pv, P);
  st->it = 0; st->maxiter = maxiter; st->run = 0; st->alpha = 0.0; st->beta = 0.0; st->dq = 0.0;
  st->stop = stop; st->rr = 0.0; st->thr = 0.0;
  st->rz = s;
  st->tol = tol;
  if (s < 0.0) { st->active = 0; st->status = PCG_NOT_POS; res[0] = 0.0; return; }
  const double r0 = sqrt(s);
  res[0] = r0;
  bool go;
  if (stop) {                       // ||r|| <= tol ||b||, ||b|| = 0 taken as 1
    const double rr = dpcg_rank_sum(pv + P, P), bb = dpcg_rank_sum(pv + 2 * P, P);
    const double bn = bb == 0.0 ? 1.0 : sqrt(bb);
    st->rr = rr;
    st->thr = tol * bn;             // the threshold itself (the host loop's tolerance * bnorm)
    rn[0] = sqrt(rr);
    go = rn[0] > st->thr;
  } else {
    st->tol = relconv ? tol * r0 : tol;
    go = r0 > st->tol;
  }
  st->active = (go && maxiter > 0) ? 1 : 0;
  st->status = st->active ? PCG_RUNNING : PCG_STOPPED;
}

// dq = <d, A d> over all ranks; alpha = rz / dq
__global__ void dpcg_alpha_kernel(const double* __restrict__ pv, int P, DPcgState* st) {
  if (threadIdx.x || blockIdx.x) return;
  st->run = st->active;
  if (!st->active) return;
  const double s = dpcg_rank_sum(pv, P);
  st->dq = s;
  if (s == 0.0) { st->active = 0; st->status = PCG_DQ_ZERO; return; }
  st->alpha = st->rz / s;
}

// x += alpha d, r -= alpha q (nothing when inactive); RR: this block's share
// of the new ||r||^2 into part[nb + block], in the same pass
template <bool RR>
__global__ __launch_bounds__(256) void dpcg_xr_kernel(int64_t n, const DPcgState* __restrict__ st,
                                                      const double* __restrict__ d, const double* __restrict__ q,
                                                      double* __restrict__ x, double* __restrict__ r,
                                                      double* __restrict__ part, int nb) {
  if (!st->active) return;          // uniform over the grid
  const double alpha = st->alpha;
  double rr = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    x[i] = x[i] + alpha * d[i];
    const double ri = r[i] - alpha * q[i];
    r[i] = ri;
    rr += ri * ri;
  }
  if (RR) block_part256(rr, part + nb + blockIdx.x);
}

// rz' = <r, B r> over all ranks: beta, the history entries, the stop test
__global__ void dpcg_beta_kernel(const double* __restrict__ pv, int P, DPcgState* st, double* res, double* rn,
                                 double* alphas, double* betas) {
  if (threadIdx.x || blockIdx.x) return;
  if (!st->active) return;
  const double s = dpcg_rank_sum(pv, P);
  if (s < 0.0) { st->active = 0; st->status = PCG_RZ_NEG; return; }
  const double beta = s / st->rz;
  const int k = st->it;
  st->beta = beta;
  st->rz = s;
  res[k + 1] = sqrt(s);
  alphas[k] = st->alpha;
  betas[k] = beta;
  st->it = k + 1;
  bool go;
  if (st->stop) {
    st->rr = dpcg_rank_sum(pv + P, P);
    rn[k + 1] = sqrt(st->rr);
    go = rn[k + 1] > st->thr;
  } else {
    go = res[k + 1] > st->tol;
  }
  if (!go || k + 1 >= st->maxiter) { st->active = 0; st->status = PCG_STOPPED; }
}

// d = z + beta d; on <r, Br> < 0 this iteration's x update is undone instead
__global__ __launch_bounds__(256) void dpcg_d_kernel(int64_t n, const DPcgState* __restrict__ st,
                                                     const double* __restrict__ z, double* __restrict__ d,
                                                     double* __restrict__ x) {
  if (!st->run || st->status == PCG_DQ_ZERO) return;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  if (st->status == PCG_RZ_NEG) x[i] = x[i] - st->alpha * d[i];
  else d[i] = z[i] + st->beta * d[i];
}

// field-major [v0; v1] (stride bs) -> node-interleaved pairs
__global__ __launch_bounds__(256) void interleave2_kernel(int64_t n, const double* __restrict__ in, int64_t bs,
                                                          double* __restrict__ out) {
  const int64_t I = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (I < n) reinterpret_cast<double2*>(out)[I] = double2{in[I], in[bs + I]};
}

// node-interleaved pairs -> out (field stride os, or node-interleaved if os == 0)
__global__ __launch_bounds__(256) void deinterleave2_kernel(int64_t n, const double* __restrict__ in,
                                                            double* __restrict__ out, int64_t os) {
  const int64_t I = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (I >= n) return;
  const double2 v = reinterpret_cast<const double2*>(in)[I];
  vset(out, os, I, 0, v.x);
  vset(out, os, I, 1, v.y);
}

// ---------------------------------------------------------------------------
// Multicolour node-block Gauss-Seidel (SMOOTHER_SGS / SMOOTHER_GS): the
// reference's SGS (src/amg_parameters.py:72) and its level-0 multiplicative
// Schwarz on the seed blocks (src/utils.py:84) in a parallel order.  The
// nodes are coloured (jp_round_kernel) so that no two nodes of a colour are
// adjacent; G = A_l with its node rows permuted colour by colour, so one
// colour is one contiguous row range [c0, c1) and one launch:
//   x(I) <- x(I) + D_i (b(I) - (A x)(I)),   I = perm[i],
// in place (a lane never reads an x(J) another lane of the launch writes).
// D_i = the unscaled inverse of node I's smoother block (permuted order).
// Lane groups of VL per row as bsr2_kernel; x node-interleaved; b with field
// stride bs (the caller's [u1; u2] r on level 0).  Oracle:
// mamg_oracle.Level.gs_sweep.
// ---------------------------------------------------------------------------
template <int VL, bool SYM>
__global__ __launch_bounds__(256) void gs2_kernel(
    int64_t c0, int64_t c1, const int32_t* __restrict__ perm, const int64_t* __restrict__ bptr,
    const int32_t* __restrict__ bcol, const double* __restrict__ bval, int64_t nbt,
    const dv4* __restrict__ D, double* x, const double* __restrict__ b, int64_t bs) {
  const int lane = threadIdx.x & (VL - 1);
  const int64_t i = c0 + ((int64_t)blockIdx.x * 256 + threadIdx.x) / VL;
  const double* offd = SYM ? bval + 2 * nbt : nullptr;
  const double2* x2 = reinterpret_cast<const double2*>(x);
  double s0 = 0.0, s1 = 0.0, t0 = 0.0, t1 = 0.0;
  if (i < c1) {
    const int64_t p0 = bptr[i], p1 = bptr[i + 1];
    for (int64_t base = p0; base < p1; base += 2 * VL) {
      const int64_t ka = base + lane, kb = ka + VL;
      const bool ha = ka < p1, hb = kb < p1;
      const int64_t la = ha ? ka : p1 - 1, lb = hb ? kb : p1 - 1;
      const int32_t ca = bcol[la], cb = bcol[lb];
      const dv4 v0 = blk<SYM>(bval, offd, la), v1 = blk<SYM>(bval, offd, lb);
      const double2 a = x2[ca], e = x2[cb];
      s0 += ha ? v0.x * a.x + v0.y * a.y : 0.0;
      s1 += ha ? v0.z * a.x + v0.w * a.y : 0.0;
      t0 += hb ? v1.x * e.x + v1.y * e.y : 0.0;
      t1 += hb ? v1.z * e.x + v1.w * e.y : 0.0;
    }
  }
  s0 += t0;
  s1 += t1;
#pragma unroll
  for (int off = VL / 2; off > 0; off >>= 1) {
    s0 += __shfl_xor(s0, off, VL);
    s1 += __shfl_xor(s1, off, VL);
  }
  if (i < c1 && lane == 0 && perm[i] >= 0) {
    const int64_t I = perm[i];
    const double r0 = vget(b, bs, I, 0) - s0, r1 = vget(b, bs, I, 1) - s1;
    const dv4 d = D[i];
    const double2 xi = x2[I];
    reinterpret_cast<double2*>(x)[I] = double2{xi.x + (d.x * r0 + d.y * r1), xi.y + (d.z * r0 + d.w * r1)};
  }
}

// ---------------------------------------------------------------------------
// Coarse tail: the whole cycle of the levels from tail_level down (the
// recursion below one coarse level, V or W), run by ONE workgroup of 512
// threads that walks the same op list the launch path would launch, with a
// workgroup barrier between ops instead of a kernel boundary.  Each op
// computes every row exactly as its kernel does (same lane groups, chunks,
// shuffle order; runtime lane count), so the results equal the launch path's
// up to FMA contraction.  For the deep levels of the reference family's
// W-cycle (HEM ratio ~4, levels visited 2^l times, one launch per colour)
// this replaces tens of thousands of ~5 us launches per apply.
// ---------------------------------------------------------------------------
// 512 threads: 256 VGPRs per lane (1024 would cap them at 128 and spill the
// interpreter's loop state to scratch); the tail's ops hold a few hundred
// rows x <= 4 lanes, so one or two passes either way
constexpr int TAIL_THREADS = 512;

// v + (v of the lane M away) inside groups of 4 lanes, by DPP quad
// permutations (one VALU op per 32-bit half) instead of an LDS-routed
// ds_bpermute; the same value and sum as __shfl_xor(v, M, 4)
template <int M>
__device__ __forceinline__ double quad_xor(double v) {
  constexpr int ctrl = M == 1 ? 0xB1 : 0x4E;   // quad_perm [1,0,3,2] / [2,3,0,1]
  const long long b = __double_as_longlong(v);
  const int lo = __builtin_amdgcn_update_dpp(0, (int)b, ctrl, 0xF, 0xF, false);
  const int hi = __builtin_amdgcn_update_dpp(0, (int)(b >> 32), ctrl, 0xF, 0xF, false);
  return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}

// a load from an operand that is always in global memory (the tail's
// matrices): the TOp fields are generic pointers (a vector field may hold an
// LDS address), so without the cast every load would be a flat load
template <class T>
__device__ __forceinline__ T gload(const T* p) {
  return *(const __attribute__((address_space(1))) T*)p;
}
template <bool SYM>
__device__ __forceinline__ dv4 tail_blk(const double* v, const double* off, int k) {
  if (SYM) {
    const dv2 d = gload(reinterpret_cast<const dv2*>(v) + k);
    const double b = gload(off + k);
    return dv4{d.x, b, b, d.y};
  }
  return gload(reinterpret_cast<const dv4*>(v) + k);
}

#define AS1 __attribute__((address_space(1)))
#define AS3 __attribute__((address_space(3)))

// A vector operand of a tail op: in the workgroup's LDS (a tagged offset,
// tail_lds_plan) or in global memory, known per op (uniform).  Every access
// is a typed ds_ / global_ instruction, never a FLAT access through a generic
// pointer (FLAT loads of LDS data returned zeros intermittently in the row
// merges; rowstage.h).
struct TVec {
  double* g = nullptr;
  AS3 double* l = nullptr;
  bool lds = false;
  __device__ __forceinline__ double ld(int64_t i) const { return lds ? l[i] : *(const AS1 double*)(g + i); }
  __device__ __forceinline__ void st(int64_t i, double v) const {
    if (lds) l[i] = v;
    else *(AS1 double*)(g + i) = v;
  }
};
__device__ __forceinline__ TVec tvec(const double* p, char* lds) {
  const uintptr_t u = (uintptr_t)p;
  TVec v;
  v.lds = (u & 1) != 0;
  if (v.lds) v.l = (AS3 double*)(lds + (u & ~(uintptr_t)1));
  else v.g = const_cast<double*>(p);
  return v;
}
struct TOpnd {   // the vector operands of one op
  TVec x, y, b, out, part;
};

// x(c) as a pair; XL: x is in LDS for every op of the program (no branch)
template <bool XL>
__device__ __forceinline__ double2 tail_x(const TVec& x, int c) {
  if (XL || x.lds) {
    const dv2 v = ((const AS3 dv2*)x.l)[c];
    return double2{v.x, v.y};
  }
  const dv2 v = ((const AS1 dv2*)x.g)[c];
  return double2{v.x, v.y};
}

// the matrix side of a tail SpMV / GS op (global arrays, typed loads)
struct TailMat {
  const TOp& o;
  const double* offd;
  __device__ explicit TailMat(const TOp& op) : o(op), offd(op.sym ? op.val + 2 * op.nb : nullptr) {}
  __device__ int P(int i) const { return (int)gload(o.ptr + i); }
  __device__ int32_t perm(int i) const { return gload(o.perm + i); }
  __device__ dv4 W(int i) const { return gload(o.W + i); }
  __device__ int32_t C(int k) const { return gload(o.col + k); }
  __device__ dv4 V(int k) const { return o.sym ? tail_blk<true>(o.val, offd, k) : tail_blk<false>(o.val, nullptr, k); }
};
// rows of a lane-group BSR2 op (bsr2_kernel's per-row code, node-major
// vectors); GS: rows [r0, r1) of the colour-permuted matrix, update in place.
// XL: the gathered vector x lives in LDS
// LIGHT (the register-resident kernel, whose generic ops are the few
// non-resident transfers): no first-chunk prefetch, fewer live registers
template <bool XL, bool LIGHT = false>
__device__ void tail_bsr(const TOp& o, const TOpnd& V, bool gs) {
  const TailMat M(o);
  // 32-bit row arithmetic (tail levels are small) and shifts by log2(VL):
  // a 64-bit division per row chunk cost more than the chunk's loads
  const int VL = o.vl, lvl = 31 - __builtin_clz(VL);
  const int lane = threadIdx.x & (VL - 1);
  const int rows = (int)(gs ? o.r1 - o.r0 : o.n);
  const int row0 = gs ? (int)o.r0 : 0;
  const TVec& X = V.x;
  for (int base = 0; base < (rows << lvl); base += TAIL_THREADS) {   // uniform trip count
    const int v = base + (int)threadIdx.x;
    const int node = row0 + (v >> lvl);
    const bool live = (v >> lvl) < rows;
    double s0 = 0.0, s1 = 0.0, t0 = 0.0, t1 = 0.0;
    // GS: the row's own operands loaded before the block loop (its latency
    // overlaps the gathers; x(I) is not written by this colour step's other rows)
    // every lane issues its row's pointer, permutation and block-inverse
    // loads together, branch-free (a dead lane reads row row0 and drops it),
    // so they form one round trip instead of a chain behind a branch
    const int nodec = live ? node : row0;
    const int p0 = M.P(nodec), p1 = live ? M.P(nodec + 1) : p0;
    int gI = -1;
    dv4 gd = {0.0, 0.0, 0.0, 0.0};
    if (gs) {
      gI = live ? M.perm(nodec) : -1;
      gd = M.W(nodec);
    }
    const int gIc = gI >= 0 ? gI : 0;
    double gb0 = 0.0, gb1 = 0.0;
    double2 gx = {0.0, 0.0};
    if (gs) {
      gb0 = V.b.ld(2 * gIc);
      gb1 = V.b.ld(2 * gIc + 1);
      gx = tail_x<XL>(X, gIc);
    }
    if (!LIGHT && p1 > p0) {
      // the first two chunks: all column and value loads issued before any
      // gather, so a row of up to 4 VL blocks is one load -> gather round trip
      {
        int kk[4], ll[4];
        bool hh[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          kk[q] = p0 + lane + q * VL;
          hh[q] = kk[q] < p1;
          ll[q] = hh[q] ? kk[q] : p1 - 1;
        }
        int32_t cc[4];
        dv4 vv[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          cc[q] = M.C(ll[q]);
          vv[q] = M.V(ll[q]);
        }
        double2 xa[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) xa[q] = tail_x<XL>(X, cc[q]);
#pragma unroll
        for (int q = 0; q < 4; q += 2) {
          s0 += hh[q] ? vv[q].x * xa[q].x + vv[q].y * xa[q].y : 0.0;
          s1 += hh[q] ? vv[q].z * xa[q].x + vv[q].w * xa[q].y : 0.0;
          t0 += hh[q + 1] ? vv[q + 1].x * xa[q + 1].x + vv[q + 1].y * xa[q + 1].y : 0.0;
          t1 += hh[q + 1] ? vv[q + 1].z * xa[q + 1].x + vv[q + 1].w * xa[q + 1].y : 0.0;
        }
      }
    }
    if (p1 > p0) {
      for (int kb0 = LIGHT ? p0 : p0 + 4 * VL; kb0 < p1; kb0 += 2 * VL) {
        const int ka = kb0 + lane, kb = ka + VL;
        const bool ha = ka < p1, hb = kb < p1;
        const int la = ha ? ka : p1 - 1, lb = hb ? kb : p1 - 1;
        const int32_t c0 = M.C(la), c1 = M.C(lb);
        const dv4 v0 = M.V(la);
        const dv4 v1 = M.V(lb);
        const double2 a = tail_x<XL>(X, c0), e = tail_x<XL>(X, c1);
        s0 += ha ? v0.x * a.x + v0.y * a.y : 0.0;
        s1 += ha ? v0.z * a.x + v0.w * a.y : 0.0;
        t0 += hb ? v1.x * e.x + v1.y * e.y : 0.0;
        t1 += hb ? v1.z * e.x + v1.w * e.y : 0.0;
      }
    }
    s0 += t0;
    s1 += t1;
    if (VL <= 4) {   // the tail's lane counts (MAMG_TAIL_VL <= 4): xor 2, then xor 1, as below
      if (VL == 4) {
        s0 += quad_xor<2>(s0);
        s1 += quad_xor<2>(s1);
      }
      if (VL >= 2) {
        s0 += quad_xor<1>(s0);
        s1 += quad_xor<1>(s1);
      }
    } else {
      for (int off = VL / 2; off > 0; off >>= 1) {
        s0 += __shfl_xor(s0, off, VL);
        s1 += __shfl_xor(s1, off, VL);
      }
    }
    if (!live || lane != 0) continue;
    if (gs) {
      if (gI < 0) continue;
      const double r0 = gb0 - s0, r1 = gb1 - s1;
      V.out.st(2 * gI, gx.x + (gd.x * r0 + gd.y * r1));
      V.out.st(2 * gI + 1, gx.y + (gd.z * r0 + gd.w * r1));
      continue;
    }
    double o0, o1;
    if (o.epi == EPI_Y) {
      o0 = s0; o1 = s1;
    } else if (o.epi == EPI_YADD) {
      o0 = V.y.ld(2 * node) + s0; o1 = V.y.ld(2 * node + 1) + s1;
    } else if (o.epi == EPI_RESID) {
      o0 = V.b.ld(2 * node) - s0; o1 = V.b.ld(2 * node + 1) - s1;
    } else if (o.epi == EPI_KPOST) {
      const double r0 = V.b.ld(2 * node), r1 = V.b.ld(2 * node + 1);
      const dv4 w = M.W(node);
      o0 = V.y.ld(2 * node) + (w.x * r0 + w.y * r1) + s0;
      o1 = V.y.ld(2 * node + 1) + (w.z * r0 + w.w * r1) + s1;
    } else {  // EPI_BJAC
      const double r0 = V.b.ld(2 * node) - s0, r1 = V.b.ld(2 * node + 1) - s1;
      const dv4 w = M.W(node);
      o0 = V.y.ld(2 * node) + (w.x * r0 + w.y * r1);
      o1 = V.y.ld(2 * node + 1) + (w.z * r0 + w.w * r1);
    }
    V.out.st(2 * node, o0);
    V.out.st(2 * node + 1, o1);
  }
}

// a thread's register-resident row (see TOp): up to RES_RB blocks; the rest
// of a longer row in the LDS region (values at ovv, 16-bit columns at ovc,
// the GS block inverse at gdo; byte offsets)
constexpr int RES_RB = 12;
struct TRes {
  int len = 0, gI = -1, ovv = 0, ovc = 0, gdo = 0;
  uint32_t c[RES_RB / 2];   // two 16-bit node columns (the tail levels have < 2^16 nodes)
  dv4 v[RES_RB];
  __device__ __forceinline__ int col(int k) const { return (int)((c[k >> 1] >> (16 * (k & 1))) & 0xffffu); }
};

// T_RLOAD: every resident row of the program from an image built at plan
// time (tail_res_plan): its blocks slot-major (val: dv4 [RES_RB][TAIL_THREADS],
// col: packed 16-bit column pairs [RES_RB / 2][TAIL_THREADS]), its header
// (ridx: length, node, first overflow block; [3][TAIL_THREADS]) and the LDS
// region's bytes (b: n bytes -> LDS byte r0: the GS block inverses, one per
// thread (TAIL_THREADS x 32 B), r1 overflow blocks' values (32 B), their
// 16-bit columns).  One coalesced round trip instead of the chain row index
// -> row pointer -> columns and values.
__device__ __forceinline__ void tail_rload(const TOp& o, TRes& R, char* lds) {
  const int t = (int)threadIdx.x;
  {   // the LDS region first (fewer live registers than after the rows' loads)
    const dv2* src = reinterpret_cast<const dv2*>(o.b);
    AS3 dv2* dst = (AS3 dv2*)(lds + o.r0);
    const int n16 = (int)(o.n / 16);
    for (int i0 = t; i0 < n16; i0 += 2 * TAIL_THREADS) {   // two 16-byte loads in flight per lane
      const bool h1 = i0 + TAIL_THREADS < n16;
      const dv2 w0 = gload(src + i0), w1 = h1 ? gload(src + i0 + TAIL_THREADS) : dv2{0.0, 0.0};
      dst[i0] = w0;
      if (h1) dst[i0 + TAIL_THREADS] = w1;
    }
  }
  const dv4* iv = reinterpret_cast<const dv4*>(o.val);
  const uint32_t* ic = reinterpret_cast<const uint32_t*>(o.col);
  R.len = gload(o.ridx + t);
  R.gI = gload(o.ridx + TAIL_THREADS + t);
  const int ovs = gload(o.ridx + 2 * TAIL_THREADS + t);
#pragma unroll
  for (int k = 0; k < RES_RB; ++k) R.v[k] = gload(iv + k * TAIL_THREADS + t);
#pragma unroll
  for (int k = 0; k < RES_RB / 2; ++k) R.c[k] = gload(ic + k * TAIL_THREADS + t);
  const int ovb = (int)o.r0 + 32 * TAIL_THREADS;
  R.ovv = ovb + 32 * ovs;
  R.ovc = ovb + 32 * (int)o.r1 + 2 * ovs;
  R.gdo = (int)o.r0 + 32 * t;
}

// a row of a T_BSR / T_GS op from the thread's resident row (tail_bsr's
// operations at node gI; one lane per row, blocks summed in row order over
// two alternating accumulators)
template <bool XL>
__device__ __forceinline__ void tail_res(const TOp& o, const TOpnd& V, const TRes& R, bool gs, const char* lds) {
  const int j = (int)threadIdx.x - o.rbase;
  if (j < (int)o.r0 || j >= (int)o.r1) return;
  const int node = R.gI;
  const TVec& X = V.x;
  double gb0 = 0.0, gb1 = 0.0;
  double2 gx = {0.0, 0.0};
  if (gs) {
    gb0 = V.b.ld(2 * node);
    gb1 = V.b.ld(2 * node + 1);
    gx = tail_x<XL>(X, node);
  }
  double s0 = 0.0, s1 = 0.0, t0 = 0.0, t1 = 0.0;
  constexpr int GQ = RES_RB / 2;   // gathers in flight
#pragma unroll
  for (int k0 = 0; k0 < RES_RB; k0 += GQ) {
    double2 xa[GQ];
#pragma unroll
    for (int q = 0; q < GQ; ++q) xa[q] = tail_x<XL>(X, R.col(k0 + q));
    // blocks past the row's length are zero (tail_rload) and gather x(0):
    // no predicate, 0 * x(0) adds +-0
#pragma unroll
    for (int q = 0; q < GQ; q += 2) {   // fused multiply-adds into four accumulators
      const int k = k0 + q;
      s0 = fma(R.v[k].y, xa[q].y, fma(R.v[k].x, xa[q].x, s0));
      s1 = fma(R.v[k].w, xa[q].y, fma(R.v[k].z, xa[q].x, s1));
      t0 = fma(R.v[k + 1].y, xa[q + 1].y, fma(R.v[k + 1].x, xa[q + 1].x, t0));
      t1 = fma(R.v[k + 1].w, xa[q + 1].y, fma(R.v[k + 1].z, xa[q + 1].x, t1));
    }
  }
  // a long row's remaining blocks, from the LDS region, four at a time:
  // their column, value and x loads issued together (two LDS round trips
  // per four blocks, not two per block); past the row's end: column 0, zero
  // values (tail_rload pads the region's last row to a multiple of 4)
  for (int k0 = 0; k0 < R.len - RES_RB; k0 += 4) {
    int c[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) c[q] = (int)*(const AS3 uint16_t*)(lds + R.ovc + 2 * (k0 + q));
    dv4 v[4];
    double2 a[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      v[q] = *(const AS3 dv4*)(lds + R.ovv + 32 * (k0 + q));
      a[q] = tail_x<XL>(X, c[q]);
    }
#pragma unroll
    for (int q = 0; q < 4; q += 2) {
      s0 = fma(v[q].y, a[q].y, fma(v[q].x, a[q].x, s0));
      s1 = fma(v[q].w, a[q].y, fma(v[q].z, a[q].x, s1));
      t0 = fma(v[q + 1].y, a[q + 1].y, fma(v[q + 1].x, a[q + 1].x, t0));
      t1 = fma(v[q + 1].w, a[q + 1].y, fma(v[q + 1].z, a[q + 1].x, t1));
    }
  }
  s0 += t0;
  s1 += t1;
  if (gs) {
    const double r0 = gb0 - s0, r1 = gb1 - s1;
    const dv4 gd = *(const AS3 dv4*)(lds + R.gdo);
    V.out.st(2 * node, gx.x + (gd.x * r0 + gd.y * r1));
    V.out.st(2 * node + 1, gx.y + (gd.z * r0 + gd.w * r1));
    return;
  }
  double o0, o1;
  if (o.epi == EPI_Y) {
    o0 = s0; o1 = s1;
  } else if (o.epi == EPI_YADD) {
    o0 = V.y.ld(2 * node) + s0; o1 = V.y.ld(2 * node + 1) + s1;
  } else if (o.epi == EPI_RESID) {
    o0 = V.b.ld(2 * node) - s0; o1 = V.b.ld(2 * node + 1) - s1;
  } else if (o.epi == EPI_KPOST) {
    const double r0 = V.b.ld(2 * node), r1 = V.b.ld(2 * node + 1);
    const dv4 w = gload(o.W + node);
    o0 = V.y.ld(2 * node) + (w.x * r0 + w.y * r1) + s0;
    o1 = V.y.ld(2 * node + 1) + (w.z * r0 + w.w * r1) + s1;
  } else {  // EPI_BJAC
    const double r0 = V.b.ld(2 * node) - s0, r1 = V.b.ld(2 * node + 1) - s1;
    const dv4 w = gload(o.W + node);
    o0 = V.y.ld(2 * node) + (w.x * r0 + w.y * r1);
    o1 = V.y.ld(2 * node + 1) + (w.z * r0 + w.w * r1);
  }
  V.out.st(2 * node, o0);
  V.out.st(2 * node + 1, o1);
}

// ---- nonlinear AMLI inside the tail (T_KDOT / T_KORTH / T_KUPD): the launch
// path's kdot_kernel / korth_kernel / kupd_kernel as one workgroup.  The
// workgroup's two halves stand for two of the launch path's 256-thread blocks
// at a time (as T_DOT2 does): the same elements per thread, the same shuffle
// tree, the same (w0 + w1) + (w2 + w3) over a block's four waves, the partials
// in the same DLevel::kpart slots and summed by the consumer in the same
// order -- so a scalar has the launch path's bits, and a replay its own.
// One vector operand of a K op from its level's table (KTable; uniform)
__device__ __forceinline__ TVec tail_kvec(const TOp& o, int slot, char* lds) {
  const uint64_t v = gload(reinterpret_cast<const uint64_t*>(o.ptr) + slot);
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(v >> 32));
  return tvec(reinterpret_cast<const double*>(((uint64_t)hi << 32) | lo), lds);
}
// kblock_sum of each half of the workgroup: the 256 threads' values summed,
// the same on every thread of the half (kred: one row per wave; free again on return)
template <int NV>
__device__ __forceinline__ void tail_half_sum(double (&v)[NV], double (*kred)[MAMG_NL_AMLI_MAX - 1]) {
  static_assert(NV <= MAMG_NL_AMLI_MAX - 1, "kred's row");
  const int t = (int)threadIdx.x, w0 = (t >> 8) * 4;
#pragma unroll
  for (int k = 0; k < NV; ++k) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v[k] += __shfl_xor(v[k], off, 64);
  }
  if ((t & 63) == 0) {
#pragma unroll
    for (int k = 0; k < NV; ++k) kred[t >> 6][k] = v[k];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < NV; ++k) v[k] = (kred[w0][k] + kred[w0 + 1][k]) + (kred[w0 + 2][k] + kred[w0 + 3][k]);
  __syncthreads();
}
// the launch path's grid: min(SCALE_BLOCKS, ceil(n / 256)) blocks (launch_kstep)
__device__ __forceinline__ int tail_kblocks(int64_t n) {
  const int64_t b = (n + 255) / 256;
  return (int)(b < SCALE_BLOCKS ? b : SCALE_BLOCKS);
}

// A K op resolves an operand where it uses it (tail_kvec in the loop bodies)
// and walks the earlier directions in a run-time loop, one dot or one
// direction at a time: a step names up to twelve vectors, and holding them all
// as TVecs costs more scalar registers than the kernel has next to the
// register-resident rows (it spilled).

// kdot_kernel<J>: part[KP_DOT + i * SCALE_BLOCKS + block] = the block's share of <z, q_i>, i < J = o.r0
__device__ __forceinline__ void tail_kdot(const TOp& o, char* lds, double (*kred)[MAMG_NL_AMLI_MAX - 1]) {
  const int J = (int)o.r0, t = (int)threadIdx.x, tt = t & 255, nbl = tail_kblocks(o.n);
  for (int i = 0; i < J; ++i) {
    for (int vb0 = 0; vb0 < nbl; vb0 += TAIL_THREADS / 256) {
      const int vb = vb0 + (t >> 8);
      double s[1] = {0.0};
      if (vb < nbl) {
        const TVec z = tail_kvec(o, KT_Z, lds), q = tail_kvec(o, KT_Q + i, lds);
        for (int64_t k = (int64_t)vb * 256 + tt; k < o.n; k += (int64_t)nbl * 256) s[0] += z.ld(k) * q.ld(k);
      }
      tail_half_sum<1>(s, kred);
      if (tt == 0 && vb < nbl) tail_kvec(o, KT_PART, lds).st(KP_DOT + i * SCALE_BLOCKS + vb, s[0]);
    }
  }
}

__device__ __forceinline__ double tail_ksel(int i, double b0, double b1, double b2) {
  return i == 0 ? b0 : i == 1 ? b1 : b2;
}

// korth_kernel<J>: the beta's from T_KDOT's partials and the stored d_i (a
// dead direction's beta is 0, never 0 / 0); J > 0: p_J, q_J written; J = 0:
// p_0 = z, q_0 = w are in place; both: the blocks' shares of <p_J, q_J>, <p_J, r>
__device__ __forceinline__ void tail_korth(const TOp& o, char* lds, double (*kred)[MAMG_NL_AMLI_MAX - 1]) {
  static_assert(MAMG_NL_AMLI_MAX - 1 == 3, "tail_ksel holds three beta's");
  const int J = (int)o.r0, t = (int)threadIdx.x, tt = t & 255, nbl = tail_kblocks(o.n);
  double b0 = 0.0, b1 = 0.0, b2 = 0.0;
  for (int i = 0; i < J; ++i) {
    const TVec part = tail_kvec(o, KT_PART, lds);
    double s[1] = {0.0};
    for (int b = tt; b < nbl; b += 256) s[0] += part.ld(KP_DOT + i * SCALE_BLOCKS + b);
    tail_half_sum<1>(s, kred);
    const double d = part.ld(KP_D + i);
    const double be = d > 0.0 ? s[0] / d : 0.0;
    if (i == 0) b0 = be;
    else if (i == 1) b1 = be;
    else b2 = be;
  }
  for (int vb0 = 0; vb0 < nbl; vb0 += TAIL_THREADS / 256) {
    const int vb = vb0 + (t >> 8);
    double a[2] = {0.0, 0.0};
    if (vb < nbl) {
      for (int64_t k = (int64_t)vb * 256 + tt; k < o.n; k += (int64_t)nbl * 256) {
        double pk, qk;
        if (J > 0) {
          pk = tail_kvec(o, KT_Z, lds).ld(k);
          for (int i = 0; i < J; ++i) pk -= tail_ksel(i, b0, b1, b2) * tail_kvec(o, KT_P + i, lds).ld(k);
          tail_kvec(o, KT_P + J, lds).st(k, pk);
          qk = tail_kvec(o, KT_W, lds).ld(k);
          for (int i = 0; i < J; ++i) qk -= tail_ksel(i, b0, b1, b2) * tail_kvec(o, KT_Q + i, lds).ld(k);
          tail_kvec(o, KT_Q + J, lds).st(k, qk);
        } else {
          pk = tail_kvec(o, KT_P, lds).ld(k);
          qk = tail_kvec(o, KT_Q, lds).ld(k);
        }
        a[0] += pk * qk;
        a[1] += pk * tail_kvec(o, J == 0 ? KT_B : KT_R, lds).ld(k);
      }
    }
    tail_half_sum<2>(a, kred);
    if (tt == 0 && vb < nbl) {
      const TVec part = tail_kvec(o, KT_PART, lds);
      part.st(KP_PQ + 2 * vb, a[0]);
      part.st(KP_PQ + 2 * vb + 1, a[1]);
    }
  }
}

// kupd_kernel: d_j (stored by one thread) and alpha from T_KORTH's partials
// (alpha = 0 for a dead direction); e = alpha p_j (step 0) or e += alpha p_j;
// r_out = r_in - alpha q_j unless this is the last step
__device__ __forceinline__ void tail_kupd(const TOp& o, char* lds, double (*kred)[MAMG_NL_AMLI_MAX - 1]) {
  const int j = (int)o.r0, t = (int)threadIdx.x, tt = t & 255, nbl = tail_kblocks(o.n);
  const bool first = j == 0, last = j == (int)o.r1 - 1;
  double a[2] = {0.0, 0.0};
  {
    const TVec part = tail_kvec(o, KT_PART, lds);
    for (int b = tt; b < nbl; b += 256) {
      a[0] += part.ld(KP_PQ + 2 * b);
      a[1] += part.ld(KP_PQ + 2 * b + 1);
    }
  }
  tail_half_sum<2>(a, kred);
  const double d = a[0];
  const double alpha = d > 0.0 ? a[1] / d : 0.0;
  if (t == 0) tail_kvec(o, KT_PART, lds).st(KP_D + j, d);
  for (int64_t k = t; k < o.n; k += TAIL_THREADS) {
    const TVec e = tail_kvec(o, KT_X, lds);
    const double pk = tail_kvec(o, KT_P + j, lds).ld(k);
    e.st(k, first ? alpha * pk : e.ld(k) + alpha * pk);
    if (!last)
      tail_kvec(o, KT_R, lds).st(k, tail_kvec(o, first ? KT_B : KT_R, lds).ld(k) - alpha * tail_kvec(o, KT_Q + j, lds).ld(k));
  }
}

// STAMP: thread 0 records the 100 MHz wall clock at the start and after every
// op's barrier (stamps[0..nops]; MAMG_TAIL_PROFILE diagnosis, dev_time_apply)
// dynamic LDS: the tail levels' work vectors (tail_lds_plan)
extern __shared__ double tail_lds[];

// XL: every SpMV / GS op of the program gathers from an LDS-resident x
// (tail_lds_plan placed all of them), so the gathers are ds_reads
// RES: the program has register-resident rows (T_RLOAD, res ops)
// KOPS: the program has nonlinear AMLI steps (T_KDOT / T_KORTH / T_KUPD).  A
// flag of their own: compiled into every variant they cost the W-cycle's
// programs, which hold none, 2.7 % per apply
template <bool STAMP, bool XL, bool RES, bool KOPS = false>
__global__ __launch_bounds__(TAIL_THREADS) void tail_kernel(const TOp* __restrict__ gprog, int nops, int prog_lds,
                                                           uint64_t* __restrict__ stamps) {
  __shared__ double red[TAIL_THREADS / 64][2];
  __shared__ double kred[TAIL_THREADS / 64][MAMG_NL_AMLI_MAX - 1];
  TRes R;
  const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
  char* lds = reinterpret_cast<char*>(tail_lds);
  if (STAMP && t == 0) { stamps[0] = wall_clock64(); stamps[nops + 1] = clock64(); }
  // the op descriptors: copied whole into the dynamic LDS at prog_lds (>= 0)
  // once, so an op starts on LDS reads, with no global round trip on the
  // way from one op to the next; else read from global memory per op
  constexpr int TW = (int)(sizeof(TOp) / 8);
  const uint64_t* gw = reinterpret_cast<const uint64_t*>(gprog);
  const AS3 uint64_t* lw = (const AS3 uint64_t*)(lds + (prog_lds > 0 ? prog_lds : 0));
  if (prog_lds >= 0) {
    AS3 uint64_t* dst = (AS3 uint64_t*)(lds + prog_lds);
    const int nw = nops * TW;
    for (int i0 = t; i0 < nw; i0 += 8 * TAIL_THREADS) {   // 8 loads in flight per lane
      uint64_t v[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) v[q] = i0 + q * TAIL_THREADS < nw ? gload(gw + i0 + q * TAIL_THREADS) : 0;
#pragma unroll
      for (int q = 0; q < 8; ++q)
        if (i0 + q * TAIL_THREADS < nw) dst[i0 + q * TAIL_THREADS] = v[q];
    }
    __syncthreads();
  }
  for (int k = 0; k < nops; ++k) {
    TOp od;
    if (prog_lds >= 0) {
      uint64_t w[TW];
#pragma unroll
      for (int q = 0; q < TW; ++q) {
        // the descriptor is uniform: into scalar registers, not 2 VGPRs per word
        const uint64_t v = lw[k * TW + q];
        const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v);
        const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(v >> 32));
        w[q] = ((uint64_t)hi << 32) | lo;
      }
      __builtin_memcpy(&od, w, sizeof(TOp));
    } else {
      od = gprog[k];
    }
    const TOp& o = od;   // uniform; matrices global, vectors through V
    TOpnd V;
    V.x = tvec(od.x, lds);
    V.y = tvec(od.y, lds);
    V.b = tvec(od.b, lds);
    V.out = tvec(od.out, lds);
    V.part = tvec(od.part, lds);
    switch (o.kind) {
      case T_COPY:
        for (int64_t i = t; i < o.n; i += TAIL_THREADS) V.out.st(i, V.x.ld(i));
        break;
      case T_BSR:
        if (RES && o.res) tail_res<XL>(o, V, R, false, lds);
        else tail_bsr<XL, RES>(o, V, false);
        break;
      case T_GS:
        if (RES && o.res) tail_res<XL>(o, V, R, true, lds);
        else tail_bsr<XL, RES>(o, V, true);
        break;
      case T_RLOAD:
        if (RES) tail_rload(o, R, lds);
        break;
      case T_BD:
        for (int64_t I = t; I < o.n; I += TAIL_THREADS) {
          const double b0 = V.b.ld(2 * I), b1 = V.b.ld(2 * I + 1);
          const dv4 w = gload(o.W + I);
          V.out.st(2 * I, w.x * b0 + w.y * b1);
          V.out.st(2 * I + 1, w.z * b0 + w.w * b1);
        }
        break;
      case T_AXPY:
        for (int64_t i = t; i < o.n; i += TAIL_THREADS) V.out.st(i, V.out.ld(i) + V.x.ld(i));
        break;
      case T_ZERO:
        for (int64_t i = t; i < o.n; i += TAIL_THREADS) V.out.st(i, 0.0);
        break;
      case T_GEMV:   // gemv_kernel: one wave per row; small: one thread per row
        if (o.n <= TAIL_THREADS) {   // no shuffle tree on the dependent chain
          if (t < o.n) {
            double s0 = 0.0, s1 = 0.0;
            int j = 0;
            if ((uintptr_t)o.w & 1) {   // the matrix in the resident rows' LDS region (tail_res_plan)
              const AS3 double* a = (const AS3 double*)(lds + ((uintptr_t)o.w & ~(uintptr_t)1)) + (int64_t)t * o.n;
              for (; j + 1 < (int)o.n; j += 2) { s0 += a[j] * V.x.ld(j); s1 += a[j + 1] * V.x.ld(j + 1); }
              if (j < (int)o.n) s0 += a[j] * V.x.ld(j);
            } else {
              const double* a = o.w + (int64_t)t * o.n;
              for (; j + 1 < (int)o.n; j += 2) { s0 += gload(a + j) * V.x.ld(j); s1 += gload(a + j + 1) * V.x.ld(j + 1); }
              if (j < (int)o.n) s0 += gload(a + j) * V.x.ld(j);
            }
            V.out.st(t, s0 + s1);
          }
          break;
        }
        for (int64_t row0 = 0; row0 < o.n; row0 += TAIL_THREADS / 64) {
          const int64_t row = row0 + wave;
          double sum = 0.0;
          if (row < o.n) {
            const double* a = o.w + row * o.n;
            for (int64_t j = lane; j < o.n; j += 64) sum += gload(a + j) * V.x.ld(j);
          }
#pragma unroll
          for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off, 64);
          if (row < o.n && lane == 0) V.out.st(row, sum);
        }
        break;
      case T_DOT2: {   // dot2_partial_kernel's SCALE_BLOCKS blocks, four at a time
        // blocks past the data hold (0 + 0) + (0 + 0) = +0.0 in the launch
        // path: written directly, so only the blocks with rows loop and sync
        const int nbl = (int)std::min<int64_t>(SCALE_BLOCKS, (o.n + 255) / 256);
        for (int i = nbl + t; i < SCALE_BLOCKS; i += TAIL_THREADS) {
          V.part.st(2 * i, 0.0);
          V.part.st(2 * i + 1, 0.0);
        }
        for (int vb0 = 0; vb0 < nbl; vb0 += TAIL_THREADS / 256) {
          const int vb = vb0 + (t >> 8), tt = t & 255;
          double a = 0.0, c = 0.0;
          for (int64_t i = (int64_t)vb * 256 + tt; i < o.n; i += (int64_t)SCALE_BLOCKS * 256) {
            a += V.b.ld(i) * V.x.ld(i);
            c += V.y.ld(i) * V.x.ld(i);
          }
#pragma unroll
          for (int off = 32; off > 0; off >>= 1) {
            a += __shfl_xor(a, off, 64);
            c += __shfl_xor(c, off, 64);
          }
          if (lane == 0) { red[wave][0] = a; red[wave][1] = c; }
          __syncthreads();
          if (tt == 0 && vb < nbl) {
            const int w0 = (t >> 8) * 4;
            V.part.st(2 * vb, (red[w0][0] + red[w0 + 1][0]) + (red[w0 + 2][0] + red[w0 + 3][0]));
            V.part.st(2 * vb + 1, (red[w0][1] + red[w0 + 1][1]) + (red[w0 + 2][1] + red[w0 + 3][1]));
          }
          __syncthreads();
        }
        break;
      }
      case T_CSCALE: {   // cscale_kernel: alpha from the partials (one block's order), then scale
        __shared__ double alpha;
        if (t < 256) {
          double a = 0.0, c = 0.0;
          for (int i = t; i < SCALE_BLOCKS; i += 256) { a += V.part.ld(2 * i); c += V.part.ld(2 * i + 1); }
#pragma unroll
          for (int off = 32; off > 0; off >>= 1) {
            a += __shfl_xor(a, off, 64);
            c += __shfl_xor(c, off, 64);
          }
          if (lane == 0) { red[wave][0] = a; red[wave][1] = c; }
        }
        __syncthreads();
        if (t == 0) {
          const double num = (red[0][0] + red[1][0]) + (red[2][0] + red[3][0]);
          const double den = (red[0][1] + red[1][1]) + (red[2][1] + red[3][1]);
          alpha = den > 0.0 ? num / den : 1.0;
        }
        __syncthreads();
        const double al = alpha;
        for (int64_t i = t; i < o.n; i += TAIL_THREADS) V.out.st(i, al * V.out.ld(i));
        break;
      }
      case T_KDOT:
        if (KOPS) tail_kdot(o, lds, kred);
        break;
      case T_KORTH:
        if (KOPS) tail_korth(o, lds, kred);
        break;
      case T_KUPD:
        if (KOPS) tail_kupd(o, lds, kred);
        break;
      default: break;
    }
    __syncthreads();   // the next op reads what this one wrote (workgroup-scope visibility)
    if (STAMP && t == 0) { stamps[k + 1] = wall_clock64(); stamps[nops + 2 + k] = clock64(); }
  }
}

// one tail_kernel launch; flags bit 0: XL, bit 1: RES, bit 2: KOPS
template <bool STAMP>
void tail_launch(int flags, const TOp* prog, int n, int prog_lds, size_t lds, uint64_t* stamps, hipStream_t s) {
  switch (flags & 7) {
    case 4: tail_kernel<STAMP, false, false, true><<<1, TAIL_THREADS, lds, s>>>(prog, n, prog_lds, stamps); break;
    case 5: tail_kernel<STAMP, true, false, true><<<1, TAIL_THREADS, lds, s>>>(prog, n, prog_lds, stamps); break;
    case 6: tail_kernel<STAMP, false, true, true><<<1, TAIL_THREADS, lds, s>>>(prog, n, prog_lds, stamps); break;
    case 7: tail_kernel<STAMP, true, true, true><<<1, TAIL_THREADS, lds, s>>>(prog, n, prog_lds, stamps); break;
    case 0: tail_kernel<STAMP, false, false><<<1, TAIL_THREADS, lds, s>>>(prog, n, prog_lds, stamps); break;
    case 1: tail_kernel<STAMP, true, false><<<1, TAIL_THREADS, lds, s>>>(prog, n, prog_lds, stamps); break;
    case 2: tail_kernel<STAMP, false, true><<<1, TAIL_THREADS, lds, s>>>(prog, n, prog_lds, stamps); break;
    default: tail_kernel<STAMP, true, true><<<1, TAIL_THREADS, lds, s>>>(prog, n, prog_lds, stamps); break;
  }
}

__device__ __forceinline__ uint32_t hash32_dev(uint64_t i, int level) {   // = host.h hash32
  uint32_t x = (uint32_t)(i & 0xFFFFFFFFu);
  const uint32_t lv = (uint32_t)(((uint64_t)(int64_t)level * 0x85EBCA77ull) & 0xFFFFFFFFull);
  x = x * 0x9E3779B1u + lv;
  x ^= x >> 16;
  x *= 0x7FEB352Du;
  x ^= x >> 15;
  x *= 0x846CA68Bu;
  x ^= x >> 16;
  return x;
}
__device__ __forceinline__ uint64_t colour_key(int64_t I, int level) {
  return ((uint64_t)hash32_dev((uint64_t)I, level + 0x4000) << 32) | (uint64_t)(uint32_t)I;
}

// one round of the Jones-Plassmann colouring (mamg_oracle.jp_colouring): an
// uncoloured node whose key beats every uncoloured neighbour's takes the
// smallest colour no coloured neighbour holds.  Reads the previous round's
// colours (cin), writes the next (cout): winners of a round are never
// adjacent, so the result is independent of the visiting order.
__global__ __launch_bounds__(256) void jp_round_kernel(int64_t nr, const int64_t* __restrict__ ptr,
                                                       const int32_t* __restrict__ col, int level,
                                                       const int8_t* __restrict__ cin, int8_t* __restrict__ cout,
                                                       unsigned long long* nleft, int* toomany) {
  const int64_t I = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (I >= nr) return;
  const int8_t ci = cin[I];
  if (ci >= 0) { cout[I] = ci; return; }
  const uint64_t key = colour_key(I, level);
  uint64_t nbmax = 0, mask = 0;
  for (int64_t k = ptr[I]; k < ptr[I + 1]; ++k) {
    const int32_t J = col[k];
    if (J == I) continue;
    const int8_t cj = cin[J];
    if (cj < 0) {
      const uint64_t kj = colour_key(J, level);
      nbmax = kj > nbmax ? kj : nbmax;
    } else {
      mask |= 1ull << cj;
    }
  }
  if (key > nbmax) {
    if (~mask == 0ull) { *toomany = 1; cout[I] = 0; }
    else cout[I] = (int8_t)(__ffsll((long long)~mask) - 1);
  } else {
    cout[I] = -1;
    atomicAdd(nleft, 1ull);
  }
}

// the colouring needs an undirected node graph: every block (I, J) must have
// its mirror (J, I) (binary search in row J)
__global__ __launch_bounds__(256) void pattern_sym_kernel(int64_t nr, const int64_t* __restrict__ ptr,
                                                          const int32_t* __restrict__ col, int* bad) {
  const int64_t I = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (I >= nr) return;
  for (int64_t k = ptr[I]; k < ptr[I + 1]; ++k) {
    const int32_t J = col[k];
    int64_t lo = ptr[J], hi = ptr[J + 1];
    while (lo < hi) {
      const int64_t m = (lo + hi) >> 1;
      if (col[m] < I) lo = m + 1; else hi = m;
    }
    if (lo >= ptr[J + 1] || col[lo] != I) { *bad = 1; return; }
  }
}

__global__ __launch_bounds__(256) void colour_count_kernel(int64_t nr, const int8_t* __restrict__ c,
                                                           int32_t* __restrict__ ci, int64_t* __restrict__ iota,
                                                           unsigned long long* cnt) {
  __shared__ unsigned int hist[64];
  if (threadIdx.x < 64) hist[threadIdx.x] = 0;
  __syncthreads();
  const int64_t I = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (I < nr) {
    ci[I] = c[I];
    iota[I] = I;
    atomicAdd(&hist[c[I]], 1u);
  }
  __syncthreads();
  if (threadIdx.x < 64 && hist[threadIdx.x]) atomicAdd(cnt + threadIdx.x, (unsigned long long)hist[threadIdx.x]);
}

// sorted position k (colour c = cs[k]) -> padded permuted row pcs[c] + k - gcs[c]
__global__ __launch_bounds__(256) void perm_place_kernel(int64_t nr, const int32_t* __restrict__ cs,
                                                         const int64_t* __restrict__ sorted,
                                                         const int64_t* __restrict__ gcs,
                                                         const int64_t* __restrict__ pcs, int32_t* __restrict__ perm) {
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (k >= nr) return;
  const int c = cs[k];
  perm[pcs[c] + k - gcs[c]] = (int32_t)sorted[k];
}

__global__ __launch_bounds__(256) void perm_len_kernel(int64_t nrp, const int32_t* __restrict__ perm,
                                                       const int64_t* __restrict__ ptr, int64_t* __restrict__ gptr) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= nrp) return;
  const int32_t I = perm[i];
  gptr[i + 1] = I < 0 ? 0 : ptr[I + 1] - ptr[I];
}

// ---------------------------------------------------------------------------
// Multiplicative node-patch Schwarz on level 0 (Schwarz_type PATCHES): the
// reference's level-0 smoother, symmetric multiplicative Schwarz on one block
// per seed = seed + its 1-ring (src/amg_parameters.py:83-87, src/utils.py:84)
// with exact local solves.  With a seed on every node (the bidomain's u2
// dofs, src/bidomain_3d.py:138) the block of node I is both fields of the
// closed neighbourhood N[I] = row I of A_0's node pattern.  Parallel order:
// patches coloured at distance 3 (two patch centres of one colour are >= 4
// hops apart: no patch of a launch reads an x another one writes).
// Oracle: mamg_oracle.Patches (colouring, inverses, sweep).
// ---------------------------------------------------------------------------
constexpr int PATCH_WORDS = 4;          // 256 colours

__device__ __forceinline__ uint64_t patch_key_dev(int64_t I) {
  return ((uint64_t)hash32_dev((uint64_t)I, 0x5000) << 32) | (uint64_t)(uint32_t)I;
}

// k[I] = key(I) while I is uncoloured, else 0
__global__ __launch_bounds__(256) void pkey_init_kernel(int64_t nr, const int16_t* __restrict__ c, uint64_t* __restrict__ k) {
  const int64_t I = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (I < nr) k[I] = c[I] < 0 ? patch_key_dev(I) : 0ull;
}

// out[I] = max of in over row I's node columns and I itself (one hop)
__global__ __launch_bounds__(256) void pkey_max_kernel(int64_t nr, const int64_t* __restrict__ ptr,
                                                       const int32_t* __restrict__ col, const uint64_t* __restrict__ in,
                                                       uint64_t* __restrict__ out) {
  const int64_t I = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (I >= nr) return;
  uint64_t m = in[I];
  for (int64_t k = ptr[I]; k < ptr[I + 1]; ++k) {
    const uint64_t v = in[col[k]];
    m = v > m ? v : m;
  }
  out[I] = m;
}

// ---- distance-3 Jones-Plassmann colouring (mamg_oracle.patch_colouring) -----
// Round-synchronous: an uncoloured node whose key is the largest uncoloured
// key within 3 hops takes the lowest colour absent within 3 hops.  That
// colours a node once every higher-keyed node within 3 hops is coloured, so
// the result is the greedy colouring in descending key order whatever the
// schedule.  Rounds 2-4 recomputed every node's 3-hop maxima and 256-bit
// colour masks each round by three full key-max and three full mask-or passes
// (12 ms per round, 341 rounds at nrefs=6: 4.2 s of the patch layout).  Since
// round 5 each round keeps, per node, the 1-, 2- and
// 3-hop maxima m1, m2, m3 of the uncoloured keys and a 1-hop colour mask:
//  * a maximum changes only when the node it names (the key's low 32 bits)
//    gets coloured, so each round re-derives just those entries (lazy refresh,
//    one level from the one below, closed neighbourhoods);
//  * a winner (m3 == own key) ORs the 1-hop masks of its 2-hop ball (= the
//    colours within 3 hops) and adds its colour bit to its neighbours' 1-hop
//    masks: two winners are > 3 hops apart, so no winner sees another's bit.
// Same keys, same rounds, same colours (tests/test_gpu_patch.py).

// m[I] refreshed from src (src == nullptr: the keys of uncoloured nodes):
// kept unless the node it names was coloured.  FIND (the 3-hop level, 1024
// threads): only uncoloured nodes, and those whose maximum is their own key
// are appended to the winner list, one atomic per workgroup.  No winner means
// no uncoloured node (the largest uncoloured key always wins).
// whether node x is coloured: one bit per node (round 6), so the lookups of
// the nodes the maxima name hit the 2 MB bitmap in L2 instead of gathering
// 2-byte colours from a 34 MB array (the same tests, the same colours)
__device__ __forceinline__ bool coloured(const uint32_t* __restrict__ cb, int64_t x) {
  return (cb[x >> 5] >> (x & 31)) & 1u;
}

template <bool FIND>
__global__ __launch_bounds__(FIND ? 1024 : 256) void pkey_refresh_kernel(
    int64_t nr, const int64_t* __restrict__ ptr, const int32_t* __restrict__ col, const uint32_t* __restrict__ cb,
    const uint64_t* __restrict__ src, uint64_t* __restrict__ m, int32_t* __restrict__ win,
    unsigned int* __restrict__ nwin) {
  constexpr int NT = FIND ? 1024 : 256;
  const int64_t I = (int64_t)blockIdx.x * NT + threadIdx.x;
  bool w = false;
  if (I < nr) {
    const bool unc = !coloured(cb, I);
    uint64_t v = m[I];
    if ((!FIND || unc) && v != 0 && coloured(cb, (uint32_t)v)) {   // its maximum was coloured: recompute
      // rows hold <= PATCH_MAX_NODES columns (build_patches checks): every
      // column load, then every gather, in flight together
      v = src ? src[I] : (unc ? patch_key_dev(I) : 0ull);
      const int64_t k0 = ptr[I];
      const int len = (int)(ptr[I + 1] - k0);
      int32_t J[PATCH_MAX_NODES];
#pragma unroll
      for (int q = 0; q < PATCH_MAX_NODES; ++q) J[q] = q < len ? col[k0 + q] : (int32_t)I;
#pragma unroll
      for (int q = 0; q < PATCH_MAX_NODES; ++q) {
        const uint64_t u = src ? src[J[q]] : (!coloured(cb, J[q]) ? patch_key_dev(J[q]) : 0ull);
        v = u > v ? u : v;
      }
      m[I] = v;
    }
    w = FIND && unc && v == patch_key_dev(I);
  }
  if constexpr (FIND) {   // workgroup-aggregated list appends
    __shared__ unsigned int wc[NT / 64 + 1];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const unsigned long long bw = __ballot(w);
    if (lane == 0) wc[wv] = (unsigned int)__popcll(bw);
    __syncthreads();
    if (threadIdx.x == 0) {
      unsigned int t = 0;
      for (int k = 0; k < NT / 64; ++k) { const unsigned int x = wc[k]; wc[k] = t; t += x; }
      wc[NT / 64] = t ? atomicAdd(nwin, t) : 0u;
    }
    __syncthreads();
    if (w) win[wc[NT / 64] + wc[wv] + __popcll(bw & ((1ull << lane) - 1))] = (int32_t)I;
  }
}

// one wave per winner: the colours within 3 hops = OR of the 1-hop masks over
// the closed 2-hop ball; the lowest free colour; the colour bit into the
// 1-hop masks of the closed 1-ring
__global__ __launch_bounds__(256) void patch_win_kernel(int64_t nwin, const int32_t* __restrict__ win,
                                                        const int64_t* __restrict__ ptr, const int32_t* __restrict__ col,
                                                        int16_t* __restrict__ c, uint32_t* __restrict__ cb,
                                                        unsigned long long* __restrict__ mask1, int* toomany) {
  const int64_t t = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (t >= nwin) return;
  const int64_t I = win[t];
  const int64_t p0 = ptr[I];
  const int d1 = (int)(ptr[I + 1] - p0) + 1;     // closed 1-ring: row I's columns, then I
  // lane a < d1 holds the ring's a-th member u and u's row range
  int64_t u = I, q0 = 0;
  int lu = 0;
  if (lane < d1) {
    if (lane + 1 < d1) u = col[p0 + lane];
    q0 = ptr[u];
    lu = (int)(ptr[u + 1] - q0) + 1;             // closed: u's columns, then u
  }
  unsigned long long mk[PATCH_WORDS] = {0ull, 0ull, 0ull, 0ull};
  // (a, b) pairs, 4 members of the ring at a time and 16 lanes per member
  for (int a0 = 0; a0 < d1; a0 += 4) {
    const int a = a0 + (lane >> 4);
    const int64_t ua = __shfl(u, a & 63), qa = __shfl(q0, a & 63);
    const int la = __shfl(lu, a & 63);
    if (a < d1)
      for (int b = lane & 15; b < la; b += 16) {
        const int64_t x = b + 1 < la ? (int64_t)col[qa + b] : ua;
#pragma unroll
        for (int w = 0; w < PATCH_WORDS; ++w) mk[w] |= mask1[PATCH_WORDS * x + w];
      }
  }
#pragma unroll
  for (int w = 0; w < PATCH_WORDS; ++w)
    for (int o = 32; o > 0; o >>= 1) mk[w] |= __shfl_xor(mk[w], o);
  int cc = -1;
  for (int w = 0; w < PATCH_WORDS && cc < 0; ++w)
    if (~mk[w]) cc = 64 * w + __ffsll((long long)~mk[w]) - 1;
  if (cc < 0) {
    if (lane == 0) *toomany = 1;
    cc = 0;
  }
  if (lane == 0) {
    c[I] = (int16_t)cc;
    atomicOr(&cb[I >> 5], 1u << (I & 31));
  }
  if (lane < d1) atomicOr(&mask1[PATCH_WORDS * u + cc / 64], 1ull << (cc % 64));
}

__global__ __launch_bounds__(256) void pcolour_count_kernel(int64_t nr, const int16_t* __restrict__ c,
                                                            int32_t* __restrict__ ci, int64_t* __restrict__ iota,
                                                            unsigned long long* cnt) {
  __shared__ unsigned int hist[64 * PATCH_WORDS];
  hist[threadIdx.x] = 0;
  __syncthreads();
  const int64_t I = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (I < nr) {
    ci[I] = c[I];
    iota[I] = I;
    atomicAdd(&hist[c[I]], 1u);
  }
  __syncthreads();
  if (hist[threadIdx.x]) atomicAdd(cnt + threadIdx.x, (unsigned long long)hist[threadIdx.x]);
}

__global__ __launch_bounds__(256) void patch_rowlen_kernel(int64_t nr, const int64_t* __restrict__ ptr, int* maxlen) {
  const int64_t I = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (I < nr) atomicMax(maxlen, (int)(ptr[I + 1] - ptr[I]));
}

__global__ __launch_bounds__(256) void i64_to_i32_kernel(int64_t n, const int64_t* __restrict__ a, int32_t* __restrict__ b) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) b[i] = (int32_t)a[i];
}

// column-packed upper triangle: U(i, j), i <= j, at j (j + 1) / 2 + i
__device__ __forceinline__ int upk(int i, int j) { return i <= j ? j * (j + 1) / 2 + i : i * (i + 1) / 2 + j; }

// lane src's double (src may differ per lane): two ds_bpermute_b32
__device__ __forceinline__ double bperm_f64(double v, int src) {
  const unsigned long long u = (unsigned long long)__double_as_longlong(v);
  const int lo = __builtin_amdgcn_ds_bpermute(src << 2, (int)(unsigned)u);
  const int hi = __builtin_amdgcn_ds_bpermute(src << 2, (int)(unsigned)(u >> 32));
  return __longlong_as_double((long long)(((unsigned long long)(unsigned)hi << 32) | (unsigned)lo));
}
// lane l's double, broadcast to the wave (l wave-uniform)
__device__ __forceinline__ double readlane_f64(double v, int l) {
  const unsigned long long u = (unsigned long long)__double_as_longlong(v);
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)u, l);
  const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(u >> 32), l);
  return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

// Patch inverses, one wave per patch (4 per workgroup).  Lane j < 2d holds
// column j of the augmented [A_p | I] (d = 2 m <= 32 rows in registers; local
// dof i = 2 a + f, a = the node's position in row I, f = field).  Gauss-Jordan
// without pivoting in mamg_oracle.batched_inverse's operation order (row k
// divided by the pivot, then M_i -= M_ik M_k, no contraction); the packed
// upper triangle of the inverse is stored (the oracle symmetrises the same).
// gcol: the rows' columns as global node ids, sorted per row (the search
// keys; = col on one GPU, the rank-local rows keep the global column order
// with local indices in col on N GPUs)
__global__ __launch_bounds__(256) void patch_inv_kernel(int64_t np, const int32_t* __restrict__ perm,
                                                        const int64_t* __restrict__ ptr, const int32_t* __restrict__ col,
                                                        const int32_t* __restrict__ gcol,
                                                        const dv4* __restrict__ val, int64_t ustride, double* __restrict__ U,
                                                        int* bad) {
#pragma clang fp contract(off)
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t i = (int64_t)blockIdx.x * 4 + wv;
  if (i >= np) return;
  const int32_t I = perm[i];
  const int64_t q0 = ptr[I];
  const int m = (int)(ptr[I + 1] - q0);
  const int d = 2 * m;
  double M[2 * PATCH_MAX_NODES];
#pragma unroll
  for (int r = 0; r < 2 * PATCH_MAX_NODES; ++r) M[r] = 0.0;
  if (lane < d) {
    const int32_t Jb = gcol[q0 + (lane >> 1)];
    const int g = lane & 1;
#pragma unroll
    for (int a = 0; a < PATCH_MAX_NODES; ++a) {
      if (a < m) {
        const int32_t Ja = col[q0 + a];
        int64_t lo = ptr[Ja], hi = ptr[Ja + 1];
        while (lo < hi) {
          const int64_t md = (lo + hi) >> 1;
          if (gcol[md] < Jb) lo = md + 1; else hi = md;
        }
        if (lo < ptr[Ja + 1] && gcol[lo] == Jb) {
          const dv4 v = val[lo];
          M[2 * a] = g ? v.y : v.x;
          M[2 * a + 1] = g ? v.w : v.z;
        }
      }
    }
  } else {
#pragma unroll
    for (int r = 0; r < 2 * PATCH_MAX_NODES; ++r) M[r] = (lane - d == r) ? 1.0 : 0.0;
  }
  // pivots unrolled (k a constant: no register selects), the pivot column's
  // entries broadcast from lane k by v_readlane rather than LDS permutes: the
  // same operations on the same values as the loop of rounds 2-4
  // (300 -> see DESIGN.md 2.11 for the measured time)
#pragma unroll
  for (int k = 0; k < 2 * PATCH_MAX_NODES; ++k) {
    if (k < d) {
      const double p = readlane_f64(M[k], k);
      if (!(p > 0.0)) { if (lane == 0) atomicOr(bad, 1); return; }
      const double mk = M[k] / p;
#pragma unroll
      for (int r = 0; r < 2 * PATCH_MAX_NODES; ++r) {
        if (r == k) continue;
        const double f = readlane_f64(M[r], k);
        const double t = f * mk;
        M[r] = M[r] - t;
      }
      M[k] = mk;
    }
  }
  if (lane >= d && lane < 2 * d) {
    const int jj = lane - d;
    double* Up = U + i * ustride + jj * (jj + 1) / 2;
#pragma unroll
    for (int r = 0; r < 2 * PATCH_MAX_NODES; ++r)
      if (r <= jj) Up[r] = M[r];
  }
}

// ---- patch matrices through LDS (round 6): the assembly and the packed
// store of the patch inverse kernels.  A patch's 32 x 32 matrix (zero past
// d, the identity on the padded diagonal when `pad`) sits column-major with
// stride PATCH_LD doubles (33: the tile reads of patch_inv3_kernel hit 32
// banks).
constexpr int PATCH_LD = 33;

// Assembly by rows: the patch's nl lanes take its row nodes, L = nl / 16
// lanes per row node a (Ja = the centre row's a-th column) and the patch
// nodes b = q, q + L, .. of lane q; each lane loads Ja's <= 16 keys at once,
// finds its nodes' keys among them by comparisons in registers, then loads
// the found blocks at once: three dependent loads instead of one five-step
// binary search per (row, column) pair.  A pair absent from Ja's row stays 0.
// The values are copies: the assembled matrix is the one the searches built.
template <int L>
__device__ __forceinline__ void patch_assemble(double* S, int sub, int q0i, int64_t q0, int m, bool pad,
                                               const int64_t* __restrict__ ptr, const int32_t* __restrict__ col,
                                               const int32_t* __restrict__ gcol, const dv4* __restrict__ val) {
  (void)q0i;
  constexpr int nl = 16 * L, NB = PATCH_MAX_NODES / L;
  const int d = 2 * m;
  for (int k = sub; k < 32 * PATCH_LD; k += nl) {
    const int j = k / PATCH_LD, r = k - j * PATCH_LD;
    S[k] = (pad && r == j && j >= d) ? 1.0 : 0.0;
  }
  const int a = sub / L, q = sub % L;
  if (a >= m) return;
  const int32_t Ja = col[q0 + a];
  const int64_t p0 = ptr[Ja];
  const int n = (int)(ptr[Ja + 1] - p0);
  int32_t kr[PATCH_MAX_NODES], kb[NB];
#pragma unroll
  for (int k = 0; k < PATCH_MAX_NODES; ++k) kr[k] = k < n ? gcol[p0 + k] : -1;
#pragma unroll
  for (int t = 0; t < NB; ++t) kb[t] = q + L * t < m ? gcol[q0 + q + L * t] : -2;
  int pos[NB];
#pragma unroll
  for (int t = 0; t < NB; ++t) {
    int x = -1;
#pragma unroll
    for (int k = 0; k < PATCH_MAX_NODES; ++k) x = kr[k] == kb[t] ? k : x;
    pos[t] = x;
  }
  dv4 v[NB];
#pragma unroll
  for (int t = 0; t < NB; ++t) v[t] = pos[t] >= 0 ? val[p0 + pos[t]] : dv4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int t = 0; t < NB; ++t)
    if (pos[t] >= 0) {
      const int b = q + L * t;
      double* c0 = S + (2 * b) * PATCH_LD + 2 * a;
      double* c1 = c0 + PATCH_LD;
      c0[0] = v[t].x; c1[0] = v[t].y; c0[1] = v[t].z; c1[1] = v[t].w;
    }
}

// the packed upper triangle (column j: rows 0 .. j, at j (j + 1) / 2) of
// sign * the LDS matrix, written by nl lanes with consecutive addresses
__device__ __forceinline__ void patch_store(const double* S, int sub, int nl, int d, double sign, double* __restrict__ Up) {
  const int nt = d * (d + 1) / 2;
  for (int k = sub; k < nt; k += nl) {
    int j = (int)((sqrtf(8.0f * (float)k + 1.0f) - 1.0f) * 0.5f);
    j += (j + 1) * (j + 2) / 2 <= k ? 1 : 0;
    j -= j * (j + 1) / 2 > k ? 1 : 0;
    Up[k] = sign * S[j * PATCH_LD + (k - j * (j + 1) / 2)];
  }
}

// Patch inverses, two patches per wave (round 6): the same
// operations on the same values as patch_inv_kernel, so the same bits, with
// half the instructions per patch.
//  * In place: half-wave h (lanes 32 h .. 32 h + 31) holds one patch, lane j
//    < d column j of A_p (d = 2 m <= 32).  At pivot k, column k of the
//    augmented [A_p | I] becomes e_k and identity column k is e_k until then
//    (exactly: every update of it adds -(f x +0) = +0), so lane k takes
//    over identity column k: row k = 1 / p, row r = 0 - f_r (1 / p), the
//    augmented code's own operations on it.  The other lanes update as
//    before (row k divided by the pivot, then M_r -= f_r M_k, no
//    contraction); f_r = column k's row r, broadcast within the half by
//    ds_bpermute (one instruction serves both patches) before lane k
//    overwrites it.
//  * Assembly: each lane's block searches in the patch rows run as
//    PATCH_MAX_NODES independent branch-free binary searches (5 steps for
//    rows of <= 16 blocks, every load in bounds), one straight-line block
//    whose loads overlap, instead of one data-dependent loop per row after
//    another.
//  * The pivot and row loops are fully unrolled (a partly rolled loop put M
//    in scratch: 272 B per lane, 1.8 s at nrefs=6).
__global__ __launch_bounds__(256) void patch_inv2_kernel(int64_t np, const int32_t* __restrict__ perm,
                                                         const int64_t* __restrict__ ptr, const int32_t* __restrict__ col,
                                                         const int32_t* __restrict__ gcol,
                                                         const dv4* __restrict__ val, int64_t ustride, double* __restrict__ U,
                                                         int* bad) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63, hl = lane & 31, hb = lane & 32;
  const int64_t i = (int64_t)blockIdx.x * 8 + (threadIdx.x >> 6) * 2 + (lane >> 5);
  const bool live = i < np;
  const int32_t I = live ? perm[i] : 0;
  const int64_t q0 = ptr[I];
  const int m = live ? (int)(ptr[I + 1] - q0) : 0;
  const int d = 2 * m;
  double M[2 * PATCH_MAX_NODES];
#pragma unroll
  for (int r = 0; r < 2 * PATCH_MAX_NODES; ++r) M[r] = 0.0;
  if (hl < d) {
    const int32_t Jb = gcol[q0 + (hl >> 1)];
    const int g = hl & 1;
    // each row's lower bound of Jb by a branch-free 5-step binary search
    // (rows of <= 16 blocks), every load in bounds, so the rows' searches
    // form one straight-line block and their loads overlap
#pragma unroll
    for (int a = 0; a < PATCH_MAX_NODES; ++a) {
      const bool va = a < m;
      const int32_t Ja = va ? col[q0 + a] : I;
      const int64_t p0 = ptr[Ja];
      const int n = va ? (int)(ptr[Ja + 1] - p0) : 0;
      int64_t b = p0;
      int l = n;
#pragma unroll
      for (int st = 0; st < 5; ++st) {
        const int h = l >> 1;
        const bool lt = gcol[l > 0 ? b + h : p0] < Jb;
        b = (l > 0 && lt) ? b + h + 1 : b;
        l = l > 0 ? (lt ? l - h - 1 : h) : 0;
      }
      if (va && b < p0 + n && gcol[b] == Jb) {
        const dv4 v = val[b];
        M[2 * a] = g ? v.y : v.x;
        M[2 * a + 1] = g ? v.w : v.z;
      }
    }
  }
  bool ok = true;
#pragma clang loop unroll(full)
  for (int k = 0; k < 2 * PATCH_MAX_NODES; ++k) {
    // every lane takes part in the broadcasts (the other half may have k < d)
    const double p = bperm_f64(M[k], hb + k);
    const bool act = k < d && ok;
    if (act && !(p > 0.0)) ok = false;
    const bool upd = act && ok && hl < d;
    const bool own = hl == k;
    const double mk = own ? 1.0 / p : M[k] / p;
#pragma clang loop unroll(full)
    for (int r = 0; r < 2 * PATCH_MAX_NODES; ++r) {
      if (r == k) continue;
      const double f = bperm_f64(M[r], hb + k);
      const double t = f * mk;
      if (upd) M[r] = (own ? 0.0 : M[r]) - t;
    }
    if (upd) M[k] = mk;
  }
  if (!ok && hl == 0) atomicOr(bad, 1);
  if (live && ok && hl < d) {
    double* Up = U + i * ustride + hl * (hl + 1) / 2;
#pragma unroll
    for (int r = 0; r < 2 * PATCH_MAX_NODES; ++r)
      if (r <= hl) Up[r] = M[r];
  }
}

// Patch inverses on the matrix cores (round 6):
// one patch per wave, the 32 x 32 (zero-padded to the identity past d)
// patch matrix as four 16 x 16 f64 tiles in the v_mfma_f64_16x16x4 C/D
// layout (lane l, register r: row 16a + (l >> 4) + 4r, column 16b + (l & 15)),
// inverted by the symmetric block sweep on 4 x 4 pivot blocks K:
//   P = M(K, K), R = M(K, :), S = P^-1 R               (one MFMA per tile column)
//   M(i, j) -= S(:, i)^T R(:, j)  for all i, j          (four MFMAs: the A operand
//                                                        is S itself, the B operand R
//                                                        itself -- no data movement)
//   M(K, :) = S, M(:, K) = S^T (ds_bpermute), M(K, K) = -P^-1,
// which leaves M = -A_p^-1 after the eight blocks (Goodnight's sweep;
// symmetry is what makes the column panel S^T, so the row panel alone feeds
// both operands).  A_p is SPD, so no pivoting: a non-positive pivot of a 4 x 4
// block sets *bad as the scalar kernels do.  Assembly as patch_inv2_kernel
// (lane j < 32 builds column j), then an LDS transpose into the tile layout.
// The rounding differs from the scalar Gauss-Jordan: the inverses equal
// patch_inv2_kernel's to ~1e-14 relative (tests/test_gpu_patch.py).
// PART (diagnosis build only, MAMG_PATCH_INV 4 / 5): 1 = assembly and
// stores without the sweep, 2 = the sweep on the identity without assembly
// Waves take patches in colour order, so the 4.2 KB inverses are written in
// address order.  (Node order -- neighbouring patches, whose rows overlap,
// assembled together from L2 -- was 1.3 ms faster in a fresh process but
// 2.9 s slower in a process that had just freed another 63 GB inverse array:
// writes scattered over 72 GB)
template <int PART = 0>
__global__ __launch_bounds__(256, 4) void patch_inv3_kernel(int64_t np, const int32_t* __restrict__ perm,
                                                         const int64_t* __restrict__ ptr, const int32_t* __restrict__ col,
                                                         const int32_t* __restrict__ gcol,
                                                         const dv4* __restrict__ val, int64_t ustride, double* __restrict__ U,
                                                         int* bad) {
  constexpr int LD = PATCH_LD;
  __shared__ double sm[4][32 * LD];
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, lr = lane >> 4, lc = lane & 15;
  const int64_t i = (int64_t)blockIdx.x * 4 + w;
  const bool live = i < np;
  const int32_t I = live ? perm[i] : 0;
  const int64_t q0 = ptr[I];
  const int m = live ? (int)(ptr[I + 1] - q0) : 0;
  const int d = 2 * m;
  double* S = sm[w];
  if (PART == 2) {   // diagnosis: the identity
    for (int k = lane; k < 32 * LD; k += 64) S[k] = (k % LD == k / LD) ? 1.0 : 0.0;
  } else {
    patch_assemble<4>(S, lane, 0, q0, m, true, ptr, col, gcol, val);
  }
  __syncthreads();
  dv4 T[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int r = 0; r < 4; ++r) T[a][b][r] = S[(16 * b + lc) * LD + 16 * a + lr + 4 * r];
  bool ok = true;
#pragma unroll
  for (int K = 0; K < (PART == 1 ? 0 : 8); ++K) {
    const int t = K >> 2, rr = K & 3;
    // the pivot block spread over 16 lanes: lane l holds Q(l & 15, l >> 4)
    // for (l & 15) < 4 (P(kk, c) sits in lane 16 kk + 4 rr + c of T[t][t][rr]),
    // swept in place (Q <- -P^-1): per pivot one broadcast and two permutes
    const bool qv = lc < 4;
    double Q = bperm_f64(T[t][t][rr], qv ? 16 * lc + 4 * rr + lr : lane);
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const double dp = readlane_f64(Q, 17 * p);
      ok = ok && dp > 0.0;
      // 1 / dp: v_rcp_f64 and two Newton steps (the IEEE division sequence
      // is a 10-deep dependent chain, four per block)
      double inv = __builtin_amdgcn_rcp(dp);
      inv = fma(inv, fma(-dp, inv, 1.0), inv);
      inv = fma(inv, fma(-dp, inv, 1.0), inv);
      const double qrp = bperm_f64(Q, 16 * p + lc), qpc = bperm_f64(Q, 16 * lr + p);
      const bool rp = lc == p, cp = lr == p;
      // every candidate computed, then selected (no divergent branches)
      const double upd = Q - qrp * qpc * inv, scl = Q * inv;
      const double q1 = (rp || cp) ? scl : upd;
      Q = (rp && cp) ? -inv : q1;
    }
    // A operand of S = P^-1 R: lane l holds (P^-1)(l & 15, l >> 4) for (l & 15) < 4, else 0
    const double pa = qv ? -Q : 0.0;
    const double R0 = T[t][0][rr], R1 = T[t][1][rr];
    const dv4 z = {0.0, 0.0, 0.0, 0.0};
    const double S0 = __builtin_amdgcn_mfma_f64_16x16x4f64(pa, R0, z, 0, 0, 0)[0];   // S(lr, lc) of column tile 0
    const double S1 = __builtin_amdgcn_mfma_f64_16x16x4f64(pa, R1, z, 0, 0, 0)[0];
    // M -= S^T R on every tile (rows and columns K are rewritten below)
#pragma unroll
    for (int a = 0; a < 2; ++a) {
      const double sa = a ? -S1 : -S0;
      T[a][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(sa, R0, T[a][0], 0, 0, 0);
      T[a][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(sa, R1, T[a][1], 0, 0, 0);
    }
    // row panel K <- S (the same lanes), column panel K <- S^T
    T[t][0][rr] = S0;
    T[t][1][rr] = S1;
    const bool inK = lc >= 4 * rr && lc < 4 * rr + 4;
    const int kk = inK ? lc - 4 * rr : 0;
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const double v = bperm_f64(a ? S1 : S0, 16 * kk + lr + 4 * r);
        T[a][t][r] = inK ? v : T[a][t][r];
      }
    // pivot block K <- -P^-1 (= Q): (lr, kk) from lane 16 kk + lr
    const double qk = bperm_f64(Q, 16 * kk + lr);
    T[t][t][rr] = inK ? qk : T[t][t][rr];
  }
  if (!ok && lane == 0 && live) atomicOr(bad, 1);
  // M = -A_p^-1: the tiles back into LDS, then the packed upper triangle of -M
  __syncthreads();
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int r = 0; r < 4; ++r) S[(16 * b + lc) * LD + 16 * a + lr + 4 * r] = T[a][b][r];
  __syncthreads();
  if (live && ok) patch_store(S, lane, 64, d, -1.0, U + i * ustride);
}

}  // namespace

// version (MAMG_PATCH_INV): 1 the round-5 kernel (one patch per wave), 2 two
// patches per wave (bitwise the same), default 3 the matrix-core block sweep
void launch_patch_inv(int version, int64_t np, const int32_t* perm, const int64_t* ptr, const int32_t* col,
                      const int32_t* gcol, const dv4* val, int64_t ustride, double* U, int* bad) {
  if (np <= 0) return;
  switch (version) {
    case 1: patch_inv_kernel<<<(unsigned)((np + 3) / 4), 256>>>(np, perm, ptr, col, gcol, val, ustride, U, bad); break;
    case 2: patch_inv2_kernel<<<(unsigned)((np + 7) / 8), 256>>>(np, perm, ptr, col, gcol, val, ustride, U, bad); break;
#if MAMG_DIAG
    case 4: patch_inv3_kernel<1><<<(unsigned)((np + 3) / 4), 256>>>(np, perm, ptr, col, gcol, val, ustride, U, bad); break;
    case 5: patch_inv3_kernel<2><<<(unsigned)((np + 3) / 4), 256>>>(np, perm, ptr, col, gcol, val, ustride, U, bad); break;
#endif
    default: patch_inv3_kernel<<<(unsigned)((np + 3) / 4), 256>>>(np, perm, ptr, col, gcol, val, ustride, U, bad); break;
  }
}

namespace {

// One colour of a patch sweep, one wave per patch (4 per workgroup), in place
// on x (node-interleaved):  x|_p += Minv_p (b - A x)|_p.  The patch's node rows
// are reduced by 4 lanes each (lanes 4a..4a+3 = node a); lane i < d then forms
// delta_i = sum_j U(min, max) r_j and updates its own dof.  b has field stride
// bs (the caller's [u1; u2] r on level 0).
__global__ __launch_bounds__(256) void patch_kernel(int64_t c0, int64_t c1, const int32_t* __restrict__ perm,
                                                    const int64_t* __restrict__ ptr, const int32_t* __restrict__ col,
                                                    const dv4* __restrict__ val, const double* __restrict__ U,
                                                    int64_t ustride, double* x, const double* __restrict__ b, int64_t bs) {
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t i = c0 + (int64_t)blockIdx.x * 4 + wv;
  if (i >= c1) return;
  const int32_t I = perm[i];
  const int64_t q0 = ptr[I];
  const int m = (int)(ptr[I + 1] - q0);
  const int a = lane >> 2, q = lane & 3;
  const double2* x2 = reinterpret_cast<const double2*>(x);
  // this lane's row of the packed inverse, loaded up front: it does not
  // depend on the residual, so its latency overlaps the row gathers
  const double* Up = U + i * ustride;
  const int li = lane < 2 * m ? lane : 0;
  double u[2 * PATCH_MAX_NODES];
#pragma unroll
  for (int j = 0; j < 2 * PATCH_MAX_NODES; ++j) u[j] = j < 2 * m ? Up[upk(li, j)] : 0.0;
  // node a's row, blocks q, q + 4, q + 8, q + 12 (a row has <= PATCH_MAX_NODES
  // blocks): loads first, then gathers, then the sums in block order
  double s0 = 0.0, s1 = 0.0;
  int32_t J = 0;
  if (a < m) {
    J = col[q0 + a];
    const int64_t p0 = ptr[J], p1 = ptr[J + 1];
    int32_t c[PATCH_MAX_NODES / 4];
    dv4 v[PATCH_MAX_NODES / 4];
    double2 xc[PATCH_MAX_NODES / 4];
#pragma unroll
    for (int t = 0; t < PATCH_MAX_NODES / 4; ++t) {
      const int64_t k = p0 + q + 4 * t;
      const int64_t kk = k < p1 ? k : p0;
      c[t] = col[kk];
      v[t] = val[kk];
    }
#pragma unroll
    for (int t = 0; t < PATCH_MAX_NODES / 4; ++t) xc[t] = x2[c[t]];
#pragma unroll
    for (int t = 0; t < PATCH_MAX_NODES / 4; ++t)
      if (p0 + q + 4 * t < p1) {
        s0 += v[t].x * xc[t].x + v[t].y * xc[t].y;
        s1 += v[t].z * xc[t].x + v[t].w * xc[t].y;
      }
  }
  s0 += __shfl_xor(s0, 1);
  s1 += __shfl_xor(s1, 1);
  s0 += __shfl_xor(s0, 2);
  s1 += __shfl_xor(s1, 2);
  double r0 = 0.0, r1 = 0.0;
  if (a < m) {
    r0 = vget(b, bs, J, 0) - s0;
    r1 = vget(b, bs, J, 1) - s1;
  }
  double delta = 0.0;
#pragma unroll
  for (int jn = 0; jn < PATCH_MAX_NODES; ++jn) {
    const double a0 = __shfl(r0, 4 * jn), a1 = __shfl(r1, 4 * jn);
    if (jn < m) delta += u[2 * jn] * a0 + u[2 * jn + 1] * a1;
  }
  if (lane < 2 * m) {
    const int64_t Ji = col[q0 + (lane >> 1)];
    x[2 * Ji + (lane & 1)] += delta;
  }
}

// ---------------------------------------------------------------------------
// Multiplicative seed-ring Schwarz (Schwarz_type RINGS, level 0): the
// reference's SCHWARZ_SYMMETRIC on one block per seed = the seed and its
// breadth-first Schwarz_maxlvl ring (src/utils.py:60-86), exact local solves.
// Blocks of one colour share no member and read no x another one writes, so
// a colour is one launch, one 128-thread workgroup per block:
//   r|_k = b|_k - (A x)|_k  (one thread per member: the member's field row of
//   A_0's node BSR2 row), then x|_k += Minv_k r|_k  (thread a: sum over c of
//   Minv(a, c) r_c from the transposed inverse, coalesced over the threads).
// x node-interleaved; b with field stride bs.  Oracle: mamg_oracle.Rings.sweep.
constexpr int RING_THREADS = 128;
__global__ __launch_bounds__(RING_THREADS) void ring_kernel(int64_t k0, const int64_t* __restrict__ mo,
                                                         const int32_t* __restrict__ mem,
                                                         const int64_t* __restrict__ io,
                                                         const double* __restrict__ minvT,
                                                         const int64_t* __restrict__ ptr,
                                                         const int32_t* __restrict__ col,
                                                         const dv4* __restrict__ val, double* x,
                                                         const double* __restrict__ b, int64_t bs) {
  __shared__ double res[RING_MAX_DOFS];
  const int64_t k = k0 + blockIdx.x;
  const int64_t m0 = mo[k];
  const int d = (int)(mo[k + 1] - m0);
  const double* T = minvT + io[k];
  const double2* x2 = reinterpret_cast<const double2*>(x);
  for (int a = threadIdx.x; a < d; a += RING_THREADS) {
    const int32_t g = mem[m0 + a];
    const int32_t I = g >> 1;
    const int f = g & 1;
    double s = 0.0;
    const int64_t p1 = ptr[I + 1];
    for (int64_t q = ptr[I]; q < p1; ++q) {
      const dv4 v = val[q];
      const double2 xj = x2[col[q]];
      s += f ? v.z * xj.x + v.w * xj.y : v.x * xj.x + v.y * xj.y;
    }
    res[a] = vget(b, bs, I, f) - s;
  }
  __syncthreads();
  for (int a = threadIdx.x; a < d; a += RING_THREADS) {
    double dl = 0.0;
    for (int c = 0; c < d; ++c) dl += T[(int64_t)c * d + a] * res[c];
    x[mem[m0 + a]] += dl;
  }
}

// The same step on the CSR layout (scalar systems, nodal ones with point
// smoothers): members are plain dof indices, a member's residual comes from
// its scalar row of A_0.  Those rows hold 15 to ~400 entries (the 3D-1D
// coupling rows), so a row is read by a group of RING_CSR_VL lanes with a
// shuffle reduction (csr_gs_row), 64 rows per pass of the 1024-thread
// workgroup; after the barrier the local solve delta_a = sum_c Minv(a, c) r_c
// reads the transposed inverse coalesced over a, the c range cut into
// RING_CSR_PARTS quarters (one per 256 threads) whose partial sums meet in
// LDS and are added in a fixed order; x is updated in place.  A ring colour
// holds a handful of blocks, so a launch is a few workgroups on an otherwise
// idle device and its time is the latency of the two serial loops: 1024
// threads instead of 256 cut a launch from 33 to 24 us at 200-dof blocks
// with member rows of up to 93 entries and from 60 to 36 us with rows of up
// to 388 (3D-1D n = 48, radius 1.0 / 5.0).  Every loop is bounded
// by the block size (<= RING_MAX_DOFS) and the row length; no scratch.
// Oracle: mamg_oracle.Rings.sweep (tests/pointrings_ref.py).
constexpr int RING_CSR_THREADS = 1024;
constexpr int RING_CSR_VL = 16;
constexpr int RING_CSR_PARTS = RING_CSR_THREADS / RING_MAX_DOFS;
static_assert(RING_CSR_PARTS == 4 && RING_CSR_PARTS * RING_MAX_DOFS == RING_CSR_THREADS, "four quarters of the local solve");
__global__ __launch_bounds__(RING_CSR_THREADS) void ring_csr_kernel(int64_t k0, const int64_t* __restrict__ mo,
                                                                 const int32_t* __restrict__ mem,
                                                                 const int64_t* __restrict__ io,
                                                                 const double* __restrict__ minvT,
                                                                 const int64_t* __restrict__ ptr,
                                                                 const int32_t* __restrict__ col,
                                                                 const double* __restrict__ val, double* x,
                                                                 const double* __restrict__ b) {
  __shared__ double res[RING_MAX_DOFS];
  __shared__ double part[RING_CSR_PARTS][RING_MAX_DOFS];
  constexpr int RPP = RING_CSR_THREADS / RING_CSR_VL;   // member rows per pass
  const int64_t k = k0 + blockIdx.x;
  const int64_t m0 = mo[k];
  const int d = (int)(mo[k + 1] - m0);                  // <= RING_MAX_DOFS (check_params)
  const double* T = minvT + io[k];
  const int lane = threadIdx.x & (RING_CSR_VL - 1), grp = threadIdx.x / RING_CSR_VL;
  for (int base = 0; base < d; base += RPP) {
    const int a = base + grp;
    const bool on = a < d;
    const int64_t g = on ? mem[m0 + a] : 0;
    const double s = csr_gs_row<RING_CSR_VL>(on, g, lane, ptr, col, val, x);
    if (on && lane == 0) res[a] = b[g] - s;
  }
  __syncthreads();
  const int a = threadIdx.x & (RING_MAX_DOFS - 1), q = threadIdx.x / RING_MAX_DOFS;
  if (a < d) {
    const int chunk = (d + RING_CSR_PARTS - 1) / RING_CSR_PARTS;
    const int c0 = q * chunk, c1 = min(d, c0 + chunk);
    double dl = 0.0;
    for (int c = c0; c < c1; ++c) dl += T[(int64_t)c * d + a] * res[c];
    part[q][a] = dl;
  }
  __syncthreads();
  if (threadIdx.x < d)
    x[mem[m0 + threadIdx.x]] += (part[0][threadIdx.x] + part[1][threadIdx.x]) + (part[2][threadIdx.x] + part[3][threadIdx.x]);
}

// the rest's point GS (RINGS on the CSR layout) colours the uncovered rows
// only: A_0's pattern with every covered row emptied and every covered column
// dropped (the coupling rows, all covered, would need more than 64 colours).
// Row lengths into flen[I + 1], then the columns in order.
__global__ __launch_bounds__(256) void rest_pattern_len_kernel(int64_t n, const int64_t* __restrict__ ptr,
                                                               const int32_t* __restrict__ col,
                                                               const uint8_t* __restrict__ cov,
                                                               int64_t* __restrict__ flen) {
  const int64_t I = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (I >= n) return;
  int64_t c = 0;
  if (!cov[I])
    for (int64_t k = ptr[I]; k < ptr[I + 1]; ++k) c += cov[col[k]] ? 0 : 1;
  flen[I + 1] = c;
}
__global__ __launch_bounds__(256) void rest_pattern_fill_kernel(int64_t n, const int64_t* __restrict__ ptr,
                                                                const int32_t* __restrict__ col,
                                                                const uint8_t* __restrict__ cov,
                                                                const int64_t* __restrict__ fptr,
                                                                int32_t* __restrict__ fcol) {
  const int64_t I = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (I >= n || cov[I]) return;
  int64_t o = fptr[I];
  for (int64_t k = ptr[I]; k < ptr[I + 1]; ++k)
    if (!cov[col[k]]) fcol[o++] = col[k];
}
// colour_count_kernel for the rest: a covered row sorts behind every colour
// (key 64) and is counted in no colour
__global__ __launch_bounds__(256) void rest_count_kernel(int64_t n, const int8_t* __restrict__ c,
                                                         const uint8_t* __restrict__ cov, int32_t* __restrict__ ci,
                                                         int64_t* __restrict__ iota, unsigned long long* cnt) {
  __shared__ unsigned int hist[64];
  if (threadIdx.x < 64) hist[threadIdx.x] = 0;
  __syncthreads();
  const int64_t I = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (I < n) {
    iota[I] = I;
    if (cov[I]) {
      ci[I] = 64;
    } else {
      ci[I] = c[I];
      atomicAdd(&hist[c[I]], 1u);
    }
  }
  __syncthreads();
  if (threadIdx.x < 64 && hist[threadIdx.x]) atomicAdd(cnt + threadIdx.x, (unsigned long long)hist[threadIdx.x]);
}

// block j of the colour order <- block ord[j] of ring_blocks_dev's output:
// its inverse transposed into rinv at rio[j]
__global__ __launch_bounds__(256) void ring_perm_inv_kernel(int64_t nb, const int32_t* __restrict__ ord,
                                                            const int64_t* __restrict__ blen,
                                                            const int64_t* __restrict__ sq,
                                                            const double* __restrict__ inv,
                                                            const int64_t* __restrict__ rio, double* __restrict__ rinv) {
  const int64_t j = blockIdx.x;
  if (j >= nb) return;
  const int64_t o = ord[j], d = blen[o];
  const double* src = inv + (o ? sq[o - 1] : 0);
  double* dst = rinv + rio[j];
  for (int64_t t = threadIdx.x; t < d * d; t += 256) {
    const int64_t a = t / d, c = t - a * d;
    dst[c * d + a] = src[t];
  }
}

}  // namespace

// the rank layout's launch of ring_perm_inv_kernel (dist_layout.hip), on the null stream
void ring_perm_inv(int64_t nb, const int32_t* ord, const int64_t* blen, const int64_t* sq, const double* inv, const int64_t* rio, double* rinv) {
  ring_perm_inv_kernel<<<(unsigned)nb, 256>>>(nb, ord, blen, sq, inv, rio, rinv);
}

namespace {

// the rest's GS (RINGS): node blocks with one covered dof become split
// (diagonal) smoother blocks, so gs_layout inverts them as two 1x1 blocks;
// cov[I]: bit f = dof f of node I lies in a seed block
__global__ __launch_bounds__(256) void rest_w_kernel(int64_t nv, const dv4* __restrict__ W,
                                                     const uint8_t* __restrict__ cov, dv4* __restrict__ Wp) {
  const int64_t I = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (I >= nv) return;
  const dv4 w = W[I];
  const uint8_t c = cov[I];
  Wp[I] = (c == 1 || c == 2) ? dv4{w.x, 0.0, 0.0, w.w} : w;
}

}  // namespace

// the rank layout's launch of rest_w_kernel (dist_layout.hip), on the null stream
void rest_w(int64_t nv, const dv4* W, const uint8_t* cov, dv4* Wp) {
  rest_w_kernel<<<nblocks(nv), 256>>>(nv, W, cov, Wp);
}

namespace {

// ... and the covered dofs take no update: their rows / columns of D zeroed
__global__ __launch_bounds__(256) void rest_mask_kernel(int64_t nr, const int32_t* __restrict__ perm,
                                                        const uint8_t* __restrict__ cov, dv4* __restrict__ D) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= nr || perm[i] < 0) return;
  const uint8_t c = cov[perm[i]];
  const dv4 d = D[i];
  if (c == 3) D[i] = dv4{0.0, 0.0, 0.0, 0.0};
  else if (c == 1) D[i] = dv4{0.0, 0.0, 0.0, d.w};
  else if (c == 2) D[i] = dv4{d.x, 0.0, 0.0, 0.0};
}

}  // namespace

// the rank layout's launch of rest_mask_kernel (dist_layout.hip), on the null stream
void rest_mask(int64_t nr, const int32_t* perm, const uint8_t* cov, dv4* D) {
  rest_mask_kernel<<<nblocks(nr), 256>>>(nr, perm, cov, D);
}

namespace {

// 2x2 Gauss-Jordan without pivoting in mamg_oracle.batched_inverse's
// operation order (no contraction), on node I's diagonal block; the
// off-diagonals are dropped when I's two dofs are separate smoother blocks
// (W_I diagonal), which gives exactly the two 1x1 inverses
__device__ dv4 gj2_inverse(double a00, double a01, double a10, double a11, int* bad) {
#pragma clang fp contract(off)
  if (!(a00 > 0.0)) { *bad = 1; return dv4{0.0, 0.0, 0.0, 0.0}; }
  const double p = a00;
  const double r01 = a01 / p, r02 = 1.0 / p, r03 = 0.0 / p;
  const double f1 = a10;
  double m11 = a11 - f1 * r01, m12 = 0.0 - f1 * r02, m13 = 1.0 - f1 * r03;
  if (!(m11 > 0.0)) { *bad = 1; return dv4{0.0, 0.0, 0.0, 0.0}; }
  const double q = m11;
  m12 = m12 / q;
  m13 = m13 / q;
  const double f0 = r01;
  const double n02 = r02 - f0 * m12, n03 = r03 - f0 * m13;
  return dv4{n02, n03, m12, m13};
}

__global__ __launch_bounds__(256) void perm_fill_kernel(int64_t nr, const int32_t* __restrict__ perm,
                                                        const int64_t* __restrict__ ptr, const int32_t* __restrict__ col,
                                                        const dv4* __restrict__ val, const dv4* __restrict__ W,
                                                        const int64_t* __restrict__ gptr, int32_t* __restrict__ gcol,
                                                        dv4* __restrict__ gval, dv4* __restrict__ Dg, int* bad) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= nr) return;
  if (perm[i] < 0) { Dg[i] = dv4{0.0, 0.0, 0.0, 0.0}; return; }
  const int64_t I = perm[i];
  int64_t o = gptr[i];
  dv4 dg = {0.0, 0.0, 0.0, 0.0};
  bool has = false;
  for (int64_t k = ptr[I]; k < ptr[I + 1]; ++k, ++o) {
    gcol[o] = col[k];
    gval[o] = val[k];
    if (col[k] == I) { dg = val[k]; has = true; }
  }
  if (!has) { *bad = 1; return; }
  const dv4 w = W[I];
  const bool split = w.y == 0.0 && w.z == 0.0;
  Dg[i] = gj2_inverse(dg.x, split ? 0.0 : dg.y, split ? 0.0 : dg.z, dg.w, bad);
}

// coarse-grid correction scaling (coarse_scaling ON, src/amg_parameters.py:78):
// alpha = <b_c, e> / <A_c e, e> (= <r, P e> / <A P e, P e> for A_c = P^T A P),
// e <- alpha e; alpha = 1 if the denominator is not positive.  Partial sums
// per block, then every block of the scaling launch reduces the partials in
// the same fixed order (so all agree on alpha).  Oracle: mamg_oracle.coarse_scale.
__global__ __launch_bounds__(256) void dot2_partial_kernel(int64_t n, const double* __restrict__ bc,
                                                           const double* __restrict__ e,
                                                           const double* __restrict__ q,
                                                           double* __restrict__ part) {
  __shared__ double red[8];
  double s = 0.0, t = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    s += bc[i] * e[i];
    t += q[i] * e[i];
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    s += __shfl_xor(s, off, 64);
    t += __shfl_xor(t, off, 64);
  }
  if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6] = s; red[4 + (threadIdx.x >> 6)] = t; }
  __syncthreads();
  if (threadIdx.x == 0) {
    part[2 * blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
    part[2 * blockIdx.x + 1] = (red[4] + red[5]) + (red[6] + red[7]);
  }
}

__global__ __launch_bounds__(256) void cscale_kernel(int64_t n, int nb, const double* __restrict__ part,
                                                     double* __restrict__ e) {
  __shared__ double red[8];
  __shared__ double alpha;
  double s = 0.0, t = 0.0;
  for (int i = threadIdx.x; i < nb; i += 256) { s += part[2 * i]; t += part[2 * i + 1]; }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    s += __shfl_xor(s, off, 64);
    t += __shfl_xor(t, off, 64);
  }
  if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6] = s; red[4 + (threadIdx.x >> 6)] = t; }
  __syncthreads();
  if (threadIdx.x == 0) {
    const double num = (red[0] + red[1]) + (red[2] + red[3]);
    const double den = (red[4] + red[5]) + (red[6] + red[7]);
    alpha = den > 0.0 ? num / den : 1.0;
  }
  __syncthreads();
  const double a = alpha;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) e[i] = a * e[i];
}

// ---- nonlinear AMLI (K-cycle, mamg.h MAMG_NL_AMLI_CYCLE): step j of the inner
// flexible CG on a level, after z = M(r) and w = A z (tests/kcycle_ref.py):
//   beta_i = d_i > 0 ? <z, q_i> / d_i : 0 (i < j), p_j = z - sum beta_i p_i,
//   q_j = w - sum beta_i q_i, d_j = <p_j, q_j>, alpha = d_j > 0 ? <p_j, r> / d_j : 0,
//   e (+)= alpha p_j, r -= alpha q_j.
// As the coarse scaling above: block partials in fixed slots, and every block
// of the consuming launch reduces them in one fixed order, so all blocks agree
// on a scalar and a replay gives the same bits.  nb: the producing launch's
// blocks.  The scalars stay in HBM (DLevel::kpart, KP_*).
struct KDirs {
  const double* p[MAMG_NL_AMLI_MAX - 1];
  const double* q[MAMG_NL_AMLI_MAX - 1];
};

// the 256 threads' values summed, the same on every thread (red: 4 * NV doubles)
template <int NV>
__device__ __forceinline__ void kblock_sum(double (&v)[NV], double* red) {
#pragma unroll
  for (int k = 0; k < NV; ++k) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v[k] += __shfl_xor(v[k], off, 64);
  }
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < NV; ++k) red[4 * k + (threadIdx.x >> 6)] = v[k];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < NV; ++k) v[k] = (red[4 * k] + red[4 * k + 1]) + (red[4 * k + 2] + red[4 * k + 3]);
}

// part[KP_DOT + i * SCALE_BLOCKS + block] = the block's share of <z, q_i>, i < J
template <int J>
__global__ __launch_bounds__(256) void kdot_kernel(int64_t n, const double* __restrict__ z, KDirs D,
                                                   double* __restrict__ part) {
  __shared__ double red[4 * J];
  double s[J];
#pragma unroll
  for (int i = 0; i < J; ++i) s[i] = 0.0;
#pragma unroll 2
  for (int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x; k < n; k += (int64_t)gridDim.x * 256) {
    const double zk = z[k];
#pragma unroll
    for (int i = 0; i < J; ++i) s[i] += zk * D.q[i][k];
  }
  kblock_sum<J>(s, red);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int i = 0; i < J; ++i) part[KP_DOT + i * SCALE_BLOCKS + blockIdx.x] = s[i];
  }
}

// J > 0: p_j, q_j from z, w and the J earlier directions (the beta's in
// registers); J = 0: p_0 = z and q_0 = w are in place already.  Both: the
// block's shares of <p_j, q_j> and <p_j, r>.
template <int J>
__global__ __launch_bounds__(256) void korth_kernel(int64_t n, int nb, const double* __restrict__ z,
                                                    const double* __restrict__ w, KDirs D,
                                                    double* __restrict__ pj, double* __restrict__ qj,
                                                    const double* __restrict__ r, double* __restrict__ part) {
  __shared__ double red[4 * (J > 2 ? J : 2)];
  double beta[J > 0 ? J : 1];
  if constexpr (J > 0) {
    double s[J];
#pragma unroll
    for (int i = 0; i < J; ++i) {
      s[i] = 0.0;
      for (int b = threadIdx.x; b < nb; b += 256) s[i] += part[KP_DOT + i * SCALE_BLOCKS + b];
    }
    kblock_sum<J>(s, red);
#pragma unroll
    for (int i = 0; i < J; ++i) {
      const double d = part[KP_D + i];
      beta[i] = d > 0.0 ? s[i] / d : 0.0;
    }
    __syncthreads();   // red is used again below
  }
  double a[2] = {0.0, 0.0};
#pragma unroll 2
  for (int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x; k < n; k += (int64_t)gridDim.x * 256) {
    double pk, qk;
    if constexpr (J > 0) {
      pk = z[k];
      qk = w[k];
#pragma unroll
      for (int i = 0; i < J; ++i) {
        pk -= beta[i] * D.p[i][k];
        qk -= beta[i] * D.q[i][k];
      }
      pj[k] = pk;
      qj[k] = qk;
    } else {
      pk = pj[k];
      qk = qj[k];
    }
    a[0] += pk * qk;
    a[1] += pk * r[k];
  }
  kblock_sum<2>(a, red);
  if (threadIdx.x == 0) {
    part[KP_PQ + 2 * blockIdx.x] = a[0];
    part[KP_PQ + 2 * blockIdx.x + 1] = a[1];
  }
}

// d_j and alpha from korth_kernel's nb block partials; e = alpha p (FIRST) or
// e += alpha p; rout = rin - alpha q unless LAST (step 0 reads the visit's
// right-hand side and writes the level's own r)
template <bool FIRST, bool LAST>
__global__ __launch_bounds__(256) void kupd_kernel(int64_t n, int nb, int j, double* __restrict__ part,
                                                   const double* __restrict__ p, const double* __restrict__ q,
                                                   double* __restrict__ e, const double* rin, double* rout) {
  __shared__ double red[8];
  double a[2] = {0.0, 0.0};
  for (int b = threadIdx.x; b < nb; b += 256) {
    a[0] += part[KP_PQ + 2 * b];
    a[1] += part[KP_PQ + 2 * b + 1];
  }
  kblock_sum<2>(a, red);
  const double d = a[0];
  const double alpha = d > 0.0 ? a[1] / d : 0.0;
  if (blockIdx.x == 0 && threadIdx.x == 0) part[KP_D + j] = d;
#pragma unroll 2
  for (int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x; k < n; k += (int64_t)gridDim.x * 256) {
    const double pk = p[k];
    e[k] = FIRST ? alpha * pk : e[k] + alpha * pk;
    if (!LAST) rout[k] = rin[k] - alpha * q[k];
  }
}

// Fixed by measurement (round 1 A/Bs; the variants
// measured slower were removed in round 2): XCD-contiguous restriction rows,
// SELL chunks of 8 blocks (K: 6), half-symmetric chunks of 4 with
// XCD-contiguous rows, symmetric-block packing, lane counts from the mean row
// length.  What stays selectable is a switch (opts.h), read from the handle.
constexpr int sell_u = 8;
constexpr int post_u = 6;
constexpr int64_t sell_max_len = 40;
__global__ void warm_kernel() {}

// every block symmetric (bitwise): then 3 doubles per block carry it exactly
bool blocks_symmetric(const HBsr& B) {
  const int64_t nb = B.ptr[B.nr];
  int64_t bad = 0;
  for (int64_t k = 0; k < nb; ++k)
    bad |= std::memcmp(&B.val[4 * k + 1], &B.val[4 * k + 2], sizeof(double)) != 0;
  return bad == 0;
}
void pack_sym(const HBsr& B, std::vector<double>* v3) {
  const int64_t nb = B.ptr[B.nr];
  v3->resize(3 * nb);
  for (int64_t k = 0; k < nb; ++k) {
    (*v3)[2 * k] = B.val[4 * k];
    (*v3)[2 * k + 1] = B.val[4 * k + 3];
    (*v3)[2 * nb + k] = B.val[4 * k + 1];
  }
}

}  // namespace

// lanes per row: ~3 entries per lane (bench/spmv_micro.hip: 8 lanes best for
// the ~30 nnz CSR rows and the ~15 block BSR rows of the level-0 operator)
int pick_lanes(int64_t n, int64_t nnz) {
  const double avg = n ? (double)nnz / (double)n : 1.0;
  int l = 2;
  while (l < 64 && 3.0 * (2 * l) <= avg + 1e-9) l *= 2;
  return l;
}

namespace {

int upload_csr(DeviceHandle* h, const CsrView& M, DCsr* D, int lanes, std::string* err) {
  D->n = M.n;
  D->m = M.m;
  D->nnz = M.nnz();
  D->lanes = lanes > 0 ? lanes : pick_lanes(M.n, D->nnz);
  int rc;
  if ((rc = dalloc(h, &D->ptr, M.n + 1, err))) return rc;
  if ((rc = dalloc(h, &D->col, std::max<int64_t>(D->nnz, 1), err))) return rc;
  if ((rc = dalloc(h, &D->val, std::max<int64_t>(D->nnz, 1), err))) return rc;
  HIPCHK(hipMemcpy(D->ptr, M.ptr, (M.n + 1) * sizeof(int64_t), hipMemcpyHostToDevice));
  if (D->nnz) {
    HIPCHK(hipMemcpy(D->col, M.col, D->nnz * sizeof(int32_t), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(D->val, M.val, D->nnz * sizeof(double), hipMemcpyHostToDevice));
  }
  return MAMG_OK;
}

// a device CSR (GPU setup output) copied into the handle's memory
int adopt_csr(DeviceHandle* h, const DevMat& M, DCsr* D, int lanes, std::string* err) {
  D->n = M.n;
  D->m = M.m;
  D->nnz = M.nnz;
  D->lanes = lanes > 0 ? lanes : pick_lanes(M.n, D->nnz);
  int rc;
  if ((rc = dalloc(h, &D->ptr, M.n + 1, err))) return rc;
  if ((rc = dalloc(h, &D->col, std::max<int64_t>(D->nnz, 1), err))) return rc;
  if ((rc = dalloc(h, &D->val, std::max<int64_t>(D->nnz, 1), err))) return rc;
  HIPCHK(dev_copy(D->ptr, M.ptr, (M.n + 1) * sizeof(int64_t)));
  if (D->nnz) {
    HIPCHK(dev_copy(D->col, M.col, D->nnz * sizeof(int32_t)));
    HIPCHK(dev_copy(D->val, M.val, D->nnz * sizeof(double)));
  }
  return MAMG_OK;
}

}  // namespace

// lanes per node row for 2x2 blocks: ~2 blocks per lane (VL = 8 for the
// ~15-block level-0 rows: 1.87 ms vs 2.00 ms at VL = 4, bench/spmv_micro.hip;
// round 3 at nrefs=6: 1/4, 1/2 and 2x these lanes on the coarse levels were
// 0.419-0.527 ms vs 0.421 ms, profiles/r03_ab_coarse_lanes.txt)
int pick_lanes_bsr(int64_t nr, int64_t nb) {
  const double avg = nr ? (double)nb / (double)nr : 1.0;
  int l = 2;
  while (l < 64 && 2.0 * (2 * l) <= 2.0 * avg) l *= 2;
  return l;
}

namespace {

// SELL-64 copy of a BSR2 matrix (host packing: convert.cpp to_sell)
int upload_sell(HandleMem* h, const HBsr& B, DBsr* D, std::string* err) {
  HSell S;
  const bool merged = (int64_t)B.ptr.size() == 2 * B.nr + 1;
  int rc = to_sell(B, D->sym, SELL_C, merged ? SELL_SIGMA : 1, &S, err);
  if (rc) return rc;
  const int64_t ns = (int64_t)S.soff.size() - 1;
  const int per = D->sym ? 3 : 4;
  D->sell = true;
  D->nbs = S.nbs;
  if ((rc = dalloc(h, &D->soff, ns + 1, err))) return rc;
  if ((rc = dalloc(h, &D->meta, std::max<int64_t>(S.nr, 1), err))) return rc;
  if ((rc = dalloc(h, &D->col, std::max<int64_t>(S.nbs, 1), err))) return rc;
  if ((rc = dalloc(h, &D->val, std::max<int64_t>(per * S.nbs, 1), err))) return rc;
  HIPCHK(hipMemcpy(D->soff, S.soff.data(), (ns + 1) * sizeof(int64_t), hipMemcpyHostToDevice));
  if (S.nr) HIPCHK(hipMemcpy(D->meta, S.meta.data(), S.nr * sizeof(int32_t), hipMemcpyHostToDevice));
  if (!S.perm.empty()) {
    if ((rc = dalloc(h, &D->perm, S.nr, err))) return rc;
    HIPCHK(hipMemcpy(D->perm, S.perm.data(), S.nr * sizeof(int32_t), hipMemcpyHostToDevice));
  }
  if (S.nbs) {
    HIPCHK(hipMemcpy(D->col, S.col.data(), S.nbs * sizeof(int32_t), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(D->val, S.val.data(), per * S.nbs * sizeof(double), hipMemcpyHostToDevice));
  }
  return MAMG_OK;
}

}  // namespace

// (also uploads a merged [P | AP] matrix: then B.ptr has 2 nr + 1 entries)
int upload_bsr(HandleMem* h, const HBsr& B, DBsr* D, int lanes, std::string* err,
               bool sym) {
  const int64_t np = (int64_t)B.ptr.size();
  D->nr = B.nr;
  D->nc = B.nc;
  D->nb = B.ptr[np - 1];
  D->lanes = lanes > 0 ? lanes : pick_lanes_bsr(B.nr, D->nb);
  int rc;
  // SELL-64 for many short rows (one lane per row needs >> 256 CUs x 64 rows)
  const bool merged_rows = np == 2 * B.nr + 1;
  if (B.nr >= h->sw.sell_min_rows && D->nb <= sell_max_len * B.nr && !merged_rows) {
    D->sym = sym && np == B.nr + 1 && blocks_symmetric(B);
    return upload_sell(h, B, D, err);
  }
  if ((rc = dalloc(h, &D->ptr, np, err))) return rc;
  if ((rc = dalloc(h, &D->col, std::max<int64_t>(D->nb, 1), err))) return rc;
  D->sym = sym && np == B.nr + 1 && blocks_symmetric(B);
  const int per = D->sym ? 3 : 4;
  if ((rc = dalloc(h, &D->val, std::max<int64_t>(per * D->nb, 1), err))) return rc;
  HIPCHK(hipMemcpy(D->ptr, B.ptr.data(), np * sizeof(int64_t), hipMemcpyHostToDevice));
  if (D->nb) {
    HIPCHK(hipMemcpy(D->col, B.col.data(), D->nb * sizeof(int32_t), hipMemcpyHostToDevice));
    if (D->sym) {
      std::vector<double> v3;
      pack_sym(B, &v3);
      HIPCHK(hipMemcpy(D->val, v3.data(), D->nb * 3 * sizeof(double), hipMemcpyHostToDevice));
    } else {
      HIPCHK(hipMemcpy(D->val, B.val.data(), D->nb * 4 * sizeof(double), hipMemcpyHostToDevice));
    }
  }
  return MAMG_OK;
}

namespace {

// ---------------------------------------------------------------------------
// Device-side layout construction: field-major CSR already in HBM (GPU setup
// output, or host CSR copied up) -> the BSR2 / symmetric / SELL-64 / merged
// [P | AP] apply layouts.  Same layouts as the host conversions in
// convert.cpp (to_bsr2, merge_bsr_rows, to_sell with sigma = 1, pack_sym);
// pure data movement, so the apply sees identical bits either way.
// ---------------------------------------------------------------------------
// node I's four sorted column segments (rowstage.h stage_segs): q = 2 f + g
// holds the entries of row f nr + I whose column lies in field g (node
// column = col - g nc)
template <bool FILL, int CAP = RS_CAP>
__global__ __launch_bounds__(64) void csr2bsr_kernel(int64_t nr, int64_t nc, const int64_t* __restrict__ ptr,
                                                     const int32_t* __restrict__ col,
                                                     const double* __restrict__ val, int64_t* bptr,
                                                     int32_t* __restrict__ bcol, dv4* __restrict__ bval) {
  __shared__ RowStageT<FILL, CAP> S;   // rowstage.h: the wave's rows staged through LDS
  const int64_t I0 = (int64_t)blockIdx.x * RS_NODES, I = I0 + threadIdx.x;
  RowView vw[2];
  stage_rows<FILL>(S, ptr, col, val, nr, I0, vw);
  if (I >= nr) return;
  Seg4 g;
  stage_segs(ptr, vw, nr, nc, I, g.k, g.e);
  g.init(vw, nc);
  int64_t o = FILL ? bptr[I] : 0;
  for (;;) {
    const int64_t J = g.next();
    if (J == INT64_MAX) break;
    dv4 v = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int q = 0; q < 4; ++q)
      if (g.c[q] == J) {
        if (FILL) v[q] = vw[q >> 1].val(g.k[q]);
        ++g.k[q];
        g.head(vw, nc, q);
      }
    if (FILL) {
      bval[o] = v;
      bcol[o] = (int32_t)J;
    }
    ++o;
  }
  if (!FILL) bptr[I + 1] = o;
}

// The fill pass with columns only in LDS (16 KB, ~10 waves per CU instead
// of 3 with the 48 KB column + value staging): each lane's merge writes, in
// place of every staged column, the entry's slot in the output (4 (o - o0) + q,
// o0 the workgroup's first block) and the zeros of its blocks' missing
// components; then the wave sweeps the value ranges with coalesced loads and
// stores each value into its slot.  Same blocks, same bits.  Ranges over
// CAP (not staged) merge from global memory as in csr2bsr_kernel.
template <int CAP>
__global__ __launch_bounds__(64) void csr2bsr_fill_kernel(int64_t nr, int64_t nc, const int64_t* __restrict__ ptr,
                                                          const int32_t* __restrict__ col,
                                                          const double* __restrict__ val, const int64_t* bptr,
                                                          int32_t* __restrict__ bcol, dv4* __restrict__ bval) {
  __shared__ RowStageT<false, CAP> S;   // columns, then each entry's slot
  const int64_t I0 = (int64_t)blockIdx.x * RS_NODES, I = I0 + threadIdx.x;
  RowView vw[2];
  stage_rows<false>(S, ptr, col, val, nr, I0, vw);
  const bool lds = vw[0].lds;      // uniform over the workgroup
  if (!lds) {                      // long ranges: values from global memory
    if (I >= nr) return;
    Seg4 g;
    stage_segs(ptr, vw, nr, nc, I, g.k, g.e);
    g.init(vw, nc);
    int64_t o = bptr[I];
    for (;;) {
      const int64_t J = g.next();
      if (J == INT64_MAX) break;
      dv4 v = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (g.c[q] == J) {
          v[q] = vw[q >> 1].val(g.k[q]);
          ++g.k[q];
          g.head(vw, nc, q);
        }
      bval[o] = v;
      bcol[o] = (int32_t)J;
      ++o;
    }
    return;
  }
  const int64_t o0 = bptr[I0];
  double* bv = reinterpret_cast<double*>(bval + o0);
  if (I < nr) {
    Seg4 g;
    stage_segs(ptr, vw, nr, nc, I, g.k, g.e);
    g.init(vw, nc);
    int64_t o = bptr[I];
    for (;;) {
      const int64_t J = g.next();
      if (J == INT64_MAX) break;
      const int32_t rel = (int32_t)(o - o0);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        if (g.c[q] == J) {
          S.c[q >> 1][g.k[q] - vw[q >> 1].off] = 4 * rel + q;   // this entry's slot (its column was read)
          ++g.k[q];
          g.head(vw, nc, q);
        } else {
          bv[4 * rel + q] = 0.0;
        }
      }
      bcol[o] = (int32_t)J;
      ++o;
    }
  }
  __syncthreads();
  const int64_t I1 = I0 + RS_NODES < nr ? I0 + RS_NODES : nr;
#pragma unroll
  for (int f = 0; f < 2; ++f) {
    const int64_t b = ptr[f * nr + I0], n = ptr[f * nr + I1] - b;
    scatter_staged(S.c[f], val, b, n, bv);
  }
}

// *bad = 1 when some block has a01 != a10 (bitwise).  Grid-stride over at most
// SYM_CHECK_BLOCKS workgroups, one atomic per workgroup: with one atomic per
// mismatching wave, a non-symmetric level-1 operator (25.8 M blocks, nearly
// all mismatching) serialised ~400 K atomics on one word (4.6 ms)
constexpr unsigned SYM_CHECK_BLOCKS = 16384;
__global__ __launch_bounds__(256) void sym_check_kernel(int64_t nb, const dv4* __restrict__ v, int* bad) {
  int d = 0;
  for (int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x; k < nb; k += (int64_t)gridDim.x * 256)
    d |= __double_as_longlong(v[k].y) != __double_as_longlong(v[k].z);
  if (__syncthreads_or(d) && threadIdx.x == 0) atomicOr(bad, 1);
}

}  // namespace

// the rank layout's launch of sym_check_kernel (dist_layout.hip), on the null stream
void sym_check(int64_t nb, const dv4* v, int* bad) {
  sym_check_kernel<<<std::min(nblocks(nb), SYM_CHECK_BLOCKS), 256>>>(nb, v, bad);
}

namespace {

__global__ __launch_bounds__(256) void pack_sym_kernel(int64_t nb, const dv4* __restrict__ v,
                                                       double* __restrict__ out) {
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (k >= nb) return;
  const dv4 a = v[k];
  out[2 * k] = a.x;
  out[2 * k + 1] = a.w;
  out[2 * nb + k] = a.y;
}

// merged [P | Q] row pointers: lengths at 2I+1, 2I+2 (scanned afterwards)
__global__ __launch_bounds__(256) void merge_len_kernel(int64_t nr, const int64_t* __restrict__ pp,
                                                        const int64_t* __restrict__ qp, int64_t* mptr) {
  const int64_t I = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (I >= nr) return;
  mptr[2 * I + 1] = pp[I + 1] - pp[I];
  mptr[2 * I + 2] = qp[I + 1] - qp[I];
  if (I == 0) mptr[0] = 0;
}

__global__ __launch_bounds__(256) void merge_fill_kernel(int64_t nr, const int64_t* __restrict__ pp,
                                                         const int32_t* __restrict__ pc, const dv4* __restrict__ pv,
                                                         const int64_t* __restrict__ qp, const int32_t* __restrict__ qc,
                                                         const dv4* __restrict__ qv, const int64_t* __restrict__ mptr,
                                                         int32_t* __restrict__ mc, dv4* __restrict__ mv) {
  const int64_t I = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (I >= nr) return;
  int64_t d = mptr[2 * I];
  for (int64_t k = pp[I]; k < pp[I + 1]; ++k, ++d) { mc[d] = pc[k]; mv[d] = pv[k]; }
  for (int64_t k = qp[I]; k < qp[I + 1]; ++k, ++d) { mc[d] = qc[k]; mv[d] = qv[k]; }
}

// K = P - W_I (A P) row by row on the union of P's and AP's block patterns
// (the fused post-smoothing operator: x1 + P e + W (r1 - AP e) = x1 + W r1 + K e);
// a block absent from one operand contributes exact zeros
template <bool FILL>
__global__ __launch_bounds__(256) void kmerge_kernel(int64_t nr, const int64_t* __restrict__ pp,
                                                     const int32_t* __restrict__ pc, const dv4* __restrict__ pv,
                                                     const int64_t* __restrict__ qp, const int32_t* __restrict__ qc,
                                                     const dv4* __restrict__ qv, const dv4* __restrict__ W,
                                                     int64_t* kp, int32_t* __restrict__ kc, dv4* __restrict__ kv) {
#pragma clang fp contract(off)   // the host's kmerge_rows (dist.cpp, -ffp-contract=off) bit for bit
  const int64_t I = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (I >= nr) return;
  int64_t a = pp[I], ae = pp[I + 1], b = qp[I], be = qp[I + 1];
  int64_t o = FILL ? kp[I] : 0;
  const dv4 w = FILL ? W[I] : dv4{0.0, 0.0, 0.0, 0.0};
  const dv4 zero = {0.0, 0.0, 0.0, 0.0};
  while (a < ae || b < be) {
    const int32_t ja = a < ae ? pc[a] : INT32_MAX, jb = b < be ? qc[b] : INT32_MAX;
    const int32_t j = min(ja, jb);
    if (FILL) {
      const dv4 p = ja == j ? pv[a] : zero, q = jb == j ? qv[b] : zero;
      dv4 k;   // blocks (0,0) (0,1) (1,0) (1,1) = x y z w;  (W q)_ab = W_a0 q_0b + W_a1 q_1b
      k.x = p.x - (w.x * q.x + w.y * q.z);
      k.y = p.y - (w.x * q.y + w.y * q.w);
      k.z = p.z - (w.z * q.x + w.w * q.z);
      k.w = p.w - (w.z * q.y + w.w * q.w);
      kc[o] = j;
      kv[o] = k;
    }
    if (ja == j) ++a;
    if (jb == j) ++b;
    ++o;
  }
  if (!FILL) kp[I + 1] = o;
}

// SELL-64: slice widths and per-row meta (length | first-part length << 16)
__global__ __launch_bounds__(256) void sell_meta_kernel(int64_t nr, const int64_t* __restrict__ bptr, int merged,
                                                        int32_t* __restrict__ meta, int64_t* __restrict__ soff,
                                                        int* bad) {
  const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t ns = (nr + SELL_C - 1) / SELL_C;
  if (s >= ns) return;
  int64_t w = 0;
  for (int64_t I = s * SELL_C; I < min(nr, (s + 1) * SELL_C); ++I) {
    const int64_t a = merged ? bptr[2 * I] : bptr[I];
    const int64_t m = merged ? bptr[2 * I + 1] : a;
    const int64_t e = merged ? bptr[2 * I + 2] : bptr[I + 1];
    if (e - a >= 0xffff) { atomicOr(bad, 1); continue; }
    meta[I] = (int32_t)((e - a) | ((m - a) << 16));
    w = max(w, e - a);
  }
  soff[s + 1] = (int64_t)SELL_C * w;
  if (s == 0) soff[0] = 0;
}

__global__ __launch_bounds__(256) void sell_fill_kernel(int64_t nr, const int64_t* __restrict__ bptr, int merged,
                                                        const int32_t* __restrict__ bcol, const dv4* __restrict__ bval,
                                                        const int64_t* __restrict__ soff, int64_t nbs, int sym,
                                                        int32_t* __restrict__ scol, double* __restrict__ sval) {
  const int64_t I = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (I >= nr) return;
  const int64_t a = merged ? bptr[2 * I] : bptr[I];
  const int64_t e = merged ? bptr[2 * I + 2] : bptr[I + 1];
  int64_t kk = soff[I / SELL_C] + (I % SELL_C);
  for (int64_t k = a; k < e; ++k, kk += SELL_C) {
    scol[kk] = bcol[k];
    const dv4 v = bval[k];
    if (sym) {
      sval[2 * kk] = v.x;
      sval[2 * kk + 1] = v.w;
      sval[2 * nbs + kk] = v.y;
    } else {
      reinterpret_cast<dv4*>(sval)[kk] = v;
    }
  }
}

// SELL-64 rows sorted by length inside each slice (DBsr::lsort): one 64-lane
// workgroup per slice; lane i's rank = rows longer than row i + equal rows
// before it (stable, longest first).  nmeta[slot] = length | (row offset << 16),
// src[slot] = the row offset the slot takes its blocks from.
__global__ __launch_bounds__(64) void sell_sort_kernel(int64_t nr, const int32_t* __restrict__ meta,
                                                      int32_t* __restrict__ nmeta, int32_t* __restrict__ src) {
  __shared__ int len[SELL_C];
  const int64_t r0 = (int64_t)blockIdx.x * SELL_C;
  const int i = threadIdx.x;
  const int cnt = (int)min((int64_t)SELL_C, nr - r0);
  const int li = i < cnt ? meta[r0 + i] & 0xffff : -1;
  len[i] = li;
  __syncthreads();
  if (i >= cnt) return;
  int rank = 0;
  for (int j = 0; j < cnt; ++j) rank += (len[j] > li) || (len[j] == li && j < i);
  nmeta[r0 + rank] = li | (i << 16);
  src[r0 + rank] = i;
}

// the slot arrays re-ordered to the sorted rows: slot p of slice s takes the
// blocks of slot src[p] (width = the slice's, so every block moves whole)
__global__ __launch_bounds__(64) void sell_permute_kernel(int64_t nr, const int64_t* __restrict__ soff,
                                                         const int32_t* __restrict__ src, int64_t nbs, int per,
                                                         const int32_t* __restrict__ col, const double* __restrict__ val,
                                                         int32_t* __restrict__ ncol, double* __restrict__ nval) {
  const int64_t s = blockIdx.x, r0 = s * SELL_C;
  const int p = threadIdx.x;
  if (r0 + p >= nr) return;
  const int64_t w = (soff[s + 1] - soff[s]) / SELL_C;
  const int64_t d0 = soff[s] + p, s0 = soff[s] + src[r0 + p];
  for (int64_t j = 0; j < w; ++j) {
    const int64_t d = d0 + SELL_C * j, o = s0 + SELL_C * j;
    ncol[d] = col[o];
    if (per == 4) {
      reinterpret_cast<dv4*>(nval)[d] = reinterpret_cast<const dv4*>(val)[o];
    } else {
      reinterpret_cast<dv2*>(nval)[d] = reinterpret_cast<const dv2*>(val)[o];
      nval[2 * nbs + d] = val[2 * nbs + o];
    }
  }
}

// half-symmetric ELL-64: per-row lower / upper / ghost counts (meta),
// widths (max), lower-entry total.  Grid-stride over at most HALF_META_BLOCKS
// workgroups, reduced in the workgroup, one atomic per counter per workgroup:
// three one-word atomics per wave serialised on their words (6.1 ms at A_0)
constexpr unsigned HALF_META_BLOCKS = 4096;
__global__ __launch_bounds__(256) void half_meta_kernel(int64_t nr, const int64_t* __restrict__ bptr,
                                                        const int32_t* __restrict__ bcol,
                                                        int32_t* __restrict__ meta, int* wmax,
                                                        unsigned long long* nlo) {
  unsigned long long snl = 0;
  int mu = 0, ml = 0, bad = 0;
  for (int64_t I = (int64_t)blockIdx.x * 256 + threadIdx.x; I < nr; I += (int64_t)gridDim.x * 256) {
    const int64_t a = bptr[I], e = bptr[I + 1];
    int64_t lo = a, hi = e;
    while (lo < hi) {            // first column >= I
      const int64_t mid = (lo + hi) >> 1;
      if (bcol[mid] < I) lo = mid + 1; else hi = mid;
    }
    const int64_t nl = lo - a;
    hi = e;
    while (lo < hi) {            // first column >= nr (ghosts)
      const int64_t mid = (lo + hi) >> 1;
      if (bcol[mid] < nr) lo = mid + 1; else hi = mid;
    }
    const int64_t ng = e - lo, nu = e - a - nl - ng;
    if (nu > 0xff || nl > 0xff || ng > 0x7fff) { bad = 1; continue; }
    snl += (unsigned long long)nl;
    meta[I] = (int32_t)(nu | (nl << 8) | (ng << 16));
    mu = max(mu, (int)nu);
    ml = max(ml, (int)nl);
  }
  for (int o = 32; o > 0; o >>= 1) {
    snl += __shfl_xor(snl, o);
    mu = max(mu, __shfl_xor(mu, o));
    ml = max(ml, __shfl_xor(ml, o));
    bad |= __shfl_xor(bad, o);
  }
  __shared__ unsigned long long ws[4];
  __shared__ int wu[4], wl[4], wb[4];
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { ws[w] = snl; wu[w] = mu; wl[w] = ml; wb[w] = bad; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int k = 1; k < 4; ++k) {
      snl += ws[k];
      mu = max(mu, wu[k]);
      ml = max(ml, wl[k]);
      bad |= wb[k];
    }
    if (snl) atomicAdd(nlo, snl);
    if (mu) atomicMax(wmax, mu);
    if (ml) atomicMax(wmax + 1, ml);
    if (bad) atomicOr(wmax + 2, 1);
  }
}

// ghost-part slice widths (slot counts, scanned into gsoff afterwards)
__global__ __launch_bounds__(256) void half_gwidth_kernel(int64_t nr, const int32_t* __restrict__ meta,
                                                          int64_t* __restrict__ gsoff) {
  const int64_t sl = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t ns = (nr + SELL_C - 1) / SELL_C;
  if (sl >= ns) return;
  int w = 0;
  for (int64_t I = sl * SELL_C; I < min(nr, (sl + 1) * SELL_C); ++I) w = max(w, meta[I] >> 16);
  gsoff[sl + 1] = (int64_t)SELL_C * w;
  if (sl == 0) gsoff[0] = 0;
}

// upper blocks into their ELL slots, ghost blocks into the ghost SELL part
// (symmetric-block packing); every lower block (I, J) must have a
// bitwise-equal mirror (J, I), whose upper slot it records
__global__ __launch_bounds__(256) void half_fill_kernel(int64_t nr, const int64_t* __restrict__ bptr,
                                                        const int32_t* __restrict__ bcol, const dv4* __restrict__ bval,
                                                        const int32_t* __restrict__ meta, int hwu, int hwl, int64_t nbs,
                                                        int32_t* __restrict__ ucol, double* __restrict__ uval,
                                                        int32_t* __restrict__ lptr, const int64_t* __restrict__ gsoff,
                                                        int64_t ngs, int32_t* __restrict__ gcol,
                                                        double* __restrict__ gval, int* bad, int check_only) {
  const int64_t I = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (I >= nr) return;
  const int mI = meta[I];
  const int64_t a = bptr[I], e = bptr[I + 1], nl = (mI >> 8) & 0xff, ng = mI >> 16;
  const int64_t ubase = (I >> 6) * (int64_t)(64 * hwu) + (I & 63);
  for (int64_t k = a + nl, j = 0; k < e - ng && !check_only; ++k, ++j) {
    const int64_t kk = ubase + 64 * j;
    const dv4 v = bval[k];
    ucol[kk] = bcol[k];
    uval[2 * kk] = v.x;
    uval[2 * kk + 1] = v.w;
    uval[2 * nbs + kk] = v.y;
  }
  if (ng && !check_only) {
    const int64_t gbase = gsoff[I >> 6] + (I & 63);
    for (int64_t k = e - ng, j = 0; k < e; ++k, ++j) {
      const int64_t kk = gbase + 64 * j;
      const dv4 v = bval[k];
      gcol[kk] = bcol[k];
      gval[2 * kk] = v.x;
      gval[2 * kk + 1] = v.w;
      gval[2 * ngs + kk] = v.y;
    }
  }
  const int64_t lbase = (I >> 6) * (int64_t)(64 * hwl) + (I & 63);
  for (int64_t k = a, j = 0; k < a + nl; ++k, ++j) {
    const int64_t J = bcol[k];
    const int mJ = meta[J];
    const int64_t uJ = bptr[J] + ((mJ >> 8) & 0xff), eJ = uJ + (mJ & 0xff);
    int64_t lo = uJ, hi = eJ;
    while (lo < hi) {
      const int64_t mid = (lo + hi) >> 1;
      if (bcol[mid] < I) lo = mid + 1; else hi = mid;
    }
    const dv4 v = bval[k];
    bool ok = lo < eJ && bcol[lo] == I;
    if (ok) {
      const dv4 t = bval[lo];
      ok = __double_as_longlong(v.x) == __double_as_longlong(t.x) &&
           __double_as_longlong(v.y) == __double_as_longlong(t.z) &&
           __double_as_longlong(v.z) == __double_as_longlong(t.y) &&
           __double_as_longlong(v.w) == __double_as_longlong(t.w);
    }
    if (!ok) { atomicOr(bad, 1); return; }
    if (check_only) continue;
    const int64_t jj = lo - uJ;
    lptr[lbase + 64 * j] = (int32_t)((J >> 6) * (int64_t)(64 * hwu) + 64 * jj + (J & 63));
  }
}

// coarsest inverse, dof order -> node-interleaved order
__global__ __launch_bounds__(256) void permute_dense_kernel(int64_t n, const double* __restrict__ in,
                                                            double* __restrict__ out) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= n * n) return;
  const int64_t i = t / n, j = t % n, nv = n / 2;
  out[(2 * (i % nv) + i / nv) * n + (2 * (j % nv) + j / nv)] = in[t];
}

}  // namespace

int dev_csr_to_bsr(TmpPool* T, const DevMat& M, int64_t nr, int64_t nc, TBsr* B, std::string* err) {
  int rc;
  B->nr = nr; B->nc = nc; B->merged = false;
  if ((rc = T->alloc(&B->ptr, nr + 1, err))) return rc;
  HIPCHK(dev_memset(B->ptr, 0, sizeof(int64_t)));
  // rows whose wave ranges average over RS_CAP (the coarse Galerkin products;
  // A_0 averages ~1900) stage through the 64 KB column-only RS_CAP_LONG
  // variant: 2 waves per CU, but coalesced (level 1: 14.9 -> 12.2 ms)
  const unsigned g = (unsigned)((nr + RS_NODES - 1) / RS_NODES);
  const bool lng = nr && (double)M.nnz / (double)(2 * nr) * RS_NODES > RS_CAP;
  if (nr && lng) csr2bsr_kernel<false, RS_CAP_LONG><<<g, RS_NODES>>>(nr, nc, M.ptr, M.col, M.val, B->ptr, nullptr, nullptr);
  else if (nr) csr2bsr_kernel<false><<<g, RS_NODES>>>(nr, nc, M.ptr, M.col, M.val, B->ptr, nullptr, nullptr);
  HIPCHK(hipGetLastError());
  if ((rc = dscan_incl_i64(B->ptr, B->ptr, nr + 1, nullptr, err))) return rc;
  HIPCHK(hipMemcpy(&B->nb, B->ptr + nr, sizeof(int64_t), hipMemcpyDeviceToHost));
  if ((rc = T->alloc(&B->col, B->nb, err))) return rc;
  if ((rc = T->alloc(&B->val, B->nb, err))) return rc;
  // MAMG_CSR2BSR_FILL=0: the column + value staged fill (csr2bsr_kernel<true>; tests, A/B)
  const bool f2 = T->sw.csr2bsr_fill;
  if (nr && f2 && lng)
    csr2bsr_fill_kernel<RS_CAP_LONG><<<g, RS_NODES>>>(nr, nc, M.ptr, M.col, M.val, B->ptr, B->col, B->val);
  else if (nr && f2)
    csr2bsr_fill_kernel<RS_CAP><<<g, RS_NODES>>>(nr, nc, M.ptr, M.col, M.val, B->ptr, B->col, B->val);
  else if (nr)
    csr2bsr_kernel<true><<<g, RS_NODES>>>(nr, nc, M.ptr, M.col, M.val, B->ptr, B->col, B->val);
  HIPCHK(hipGetLastError());
  return MAMG_OK;
}

int dev_merge_rows(TmpPool* T, const TBsr& P, const TBsr& Q, TBsr* M, std::string* err) {
  int rc;
  const int64_t nr = P.nr;
  M->nr = nr; M->nc = P.nc; M->merged = true;
  if ((rc = T->alloc(&M->ptr, 2 * nr + 1, err))) return rc;
  if (nr) merge_len_kernel<<<nblocks(nr), 256>>>(nr, P.ptr, Q.ptr, M->ptr);
  HIPCHK(hipGetLastError());
  if ((rc = dscan_incl_i64(M->ptr, M->ptr, 2 * nr + 1, nullptr, err))) return rc;
  M->nb = P.nb + Q.nb;
  if ((rc = T->alloc(&M->col, M->nb, err))) return rc;
  if ((rc = T->alloc(&M->val, M->nb, err))) return rc;
  if (nr) merge_fill_kernel<<<nblocks(nr), 256>>>(nr, P.ptr, P.col, P.val, Q.ptr, Q.col, Q.val, M->ptr, M->col, M->val);
  HIPCHK(hipGetLastError());
  return MAMG_OK;
}

int dev_kmerge(TmpPool* T, const TBsr& P, const TBsr& Q, const double* W, TBsr* K, std::string* err) {
  int rc;
  const int64_t nr = P.nr;
  K->nr = nr; K->nc = P.nc; K->merged = false;
  if ((rc = T->alloc(&K->ptr, nr + 1, err))) return rc;
  HIPCHK(dev_memset(K->ptr, 0, sizeof(int64_t)));
  const dv4* Wv = reinterpret_cast<const dv4*>(W);
  if (nr) kmerge_kernel<false><<<nblocks(nr), 256>>>(nr, P.ptr, P.col, P.val, Q.ptr, Q.col, Q.val, Wv, K->ptr,
                                                      nullptr, nullptr);
  HIPCHK(hipGetLastError());
  if ((rc = dscan_incl_i64(K->ptr, K->ptr, nr + 1, nullptr, err))) return rc;
  HIPCHK(hipMemcpy(&K->nb, K->ptr + nr, sizeof(int64_t), hipMemcpyDeviceToHost));
  if ((rc = T->alloc(&K->col, K->nb, err))) return rc;
  if ((rc = T->alloc(&K->val, K->nb, err))) return rc;
  if (nr) kmerge_kernel<true><<<nblocks(nr), 256>>>(nr, P.ptr, P.col, P.val, Q.ptr, Q.col, Q.val, Wv, K->ptr,
                                                     K->col, K->val);
  HIPCHK(hipGetLastError());
  return MAMG_OK;
}

namespace {

// the schedule of G 256-row blocks for plane stride S (empty: keep row order)
std::vector<int32_t> band_sched(int64_t G, int64_t S, int nsub) {
  std::vector<int32_t> sched;
  const int64_t Pb = std::max<int64_t>(1, (S + 128) / 256), nb = 8 * (int64_t)nsub;
  if (nsub <= 0 || G < 64 || Pb < 4 * nb) return sched;
  std::vector<std::vector<int32_t>> L(8);
  for (int x = 0; x < 8; ++x)
    for (int sb = 0; sb < nsub; ++sb) {
      const int64_t band = (int64_t)x * nsub + sb, c0 = band * Pb / nb, c1 = (band + 1) * Pb / nb;
      for (int64_t p0 = 0; p0 < G; p0 += Pb)
        for (int64_t c = c0; c < c1 && p0 + c < G; ++c) L[x].push_back((int32_t)(p0 + c));
    }
  // balance to the round-robin dispatch: XCD x runs ceil / floor(G / 8)
  // workgroups; surplus tails move to the short lists
  std::vector<int32_t> spill;
  for (int x = 0; x < 8; ++x) {
    const size_t want = (size_t)(G / 8 + (x < G % 8 ? 1 : 0));
    while (L[x].size() > want) { spill.push_back(L[x].back()); L[x].pop_back(); }
  }
  for (int x = 0; x < 8; ++x) {
    const size_t want = (size_t)(G / 8 + (x < G % 8 ? 1 : 0));
    while (L[x].size() < want) { L[x].push_back(spill.back()); spill.pop_back(); }
  }
  sched.resize(G);
  std::vector<char> seen(G, 0);
  for (int64_t b = 0; b < G; ++b) {
    sched[b] = L[b % 8][b / 8];
    if (sched[b] < 0 || sched[b] >= G || seen[sched[b]]++) return std::vector<int32_t>();
  }
  return sched;
}

int upload_sched(HandleMem* h, const std::vector<int32_t>& sched, int32_t** d, int64_t* n, std::string* err) {
  int rc;
  if ((rc = dalloc(h, d, (int64_t)sched.size(), err))) return rc;
  HIPCHK(hipMemcpy(*d, sched.data(), sched.size() * sizeof(int32_t), hipMemcpyHostToDevice));
  *n = (int64_t)sched.size();
  return MAMG_OK;
}

// Band schedule for the half-symmetric kernel.  A lower block (I, J < I) is
// re-read from row J's upper part; with the rows of a structured 3-D mesh in
// lexicographic order the farthest mirror sits one plane (stride S rows)
// back.  Row order alone puts a whole plane (~16 MB at n = 256) between the
// two reads, more than an XCD's 4 MB L2.  The schedule cuts each plane of
// 256-row blocks into 8 x nsub bands, gives XCD x (workgroups b = x mod 8)
// the bands x nsub .. x nsub + nsub - 1 and walks each band plane by plane,
// so the mirror was streamed one band (S / (8 nsub) rows) earlier on the same
// XCD.  S = the median, over sampled rows, of the distance to the row's first
// (smallest) column.  The schedule only permutes which workgroup computes
// which rows: every row is still summed by one lane in its own order, so the
// result is bitwise that of any other order.  Unstructured or narrow-band
// matrices (< 4 blocks per band) keep the row_block order.
int build_band_sched(HandleMem* h, const TBsr& B, DBsr* D, std::string* err) {
  const int64_t nr = B.nr, G = (nr + 255) / 256;
  if (h->sw.half_bands <= 0 || G < 64) return MAMG_OK;
  const int ns = 257;
  std::vector<int64_t> off;
  for (int i = 0; i < ns; ++i) {
    const int64_t I = nr / 4 + (nr / 2) * i / ns;
    int64_t p = 0;
    int32_t c = 0;
    HIPCHK(hipMemcpy(&p, B.ptr + I, sizeof(int64_t), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(&c, B.col + p, sizeof(int32_t), hipMemcpyDeviceToHost));
    if (c < I) off.push_back(I - c);
  }
  if (off.size() < ns / 2) return MAMG_OK;
  std::nth_element(off.begin(), off.begin() + off.size() / 2, off.end());
  const std::vector<int32_t> sched = band_sched(G, off[off.size() / 2], h->sw.half_bands);
  if (sched.empty()) return MAMG_OK;
  D->band_stride = off[off.size() / 2];
  return upload_sched(h, sched, &D->sched, &D->nsched, err);
}

}  // namespace

// the same for the launch over rows [r0, r1) only (block b covers rows
// r0 + 256 b ..): the multi-GPU interior run
int build_band_sched_range(HandleMem* h, DBsr* D, int64_t r0, int64_t r1, std::string* err) {
  if (!D->half || D->band_stride <= 0 || r1 <= r0) return MAMG_OK;
  const std::vector<int32_t> sched = band_sched((r1 - r0 + 255) / 256, D->band_stride, h->sw.half_bands);
  if (sched.empty()) return MAMG_OK;
  D->sr0 = r0;
  D->sr1 = r1;
  return upload_sched(h, sched, &D->sched_r, &D->nsched_r, err);
}

namespace {

// first column of the first non-empty row of each group of rpw rows (-1: none)
__global__ void wg_first_col_kernel(int64_t G, int rpw, int64_t nr, const int64_t* __restrict__ ptr,
                                    const int32_t* __restrict__ col, int32_t* __restrict__ out) {
  const int64_t b = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (b >= G) return;
  int32_t c = -1;
  for (int64_t i = b * rpw; i < nr && i < (b + 1) * rpw; ++i)
    if (ptr[i] < ptr[i + 1]) { c = col[ptr[i]]; break; }
  out[b] = c;
}

// Plane-band schedule of the level-0 restriction R_0 (coarse rows, fine
// columns).  A coarse row gathers r_1 over its smoothed aggregate, ~5 fine
// planes deep; coarse rows come in aggregate order, i.e. coarse plane after
// coarse plane, so a fine plane is gathered again by the next coarse plane's
// rows -- one coarse plane of R_0 (~30 MB at n = 256) later, long gone from
// an XCD's 4 MB L2 when each XCD walks whole planes.  Here a workgroup's key
// is the in-plane position (first column mod the fine plane stride Sf) of its
// first row: the plane is cut into 8 nsub bands, XCD x (workgroups b = x mod
// 8) takes the bands x nsub .. x nsub + nsub - 1 and walks each through all
// planes, so the re-gather is one band-plane of R_0 later and still in L2.
// Only which workgroup computes which rows changes: results are bitwise.
std::vector<int32_t> rest_band_sched(const std::vector<int32_t>& c0, int64_t Sf, int nsub) {
  std::vector<int32_t> sched;
  const int64_t G = (int64_t)c0.size(), nb = 8 * (int64_t)nsub;
  if (nsub <= 0 || Sf <= 0 || G < 64 * nb) return sched;
  std::vector<std::vector<int32_t>> L(8);
  std::vector<std::vector<int32_t>> band(nb);
  int64_t last = 0;
  for (int64_t b = 0; b < G; ++b) {
    const int64_t c = c0[b] >= 0 ? c0[b] : last;
    last = c;
    band[std::min<int64_t>(nb - 1, (c % Sf) * nb / Sf)].push_back((int32_t)b);
  }
  for (int64_t k = 0; k < nb; ++k) L[k / nsub].insert(L[k / nsub].end(), band[k].begin(), band[k].end());
  std::vector<int32_t> spill;   // balance to the round-robin dispatch, as band_sched
  for (int x = 0; x < 8; ++x) {
    const size_t want = (size_t)(G / 8 + (x < G % 8 ? 1 : 0));
    while (L[x].size() > want) { spill.push_back(L[x].back()); L[x].pop_back(); }
  }
  for (int x = 0; x < 8; ++x) {
    const size_t want = (size_t)(G / 8 + (x < G % 8 ? 1 : 0));
    while (L[x].size() < want && !spill.empty()) { L[x].push_back(spill.back()); spill.pop_back(); }
  }
  sched.resize(G);
  std::vector<char> seen(G, 0);
  for (int64_t b = 0; b < G; ++b) {
    if ((size_t)(b / 8) >= L[b % 8].size()) return std::vector<int32_t>();
    sched[b] = L[b % 8][b / 8];
    if (sched[b] < 0 || sched[b] >= G || seen[sched[b]]++) return std::vector<int32_t>();
  }
  return sched;
}

// the schedule for D (a lane-group BSR, not SELL / merged) given the fine
// plane stride Sf of its columns
int build_rest_sched(HandleMem* h, TmpPool* T, DBsr* D, int64_t Sf, std::string* err) {
  if (h->sw.r_bands <= 0 || Sf <= 0 || D->sell || D->half || !D->ptr || D->lanes <= 0) return MAMG_OK;
  const int rpw = 256 / D->lanes;
  const int64_t G = (D->nr * (int64_t)D->lanes + 255) / 256;
  if (G < 64 * 8 * (int64_t)h->sw.r_bands || G >= ((int64_t)1 << 31)) return MAMG_OK;
  int rc;
  int32_t* c0 = nullptr;
  if ((rc = T->alloc(&c0, G, err))) return rc;
  wg_first_col_kernel<<<nblocks(G), 256>>>(G, rpw, D->nr, D->ptr, D->col, c0);
  HIPCHK(hipGetLastError());
  std::vector<int32_t> hc(G);
  HIPCHK(hipMemcpy(hc.data(), c0, G * sizeof(int32_t), hipMemcpyDeviceToHost));
  T->release(c0);
  const std::vector<int32_t> sched = rest_band_sched(hc, Sf, h->sw.r_bands);
  if (sched.empty()) return MAMG_OK;
  if ((rc = upload_sched(h, sched, &D->rsched, &D->nrsched, err))) return rc;
  D->rsched_vl = D->lanes;
  return MAMG_OK;
}

// ---- row-pattern dictionary (DBsr::rowdict, rowdict2_kernel) ----------------
constexpr int RD_SLOTS = 4096;   // hash table slots (>= 2 x the cap on types)

__device__ __forceinline__ unsigned long long rd_mix(unsigned long long h, unsigned long long w) {
  h = (h ^ w) * 0x9E3779B97F4A7C15ull;
  return h ^ (h >> 29);
}
__device__ __forceinline__ int rd_slot0(unsigned long long key) {
  return (int)((key * 0xD6E8FEB86659FD93ull) >> 52);   // RD_SLOTS = 2^12
}

// Key of every node row: the hash of (length, column - row and value bits of
// each block) masked to `bits` bits, plus 1 (0 marks an empty slot).  The key
// goes into a small open-addressed table with the smallest row that holds it.
// flags: [0] distinct keys, [1] abort (too many keys), [2] a row longer than
// maxlen, [3] longest row.  Nearly every row meets its key already in the
// table with a smaller row: those issue no atomic.
__global__ __launch_bounds__(256) void rowdict_hash_kernel(int64_t nr, const int64_t* __restrict__ ptr,
                                                           const int32_t* __restrict__ col,
                                                           const dv4* __restrict__ val, int bits, int max_types,
                                                           int maxlen, unsigned long long* keys,
                                                           unsigned long long* minrow, int* flags,
                                                           unsigned long long* __restrict__ rowkey) {
  const int64_t I = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (I >= nr) return;
  // every row's length is looked at (the refusal reason does not depend on
  // timing); the hashing stops once the attempt is lost
  const int64_t p0 = ptr[I], p1 = ptr[I + 1];
  const int64_t len = p1 - p0;
  if (len > __hip_atomic_load(flags + 3, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
    atomicMax(flags + 3, (int)(len < 0x7fffffff ? len : 0x7fffffff));
  if (len > maxlen) { atomicOr(flags + 2, 1); return; }
  if (__hip_atomic_load(flags + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) |
      __hip_atomic_load(flags + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
    return;
  unsigned long long h = rd_mix(0x243F6A8885A308D3ull, (unsigned long long)len);
  for (int64_t k = p0; k < p1; ++k) {
    const dv4 v = val[k];
    h = rd_mix(h, (unsigned long long)(int64_t)(col[k] - I));
    h = rd_mix(h, (unsigned long long)__double_as_longlong(v.x));
    h = rd_mix(h, (unsigned long long)__double_as_longlong(v.y));
    h = rd_mix(h, (unsigned long long)__double_as_longlong(v.z));
    h = rd_mix(h, (unsigned long long)__double_as_longlong(v.w));
  }
  const unsigned long long key = (h & ((1ull << bits) - 1ull)) + 1ull;
  rowkey[I] = key;
  int s = rd_slot0(key);
  for (int probe = 0; probe < RD_SLOTS; ++probe, s = (s + 1) & (RD_SLOTS - 1)) {
    unsigned long long cur = __hip_atomic_load(keys + s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (cur == 0ull) {
      cur = atomicCAS(keys + s, 0ull, key);
      if (cur == 0ull) {
        if (atomicAdd(flags, 1) + 1 > max_types) atomicOr(flags + 1, 1);
        cur = key;
      }
    }
    if (cur == key) {
      if (__hip_atomic_load(minrow + s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > (unsigned long long)I)
        atomicMin(minrow + s, (unsigned long long)I);
      return;
    }
  }
  atomicOr(flags + 1, 1);   // table full
}

// the table: entry j of type t from the type's first row reps[t]
__global__ __launch_bounds__(256) void rowdict_table_kernel(int nt, int rw, const int64_t* __restrict__ reps,
                                                            const int64_t* __restrict__ ptr,
                                                            const int32_t* __restrict__ col,
                                                            const dv4* __restrict__ val, int sym,
                                                            int32_t* __restrict__ rlen, int32_t* __restrict__ rdelta,
                                                            double* __restrict__ rval) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= nt * rw) return;
  const int t = i / rw, j = i % rw;
  const int64_t I = reps[t], p0 = ptr[I];
  const int len = (int)(ptr[I + 1] - p0);
  if (j == 0) rlen[t] = len;
  dv4 a = {0.0, 0.0, 0.0, 0.0};
  int32_t d = 0;
  if (j < len) {
    a = val[p0 + j];
    d = (int32_t)(col[p0 + j] - I);
  }
  rdelta[i] = d;
  if (sym) {
    const int64_t nbs = (int64_t)nt * rw;
    rval[2 * i] = a.x;
    rval[2 * i + 1] = a.w;
    rval[2 * nbs + i] = a.y;
  } else {
    reinterpret_cast<dv4*>(rval)[i] = a;
  }
}

// Every row against its type's table, entry by entry and bitwise (length,
// column - row, all four value words) and 0 <= row + delta < nc; the row's
// code is written.  Any difference (a hash collision included) sets *bad.
__global__ __launch_bounds__(256) void rowdict_verify_kernel(int64_t nr, int64_t nc, const int64_t* __restrict__ ptr,
                                                             const int32_t* __restrict__ col,
                                                             const dv4* __restrict__ val,
                                                             const unsigned long long* __restrict__ rowkey,
                                                             const unsigned long long* __restrict__ keys,
                                                             const int32_t* __restrict__ slot_type, int rw,
                                                             const int64_t* __restrict__ reps,
                                                             const int32_t* __restrict__ rlen,
                                                             const int32_t* __restrict__ rdelta,
                                                             uint16_t* __restrict__ rcode, int* bad) {
  const int64_t I = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (I >= nr) return;
  const unsigned long long key = rowkey[I];
  int s = rd_slot0(key), t = -1;
  for (int probe = 0; probe < RD_SLOTS; ++probe, s = (s + 1) & (RD_SLOTS - 1)) {
    const unsigned long long cur = keys[s];
    if (cur == key) { t = slot_type[s]; break; }
    if (cur == 0ull) break;
  }
  if (t < 0) { atomicOr(bad, 1); rcode[I] = 0; return; }
  rcode[I] = (uint16_t)t;
  const int64_t p0 = ptr[I], q0 = ptr[reps[t]];
  const int len = rlen[t];
  bool ok = ptr[I + 1] - p0 == (int64_t)len;
  if (ok)
    for (int j = 0; j < len; ++j) {
      const int64_t d = (int64_t)col[p0 + j] - I, c = I + d;
      const dv4 a = val[p0 + j], r = val[q0 + j];
      ok = ok && d == (int64_t)rdelta[t * rw + j] && c >= 0 && c < nc &&
           __double_as_longlong(a.x) == __double_as_longlong(r.x) &&
           __double_as_longlong(a.y) == __double_as_longlong(r.y) &&
           __double_as_longlong(a.z) == __double_as_longlong(r.z) &&
           __double_as_longlong(a.w) == __double_as_longlong(r.w);
    }
  if (!ok) atomicOr(bad, 1);
}

// Row-pattern dictionary for the one-GPU level-0 A (nr == nc).  Returns
// MAMG_OK with D->rowdict set, or MAMG_OK with it false and the reason in
// D->rdinfo[RD_REASON] (the caller then builds the half / SELL layout exactly
// as without the attempt; the temporaries of a refused attempt go back to the
// pool).  The types are numbered by the smallest row that holds each, which
// does not depend on the order the atomics ran in.
int try_rowdict(HandleMem* h, TmpPool* T, const TBsr& B, DBsr* D, bool sym, std::string* err) {
  int rc;
  const int64_t nr = B.nr;
  int64_t* info = D->rdinfo;
  info[RD_TAKEN] = 0;
  auto refuse = [&](int why) { info[RD_REASON] = why; return MAMG_OK; };
  if (nr != B.nc) return refuse(RDR_NOT_SQUARE);
  if (nr < h->sw.rowdict_min_rows || nr < 1 || B.nb < 1) return refuse(RDR_THRESHOLD);
  const int max_types = h->sw.rowdict_max_types;
  unsigned long long *keys = nullptr, *minrow = nullptr, *rowkey = nullptr;
  int* flags = nullptr;   // + [4]: the verification's mismatch flag
  if ((rc = T->alloc(&keys, RD_SLOTS, err))) return rc;
  if ((rc = T->alloc(&minrow, RD_SLOTS, err))) return rc;
  if ((rc = T->alloc(&flags, 8, err))) return rc;
  if ((rc = T->alloc(&rowkey, nr, err))) return rc;
  auto drop = [&](int why) {
    T->release(keys); T->release(minrow); T->release(flags); T->release(rowkey);
    return refuse(why);
  };
  HIPCHK(dev_memset(keys, 0, RD_SLOTS * sizeof(unsigned long long)));
  HIPCHK(dev_memset(minrow, 0xff, RD_SLOTS * sizeof(unsigned long long)));
  HIPCHK(dev_memset(flags, 0, 8 * sizeof(int)));
  rowdict_hash_kernel<<<nblocks(nr), 256>>>(nr, B.ptr, B.col, B.val, h->sw.rowdict_hash_bits, max_types,
                                            ROWDICT_MAX_LEN, keys, minrow, flags, rowkey);
  HIPCHK(hipGetLastError());
  int hf[4] = {0, 0, 0, 0};
  HIPCHK(hipMemcpy(hf, flags, sizeof hf, hipMemcpyDeviceToHost));
  info[RD_TYPES] = hf[0];
  info[RD_MAXLEN] = hf[3];
  if (hf[2]) return drop(RDR_LENGTH);
  if (hf[1] || hf[0] > max_types) return drop(RDR_TYPES);
  std::vector<unsigned long long> hk(RD_SLOTS), hm(RD_SLOTS);
  HIPCHK(hipMemcpy(hk.data(), keys, RD_SLOTS * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(hm.data(), minrow, RD_SLOTS * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  std::vector<std::pair<int64_t, int>> occ;   // (first row, slot)
  for (int s = 0; s < RD_SLOTS; ++s)
    if (hk[s]) occ.push_back({(int64_t)hm[s], s});
  std::sort(occ.begin(), occ.end());
  const int nt = (int)occ.size(), rw = hf[3];
  if (nt < 1 || rw < 1) return drop(RDR_THRESHOLD);
  const int per = sym ? 3 : 4;
  const int64_t nbs = (int64_t)nt * rw;
  const int64_t table = 4 * (int64_t)nt + nbs * (4 + 8 * per);
  info[RD_TABLE_BYTES] = table;
  if (table > ROWDICT_MAX_TABLE) return drop(RDR_TABLE);
  std::vector<int32_t> st(RD_SLOTS, -1);
  std::vector<int64_t> reps(nt);
  for (int t = 0; t < nt; ++t) {
    st[occ[t].second] = t;
    reps[t] = occ[t].first;
  }
  int32_t *slot_type = nullptr, *rlen = nullptr, *rdelta = nullptr;
  int64_t* dreps = nullptr;
  double* rval = nullptr;
  uint16_t* rcode = nullptr;
  if ((rc = T->alloc(&slot_type, RD_SLOTS, err))) return rc;
  if ((rc = T->alloc(&dreps, nt, err))) return rc;
  if ((rc = T->alloc(&rlen, nt, err))) return rc;
  if ((rc = T->alloc(&rdelta, nbs, err))) return rc;
  if ((rc = T->alloc(&rval, per * nbs, err))) return rc;
  if ((rc = T->alloc(&rcode, nr, err))) return rc;
  auto drop2 = [&](int why) {
    T->release(slot_type); T->release(dreps); T->release(rlen); T->release(rdelta); T->release(rval);
    T->release(rcode);
    return drop(why);
  };
  HIPCHK(hipMemcpy(slot_type, st.data(), RD_SLOTS * sizeof(int32_t), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(dreps, reps.data(), nt * sizeof(int64_t), hipMemcpyHostToDevice));
  rowdict_table_kernel<<<nblocks(nbs), 256>>>(nt, rw, dreps, B.ptr, B.col, B.val, sym ? 1 : 0, rlen, rdelta, rval);
  HIPCHK(hipGetLastError());
  rowdict_verify_kernel<<<nblocks(nr), 256>>>(nr, B.nc, B.ptr, B.col, B.val, rowkey, keys, slot_type, rw, dreps, rlen,
                                              rdelta, rcode, flags + 4);
  HIPCHK(hipGetLastError());
  int bad = 1;
  HIPCHK(hipMemcpy(&bad, flags + 4, sizeof(int), hipMemcpyDeviceToHost));
  if (bad) return drop2(RDR_VERIFY);
  if ((rc = dalloc(h, &D->rcode, nr, err))) return rc;
  if ((rc = dalloc(h, &D->rlen, nt, err))) return rc;
  if ((rc = dalloc(h, &D->rdelta, nbs, err))) return rc;
  if ((rc = dalloc(h, &D->val, per * nbs, err))) return rc;
  HIPCHK(dev_copy(D->rcode, rcode, nr * sizeof(uint16_t)));
  HIPCHK(dev_copy(D->rlen, rlen, nt * sizeof(int32_t)));
  HIPCHK(dev_copy(D->rdelta, rdelta, nbs * sizeof(int32_t)));
  HIPCHK(dev_copy(D->val, rval, per * nbs * sizeof(double)));
  drop2(RDR_NONE);
  D->rowdict = true;
  D->rw = rw;
  D->rtypes = nt;
  D->nbs = nbs;
  info[RD_TAKEN] = 1;
  info[RD_TYPES] = nt;
  return build_band_sched(h, B, D, err);
}

}  // namespace

// half-symmetric ELL-64 for a symmetric-block A whose owned part (columns
// < nr) is symmetric bitwise; columns >= nr (ghosts of a rank-local A) go to
// the ghost part (hsell2_kernel).  Returns MAMG_OK with D->half set, or
// MAMG_OK with D->half false when a mirror is missing or differs, a row part
// is too long, or the ELL padding would exceed ~30 % (the caller then builds
// SELL-64); temporaries of a rejected attempt are freed with the pool.
int try_half(HandleMem* h, TmpPool* T, const TBsr& B, DBsr* D, std::string* err) {
  int rc;
  const int64_t nr = B.nr, ns = (nr + SELL_C - 1) / SELL_C;
  int* wm = nullptr;   // [0] max upper, [1] max lower, [2] part too long, [3] not symmetric
  int32_t* meta = nullptr;
  unsigned long long* nlod = nullptr;
  int64_t* gsoff = nullptr;
  if ((rc = T->alloc(&wm, 4, err))) return rc;
  if ((rc = T->alloc(&meta, nr, err))) return rc;
  if ((rc = T->alloc(&nlod, 1, err))) return rc;
  if ((rc = T->alloc(&gsoff, ns + 1, err))) return rc;
  HIPCHK(dev_memset(wm, 0, 4 * sizeof(int)));
  HIPCHK(dev_memset(nlod, 0, sizeof(unsigned long long)));
  half_meta_kernel<<<std::min(nblocks(nr), HALF_META_BLOCKS), 256>>>(nr, B.ptr, B.col, meta, wm, nlod);
  HIPCHK(hipGetLastError());
  int hw[4] = {0, 0, 0, 0};
  unsigned long long nloh = 0;
  HIPCHK(hipMemcpy(hw, wm, 4 * sizeof(int), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(&nloh, nlod, sizeof(nloh), hipMemcpyDeviceToHost));
  if (hw[2]) return MAMG_OK;
  half_gwidth_kernel<<<nblocks(ns), 256>>>(nr, meta, gsoff);
  HIPCHK(hipGetLastError());
  if ((rc = dscan_incl_i64(gsoff, gsoff, ns + 1, nullptr, err))) return rc;
  int64_t ngs = 0;
  HIPCHK(hipMemcpy(&ngs, gsoff + ns, sizeof(int64_t), hipMemcpyDeviceToHost));
  const int64_t nlo = (int64_t)nloh;
  const int64_t su = 64 * ns * (int64_t)hw[0], sl = 64 * ns * (int64_t)hw[1];
  const int64_t nup = B.nb - nlo;   // upper + ghost entries
  if (su >= (int64_t)1 << 31 || (double)(su + ngs) > 1.3 * nup + 4096 || (double)sl > 1.3 * nlo + 4096)
    return MAMG_OK;
  half_fill_kernel<<<nblocks(nr), 256>>>(nr, B.ptr, B.col, B.val, meta, hw[0], hw[1], su, nullptr, nullptr,
                                         nullptr, nullptr, 0, nullptr, nullptr, wm + 3, 1);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpy(&hw[3], wm + 3, sizeof(int), hipMemcpyDeviceToHost));
  if (hw[3]) return MAMG_OK;   // a mirror is missing or differs
  if ((rc = dalloc(h, &D->meta, std::max<int64_t>(nr, 1), err))) return rc;
  if ((rc = dalloc(h, &D->col, std::max<int64_t>(su, 1), err))) return rc;
  if ((rc = dalloc(h, &D->val, std::max<int64_t>(3 * su, 1), err))) return rc;
  if ((rc = dalloc(h, &D->lptr, std::max<int64_t>(sl, 1), err))) return rc;
  if (ngs) {
    if ((rc = dalloc(h, &D->gsoff, ns + 1, err))) return rc;
    if ((rc = dalloc(h, &D->gcol, ngs, err))) return rc;
    if ((rc = dalloc(h, &D->gval, 3 * ngs, err))) return rc;
    HIPCHK(dev_copy(D->gsoff, gsoff, (ns + 1) * sizeof(int64_t)));
    HIPCHK(dev_memset(D->gcol, 0, ngs * sizeof(int32_t)));
    HIPCHK(dev_memset(D->gval, 0, 3 * ngs * sizeof(double)));
  }
  HIPCHK(dev_copy(D->meta, meta, nr * sizeof(int32_t)));
  HIPCHK(dev_memset(D->col, 0, std::max<int64_t>(su, 1) * sizeof(int32_t)));
  HIPCHK(dev_memset(D->val, 0, std::max<int64_t>(3 * su, 1) * sizeof(double)));
  HIPCHK(dev_memset(D->lptr, 0, std::max<int64_t>(sl, 1) * sizeof(int32_t)));
  half_fill_kernel<<<nblocks(nr), 256>>>(nr, B.ptr, B.col, B.val, meta, hw[0], hw[1], su, D->col, D->val, D->lptr,
                                         D->gsoff, ngs, D->gcol, D->gval, wm + 3, 0);
  HIPCHK(hipGetLastError());
  D->half = true;
  D->hwu = hw[0];
  D->hwl = hw[1];
  D->nbs = su;
  D->nlo = nlo;
  D->ngs = ngs;
  return build_band_sched(h, B, D, err);
}

// host BSR2 (multi-GPU rank-local level-0 A: owned rows, [owned | ghost]
// columns) -> half-symmetric ELL-64 when its owned part is symmetric bitwise,
// else upload_bsr (SELL-64 / lane groups)
int upload_half_or_bsr(HandleMem* h, const HBsr& B, DBsr* D, std::string* err) {
  const int64_t np = (int64_t)B.ptr.size();
  if (h->sw.half && B.nr >= h->sw.sell_min_rows && np == B.nr + 1 && blocks_symmetric(B)) {
    int rc;
    TmpPool T(h->sw);
    TBsr tb;
    tb.nr = B.nr; tb.nc = B.nc; tb.nb = B.ptr[B.nr];
    if ((rc = T.alloc(&tb.ptr, np, err))) return rc;
    if ((rc = T.alloc(&tb.col, tb.nb, err))) return rc;
    if ((rc = T.alloc(&tb.val, tb.nb, err))) return rc;
    HIPCHK(hipMemcpy(tb.ptr, B.ptr.data(), np * sizeof(int64_t), hipMemcpyHostToDevice));
    if (tb.nb) {
      HIPCHK(hipMemcpy(tb.col, B.col.data(), tb.nb * sizeof(int32_t), hipMemcpyHostToDevice));
      HIPCHK(hipMemcpy(tb.val, B.val.data(), tb.nb * sizeof(dv4), hipMemcpyHostToDevice));
    }
    D->nr = B.nr;
    D->nc = B.nc;
    D->nb = tb.nb;
    D->lanes = pick_lanes_bsr(B.nr, D->nb);
    D->sym = true;
    if ((rc = try_half(h, &T, tb, D, err))) return rc;
    if (D->half) return MAMG_OK;
  }
  return upload_bsr(h, B, D, 0, err, true);
}

// final apply layout from a raw device BSR (the device-side counterpart of
// upload_bsr): SELL-64 for large short-row plain matrices, symmetric-block
// packing where every block has (0,1) == (1,0) bitwise, else 4 doubles/block
int finalize_bsr(HandleMem* h, TmpPool* T, TBsr& B, DBsr* D, int lanes, bool sym_ok, std::string* err,
                 bool allow_sell, bool allow_half, bool allow_msell) {
  int rc;
  const int64_t nr = B.nr, np = B.merged ? 2 * nr + 1 : nr + 1;
  D->nr = nr;
  D->nc = B.nc;
  D->nb = B.nb;
  D->lanes = lanes > 0 ? lanes : pick_lanes_bsr(nr, D->nb);
  bool sym = false;
  if (sym_ok && !B.merged && B.nb > 0) {
    int* bad = nullptr;
    if ((rc = T->alloc(&bad, 1, err))) return rc;
    HIPCHK(dev_memset(bad, 0, sizeof(int)));
    sym_check_kernel<<<std::min(nblocks(B.nb), SYM_CHECK_BLOCKS), 256>>>(B.nb, B.val, bad);
    int hb = 1;
    HIPCHK(hipMemcpy(&hb, bad, sizeof(int), hipMemcpyDeviceToHost));
    sym = hb == 0;
  }
  D->sym = sym;
  const int per = sym ? 3 : 4;
  // multi-lane SELL (msell_kernel) for the coarse levels' A and K: lanes per
  // row from the mean row length, chunks of 5 blocks per lane
  const bool msell = allow_sell && allow_msell && !B.merged && nr >= h->sw.msell_min_rows &&
                     nr < h->sw.sell_min_rows;
  if (msell) {
    const double mean = nr ? (double)D->nb / (double)nr : 0.0;
    D->lpr = mean <= 10.0 ? 2 : mean <= 20.0 ? 4 : mean <= 40.0 ? 8 : 16;
  }
  if (allow_half) D->rdinfo[RD_REASON] = RDR_THRESHOLD;   // the one-GPU level-0 A: below the SELL threshold
  if (allow_sell && ((nr >= h->sw.sell_min_rows && D->nb <= sell_max_len * nr) || msell) && !B.merged) {
    if (allow_half) {   // rows that repeat: the row-pattern dictionary, no matrix stream at all
      if ((rc = try_rowdict(h, T, B, D, sym, err))) return rc;
      if (D->rowdict) return MAMG_OK;
    }
    if (allow_half && h->sw.half && sym && nr == B.nc) {
      if ((rc = try_half(h, T, B, D, err))) return rc;
      if (D->half) return MAMG_OK;
    }
    const int64_t ns = (nr + SELL_C - 1) / SELL_C;
    int* bad = nullptr;
    if ((rc = T->alloc(&bad, 1, err))) return rc;
    HIPCHK(dev_memset(bad, 0, sizeof(int)));
    D->sell = true;
    if ((rc = dalloc(h, &D->soff, ns + 1, err))) return rc;
    if ((rc = dalloc(h, &D->meta, std::max<int64_t>(nr, 1), err))) return rc;
    sell_meta_kernel<<<nblocks(ns), 256>>>(nr, B.ptr, 0, D->meta, D->soff, bad);
    HIPCHK(hipGetLastError());
    int hb = 0;
    HIPCHK(hipMemcpy(&hb, bad, sizeof(int), hipMemcpyDeviceToHost));
    if (hb) { *err = "SELL: row longer than 65534 blocks"; return MAMG_ERR_UNSUPPORTED; }
    if ((rc = dscan_incl_i64(D->soff, D->soff, ns + 1, nullptr, err))) return rc;
    HIPCHK(hipMemcpy(&D->nbs, D->soff + ns, sizeof(int64_t), hipMemcpyDeviceToHost));
    if ((rc = dalloc(h, &D->col, std::max<int64_t>(D->nbs, 1), err))) return rc;
    if ((rc = dalloc(h, &D->val, std::max<int64_t>(per * D->nbs, 1), err))) return rc;
    HIPCHK(dev_memset(D->col, 0, std::max<int64_t>(D->nbs, 1) * sizeof(int32_t)));
    HIPCHK(dev_memset(D->val, 0, std::max<int64_t>(per * D->nbs, 1) * sizeof(double)));
    sell_fill_kernel<<<nblocks(nr), 256>>>(nr, B.ptr, 0, B.col, B.val, D->soff, D->nbs, sym ? 1 : 0, D->col, D->val);
    HIPCHK(hipGetLastError());
    return MAMG_OK;
  }
  if ((rc = dalloc(h, &D->ptr, np, err))) return rc;
  if ((rc = dalloc(h, &D->col, std::max<int64_t>(D->nb, 1), err))) return rc;
  if ((rc = dalloc(h, &D->val, std::max<int64_t>(per * D->nb, 1), err))) return rc;
  HIPCHK(dev_copy(D->ptr, B.ptr, np * sizeof(int64_t)));
  if (D->nb) {
    HIPCHK(dev_copy(D->col, B.col, D->nb * sizeof(int32_t)));
    if (sym) pack_sym_kernel<<<nblocks(D->nb), 256>>>(D->nb, B.val, D->val);
    else HIPCHK(dev_copy(D->val, B.val, D->nb * sizeof(dv4)));
    HIPCHK(hipGetLastError());
  }
  return MAMG_OK;
}

// Level-0 K's rows sorted by length inside each SELL slice (MAMG_K_SORT, default
// on).  A 128-byte line of one block slot holds 4 neighbouring rows' blocks;
// in row order their lengths differ, so the last slots of the longer rows pull
// whole lines whose other quarters are padding: 13 % more line bytes than
// stored blocks for the bidomain K.  Sorted, the rows sharing a line have equal
// or neighbouring lengths (1.9 %).  Each row keeps its blocks and their order:
// results are bitwise those of row order (test_k_row_sort_bitwise).
int sort_sell_slices(HandleMem* h, TmpPool* T, DBsr* D, std::string* err) {
  int rc;
  if (!D->sell || D->split || D->nr == 0) return MAMG_OK;
  const int64_t ns = (D->nr + SELL_C - 1) / SELL_C, per = D->sym ? 3 : 4;
  int32_t *nmeta = nullptr, *src = nullptr, *ncol = nullptr;
  double* nval = nullptr;
  if ((rc = T->alloc(&nmeta, D->nr, err)) || (rc = T->alloc(&src, D->nr, err)) ||
      (rc = T->alloc(&ncol, std::max<int64_t>(D->nbs, 1), err)) ||
      (rc = T->alloc(&nval, std::max<int64_t>(per * D->nbs, 1), err)))
    return rc;
  HIPCHK(dev_memset(ncol, 0, std::max<int64_t>(D->nbs, 1) * sizeof(int32_t)));
  HIPCHK(dev_memset(nval, 0, std::max<int64_t>(per * D->nbs, 1) * sizeof(double)));
  sell_sort_kernel<<<(unsigned)ns, SELL_C>>>(D->nr, D->meta, nmeta, src);
  HIPCHK(hipGetLastError());
  sell_permute_kernel<<<(unsigned)ns, SELL_C>>>(D->nr, D->soff, src, D->nbs, (int)per, D->col, D->val, ncol, nval);
  HIPCHK(hipGetLastError());
  HIPCHK(dev_copy(D->meta, nmeta, D->nr * sizeof(int32_t)));
  HIPCHK(dev_copy(D->col, ncol, D->nbs * sizeof(int32_t)));
  HIPCHK(dev_copy(D->val, nval, per * D->nbs * sizeof(double)));
  T->release(nmeta); T->release(src); T->release(ncol); T->release(nval);
  D->lsort = true;
  return MAMG_OK;
}

namespace {

// SELL columns as 16-bit offsets from a per-slice base (round 6, level-0 K:
// MAMG_K_COL16, default on).  K's columns are coarse node ids; the 64 rows of
// a slice reach the aggregates of a few neighbouring planes, so every slice's
// columns span far less than 2^16 (at nrefs=6: 4-byte columns are 11 % of K's
// stream).  cbase[s] = the slice's smallest column; a matrix with any slice
// spanning more keeps its 32-bit columns (then nothing changes).  The kernel
// adds the base back: the same columns, the same sums, bitwise the 32-bit
// layout (tests/test_gpu.py::test_k_col16_bitwise).
__global__ __launch_bounds__(64) void sell_span_kernel(int64_t nr, const int64_t* __restrict__ soff,
                                                       const int32_t* __restrict__ meta,
                                                       const int32_t* __restrict__ col, int32_t* __restrict__ cbase,
                                                       int* wide) {
  const int64_t s = blockIdx.x, slot = s * SELL_C + threadIdx.x;
  int32_t lo = INT32_MAX, hi = INT32_MIN;
  if (slot < nr) {
    const int len = meta[slot] & 0xffff;
    const int64_t k = soff[s] + threadIdx.x;
    for (int j = 0; j < len; ++j) {
      const int32_t c = col[k + (int64_t)SELL_C * j];
      lo = c < lo ? c : lo;
      hi = c > hi ? c : hi;
    }
  }
  for (int o = 32; o > 0; o >>= 1) {
    const int32_t a = __shfl_xor(lo, o), b = __shfl_xor(hi, o);
    lo = a < lo ? a : lo;
    hi = b > hi ? b : hi;
  }
  if (threadIdx.x == 0) {
    cbase[s] = lo == INT32_MAX ? 0 : lo;
    if (hi != INT32_MIN && (int64_t)hi - (int64_t)lo > 65535) atomicOr(wide, 1);
  }
}
__global__ __launch_bounds__(64) void sell_col16_kernel(int64_t nr, const int64_t* __restrict__ soff,
                                                        const int32_t* __restrict__ meta,
                                                        const int32_t* __restrict__ col,
                                                        const int32_t* __restrict__ cbase, uint16_t* __restrict__ c16) {
  const int64_t s = blockIdx.x, slot = s * SELL_C + threadIdx.x;
  if (slot >= nr) return;
  const int len = meta[slot] & 0xffff;
  const int64_t k = soff[s] + threadIdx.x;
  const int32_t b = cbase[s];
  for (int j = 0; j < len; ++j) c16[k + (int64_t)SELL_C * j] = (uint16_t)(col[k + (int64_t)SELL_C * j] - b);
}
int compress_sell_cols(HandleMem* h, TmpPool* T, DBsr* D, std::string* err) {
  int rc;
  if (!D->sell || D->half || D->nr == 0 || D->nbs == 0) return MAMG_OK;
  const int64_t ns = (D->nr + SELL_C - 1) / SELL_C;
  int32_t* base = nullptr;
  int* wide = nullptr;
  if ((rc = T->alloc(&wide, 1, err))) return rc;
  HIPCHK(dev_memset(wide, 0, sizeof(int)));
  if ((rc = dalloc(h, &base, ns, err))) return rc;
  sell_span_kernel<<<(unsigned)ns, SELL_C>>>(D->nr, D->soff, D->meta, D->col, base, wide);
  HIPCHK(hipGetLastError());
  int hw = 1;
  HIPCHK(hipMemcpy(&hw, wide, sizeof(int), hipMemcpyDeviceToHost));
  T->release(wide);
  if (hw) return MAMG_OK;   // a slice spans more than 16 bits: 32-bit columns (base stays unused)
  uint16_t* c16 = nullptr;
  if ((rc = dalloc(h, &c16, D->nbs, err))) return rc;
  HIPCHK(dev_memset(c16, 0, D->nbs * sizeof(uint16_t)));
  sell_col16_kernel<<<(unsigned)ns, SELL_C>>>(D->nr, D->soff, D->meta, D->col, base, c16);
  HIPCHK(hipGetLastError());
  D->col16 = c16;
  D->cbase = base;
  return MAMG_OK;
}
const dv4* step_wd(const DLevel& L, int s, bool pre) {
  return L.Wk.empty() ? L.Wd : L.Wk[step_index((int)L.Wk.size(), s, pre)];
}
const DCsr& step_wb(const DLevel& L, int s, bool pre) {
  return L.WBk.empty() ? L.WB : L.WBk[step_index((int)L.WBk.size(), s, pre)];
}
const double* step_winv(const DLevel& L, int s, bool pre) {
  return L.winvk.empty() ? L.winv : L.winvk[step_index((int)L.winvk.size(), s, pre)];
}

// SMOOTHER_POLY step smoothers w_k W of n doubles each (device copies)
int poly_scaled(DeviceHandle* h, const double* W, int64_t n, std::vector<double*>* out, std::string* err) {
  double w[MAMG_POLY_MAX];
  const int m = poly_weights(h->p, w);
  for (int k = 0; k < m; ++k) {
    double* o = nullptr;
    int rc = dalloc(h, &o, n, err);
    if (rc) return rc;
    if (n) wscale_kernel<<<nblocks(n), 256>>>(n, w[k], W, o);
    HIPCHK(hipGetLastError());
    out->push_back(o);
  }
  return MAMG_OK;
}

}  // namespace

// Jones-Plassmann colouring of the node graph of B (every node of the level;
// jp_round_kernel rounds, one 8-byte readback each): *ca (TmpPool-owned, nr
// bytes) = colour per node, *ncol = colours used
int gs_colour(TmpPool* T, const TBsr& B, int level, int8_t** ca_out, int* ncol_out, std::string* err) {
  int rc;
  const int64_t nr = B.nr;
  int* flags = nullptr;                 // [0] asymmetric pattern, [1] > 64 colours
  unsigned long long* left = nullptr;
  unsigned long long* cnt = nullptr;
  int8_t *ca = nullptr, *cb = nullptr;
  if ((rc = T->alloc(&flags, 4, err))) return rc;
  if ((rc = T->alloc(&left, 1, err))) return rc;
  if ((rc = T->alloc(&cnt, 64, err))) return rc;
  if ((rc = T->alloc(&ca, nr, err))) return rc;
  if ((rc = T->alloc(&cb, nr, err))) return rc;
  HIPCHK(dev_memset(flags, 0, 4 * sizeof(int)));
  HIPCHK(dev_memset(cnt, 0, 64 * sizeof(unsigned long long)));
  pattern_sym_kernel<<<nblocks(nr), 256>>>(nr, B.ptr, B.col, flags);
  HIPCHK(hipGetLastError());
  int hf[4] = {0, 0, 0, 0};
  HIPCHK(hipMemcpy(hf, flags, 4 * sizeof(int), hipMemcpyDeviceToHost));
  if (hf[0]) { *err = "multicolour GS: node pattern of level " + std::to_string(level) + " not symmetric"; return MAMG_ERR_UNSUPPORTED; }
  HIPCHK(dev_memset(ca, 0xff, nr));
  for (int round = 0;; ++round) {
    unsigned long long nl = 0;
    HIPCHK(dev_memset(left, 0, sizeof(unsigned long long)));
    jp_round_kernel<<<nblocks(nr), 256>>>(nr, B.ptr, B.col, level, ca, cb, left, flags + 1);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpy(&nl, left, sizeof(nl), hipMemcpyDeviceToHost));
    std::swap(ca, cb);
    if (nl == 0) break;
    if (round > 100000) { *err = "multicolour GS: colouring did not finish"; return MAMG_ERR_SETUP; }
  }
  HIPCHK(hipMemcpy(hf, flags, 4 * sizeof(int), hipMemcpyDeviceToHost));
  if (hf[1]) { *err = "multicolour GS: more than 64 colours on level " + std::to_string(level); return MAMG_ERR_UNSUPPORTED; }
  int32_t* ci = nullptr;
  int64_t* iota = nullptr;
  if ((rc = T->alloc(&ci, nr, err))) return rc;
  if ((rc = T->alloc(&iota, nr, err))) return rc;
  colour_count_kernel<<<nblocks(nr), 256>>>(nr, ca, ci, iota, cnt);
  HIPCHK(hipGetLastError());
  unsigned long long hc[64];
  HIPCHK(hipMemcpy(hc, cnt, sizeof(hc), hipMemcpyDeviceToHost));
  int ncol = 0;
  for (int c = 0; c < 64; ++c)
    if (hc[c]) ncol = c + 1;
  for (void* q : {(void*)cb, (void*)ci, (void*)iota}) T->release(q);
  *ca_out = ca;
  *ncol_out = ncol;
  return MAMG_OK;
}

// GS layout of the rows of B with colours ca (ncol colours; a colour may have
// no rows here, as on one rank of a multi-GPU level): permutation by a stable
// radix sort of the rows by colour (ascending row within a colour), the
// permuted BSR2 copy, its block inverses (node blocks from W's pattern) and
// the colour ranges (each colour padded to whole 64-row slices)
int gs_layout(HandleMem* h, TmpPool* T, const TBsr& B, const double* W, const int8_t* ca, int ncol, int level,
              DBsr* Gb, int32_t** gperm, dv4** Gd, std::vector<int64_t>* gcs_out, std::vector<int64_t>* gbk,
              std::string* err) {
  int rc;
  const int64_t nr = B.nr;
  int* flags = nullptr;
  unsigned long long* cnt = nullptr;
  int32_t *ci = nullptr, *cs = nullptr;
  int64_t *iota = nullptr, *sorted = nullptr;
  if ((rc = T->alloc(&flags, 4, err))) return rc;
  if ((rc = T->alloc(&cnt, 64, err))) return rc;
  if ((rc = T->alloc(&ci, nr, err))) return rc;
  if ((rc = T->alloc(&cs, nr, err))) return rc;
  if ((rc = T->alloc(&iota, nr, err))) return rc;
  if ((rc = T->alloc(&sorted, nr, err))) return rc;
  HIPCHK(dev_memset(flags, 0, 4 * sizeof(int)));
  HIPCHK(dev_memset(cnt, 0, 64 * sizeof(unsigned long long)));
  if (nr) colour_count_kernel<<<nblocks(nr), 256>>>(nr, ca, ci, iota, cnt);
  HIPCHK(hipGetLastError());
  if ((rc = dsort_pairs_i32_i64(ci, cs, iota, sorted, nr, 6, nullptr, err))) return rc;
  unsigned long long hc[64];
  HIPCHK(hipMemcpy(hc, cnt, sizeof(hc), hipMemcpyDeviceToHost));
  // colour c: sorted positions [gcs[c], gcs[c+1]); permuted rows from pcs[c],
  // each colour padded to whole 64-row slices
  std::vector<int64_t> gcs(65, 0), pcs(65, 0);
  for (int c = 0; c < ncol; ++c) {
    gcs[c + 1] = gcs[c] + (int64_t)hc[c];
    pcs[c + 1] = pcs[c] + ((int64_t)hc[c] + SELL_C - 1) / SELL_C * SELL_C;
  }
  const int64_t nrp = pcs[ncol];
  int64_t *gcs_d = nullptr, *pcs_d = nullptr;
  if ((rc = T->alloc(&gcs_d, 65, err))) return rc;
  if ((rc = T->alloc(&pcs_d, 65, err))) return rc;
  HIPCHK(hipMemcpy(gcs_d, gcs.data(), 65 * sizeof(int64_t), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(pcs_d, pcs.data(), 65 * sizeof(int64_t), hipMemcpyHostToDevice));
  gcs_out->assign(pcs.begin(), pcs.begin() + ncol + 1);
  TBsr G;
  G.nr = nrp; G.nc = B.nc; G.nb = B.nb;
  if ((rc = T->alloc(&G.ptr, nrp + 1, err))) return rc;
  HIPCHK(dev_memset(G.ptr, 0, sizeof(int64_t)));
  if ((rc = dalloc(h, gperm, std::max<int64_t>(nrp, 1), err))) return rc;
  if ((rc = dalloc(h, Gd, std::max<int64_t>(nrp, 1), err))) return rc;
  HIPCHK(dev_memset(*gperm, 0xff, std::max<int64_t>(nrp, 1) * sizeof(int32_t)));
  if (nr) perm_place_kernel<<<nblocks(nr), 256>>>(nr, cs, sorted, gcs_d, pcs_d, *gperm);
  HIPCHK(hipGetLastError());
  if (nrp) perm_len_kernel<<<nblocks(nrp), 256>>>(nrp, *gperm, B.ptr, G.ptr);
  HIPCHK(hipGetLastError());
  if ((rc = dscan_incl_i64(G.ptr, G.ptr, nrp + 1, nullptr, err))) return rc;
  if ((rc = T->alloc(&G.col, G.nb, err))) return rc;
  if ((rc = T->alloc(&G.val, G.nb, err))) return rc;
  if (nrp)
    perm_fill_kernel<<<nblocks(nrp), 256>>>(nrp, *gperm, B.ptr, B.col, B.val, reinterpret_cast<const dv4*>(W),
                                            G.ptr, G.col, G.val, *Gd, flags + 2);
  HIPCHK(hipGetLastError());
  int hf[4] = {0, 0, 0, 0};
  HIPCHK(hipMemcpy(hf, flags, 4 * sizeof(int), hipMemcpyDeviceToHost));
  if (hf[2]) { *err = "multicolour GS: a smoother block is missing or not SPD on level " + std::to_string(level); return MAMG_ERR_SETUP; }
  gbk->assign(ncol + 1, 0);
  for (int c = 0; c <= ncol; ++c) HIPCHK(hipMemcpy(&(*gbk)[c], G.ptr + (*gcs_out)[c], sizeof(int64_t), hipMemcpyDeviceToHost));
  // lane groups, not SELL-64: one lane per row over a colour's rows measured
  // 19.7 vs 11.5 ms for the four level-0 sweeps at nrefs=6
  if ((rc = finalize_bsr(h, T, G, Gb, 0, true, err, false))) return rc;
  for (void* q : {(void*)ci, (void*)cs, (void*)iota, (void*)sorted, (void*)G.ptr, (void*)G.col, (void*)G.val})
    T->release(q);
  return MAMG_OK;
}

namespace {

// Multicolour GS layout of one level from A_l's device BSR2 B and the
// level's (scaled) smoother blocks W (only their pattern is used: a node
// whose W block is diagonal has two 1x1 smoother blocks)
int build_gs(HandleMem* h, TmpPool* T, const TBsr& B, const double* W, int level, DLevel* D, std::string* err) {
  int8_t* ca = nullptr;
  int ncol = 0;
  int rc = gs_colour(T, B, level, &ca, &ncol, err);
  if (rc) return rc;
  rc = gs_layout(h, T, B, W, ca, ncol, level, &D->Gb, &D->gperm, &D->Gd, &D->gcs, &D->gbk, err);
  T->release(ca);
  // the colour steps of small coarse levels (<= 20000 node rows: a launch of
  // a few hundred rows, bound by its dependent load chain) take the largest
  // power of two <= 1.25 x the mean row length as lanes per row (about one
  // block per lane) instead of the SpMV rule's ~two: the reference family at
  // nrefs=6, level 7 8 -> 16 lanes, 142.4 -> 139.9 ms per apply
  // (profiles/r06_ab_misc.txt)
  if (rc == MAMG_OK && level > 0 && B.nr <= 20000 && D->Gb.nr > 0) {
    const double avg = (double)D->Gb.nb / (double)std::max<int64_t>(1, (int64_t)(B.nr));
    int l = 2;
    while (l < 64 && (double)(2 * l) <= 1.25 * avg) l *= 2;
    D->Gb.lanes = l;
  }
#if MAMG_DIAG   // diagnosis: lanes per row of the launched colour steps on levels of <= 20000 node rows
  if (const char* e = std::getenv("MAMG_GS_LANES"))
    if (rc == MAMG_OK && level > 0 && B.nr <= 20000 && std::atoi(e) > 0) D->Gb.lanes = std::atoi(e);
#endif
  return rc;
}

// rows of a level whose whole smoothing call runs as one launch of one
// workgroup (csr_gs_small_kernel: x in LDS, 8 bytes per row).  Measured at
// 1024 / 2048 / 4096 / 8192 on the hazmath preset, 2-D n = 128 (DESIGN.md
// section 2.8).  MAMG_CSR_GS_SMALL (diagnosis build) overrides it, at most
// 8192 (64 KB of LDS).
constexpr int64_t CSR_GS_SMALL_ROWS = 4096;
constexpr int64_t CSR_GS_SMALL_MAX = 8192;
static_assert(CSR_GS_SMALL_ROWS <= CSR_GS_SMALL_MAX && CSR_GS_SMALL_MAX * 8 <= 64 * 1024, "x of a small level in LDS");
inline int64_t csr_gs_small_rows() {
#if MAMG_DIAG
  if (const char* e = std::getenv("MAMG_CSR_GS_SMALL"))
    return std::min<int64_t>(std::max<int64_t>(std::atoll(e), 0), CSR_GS_SMALL_MAX);
#endif
  return CSR_GS_SMALL_ROWS;
}

// Point-wise multicolour GS layout of one CSR level from A_l on the device
// (A: the handle's copy): the rows coloured on A's off-diagonal pattern
// (gs_colour: the node-block GS's pattern check and Jones-Plassmann rounds on
// the scalar graph), a stable radix sort of the rows by colour, the
// colour-contiguous permuted copy (D->Gc), perm, 1 / a_ii per permuted row and
// the colour ranges.  Shared by dev_upload and dev_from_ghier.
// With cov (one byte per row, device; the seed rings' rest, build_rings_csr)
// the colouring runs on *pattern instead, and only the rows with cov == 0
// enter the colour lists and the permuted copy (G.ptr then has one entry per
// listed row + 1; G.n stays the length of x).
int build_gs_csr(HandleMem* h, TmpPool* T, const DCsr& A, int level, int lanes, DLevel* D, std::string* err,
                 const TBsr* pattern = nullptr, const uint8_t* cov = nullptr) {
  int rc;
  const int64_t n = A.n;
  TBsr B;                        // the scalar graph as gs_colour reads it (ptr, col)
  B.nr = n; B.nc = A.m; B.nb = A.nnz; B.ptr = A.ptr; B.col = A.col;
  int8_t* ca = nullptr;
  int ncol = 0;
  if ((rc = gs_colour(T, pattern ? *pattern : B, level, &ca, &ncol, err))) return rc;
  int* flag = nullptr;
  unsigned long long* cnt = nullptr;
  int32_t *ci = nullptr, *cs = nullptr;
  int64_t *iota = nullptr, *sorted = nullptr, *gcs_t = nullptr;
  if ((rc = T->alloc(&flag, 1, err))) return rc;
  if ((rc = T->alloc(&cnt, 64, err))) return rc;
  if ((rc = T->alloc(&ci, n, err))) return rc;
  if ((rc = T->alloc(&cs, n, err))) return rc;
  if ((rc = T->alloc(&iota, n, err))) return rc;
  if ((rc = T->alloc(&sorted, n, err))) return rc;
  if ((rc = T->alloc(&gcs_t, 65, err))) return rc;
  HIPCHK(dev_memset(flag, 0, sizeof(int)));
  HIPCHK(dev_memset(cnt, 0, 64 * sizeof(unsigned long long)));
  if (cov) rest_count_kernel<<<nblocks(n), 256>>>(n, ca, cov, ci, iota, cnt);
  else colour_count_kernel<<<nblocks(n), 256>>>(n, ca, ci, iota, cnt);
  HIPCHK(hipGetLastError());
  if ((rc = dsort_pairs_i32_i64(ci, cs, iota, sorted, n, cov ? 7 : 6, nullptr, err))) return rc;
  unsigned long long hc[64];
  HIPCHK(hipMemcpy(hc, cnt, sizeof(hc), hipMemcpyDeviceToHost));
  std::vector<int64_t> gcs(65, 0);
  for (int c = 0; c < 64; ++c) gcs[c + 1] = gcs[c] + (c < ncol ? (int64_t)hc[c] : 0);
  const int64_t nr = gcs[64];    // listed rows: n, or the uncovered ones (sorted first)
  HIPCHK(hipMemcpy(gcs_t, gcs.data(), 65 * sizeof(int64_t), hipMemcpyHostToDevice));
  D->gcs.assign(gcs.begin(), gcs.begin() + ncol + 1);
  if ((rc = dalloc(h, &D->gcs_d, 65, err))) return rc;
  HIPCHK(dev_copy(D->gcs_d, gcs_t, 65 * sizeof(int64_t)));
  DCsr& G = D->Gc;
  G.n = n; G.m = A.m; G.nnz = A.nnz;
  if ((rc = dalloc(h, &G.ptr, nr + 1, err))) return rc;
  if (!cov) {
    if ((rc = dalloc(h, &G.col, std::max<int64_t>(A.nnz, 1), err))) return rc;
    if ((rc = dalloc(h, &G.val, std::max<int64_t>(A.nnz, 1), err))) return rc;
  }
  if ((rc = dalloc(h, &D->gperm, std::max<int64_t>(nr, 1), err))) return rc;
  if ((rc = dalloc(h, &D->gdinv, std::max<int64_t>(nr, 1), err))) return rc;
  HIPCHK(dev_memset(G.ptr, 0, sizeof(int64_t)));
  // unpadded: permuted row = sorted position (pcs = gcs)
  if (nr) perm_place_kernel<<<nblocks(nr), 256>>>(nr, cs, sorted, gcs_t, gcs_t, D->gperm);
  HIPCHK(hipGetLastError());
  if (nr) perm_len_kernel<<<nblocks(nr), 256>>>(nr, D->gperm, A.ptr, G.ptr);
  HIPCHK(hipGetLastError());
  if ((rc = dscan_incl_i64(G.ptr, G.ptr, nr + 1, nullptr, err))) return rc;
  if (cov) {                     // the listed rows' entries only
    HIPCHK(hipMemcpy(&G.nnz, G.ptr + nr, sizeof(int64_t), hipMemcpyDeviceToHost));
    if ((rc = dalloc(h, &G.col, std::max<int64_t>(G.nnz, 1), err))) return rc;
    if ((rc = dalloc(h, &G.val, std::max<int64_t>(G.nnz, 1), err))) return rc;
  }
  G.lanes = lanes > 0 ? lanes : pick_lanes(std::max<int64_t>(nr, 1), G.nnz);
  if (nr) csr_gs_fill_kernel<<<nblocks(nr), 256>>>(nr, D->gperm, A.ptr, A.col, A.val, G.ptr, G.col, G.val, D->gdinv, flag);
  HIPCHK(hipGetLastError());
  int hf = 0;
  HIPCHK(hipMemcpy(&hf, flag, sizeof(int), hipMemcpyDeviceToHost));
  if (hf) {
    *err = "point-wise multicolour GS: a diagonal entry of level " + std::to_string(level) + " is missing or not positive";
    return MAMG_ERR_SETUP;
  }
  D->gbk.assign(ncol + 1, 0);
  for (int c = 0; c <= ncol; ++c)
    HIPCHK(hipMemcpy(&D->gbk[c], G.ptr + D->gcs[c], sizeof(int64_t), hipMemcpyDeviceToHost));
  D->gsmall = n <= csr_gs_small_rows();
  for (void* q : {(void*)ca, (void*)flag, (void*)cnt, (void*)ci, (void*)cs, (void*)iota, (void*)sorted, (void*)gcs_t})
    T->release(q);
  return MAMG_OK;
}

int build_ring_blocks(DeviceHandle* h, TmpPool* T, const DevMat& A, const std::vector<int32_t>& seeds, DLevel* D,
                      std::vector<int32_t>* rm, std::string* err);

// Seed-ring Schwarz data of level 0 on the CSR layout (SCHWARZ_RINGS on a
// scalar system, or a nodal one with point smoothers) from the handle's A_0:
// the blocks (build_ring_blocks) with their members as plain dof indices, and
// the rest's point-wise multicolour GS over the rows in no block.  The rest
// is coloured on A_0's pattern restricted to uncovered x uncovered: with the
// 3D-1D averaging the coupling rows hold ~400 entries and the whole graph
// needs more than 64 colours, while every such row lies in a block (DESIGN.md
// section 2.12.1).  Covered rows take no update and enter no colour list.
int build_rings_csr(DeviceHandle* h, TmpPool* T, const std::vector<int32_t>& seeds, int lanes, DLevel* D,
                    std::string* err) {
  const DCsr& A = D->A;
  const int64_t n = A.n;
  DevMat Am;
  Am.n = A.n; Am.m = A.m; Am.nnz = A.nnz; Am.ptr = A.ptr; Am.col = A.col; Am.val = A.val;
  std::vector<int32_t> rm;
  int rc = build_ring_blocks(h, T, Am, seeds, D, &rm, err);
  if (rc) return rc;
  HIPCHK(hipMemcpy(D->rmem, rm.data(), rm.size() * sizeof(int32_t), hipMemcpyHostToDevice));
  std::vector<uint8_t> cov(n, 0);
  for (int32_t g : rm) cov[g] = 1;
  uint8_t* dcov = nullptr;
  TBsr F;                        // the filtered pattern (ptr, col)
  F.nr = n; F.nc = n;
  if ((rc = T->alloc(&dcov, n, err))) return rc;
  if ((rc = T->alloc(&F.ptr, n + 1, err))) return rc;
  HIPCHK(hipMemcpy(dcov, cov.data(), n, hipMemcpyHostToDevice));
  HIPCHK(dev_memset(F.ptr, 0, sizeof(int64_t)));
  rest_pattern_len_kernel<<<nblocks(n), 256>>>(n, A.ptr, A.col, dcov, F.ptr);
  HIPCHK(hipGetLastError());
  if ((rc = dscan_incl_i64(F.ptr, F.ptr, n + 1, nullptr, err))) return rc;
  HIPCHK(hipMemcpy(&F.nb, F.ptr + n, sizeof(int64_t), hipMemcpyDeviceToHost));
  if ((rc = T->alloc(&F.col, F.nb, err))) return rc;
  rest_pattern_fill_kernel<<<nblocks(n), 256>>>(n, A.ptr, A.col, dcov, F.ptr, F.col);
  HIPCHK(hipGetLastError());
  if ((rc = build_gs_csr(h, T, A, 0, lanes, D, err, &F, dcov))) return rc;
  T->release(F.ptr); T->release(F.col); T->release(dcov);
  return MAMG_OK;
}

__global__ __launch_bounds__(256) void split_blocks_kernel(int64_t nbs, const dv4* __restrict__ in, dv2* __restrict__ out) {
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (k >= nbs) return;
  const dv4 v = in[k];
  out[k] = dv2{v.x, v.y};
  out[nbs + k] = dv2{v.z, v.w};
}

__global__ __launch_bounds__(256) void split_local_kernel(int64_t nbs, const dv4* __restrict__ in, double* __restrict__ out) {
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (k >= nbs) return;
  const dv4 v = in[k];
  const int64_t r = k & ~(int64_t)63, i = k & 63;
  reinterpret_cast<dv2*>(out + 4 * r)[i] = dv2{v.x, v.y};
  reinterpret_cast<dv2*>(out + 4 * r + 128)[i] = dv2{v.z, v.w};
}
__global__ __launch_bounds__(256) void unsplit_local_kernel(int64_t nbs, const double* __restrict__ in, dv4* __restrict__ out) {
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (k >= nbs) return;
  out[k] = blk_split_local(in, k);
}
// SELL slice s (64 w_s slots) moved from soff_old[s] to soff_new[s] (one workgroup per slice)
__global__ __launch_bounds__(256) void unsplit_blocks_kernel(int64_t nbs, const dv2* __restrict__ in, dv4* __restrict__ out) {
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (k >= nbs) return;
  const dv2 a = in[k], b = in[nbs + k];
  out[k] = dv4{a.x, a.y, b.x, b.y};
}

}  // namespace

// the distance-3 colouring of the node graph of B (c[I], device, from T), its
// colour count bound check and the longest row (node patches: <= 16 nodes)
int patch_colour(TmpPool* T, const TBsr& B, int16_t** cout, int* maxlen, std::string* err) {
  int rc;
  const int64_t nr = B.nr;
  int* flags = nullptr;                 // [0] asymmetric pattern, [1] > 256 colours, [3] max row length
  if ((rc = T->alloc(&flags, 4, err))) return rc;
  HIPCHK(dev_memset(flags, 0, 4 * sizeof(int)));
  pattern_sym_kernel<<<nblocks(nr), 256>>>(nr, B.ptr, B.col, flags);
  patch_rowlen_kernel<<<nblocks(nr), 256>>>(nr, B.ptr, flags + 3);
  HIPCHK(hipGetLastError());
  int hf[4] = {0, 0, 0, 0};
  HIPCHK(hipMemcpy(hf, flags, 4 * sizeof(int), hipMemcpyDeviceToHost));
  if (hf[0]) { *err = "node patches: node pattern of level 0 not symmetric"; return MAMG_ERR_UNSUPPORTED; }
  if (hf[3] > PATCH_MAX_NODES) {
    *err = "node patches: a node has " + std::to_string(hf[3]) + " neighbours (at most " +
           std::to_string(PATCH_MAX_NODES) + " nodes per patch)";
    return MAMG_ERR_UNSUPPORTED;
  }
  *maxlen = hf[3];
  int16_t* c = nullptr;
  uint64_t *m1 = nullptr, *m2 = nullptr, *m3 = nullptr;
  unsigned long long* mask1 = nullptr;
  int32_t* win = nullptr;
  unsigned int* wcnt = nullptr;                // winners of the round
  uint32_t* cb = nullptr;                      // coloured nodes, one bit each
  if ((rc = T->alloc(&c, nr, err))) return rc;
  if ((rc = T->alloc(&cb, nr / 32 + 1, err))) return rc;
  HIPCHK(dev_memset(cb, 0, (nr / 32 + 1) * sizeof(uint32_t)));
  if ((rc = T->alloc(&m1, nr, err))) return rc;
  if ((rc = T->alloc(&m2, nr, err))) return rc;
  if ((rc = T->alloc(&m3, nr, err))) return rc;
  if ((rc = T->alloc(&mask1, PATCH_WORDS * nr, err))) return rc;
  if ((rc = T->alloc(&win, nr, err))) return rc;
  if ((rc = T->alloc(&wcnt, 1, err))) return rc;
  HIPCHK(dev_memset(c, 0xff, nr * sizeof(int16_t)));
  HIPCHK(dev_memset(mask1, 0, PATCH_WORDS * nr * sizeof(unsigned long long)));
  // the 3-hop maxima of all keys (three full passes), then the winner list
  pkey_init_kernel<<<nblocks(nr), 256>>>(nr, c, m3);
  pkey_max_kernel<<<nblocks(nr), 256>>>(nr, B.ptr, B.col, m3, m1);
  pkey_max_kernel<<<nblocks(nr), 256>>>(nr, B.ptr, B.col, m1, m2);
  pkey_max_kernel<<<nblocks(nr), 256>>>(nr, B.ptr, B.col, m2, m3);
  const unsigned g1k = (unsigned)((nr + 1023) / 1024);
  HIPCHK(dev_memset(wcnt, 0, sizeof(unsigned int)));
  pkey_refresh_kernel<true><<<g1k, 1024>>>(nr, B.ptr, B.col, cb, m2, m3, win, wcnt);
  HIPCHK(hipGetLastError());
  for (int round = 0;; ++round) {
    unsigned int nw = 0;
    HIPCHK(hipMemcpy(&nw, wcnt, sizeof(nw), hipMemcpyDeviceToHost));
    if (nw == 0) break;                        // every node coloured
    if (round > 100000) { *err = "node patches: colouring did not finish"; return MAMG_ERR_SETUP; }
    patch_win_kernel<<<(unsigned)((nw + 3) / 4), 256>>>(nw, win, B.ptr, B.col, c, cb, mask1, flags + 1);
    pkey_refresh_kernel<false><<<nblocks(nr), 256>>>(nr, B.ptr, B.col, cb, nullptr, m1, nullptr, nullptr);
    pkey_refresh_kernel<false><<<nblocks(nr), 256>>>(nr, B.ptr, B.col, cb, m1, m2, nullptr, nullptr);
    HIPCHK(dev_memset(wcnt, 0, sizeof(unsigned int)));
    pkey_refresh_kernel<true><<<g1k, 1024>>>(nr, B.ptr, B.col, cb, m2, m3, win, wcnt);
    HIPCHK(hipGetLastError());
  }
  HIPCHK(hipMemcpy(hf, flags, 4 * sizeof(int), hipMemcpyDeviceToHost));
  if (hf[1]) { *err = "node patches: more than 256 colours"; return MAMG_ERR_UNSUPPORTED; }
  T->release(m1); T->release(m2); T->release(m3); T->release(mask1); T->release(win); T->release(wcnt);
  T->release(flags); T->release(cb);
  *cout = c;
  return MAMG_OK;
}

namespace {

// Node-patch Schwarz data of level 0 from A_0's device BSR2 B: the distance-3
// colouring (patch_colour), patches sorted by colour (stable radix sort,
// ascending centre within a colour), A_0 kept as plain BSR2 for the patch
// rows, and the patch inverses (patch_inv_kernel).
int build_patches(DeviceHandle* h, TmpPool* T, const TBsr& B, DLevel* D, std::string* err) {
  int rc;
  const int64_t nr = B.nr;
  int* flags = nullptr;                 // [2] bad pivot
  unsigned long long* cnt = nullptr;
  if ((rc = T->alloc(&flags, 4, err))) return rc;
  if ((rc = T->alloc(&cnt, 64 * PATCH_WORDS, err))) return rc;
  HIPCHK(dev_memset(flags, 0, 4 * sizeof(int)));
  HIPCHK(dev_memset(cnt, 0, 64 * PATCH_WORDS * sizeof(unsigned long long)));
  int16_t* c = nullptr;
  int hf[4] = {0, 0, 0, 0};
  if ((rc = patch_colour(T, B, &c, &hf[3], err))) return rc;
  int32_t *ci = nullptr, *cs = nullptr;
  int64_t *iota = nullptr, *sorted = nullptr;
  if ((rc = T->alloc(&ci, nr, err))) return rc;
  if ((rc = T->alloc(&cs, nr, err))) return rc;
  if ((rc = T->alloc(&iota, nr, err))) return rc;
  if ((rc = T->alloc(&sorted, nr, err))) return rc;
  pcolour_count_kernel<<<nblocks(nr), 256>>>(nr, c, ci, iota, cnt);
  HIPCHK(hipGetLastError());
  if ((rc = dsort_pairs_i32_i64(ci, cs, iota, sorted, nr, 8, nullptr, err))) return rc;
  std::vector<unsigned long long> hc(64 * PATCH_WORDS);
  HIPCHK(hipMemcpy(hc.data(), cnt, hc.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  int ncol = 0;
  for (int k = 0; k < 64 * PATCH_WORDS; ++k)
    if (hc[k]) ncol = k + 1;
  D->pcs.assign(ncol + 1, 0);
  for (int k = 0; k < ncol; ++k) D->pcs[k + 1] = D->pcs[k] + (int64_t)hc[k];
  if ((rc = dalloc(h, &D->pperm, nr, err))) return rc;
  i64_to_i32_kernel<<<nblocks(nr), 256>>>(nr, sorted, D->pperm);
  HIPCHK(hipGetLastError());
  for (void* q : {(void*)c, (void*)ci, (void*)cs, (void*)iota, (void*)sorted}) T->release(q);
  // A_0's patch rows: plain BSR2 in node order
  D->Snb = B.nb;
  if ((rc = dalloc(h, &D->Sptr, nr + 1, err))) return rc;
  if ((rc = dalloc(h, &D->Scol, B.nb, err))) return rc;
  if ((rc = dalloc(h, &D->Sval, B.nb, err))) return rc;
  HIPCHK(dev_copy(D->Sptr, B.ptr, (nr + 1) * sizeof(int64_t)));
  HIPCHK(dev_copy(D->Scol, B.col, B.nb * sizeof(int32_t)));
  HIPCHK(dev_copy(D->Sval, B.val, B.nb * sizeof(dv4)));
  const int64_t dmax = 2 * (int64_t)hf[3];
  D->pus = dmax * (dmax + 1) / 2;
  if ((rc = dalloc(h, &D->pu, nr * D->pus, err))) return rc;
  launch_patch_inv(h->sw.patch_inv, nr, D->pperm, D->Sptr, D->Scol, D->Scol, D->Sval, D->pus, D->pu, flags + 2);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpy(hf, flags, 4 * sizeof(int), hipMemcpyDeviceToHost));
  if (hf[2]) { *err = "node patches: a patch matrix is not SPD (non-positive Gauss-Jordan pivot)"; return MAMG_ERR_SETUP; }
  return MAMG_OK;
}

// The layout-independent half of the seed-ring Schwarz data of level 0
// (Schwarz_type RINGS) from A_0's device CSR: the blocks and their inverses on
// the device (ring_blocks_dev: the additive form's breadth-first rings and
// Gauss-Jordan kernels), the greedy conflict colouring on the host (setup.cpp
// ring_colouring, in seed order: the sequential step, as VMB's), the blocks
// re-ordered colour by colour (rcs, rmo, rio) with their inverses transposed
// (rinv).  *rm: the members as plain dof indices in that order; the caller
// stores them in its layout's numbering (rmem).
int build_ring_blocks(DeviceHandle* h, TmpPool* T, const DevMat& A, const std::vector<int32_t>& seeds, DLevel* D,
                      std::vector<int32_t>* rm, std::string* err) {
  const mamg_params& p = h->p;
  if (seeds.empty()) { *err = "seed rings: no seeds"; return MAMG_ERR_ARG; }
  const int64_t n = A.n, ns = (int64_t)seeds.size();
  const auto t0 = std::chrono::steady_clock::now();
  auto ms_since = [](std::chrono::steady_clock::time_point a) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - a).count();
  };
  RingBlocks RB;
  int rc = ring_blocks_dev(A, seeds.data(), ns, p.Schwarz_maxlvl, p.Schwarz_mmsize, &RB, err);
  if (rc) return rc;
  struct Guard { RingBlocks* r; ~Guard() { ring_blocks_free(r); } } guard{&RB};
  const int mm = RB.mm;
  std::vector<int32_t> blk((size_t)ns * mm);
  std::vector<int64_t> blen(ns), sq(ns);
  HIPCHK(hipMemcpy(blk.data(), RB.blk, blk.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(blen.data(), RB.blen, ns * sizeof(int64_t), hipMemcpyDeviceToHost));
  std::vector<int64_t> bptr(ns + 1, 0);
  for (int64_t k = 0; k < ns; ++k) bptr[k + 1] = bptr[k] + blen[k];
  std::vector<int32_t> mem(bptr[ns]);
  for (int64_t k = 0; k < ns; ++k) std::copy(blk.begin() + k * mm, blk.begin() + k * mm + blen[k], mem.begin() + bptr[k]);
  // A_0's pattern for the conflict graph
  std::vector<int64_t> aptr(n + 1);
  std::vector<int32_t> acol(A.nnz);
  HIPCHK(hipMemcpy(aptr.data(), A.ptr, (n + 1) * sizeof(int64_t), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(acol.data(), A.col, A.nnz * sizeof(int32_t), hipMemcpyDeviceToHost));
  CsrView Av;
  Av.n = Av.m = n; Av.ptr = aptr.data(); Av.col = acol.data();
  std::vector<int32_t> colour;
  const double t_blocks = ms_since(t0);
  const auto t1 = std::chrono::steady_clock::now();
  ring_colouring(Av, bptr, mem, &colour);
  const double t_colour = ms_since(t1);
  std::vector<int32_t>().swap(acol);
  int ncol = 0;
  for (int32_t c : colour) ncol = std::max(ncol, c + 1);
  if (p.print_level >= 1)   // what the seed rings cost at the drivers' sizes
    std::fprintf(stderr, "[mamg] seed rings: %lld blocks, %lld member dofs (max %d per block), %d colours, "
                 "blocks + inverses %.1f ms, host colouring %.1f ms, %.3f GB of inverses\n",
                 (long long)ns, (long long)bptr[ns], mm, ncol, t_blocks, t_colour,
                 [&] { double q = 0; for (int64_t k = 0; k < ns; ++k) q += (double)blen[k] * blen[k]; return 8e-9 * q; }());
  std::vector<int32_t> ord(ns);
  std::iota(ord.begin(), ord.end(), 0);
  std::stable_sort(ord.begin(), ord.end(), [&](int32_t a, int32_t b) { return colour[a] < colour[b]; });
  D->rcs.assign(ncol + 1, 0);
  for (int32_t c : colour) D->rcs[c + 1]++;
  for (int c = 0; c < ncol; ++c) D->rcs[c + 1] += D->rcs[c];
  std::vector<int64_t> mo(ns + 1, 0), io(ns + 1, 0);
  rm->clear();
  rm->reserve(mem.size());
  for (int64_t j = 0; j < ns; ++j) {
    const int64_t o = ord[j], d = blen[o];
    mo[j + 1] = mo[j] + d;
    io[j + 1] = io[j] + d * d;
    rm->insert(rm->end(), mem.begin() + bptr[o], mem.begin() + bptr[o + 1]);
  }
  D->rnm = mo[ns];
  D->rinv_n = (double)io[ns];
  D->rcm.assign(ncol + 1, 0);
  D->rci.assign(ncol + 1, 0);
  D->rce.assign(ncol + 1, 0);
  for (int c = 0; c < ncol; ++c) {
    D->rcm[c + 1] = mo[D->rcs[c + 1]];
    D->rci[c + 1] = io[D->rcs[c + 1]];
    int64_t e = D->rce[c];
    for (int64_t t = mo[D->rcs[c]]; t < mo[D->rcs[c + 1]]; ++t) e += aptr[(*rm)[t] + 1] - aptr[(*rm)[t]];
    D->rce[c + 1] = e;
  }
  if ((rc = dalloc(h, &D->rmo, ns + 1, err))) return rc;
  if ((rc = dalloc(h, &D->rio, ns + 1, err))) return rc;
  if ((rc = dalloc(h, &D->rmem, std::max<int64_t>(D->rnm, 1), err))) return rc;
  if ((rc = dalloc(h, &D->rinv, std::max<int64_t>(io[ns], 1), err))) return rc;
  HIPCHK(hipMemcpy(D->rmo, mo.data(), (ns + 1) * sizeof(int64_t), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(D->rio, io.data(), (ns + 1) * sizeof(int64_t), hipMemcpyHostToDevice));
  int32_t* dord = nullptr;
  if ((rc = T->alloc(&dord, ns, err))) return rc;
  HIPCHK(hipMemcpy(dord, ord.data(), ns * sizeof(int32_t), hipMemcpyHostToDevice));
  ring_perm_inv_kernel<<<(unsigned)ns, 256>>>(ns, dord, RB.blen, RB.sq, RB.inv, D->rio, D->rinv);
  HIPCHK(hipGetLastError());
  return MAMG_OK;   // ring_blocks_dev's buffers: freed by the guard, null-stream ordered
}

// Seed-ring Schwarz data of level 0 on the BSR2 layout from A_0's device CSR
// S.A and node BSR2 B: the blocks (build_ring_blocks) with their members as
// node-interleaved dof indices, A_0's plain BSR2 copy for the block rows, and
// the rest's multicolour node-block GS with the covered dofs masked out
// (mamg_oracle.rest_gs_inverse).
int build_rings(DeviceHandle* h, TmpPool* T, const TBsr& B, const LevelSrc& S, DLevel* D, std::string* err) {
  if (!S.seeds || S.seeds->empty()) { *err = "seed rings: no seeds"; return MAMG_ERR_ARG; }
  const int64_t n = S.A.n, nv = n / 2;
  std::vector<int32_t> rm;
  int rc = build_ring_blocks(h, T, S.A, *S.seeds, D, &rm, err);
  if (rc) return rc;
  std::vector<uint8_t> cov(nv, 0);
  for (int32_t& g : rm) {
    const int64_t I = g % nv, f = g / nv;
    g = (int32_t)(2 * I + f);
    cov[I] |= (uint8_t)(1u << f);
  }
  HIPCHK(hipMemcpy(D->rmem, rm.data(), rm.size() * sizeof(int32_t), hipMemcpyHostToDevice));
  // A_0's block rows: plain BSR2 in node order
  D->Snb = B.nb;
  if ((rc = dalloc(h, &D->Sptr, B.nr + 1, err))) return rc;
  if ((rc = dalloc(h, &D->Scol, B.nb, err))) return rc;
  if ((rc = dalloc(h, &D->Sval, B.nb, err))) return rc;
  HIPCHK(dev_copy(D->Sptr, B.ptr, (B.nr + 1) * sizeof(int64_t)));
  HIPCHK(dev_copy(D->Scol, B.col, B.nb * sizeof(int32_t)));
  HIPCHK(dev_copy(D->Sval, B.val, B.nb * sizeof(dv4)));
  // the rest's GS: multicolour node-block GS, covered dofs masked
  uint8_t* dcov = nullptr;
  dv4* Wp = nullptr;
  if ((rc = T->alloc(&dcov, nv, err))) return rc;
  if ((rc = T->alloc(&Wp, nv, err))) return rc;
  HIPCHK(hipMemcpy(dcov, cov.data(), nv, hipMemcpyHostToDevice));
  rest_w_kernel<<<nblocks(nv), 256>>>(nv, reinterpret_cast<const dv4*>(S.W), dcov, Wp);
  HIPCHK(hipGetLastError());
  if ((rc = build_gs(h, T, B, reinterpret_cast<const double*>(Wp), 0, D, err))) return rc;
  const int64_t nrp = D->gcs.empty() ? 0 : D->gcs.back();
  if (nrp) rest_mask_kernel<<<nblocks(nrp), 256>>>(nrp, D->gperm, dcov, D->Gd);
  HIPCHK(hipGetLastError());
  return MAMG_OK;
}

// ---- matrix-free level-0 post step (DLevel::post_mf) --
// Wp[t] = w D_t^-1 per row type of the dictionary: D_t is the type's diagonal
// block (the entry with column - row == 0), inverted by the setup's 2x2
// Gauss-Jordan without pivoting (gsetup.hip node_inverse_kernel).  *bad is
// set for a type without a diagonal entry or with a non-positive pivot.
__global__ __launch_bounds__(256) void post_mf_table_kernel(int nt, int rw, int sym, int64_t nbs,
                                                            const int32_t* __restrict__ rlen,
                                                            const int32_t* __restrict__ rdelta,
                                                            const double* __restrict__ rval, double w,
                                                            dv4* __restrict__ Wp, int* bad) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= nt) return;
  int k = -1;
  for (int j = 0; j < rlen[t]; ++j)
    if (rdelta[t * rw + j] == 0) { k = t * rw + j; break; }
  if (k < 0) { atomicOr(bad, 1); Wp[t] = dv4{0.0, 0.0, 0.0, 0.0}; return; }
  const dv4 a = sym ? dv4{rval[2 * k], rval[2 * nbs + k], rval[2 * nbs + k], rval[2 * k + 1]}
                    : reinterpret_cast<const dv4*>(rval)[k];
  double M[2][4] = {{a.x, a.y, 1.0, 0.0}, {a.z, a.w, 0.0, 1.0}};
  bool ok = true;
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const double p = M[q][q];
    if (!(p > 0.0)) ok = false;
#pragma unroll
    for (int j = 0; j < 4; ++j) M[q][j] = M[q][j] / p;
    const int i = 1 - q;
    const double fi = M[i][q];
#pragma unroll
    for (int j = 0; j < 4; ++j) M[i][j] = M[i][j] - fi * M[q][j];
  }
  if (!ok) atomicOr(bad, 1);
  Wp[t] = dv4{w * M[0][2], w * M[0][3], w * M[1][2], w * M[1][3]};
}

__global__ __launch_bounds__(256) void agg_i32_kernel(int64_t nv, const int64_t* __restrict__ agg,
                                                      int32_t* __restrict__ out) {
  const int64_t I = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (I < nv) out[I] = agg[I] < 0 ? -1 : (int32_t)agg[I];
}

// Decides whether level 0 prolongates through the aggregate index and A's
// dictionary instead of a stored K (or P): P = (I - w D_B^-1 A) T holds for
// the nodal SA prolongator only, and the post sweeps must be the block-Jacobi
// passes.  MAMG_OK with D->post_mf set, or with it false and the reason in
// D->mfinfo[PM_REASON] (the caller then builds K / P as without the attempt).
int try_post_mf(DeviceHandle* h, TmpPool* T, const LevelSrc& S, int64_t nvc, DLevel* D, std::string* err) {
  const mamg_params& p = h->p;
  int64_t* info = D->mfinfo;
  info[PM_TAKEN] = 0;
  info[PM_TABLE_BYTES] = 0;
  auto refuse = [&](int why) { info[PM_REASON] = why; return MAMG_OK; };
  const DBsr& A = D->Ab;
  if (h->sw.post_mf_mode == 0) return refuse(PMR_OFF);
  if (!p.post_fusion || p.postsmooth_iter < 1) return refuse(PMR_NO_FUSION);
  if (gs_smoother(p) || patch_schwarz(p) || rings_schwarz(p)) return refuse(PMR_SMOOTHER);
  if (p.AMG_type != MAMG_SA_AMG || !p.sa_block_diag || !S.agg || !(S.w_sa > 0.0)) return refuse(PMR_NOT_SA);
  if (!A.rowdict) return refuse(PMR_NO_DICT);
  if (A.nr < h->sw.post_mf_min_rows) return refuse(PMR_THRESHOLD);
  if (nvc > (int64_t)INT32_MAX) return refuse(PMR_NOT_SA);
  int rc;
  dv4* wp = nullptr;
  int* bad = nullptr;
  if ((rc = T->alloc(&wp, A.rtypes, err))) return rc;
  if ((rc = T->alloc(&bad, 1, err))) return rc;
  HIPCHK(dev_memset(bad, 0, sizeof(int)));
  post_mf_table_kernel<<<nblocks(A.rtypes), 256>>>(A.rtypes, A.rw, A.sym ? 1 : 0, A.nbs, A.rlen, A.rdelta, A.val,
                                                   S.w_sa, wp, bad);
  HIPCHK(hipGetLastError());
  int hb = 1;
  HIPCHK(hipMemcpy(&hb, bad, sizeof(int), hipMemcpyDeviceToHost));
  if (hb) {
    T->release(wp); T->release(bad);
    return refuse(PMR_DIAG);
  }
  if ((rc = dalloc(h, &D->mf_wp, A.rtypes, err))) return rc;
  if ((rc = dalloc(h, &D->mf_agg, A.nr, err))) return rc;
  HIPCHK(dev_copy(D->mf_wp, wp, (size_t)A.rtypes * sizeof(dv4)));
  agg_i32_kernel<<<nblocks(A.nr), 256>>>(A.nr, S.agg, D->mf_agg);
  HIPCHK(hipGetLastError());
  T->release(wp); T->release(bad);
  D->post_mf = true;
  info[PM_TAKEN] = 1;
  info[PM_REASON] = PMR_NONE;
  info[PM_TABLE_BYTES] = 32 * (int64_t)A.rtypes;
  return MAMG_OK;
}

int build_bsr_level(DeviceHandle* h, int l, const LevelSrc& S, int64_t nvc, int lanesA, std::string* err) {
  DLevel& D = h->L[l];
  const mamg_params& p = h->p;
  const int64_t nv = D.n / 2;
  int rc;
  TmpPool T(h->sw);
  if (D.coarsest) {
    if ((rc = dalloc(h, &D.Ainv, D.n * D.n, err))) return rc;
    permute_dense_kernel<<<nblocks(D.n * D.n), 256>>>(D.n, S.Ainv, D.Ainv);
    HIPCHK(hipGetLastError());
    TBsr B;
    if ((rc = dev_csr_to_bsr(&T, S.A, nv, nv, &B, err))) return rc;
    return finalize_bsr(h, &T, B, &D.Ab, 0, false, err);
  }
  {
    TBsr B;
    if ((rc = dev_csr_to_bsr(&T, S.A, nv, nv, &B, err))) return rc;
    if ((rc = finalize_bsr(h, &T, B, &D.Ab, lanesA, true, err, true, l == 0, l > 0)))
      return rc;
    const bool patches = l == 0 && patch_schwarz(p);
    const bool rings = l == 0 && rings_schwarz(p) && S.seeds && !S.seeds->empty();
    if (gs_smoother(p) && !patches && !rings)
      if ((rc = build_gs(h, &T, B, S.W, l, &D, err))) return rc;
    if (patches)
      if ((rc = build_patches(h, &T, B, &D, err))) return rc;
    if (rings)
      if ((rc = build_rings(h, &T, B, S, &D, err))) return rc;
    T.release(B.ptr); T.release(B.col); T.release(B.val);
  }
  if ((rc = dalloc(h, &D.Wd, nv, err))) return rc;
  HIPCHK(dev_copy(D.Wd, S.W, 4 * nv * sizeof(double)));
  if (p.smoother == MAMG_SMOOTHER_POLY) {
    std::vector<double*> wk;
    if ((rc = poly_scaled(h, S.W, 4 * nv, &wk, err))) return rc;
    for (double* q : wk) D.Wk.push_back(reinterpret_cast<dv4*>(q));
  }
  if (l == 0 && (rc = try_post_mf(h, &T, S, nvc, &D, err))) return rc;
  if (D.post_mf) {
    // level 0 prolongates through agg and A's dictionary: no K, no [P | AP], and
    // no P either (its only other readers are the GS and unfused paths, which
    // the eligibility rules out)
  } else if (p.post_fusion && p.postsmooth_iter >= 1 && S.AP.n == D.n && !gs_smoother(p) &&
             !(l == 0 && (patch_schwarz(p) || rings_schwarz(p)))) {
    TBsr Pb, Qb, M;
    if ((rc = dev_csr_to_bsr(&T, S.P, nv, nvc, &Pb, err))) return rc;
    if ((rc = dev_csr_to_bsr(&T, S.AP, nv, nvc, &Qb, err))) return rc;
    if (h->sw.post_k) {   // one operator K = P - W (A P) on AP's pattern,
                      // W = the first post-smoothing step's smoother
      const double* Wpost = reinterpret_cast<const double*>(step_wd(D, 0, false));
      if ((rc = dev_kmerge(&T, Pb, Qb, Wpost, &M, err))) return rc;
    } else {          // P and AP blocks side by side in one row window
      if ((rc = dev_merge_rows(&T, Pb, Qb, &M, err))) return rc;
    }
    T.release(Pb.ptr); T.release(Pb.col); T.release(Pb.val);
    T.release(Qb.ptr); T.release(Qb.col); T.release(Qb.val);
    // K: SELL-64 with 4-block chunks (K rows hold ~9 blocks at level 0; A/B in
    // DESIGN.md section 4), lane-group BSR if MAMG_POST_SELL=0; the merged
    // window is never SELL on this path
    if ((rc = finalize_bsr(h, &T, M, h->sw.post_k ? &D.KPb : &D.PAb, 0, false, err, h->sw.post_k != 0, false,
                           l > 0 && h->sw.post_k != 0)))
      return rc;
    D.KPb.kvar = h->sw.k_variant;
    if (l == 0 && h->sw.post_k && h->sw.k_sort && D.KPb.sell && D.KPb.lpr <= 1)
      if ((rc = sort_sell_slices(h, &T, &D.KPb, err))) return rc;
    if (l == 0 && h->sw.post_k && D.KPb.sell && h->sw.k_col16)
      if ((rc = compress_sell_cols(h, &T, &D.KPb, err))) return rc;
  } else {
    TBsr Pb;
    if ((rc = dev_csr_to_bsr(&T, S.P, nv, nvc, &Pb, err))) return rc;
    if ((rc = finalize_bsr(h, &T, Pb, &D.Pb, 0, false, err))) return rc;
  }
  {
    TBsr Rb;
    if ((rc = dev_csr_to_bsr(&T, S.R, nvc, nv, &Rb, err))) return rc;
    if ((rc = finalize_bsr(h, &T, Rb, &D.Rb, 0, false, err))) return rc;
    if (l == 0 && (rc = build_rest_sched(h, &T, &D.Rb, D.Ab.band_stride, err))) return rc;
  }
  return MAMG_OK;
}

// host CSR -> temporary device CSR
int upload_tmp(TmpPool* T, const CsrView& M, DevMat* D, std::string* err) {
  int rc;
  D->n = M.n; D->m = M.m; D->nnz = M.nnz();
  if ((rc = T->alloc(&D->ptr, M.n + 1, err))) return rc;
  if ((rc = T->alloc(&D->col, D->nnz, err))) return rc;
  if ((rc = T->alloc(&D->val, D->nnz, err))) return rc;
  HIPCHK(hipMemcpy(D->ptr, M.ptr, (M.n + 1) * sizeof(int64_t), hipMemcpyHostToDevice));
  if (D->nnz) {
    HIPCHK(hipMemcpy(D->col, M.col, D->nnz * sizeof(int32_t), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(D->val, M.val, D->nnz * sizeof(double), hipMemcpyHostToDevice));
  }
  return MAMG_OK;
}

// ---- algorithmic bytes (per layout) ------------------------------
double csr_bytes(const DCsr& M, int epi) {
  double b = 12.0 * M.nnz + 8.0 * (M.n + 1) + 8.0 * M.m + 8.0 * M.n;  // A, x, out
  if (epi == EPI_YADD) b += 8.0 * M.n;
  if (epi == EPI_RESID) b += 8.0 * M.n;
  if (epi == EPI_JACOBI) b += 16.0 * M.n;
  return b;
}

double index_bytes(const DBsr& M, int64_t ptr_entries) {
  return M.sell ? 4.0 * M.nr + 8.0 * (M.nr / SELL_C + 2) : 8.0 * ptr_entries;
}

double bsr_bytes(const DBsr& M, int epi) {
  // half-symmetric: upper blocks (28 B with column) + 4-byte mirror slot per
  // lower block + row meta; the mirrors' values are re-reads, not counted
  // fp32 storage (M.f32): 4 bytes per stored value instead of 8, so a block
  // with its column is 16 B (SYM / half), 18 B (16-bit column) or 20 B
  const double vb = M.f32 ? 4.0 : 8.0;
  const double sym_b = 3.0 * vb + 4.0, c16_b = 4.0 * vb + 2.0, gen_b = 4.0 * vb + 4.0;
  // row-pattern dictionary: one 16-bit code per row and the type table
  // (lengths, column offsets, blocks), x and out; no matrix stream
  if (M.rowdict) {
    double b = 2.0 * M.nr + 4.0 * M.rtypes + (4.0 + (M.sym ? 3.0 : 4.0) * vb) * M.nbs + 16.0 * M.nc + 16.0 * M.nr;
    if (epi == EPI_YADD) b += 16.0 * M.nr;
    if (epi == EPI_RESID) b += 16.0 * M.nr;
    if (epi == EPI_BJAC || epi == EPI_KPOST) b += 16.0 * M.nr + 16.0 * M.nr + 32.0 * M.nr;   // y, b, W
    if (epi == EPI_PSM) b += 16.0 * M.nr + 32.0 * M.rtypes;   // x1 and the per-type table w D_B^-1
    return b;
  }
  double b = M.half ? sym_b * (M.nb - M.nlo) + 4.0 * M.nlo + 4.0 * M.nr + (M.ngs ? 8.0 * (M.nr / SELL_C + 2) : 0.0) +
                          16.0 * M.nc + 16.0 * M.nr
                    : (M.sym ? sym_b : M.col16 ? c16_b : gen_b) * M.nb + index_bytes(M, M.nr + 1) +
                          (M.col16 ? 4.0 * (M.nr / SELL_C + 1) : 0.0) + 16.0 * M.nc + 16.0 * M.nr;
  if (epi == EPI_YADD) b += 16.0 * M.nr;
  if (epi == EPI_RESID) b += 16.0 * M.nr;
  if (epi == EPI_BJAC || epi == EPI_KPOST) b += 16.0 * M.nr + 16.0 * M.nr + 32.0 * M.nr;   // y, b, W
  return b;
}

}  // namespace

Op csr_op(const DCsr& M, int epi, int cls, int tag, const double* x, const double* y,
          const double* b, const double* w, double* out) {
  Op o;
  o.kind = OP_CSR; o.epi = epi; o.cls = cls; o.tag = tag; o.M = &M; o.n = M.n;
  o.x = x; o.y = y; o.b = b; o.w = w; o.out = out;
  o.bytes = csr_bytes(M, epi);
  return o;
}

Op bsr_op(const DBsr& M, int epi, int cls, int tag, const double* x, int64_t xs, const double* y,
          const double* b, int64_t bs, const dv4* W, double* out, int64_t os) {
  Op o;
  o.kind = OP_BSR; o.epi = epi; o.cls = cls; o.tag = tag; o.Mb = &M; o.n = M.nr;
  o.x = x; o.xs = xs; o.xfm = xs != 0; o.y = y; o.b = b; o.bs = bs; o.W = W; o.out = out; o.os = os;
  o.bytes = bsr_bytes(M, epi);
  return o;
}

// merged [P | AP] blocks + 2 nr + 1 pointers, e gathered once, x1 r1 W out
Op post_op(const DBsr& M, const double* r1, const dv4* W, int cls, int tag, const double* e,
           const double* x1, double* out, int64_t os) {
  Op o;
  o.kind = OP_POST; o.cls = cls; o.tag = tag; o.Mb = &M; o.n = M.nr;
  o.x = e; o.y = x1; o.b = r1; o.W = W; o.out = out; o.os = os;
  o.bytes = 36.0 * M.nb + index_bytes(M, 2 * M.nr + 1) + 16.0 * M.nc + 16.0 * M.nr * 3 + 32.0 * M.nr;
  return o;
}

namespace {

Op gemv_op(const DLevel& L, const double* b, double* out) {
  Op o;
  o.kind = OP_GEMV; o.cls = C_DENSE; o.n = L.n; o.x = b; o.w = L.Ainv; o.out = out;
  o.bytes = 8.0 * L.n * L.n + 16.0 * L.n;
  return o;
}

}  // namespace

Op axpy_op(int64_t n, const double* e, double* x) {
  Op o;
  o.kind = OP_AXPY; o.cls = C_MISC; o.n = n; o.x = e; o.out = x; o.bytes = 24.0 * n;
  return o;
}

namespace {

void scale_ops(const DeviceHandle* h, int lc, std::vector<Op>* ops);

inline bool kcycle(const mamg_params& p) { return p.cycle_type == MAMG_NL_AMLI_CYCLE; }

// nonlinear AMLI: the vector ops of step j of level lc's inner flexible CG,
// after z = M(r) and w = A_c z (step 0: straight into p_0 / q_0): the j dots
// <z, q_i> in one pass over z; p_j, q_j and the partials of <p_j, q_j>,
// <p_j, r> in one pass; then e (+)= alpha p_j and, but for the last step,
// r -= alpha q_j (step 0 reads the visit's right-hand side C.b, writes C.kr)
void kstep_ops(const DeviceHandle* h, int lc, int j, std::vector<Op>* ops) {
  const DLevel& C = h->L[lc];
  const int m = h->p.amli_degree;
  const bool last = j == m - 1;
  Op o;
  o.cls = C_MISC; o.n = C.n; o.lev = &C; o.r0 = j; o.r1 = m; o.part = C.kpart;
  if (j > 0) {
    o.kind = OP_KDOT; o.bytes = 8.0 * (1 + j) * C.n;
    ops->push_back(o);
  }
  o.kind = OP_KORTH; o.bytes = 8.0 * (j > 0 ? 2 + 2 * j + 2 + 1 : 3) * C.n;
  ops->push_back(o);
  o.kind = OP_KUPD; o.bytes = 8.0 * ((j > 0 ? 3 : 2) + (last ? 0 : 3)) * C.n;
  ops->push_back(o);
}

// algorithmic bytes of one point-wise GS colour step (mamg.h mamg_apply_bytes):
// values + columns, pointers, perm, 1 / a_ii, b, own x read and written, and
// the gathered x (every entry once per sweep, spread over the colours)
double cgs_bytes(const DLevel& L, int c) {
  const double rows = (double)(L.gcs[c + 1] - L.gcs[c]), ncol = (double)(L.gcs.size() - 1);
  return 12.0 * (double)(L.gbk[c + 1] - L.gbk[c]) + 8.0 * (rows + 1) + 4.0 * rows + 8.0 * rows + 8.0 * rows +
         16.0 * rows + 8.0 * (double)L.n / ncol;
}

// one point-wise GS sweep of a CSR level in place on x, one launch per colour
// (colours ascending if fwd, else descending)
void cgs_sweep_ops(const DLevel& L, bool fwd, double* x, const double* b, int cls, std::vector<Op>* ops) {
  const int nc = (int)L.gcs.size() - 1;
  for (int k = 0; k < nc; ++k) {
    const int c = fwd ? k : nc - 1 - k;
    if (L.gcs[c + 1] <= L.gcs[c]) continue;
    Op o;
    o.kind = OP_CGS; o.cls = cls; o.M = &L.Gc; o.perm = L.gperm; o.w = L.gdinv;
    o.x = x; o.out = x; o.b = b;
    o.r0 = L.gcs[c]; o.r1 = L.gcs[c + 1]; o.n = o.r1 - o.r0;
    o.bytes = cgs_bytes(L, c);
    ops->push_back(o);
  }
}

// a whole point-wise GS smoothing call on x: nu x (sweep d0, sweep d1), d > 0
// forward, d < 0 backward, 0 none; from x = 0 if zero.  A small level
// (L.gsmall): one launch (csr_gs_small_kernel, which then starts from zero in
// LDS and never reads x); else an OP_ZERO and one launch per colour.
void cgs_smooth_ops(const DLevel& L, bool zero, int nu, int d0, int d1, double* x, const double* b, int clsS,
                    int clsW, std::vector<Op>* ops) {
  const int nc = (int)L.gcs.size() - 1;
  if (L.gsmall) {
    Op o;
    o.kind = OP_CGSF; o.cls = clsS; o.lev = &L; o.M = &L.Gc; o.perm = L.gperm; o.w = L.gdinv;
    o.x = x; o.out = x; o.b = b; o.n = nu;
    o.epi = (zero ? 1 : 0) | ((d0 > 0 ? 1 : d0 < 0 ? 2 : 0) << 1) | ((d1 > 0 ? 1 : d1 < 0 ? 2 : 0) << 3);
    double per = 0.0;
    for (int c = 0; c < nc; ++c) per += cgs_bytes(L, c);
    o.bytes = nu * ((d0 ? 1 : 0) + (d1 ? 1 : 0)) * per;
    ops->push_back(o);
    return;
  }
  if (zero) {
    Op z;
    z.kind = OP_ZERO; z.cls = clsW; z.n = L.n; z.out = x; z.bytes = 8.0 * L.n;
    ops->push_back(z);
  }
  for (int s = 0; s < nu; ++s) {
    if (d0) cgs_sweep_ops(L, d0 > 0, x, b, clsS, ops);
    if (d1) cgs_sweep_ops(L, d1 > 0, x, b, clsS, ops);
  }
}

// one colour of a seed-ring sweep on the CSR layout (mamg.h mamg_apply_bytes,
// ring_op's count restated for scalar rows): the blocks' transposed inverses,
// their members' rows of A_0 (values + columns and the gathered x per entry,
// two pointers per row), members, b, own x read and written, two offsets per
// block
Op ring_csr_op(const DLevel& L, int c, double* x, const double* b, int cls) {
  Op o;
  o.kind = OP_CRING; o.cls = cls; o.lev = &L; o.M = &L.A;
  o.out = x; o.b = b;
  o.r0 = L.rcs[c]; o.r1 = L.rcs[c + 1]; o.n = o.r1 - o.r0;
  const double m = (double)(L.rcm[c + 1] - L.rcm[c]), ent = (double)(L.rce[c + 1] - L.rce[c]);
  o.bytes = 8.0 * (double)(L.rci[c + 1] - L.rci[c]) + 20.0 * ent + m * (16.0 + 4.0 + 8.0 + 16.0) + 16.0 * o.n;
  return o;
}

// one symmetric level-0 step of the seed rings on the CSR layout
// (tests/pointrings_ref.py step): ring colours ascending, the rest's point GS
// forward then backward, ring colours descending.  A level of at most
// CSR_GS_SMALL_ROWS rows runs the rest's two sweeps as one launch.
void ring_csr_step_ops(const DLevel& L, double* x, const double* b, std::vector<Op>* ops) {
  const int nc = (int)L.rcs.size() - 1;
  for (int c = 0; c < nc; ++c)
    if (L.rcs[c + 1] > L.rcs[c]) ops->push_back(ring_csr_op(L, c, x, b, C_L0_SMOOTH));
  if (L.gcs.size() > 1 && L.gcs.back() > 0) cgs_smooth_ops(L, false, 1, 1, -1, x, b, C_L0_SMOOTH, C_L0_WB, ops);
  for (int c = nc - 1; c >= 0; --c)
    if (L.rcs[c + 1] > L.rcs[c]) ops->push_back(ring_csr_op(L, c, x, b, C_L0_SMOOTH));
}

// CSR cycle of level 0 with the seed-ring Schwarz (SCHWARZ_RINGS on the CSR
// layout): x = 0, nu1 steps, r = b - A x, restrict, the level smoother's own
// CSR cycle below (W: a second visit), coarse scaling, x += P e, nu2 steps;
// the step is palindromic, so it serves both sides; in place on xout
void cycle_ops_csr(const DeviceHandle* h, int l, const double* b, double* xout, std::vector<Op>* ops);

// the coarse visit of a CSR cycle: C.x ~ A_c^-1 C.b on level c.  V: the cycle
// of level c; W: a second one on the updated residual; nonlinear AMLI (c not
// the coarsest): amli_degree steps of flexible CG preconditioned by that
// cycle, step 0 on C.b itself and straight into p_0 / q_0, e in C.x
void coarse_visit_ops_csr(const DeviceHandle* h, int c, std::vector<Op>* ops) {
  const DLevel& C = h->L[c];
  const mamg_params& p = h->p;
  if (kcycle(p) && !C.coarsest) {
    for (int j = 0; j < p.amli_degree; ++j) {
      double* z = j == 0 ? C.kp[0] : C.kz;
      cycle_ops_csr(h, c, j == 0 ? C.b : C.kr, z, ops);
      ops->push_back(csr_op(C.A, EPI_Y, C_MISC, 1, z, nullptr, nullptr, nullptr, j == 0 ? C.kq[0] : C.kw));
      kstep_ops(h, c, j, ops);
    }
    return;
  }
  cycle_ops_csr(h, c, C.b, C.x, ops);
  if (p.cycle_type == MAMG_W_CYCLE && !C.coarsest) {
    ops->push_back(csr_op(C.A, EPI_RESID, C_MISC, 1, C.x, nullptr, C.b, nullptr, C.c));
    cycle_ops_csr(h, c, C.c, C.e, ops);
    ops->push_back(axpy_op(C.n, C.e, C.x));
  }
}

void cycle_ops_csr_rings(const DeviceHandle* h, const double* b, double* xout, std::vector<Op>* ops) {
  const DLevel& L = h->L[0];
  const DLevel& C = h->L[1];
  const mamg_params& p = h->p;
  double* X = xout;
  Op z;
  z.kind = OP_ZERO; z.cls = C_L0_WB; z.n = L.n; z.out = X; z.bytes = 8.0 * L.n;
  ops->push_back(z);
  for (int s = 0; s < p.presmooth_iter; ++s) ring_csr_step_ops(L, X, b, ops);
  ops->push_back(csr_op(L.A, EPI_RESID, C_L0_RESID, 0, X, nullptr, b, nullptr, L.r));
  ops->push_back(csr_op(L.R, EPI_Y, C_L0_R, 0, L.r, nullptr, nullptr, nullptr, C.b));
  coarse_visit_ops_csr(h, 1, ops);
  if (p.coarse_scaling) scale_ops(h, 1, ops);
  ops->push_back(csr_op(L.P, EPI_YADD, C_L0_P, 0, C.x, X, nullptr, nullptr, X));
  for (int s = 0; s < p.postsmooth_iter; ++s) ring_csr_step_ops(L, X, b, ops);
}

// CSR cycle with the point-wise multicolour GS / SGS (cycle_ops_bsr's GS
// branch restated for CSR): x = 0, nu1 x (forward [+ backward if SGS]),
// r = b - A x, restrict, recurse (W: a second visit on the updated residual),
// coarse scaling, x += P e, nu2 x ([forward if SGS] + backward); in place on xout
void cycle_ops_csr_gs(const DeviceHandle* h, int l, const double* b, double* xout, std::vector<Op>* ops) {
  const DLevel& L = h->L[l];
  const DLevel& C = h->L[l + 1];
  const mamg_params& p = h->p;
  const bool l0 = l == 0, sgs = p.smoother == MAMG_SMOOTHER_SGS_POINT;
  const int tagA = l0 ? 0 : 1;
  const int clsS = l0 ? C_L0_SMOOTH : C_COARSE;
  const int clsW = l0 ? C_L0_WB : C_COARSE;
  double* X = xout;
  cgs_smooth_ops(L, true, p.presmooth_iter, 1, sgs ? -1 : 0, X, b, clsS, clsW, ops);
  ops->push_back(csr_op(L.A, EPI_RESID, l0 ? C_L0_RESID : C_COARSE, tagA, X, nullptr, b, nullptr, L.r));
  ops->push_back(csr_op(L.R, EPI_Y, l0 ? C_L0_R : C_COARSE, tagA, L.r, nullptr, nullptr, nullptr, C.b));
  coarse_visit_ops_csr(h, l + 1, ops);
  if (p.coarse_scaling) scale_ops(h, l + 1, ops);
  ops->push_back(csr_op(L.P, EPI_YADD, l0 ? C_L0_P : C_COARSE, tagA, C.x, X, nullptr, nullptr, X));
  cgs_smooth_ops(L, false, p.postsmooth_iter, sgs ? 1 : 0, -1, X, b, clsS, clsW, ops);
}

// ---- CSR layout: cycle from zero initial guess: xout = MG_l(b) --------------
void cycle_ops_csr(const DeviceHandle* h, int l, const double* b, double* xout, std::vector<Op>* ops) {
  const DLevel& L = h->L[l];
  const mamg_params& p = h->p;
  const bool l0 = l == 0;
  if (L.coarsest) { ops->push_back(gemv_op(L, b, xout)); return; }
  if (l0 && L.rcs.size() > 1) { cycle_ops_csr_rings(h, b, xout, ops); return; }
  if (L.gcs.size() > 1) { cycle_ops_csr_gs(h, l, b, xout, ops); return; }
  const DLevel& C = h->L[l + 1];
  const bool blk = L.WB.n > 0;
  const int tagA = l0 ? 0 : 1;
  const int clsS = l0 ? C_L0_SMOOTH : C_COARSE;
  const int clsW = l0 ? C_L0_WB : C_COARSE;
  double* X = L.t;
  double* X2 = L.t2;
  const int steps = smoother_steps(p);
  const int npre = p.presmooth_iter * steps, npost = p.postsmooth_iter * steps;
  if (blk) {
    ops->push_back(csr_op(step_wb(L, 0, true), EPI_Y, clsW, tagA, b, nullptr, nullptr, nullptr, X));
  } else {
    Op o;
    o.kind = OP_SCALE; o.cls = clsW; o.n = L.n; o.w = step_winv(L, 0, true); o.x = b; o.out = X;
    o.bytes = 24.0 * L.n;
    ops->push_back(o);
  }
  for (int s = 1; s < npre; ++s) {
    if (blk) {
      ops->push_back(csr_op(L.A, EPI_RESID, clsS, tagA, X, nullptr, b, nullptr, L.r));
      ops->push_back(csr_op(step_wb(L, s, true), EPI_YADD, clsW, tagA, L.r, X, nullptr, nullptr, X2));
    } else {
      ops->push_back(csr_op(L.A, EPI_JACOBI, clsS, tagA, X, X, b, step_winv(L, s, true), X2));
    }
    std::swap(X, X2);
  }
  ops->push_back(csr_op(L.A, EPI_RESID, l0 ? C_L0_RESID : C_COARSE, tagA, X, nullptr, b, nullptr, L.r));
  ops->push_back(csr_op(L.R, EPI_Y, l0 ? C_L0_R : C_COARSE, tagA, L.r, nullptr, nullptr, nullptr, C.b));
  coarse_visit_ops_csr(h, l + 1, ops);
  if (p.coarse_scaling) scale_ops(h, l + 1, ops);
  ops->push_back(csr_op(L.P, EPI_YADD, l0 ? C_L0_P : C_COARSE, tagA, C.x, X, nullptr, nullptr, X));
  for (int s = 0; s < npost; ++s) {
    double* out = (s == npost - 1) ? xout : X2;
    if (blk) {
      ops->push_back(csr_op(L.A, EPI_RESID, clsS, tagA, X, nullptr, b, nullptr, L.r));
      ops->push_back(csr_op(step_wb(L, s, false), EPI_YADD, clsW, tagA, L.r, X, nullptr, nullptr, out));
    } else {
      ops->push_back(csr_op(L.A, EPI_JACOBI, clsS, tagA, X, X, b, step_winv(L, s, false), out));
    }
    if (out == X2) std::swap(X, X2);
  }
}

}  // namespace

// ---- BSR2 layout.  b / xout of level 0 are the caller's field-major vectors
// (stride nv0); all other vectors are node-interleaved (stride 0).

// one colour of a node-patch sweep: per patch its packed inverse, its node
// rows (blocks + pointers), b and x read/write for its dofs, the gathered x
Op patch_op(const DLevel& L, int c, double* x, const double* b, int64_t bs, int cls) {
  Op o;
  o.kind = OP_PATCH; o.cls = cls; o.lev = &L;
  o.out = x; o.b = b; o.bs = bs;
  o.r0 = L.pcs[c]; o.r1 = L.pcs[c + 1]; o.n = o.r1 - o.r0;
  const double np = (double)o.n, nv = (double)(L.n / 2);
  const double mavg = nv > 0 ? (double)L.Snb / nv : 0.0;   // nodes per patch = blocks per row
  o.bytes = np * (8.0 * (double)L.pus + mavg * (36.0 * mavg + 8.0) + mavg * (16.0 + 32.0) + 12.0);
  return o;
}

// one colour of a seed-ring sweep: per block its transposed inverse, its
// members' rows of A_0 (blocks + pointers), b and x read/write for its
// members, the gathered x
Op ring_op(const DLevel& L, int c, double* x, const double* b, int64_t bs, int cls) {
  Op o;
  o.kind = OP_RING; o.cls = cls; o.lev = &L;
  o.out = x; o.b = b; o.bs = bs;
  o.r0 = L.rcs[c]; o.r1 = L.rcs[c + 1]; o.n = o.r1 - o.r0;
  const double nb = (double)(L.rcs.back()), frac = nb > 0 ? (double)o.n / nb : 0.0;
  const double nv = (double)(L.n / 2), bpr = nv > 0 ? (double)L.Snb / nv : 0.0;   // blocks per node row
  const double m = frac * (double)L.rnm;                                          // members of this colour
  o.bytes = frac * 8.0 * L.rinv_n + m * (bpr * 36.0 + 16.0 + 4.0 + 8.0 + 16.0 + bpr * 16.0) + 16.0 * o.n;
  return o;
}

namespace {

void ring_sweep_ops(const DLevel& L, bool fwd, double* x, const double* b, int64_t bs, int cls, std::vector<Op>* ops) {
  const int nc = (int)L.rcs.size() - 1;
  for (int k = 0; k < nc; ++k) {
    const int c = fwd ? k : nc - 1 - k;
    if (L.rcs[c + 1] > L.rcs[c]) ops->push_back(ring_op(L, c, x, b, bs, cls));
  }
}

void patch_sweep_ops(const DLevel& L, bool fwd, double* x, const double* b, int64_t bs, int cls, std::vector<Op>* ops) {
  const int nc = (int)L.pcs.size() - 1;
  for (int k = 0; k < nc; ++k) {
    const int c = fwd ? k : nc - 1 - k;
    if (L.pcs[c + 1] > L.pcs[c]) ops->push_back(patch_op(L, c, x, b, bs, cls));
  }
}

void gs_sweep_ops(const DLevel& L, bool fwd, double* x, const double* b, int64_t bs, int cls, std::vector<Op>* ops) {
  const int nc = (int)L.gcs.size() - 1;
  for (int k = 0; k < nc; ++k) {
    const int c = fwd ? k : nc - 1 - k;
    if (L.gcs[c + 1] > L.gcs[c]) ops->push_back(gs_op(L, c, x, b, bs, cls));
  }
}

// coarse-grid correction scaling of level lc's correction e = C.x against its
// right-hand side C.b: q = A_c e, then alpha and e <- alpha e
void scale_ops(const DeviceHandle* h, int lc, std::vector<Op>* ops) {
  const DLevel& C = h->L[lc];
  if (h->bsr) ops->push_back(bsr_op(C.Ab, EPI_Y, C_MISC, 1, C.x, 0, nullptr, nullptr, 0, nullptr, C.q, 0));
  else ops->push_back(csr_op(C.A, EPI_Y, C_MISC, 1, C.x, nullptr, nullptr, nullptr, C.q));
  Op d;
  d.kind = OP_DOT2; d.cls = C_MISC; d.n = C.n; d.b = C.b; d.x = C.x; d.y = C.q; d.part = C.part2;
  d.bytes = 24.0 * C.n;
  ops->push_back(d);
  Op sc;
  sc.kind = OP_CSCALE; sc.cls = C_MISC; sc.n = C.n; sc.part = C.part2; sc.out = C.x; sc.bytes = 16.0 * C.n;
  ops->push_back(sc);
}

// ---- BSR2 layout.  b / xout of level 0 are the caller's field-major vectors
// (stride nv0); all other vectors are node-interleaved (stride 0).
// one op of the launch path as a coarse-tail op (tail_kernel; at most vl_cap
// lanes per row, MAMG_TAIL_VL); false if the tail cannot express it (level-0
// formats and strides, patches, CSR; the nonlinear AMLI steps unless the
// handle has opted in: ktail, mamg_set_kcycle_tail).  A K op's operands are
// its level's (o.lev): the caller gives it the level's table (TOp::nb)
bool to_tail(const Op& o, int vl_cap, bool ktail, TOp* t) {
  *t = TOp();
  switch (o.kind) {
    case OP_BSR:
    case OP_GS: {
      const DBsr& M = *o.Mb;
      if (M.sell || M.half || M.rowdict || M.split || o.xs || o.bs || o.os || o.xfm || M.lanes < 1 || M.lanes > 64) return false;
      t->kind = o.kind == OP_GS ? T_GS : T_BSR;
      t->epi = o.epi; t->vl = std::min(M.lanes, vl_cap); t->sym = M.sym ? 1 : 0; t->n = M.nr; t->nb = M.nb;
      t->ptr = M.ptr; t->col = M.col; t->val = M.val;
      t->x = o.kind == OP_GS ? o.out : o.x; t->y = o.y; t->b = o.b; t->W = o.W; t->out = o.out;
      t->r0 = o.r0; t->r1 = o.r1; t->perm = o.perm;
      return true;
    }
    case OP_BD:
      if (o.bs || o.os) return false;
      t->kind = T_BD; t->n = o.n; t->W = o.W; t->b = o.b; t->out = o.out;
      return true;
    case OP_GEMV: t->kind = T_GEMV; t->n = o.n; t->w = o.w; t->x = o.x; t->out = o.out; return true;
    case OP_AXPY: t->kind = T_AXPY; t->n = o.n; t->x = o.x; t->out = o.out; return true;
    case OP_ZERO: t->kind = T_ZERO; t->n = o.n; t->out = o.out; return true;
    case OP_DOT2: t->kind = T_DOT2; t->n = o.n; t->b = o.b; t->x = o.x; t->y = o.y; t->part = o.part; return true;
    case OP_CSCALE: t->kind = T_CSCALE; t->n = o.n; t->part = o.part; t->out = o.out; return true;
    case OP_KDOT:
    case OP_KORTH:
    case OP_KUPD:
      if (!ktail || !o.lev) return false;
      t->kind = o.kind == OP_KDOT ? T_KDOT : o.kind == OP_KORTH ? T_KORTH : T_KUPD;
      t->n = o.n; t->r0 = o.r0; t->r1 = o.r1;
      return true;
    default: return false;
  }
}

void cycle_ops_bsr(const DeviceHandle* h, int l, const double* b, int64_t bs, double* xout,
                   int64_t os, std::vector<Op>* ops, bool tail_ok = true, bool x1_ready = false);

static_assert(sizeof(TOp) % 8 == 0, "TOp is copied into LDS as 8-byte words");
constexpr int64_t TAIL_LDS_MAX = 160 * 1024 - 1024;   // gfx950: 160 KB per workgroup, minus the static arrays

// LDS residency of a coarse-tail program (see T_COPY): every work vector of
// levels >= l the program touches gets an LDS slot; the fields are rewritten
// to tagged LDS offsets, vectors read before written are copied in first and
// written ones copied out last.  Returns the dynamic LDS bytes, or 0 (program
// unchanged: global vectors) when the plan exceeds the LDS.
// the vectors step j of m reads, then the ones it writes, as slots of its level's table (kstep_ops, tail_k*)
void kop_touches(const TOp& o, std::vector<int>* rd, std::vector<int>* wr) {
  const int j = (int)o.r0;
  const bool first = j == 0, last = j == (int)o.r1 - 1;
  rd->clear();
  wr->clear();
  if (o.kind == T_KDOT) {
    rd->push_back(KT_Z);
    for (int i = 0; i < j; ++i) rd->push_back(KT_Q + i);
    wr->push_back(KT_PART);
  } else if (o.kind == T_KORTH) {
    if (j > 0) rd->push_back(KT_PART);
    for (int i = 0; i < j; ++i) { rd->push_back(KT_P + i); rd->push_back(KT_Q + i); }
    if (j > 0) { rd->push_back(KT_Z); rd->push_back(KT_W); }
    else { rd->push_back(KT_P); rd->push_back(KT_Q); }
    rd->push_back(first ? KT_B : KT_R);
    if (j > 0) { wr->push_back(KT_P + j); wr->push_back(KT_Q + j); }
    wr->push_back(KT_PART);
  } else {   // T_KUPD
    rd->push_back(KT_PART);
    rd->push_back(KT_P + j);
    if (!first) rd->push_back(KT_X);
    if (!last) { rd->push_back(KT_Q + j); rd->push_back(first ? KT_B : KT_R); }
    wr->push_back(KT_PART);
    wr->push_back(KT_X);
    if (!last) wr->push_back(KT_R);
  }
}
inline bool is_kop(const TOp& o) { return o.kind == T_KDOT || o.kind == T_KORTH || o.kind == T_KUPD; }

int64_t tail_lds_plan(const DeviceHandle* h, int l, std::vector<TOp>* prog, std::vector<KTable>* ktabs,
                      int64_t reserve = 0) {
  if (!h->sw.tail_lds) return 0;
  struct Vec {
    double* base;
    int64_t n;
    bool used = false, in = false, out = false, seen = false, lds = false;
    int64_t off = 0, uses = 0;
  };
  std::vector<Vec> vecs;
  for (size_t ll = l; ll < h->L.size(); ++ll) {
    const DLevel& L = h->L[ll];
    for (double* v : {L.b, L.x, L.t, L.t2, L.r, L.c, L.e, L.q})
      if (v) vecs.push_back({v, L.n});
    // nonlinear AMLI: the cycle of a Krylov level runs on its r and writes its z or p_0
    for (double* v : {L.kr, L.kz, L.kw, L.kp[0], L.kq[0]})
      if (v) vecs.push_back({v, L.n});
    if (L.part2) vecs.push_back({L.part2, 2 * SCALE_BLOCKS});
    // the Krylov levels inside the program: the later directions and the steps' scalars and partials
    for (int i = 1; i < MAMG_NL_AMLI_MAX; ++i)
      for (double* v : {L.kp[i], L.kq[i]})
        if (v) vecs.push_back({v, L.n});
    if (L.kpart) vecs.push_back({L.kpart, KP_SIZE});
  }
  auto find = [&](const double* p) -> Vec* {
    for (auto& v : vecs)
      if (p >= v.base && p < v.base + v.n) return &v;
    return nullptr;
  };
  auto touch = [&](const double* p, bool write) {
    Vec* v = find(p);
    if (!v) return;
    v->used = true;
    ++v->uses;
    if (!v->seen && !write) v->in = true;
    v->seen = true;
    if (write) v->out = true;
  };
  std::vector<int> krd, kwr;
  for (const TOp& o : *prog) {   // reads of an op before its writes
    if (is_kop(o)) {
      const KTable& T = (*ktabs)[(size_t)o.nb];
      kop_touches(o, &krd, &kwr);
      for (int sl : krd) touch(T.v[sl], false);
      for (int sl : kwr) touch(T.v[sl], true);
      continue;
    }
    const bool rmw = o.kind == T_GS || o.kind == T_AXPY || o.kind == T_CSCALE;
    for (const double* r : {o.x, o.y, o.b}) if (r) touch(r, false);
    if (o.part) touch(o.part, o.kind != T_CSCALE ? true : false);
    if (o.out) { if (rmw) touch(o.out, false); touch(o.out, true); }
  }
  // the most-used bytes first (the deepest levels: small and visited most
  // often) until the LDS is full; the rest stay global
  std::vector<Vec*> order;
  for (auto& v : vecs)
    if (v.used) order.push_back(&v);
  std::stable_sort(order.begin(), order.end(),
                   [](const Vec* a, const Vec* b) { return a->uses * b->n > b->uses * a->n; });
  int64_t off = 0;
  for (Vec* v : order) {
    const int64_t sz = (v->n * 8 + 15) / 16 * 16;
    if (off + sz > TAIL_LDS_MAX - reserve) continue;
    v->lds = true;
    v->off = off;
    off += sz;
  }
  if (off == 0) return 0;
  static std::atomic<uint64_t> attr_devices{0};   // the attribute is set once per device
  const int dev = h->device & 63;
  if (!(attr_devices >> dev & 1)) {
    const void* fns[] = {(const void*)tail_kernel<false, false, false>, (const void*)tail_kernel<false, true, false>,
                         (const void*)tail_kernel<false, false, true>, (const void*)tail_kernel<false, true, true>,
                         (const void*)tail_kernel<false, false, false, true>, (const void*)tail_kernel<false, true, false, true>,
                         (const void*)tail_kernel<false, false, true, true>, (const void*)tail_kernel<false, true, true, true>,
#if MAMG_DIAG   // the stamped (profiling) variants
                         (const void*)tail_kernel<true, false, false>, (const void*)tail_kernel<true, true, false>,
                         (const void*)tail_kernel<true, false, true>, (const void*)tail_kernel<true, true, true>,
                         (const void*)tail_kernel<true, false, false, true>, (const void*)tail_kernel<true, true, false, true>,
                         (const void*)tail_kernel<true, false, true, true>, (const void*)tail_kernel<true, true, true, true>,
#endif
    };
    bool ok = true;
    for (const void* f : fns)
      ok = ok && hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)TAIL_LDS_MAX) == hipSuccess;
    if (!ok) {
      (void)hipGetLastError();
      return 0;                        // no large dynamic LDS: keep the global-vector program
    }
    attr_devices.fetch_or(1ull << dev);
  }
  auto tag = [&](const double* p) -> double* {
    Vec* v = find(p);
    if (!v || !v->lds) return const_cast<double*>(p);
    return reinterpret_cast<double*>((uintptr_t)(v->off + 8 * (p - v->base)) | 1);
  };
  for (TOp& o : *prog) {
    o.x = tag(o.x); o.y = tag(o.y); o.b = tag(o.b); o.out = tag(o.out); o.part = tag(o.part);
  }
  for (KTable& T : *ktabs)
    for (const double*& v : T.v) v = tag(v);
  std::vector<TOp> full;
  for (const auto& v : vecs)
    if (v.lds && v.in) {
      TOp c;
      c.kind = T_COPY; c.n = v.n; c.x = v.base; c.out = reinterpret_cast<double*>((uintptr_t)v.off | 1);
      full.push_back(c);
    }
  full.insert(full.end(), prog->begin(), prog->end());
  for (const auto& v : vecs)
    if (v.lds && v.out) {
      TOp c;
      c.kind = T_COPY; c.n = v.n; c.x = reinterpret_cast<double*>((uintptr_t)v.off | 1); c.out = v.base;
      full.push_back(c);
    }
  prog->swap(full);
  return off;
}

// Register residency of a coarse-tail program (TOp, tail_kernel RES): the
// operators of levels l, l + 1, .. get one row per thread, while their rows
// fit the workgroup.  A level with a multicolour GS layout holds it (Gb:
// colour-permuted, each colour padded to 64-row slices); the level's other
// ops on A (residual, scaling) then read Gb's row i at node perm(i) -- the
// same blocks in the same order as A's row.  One T_RLOAD op in front loads
// every resident row from an image (see tail_rload) built here from the
// matrices; img holds it, and the T_RLOAD's val / col / ridx / b fields hold
// (byte offset in img + 1) until the caller sets device pointers, its r0 / r1
// the LDS region's place once the LDS plan is known.  Returns false when
// nothing is resident.
bool tail_res_plan(const DeviceHandle* h, int l, std::vector<TOp>* prog, std::vector<char>* img, int64_t* nov,
                   int* rrows) {
  *nov = 0;
  *rrows = 0;
  if (!h->sw.tail_res) return false;
  constexpr int T = TAIL_THREADS;
  std::vector<dv4> iv((size_t)RES_RB * T, dv4{0.0, 0.0, 0.0, 0.0});
  std::vector<uint32_t> ic((size_t)RES_RB / 2 * T, 0u);
  std::vector<int32_t> hdr((size_t)3 * T, 0);
  std::vector<dv4> gd(T, dv4{0.0, 0.0, 0.0, 0.0});
  std::vector<dv4> ovv;
  std::vector<uint16_t> ovc;
  auto get = [](void* dst, const void* src, size_t bytes) {
    if (hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost) == hipSuccess) return true;
    (void)hipGetLastError();
    return false;
  };
  int rbase = 0;
  for (size_t ll = (size_t)l; ll < h->L.size(); ++ll) {
    const DLevel& L = h->L[ll];
    const bool hasg = L.gcs.size() > 1;
    const DBsr& M = hasg ? L.Gb : L.Ab;
    if (!M.ptr || M.sell || M.half || M.split || M.nr <= 0 || M.nc > 65536) continue;
    std::vector<int32_t> pm(hasg ? M.nr : 0);
    std::vector<int64_t> ptr(M.nr + 1);
    if ((hasg && !get(pm.data(), L.gperm, M.nr * sizeof(int32_t))) ||
        !get(ptr.data(), M.ptr, (M.nr + 1) * sizeof(int64_t)))
      return false;
    std::vector<int64_t> comp(M.nr + 1, 0);   // rows before -> compact rows before
    std::vector<int32_t> rows;                // compact -> M row
    for (int64_t i = 0; i < M.nr; ++i) {
      if (!hasg || pm[i] >= 0) rows.push_back((int32_t)i);
      comp[i + 1] = (int64_t)rows.size();
    }
    const int n = (int)rows.size();
    if (rbase + n > T) continue;   // a deeper level may still fit
    const int64_t nb = M.nb;
    std::vector<int32_t> col(nb);
    std::vector<double> val((size_t)(M.sym ? 3 : 4) * nb);
    std::vector<dv4> W(hasg ? M.nr : 0);
    if (!get(col.data(), M.col, nb * sizeof(int32_t)) || !get(val.data(), M.val, val.size() * sizeof(double)) ||
        (hasg && !get(W.data(), L.Gd, M.nr * sizeof(dv4))))
      return false;
    auto blk = [&](int64_t k) {
      if (!M.sym) return dv4{val[4 * k], val[4 * k + 1], val[4 * k + 2], val[4 * k + 3]};
      const double b = val[2 * nb + k];
      return dv4{val[2 * k], b, b, val[2 * k + 1]};
    };
    for (int j = 0; j < n; ++j) {
      const int t = rbase + j, i = rows[j];
      const int64_t p0 = ptr[i], len = ptr[i + 1] - p0;
      hdr[t] = (int)len;
      hdr[T + t] = hasg ? pm[i] : i;
      hdr[2 * T + t] = (int)ovv.size();
      for (int k = 0; k < RES_RB && k < len; ++k) {
        iv[(size_t)k * T + t] = blk(p0 + k);
        ic[(size_t)(k / 2) * T + t] |= (uint32_t)col[p0 + k] << (16 * (k & 1));
      }
      if (len > RES_RB) {   // whole fours (tail_res), zero-padded
        const int64_t nk = (len - RES_RB + 3) / 4 * 4;
        for (int64_t k = 0; k < nk; ++k) {
          const bool in = RES_RB + k < len;
          ovv.push_back(in ? blk(p0 + RES_RB + k) : dv4{0.0, 0.0, 0.0, 0.0});
          ovc.push_back(in ? (uint16_t)col[p0 + RES_RB + k] : (uint16_t)0);
        }
      }
      if (hasg) gd[t] = W[i];
    }
    for (TOp& t : *prog) {
      if (t.kind == T_GS && hasg && t.ptr == L.Gb.ptr) {
        t.res = 1; t.rbase = rbase; t.r0 = comp[t.r0]; t.r1 = comp[t.r1];
      } else if (t.kind == T_BSR && t.ptr == L.Ab.ptr) {
        t.res = 1; t.rbase = rbase; t.r0 = 0; t.r1 = n;
        t.ptr = M.ptr; t.col = M.col; t.val = M.val; t.sym = M.sym ? 1 : 0; t.nb = M.nb;
        t.perm = hasg ? L.gperm : nullptr;
      }
    }
    rbase += n;
  }
  if (rbase == 0) return false;
  *nov = (int64_t)ovv.size();
  *rrows = rbase;
  // the image: values, columns, header, then the LDS region's bytes (block
  // inverses, overflow values, overflow columns padded to 16 B)
  auto put = [&](const void* p, size_t bytes) {
    const size_t off = img->size();
    img->insert(img->end(), static_cast<const char*>(p), static_cast<const char*>(p) + bytes);
    img->resize((img->size() + 15) / 16 * 16, 0);
    return off;
  };
  TOp ld;
  ld.kind = T_RLOAD; ld.r0 = -1; ld.r1 = *nov;
  // the coarsest level's dense inverse (T_GEMV, n <= 64) joins the region:
  // its op's w becomes (offset in the region + 1) with res = 2, turned into
  // a tagged LDS address with the region's (tail_ops)
  std::vector<double> dense;
  std::vector<std::pair<const double*, size_t>> dmap;
  for (TOp& t : *prog) {
    if (t.kind != T_GEMV || !t.w || t.n > 64 || t.n <= 0) continue;
    size_t at = SIZE_MAX;
    for (const auto& q : dmap)
      if (q.first == t.w) at = q.second;
    if (at == SIZE_MAX) {
      at = dense.size();
      dense.resize(at + (size_t)(t.n * t.n));
      if (!get(dense.data() + at, t.w, (size_t)(t.n * t.n) * sizeof(double))) return false;
      dmap.push_back({t.w, at});
    }
    t.res = 2;
    t.w = reinterpret_cast<const double*>((uintptr_t)at);   // doubles into the dense part
  }
  const size_t ov = put(iv.data(), iv.size() * sizeof(dv4));
  const size_t oc = put(ic.data(), ic.size() * sizeof(uint32_t));
  const size_t oh = put(hdr.data(), hdr.size() * sizeof(int32_t));
  const size_t og = put(gd.data(), gd.size() * sizeof(dv4));
  if (!ovv.empty()) put(ovv.data(), ovv.size() * sizeof(dv4));
  if (!ovc.empty()) put(ovc.data(), ovc.size() * sizeof(uint16_t));
  const size_t odn = img->size();
  if (!dense.empty()) put(dense.data(), dense.size() * sizeof(double));
  for (TOp& t : *prog)   // byte offset of each dense matrix in the region
    if (t.kind == T_GEMV && t.res == 2) t.w = reinterpret_cast<const double*>((uintptr_t)(odn - og + 8 * (uintptr_t)t.w));
  ld.n = (int64_t)(img->size() - og);   // the LDS region's bytes (a multiple of 16)
  ld.val = reinterpret_cast<const double*>((uintptr_t)ov + 1);
  ld.col = reinterpret_cast<const int32_t*>((uintptr_t)oc + 1);
  ld.ridx = reinterpret_cast<const int32_t*>((uintptr_t)oh + 1);
  ld.b = reinterpret_cast<const double*>((uintptr_t)og + 1);
  prog->insert(prog->begin(), ld);
  return true;
}

// the cycle of level l and everything below as one tail_kernel launch; the
// device op list is built once per (b, x) and kept on the handle
bool tail_ops(const DeviceHandle* h, int l, const double* b, double* xout, std::vector<Op>* ops) {
  const DeviceHandle::TailProg* tp = nullptr;
  for (const auto& t : h->tails)
    if (t.b == b && t.x == xout) tp = &t;
  if (!tp) {
    std::vector<Op> sub;
    cycle_ops_bsr(h, l, b, 0, xout, 0, &sub, false);
    std::vector<TOp> prog(sub.size());
    std::vector<KTable> ktabs;            // one per Krylov level inside the program
    std::vector<const DLevel*> klev;
    double bytes = 0.0;
    for (size_t k = 0; k < sub.size(); ++k) {
      if (!to_tail(sub[k], h->sw.tail_vl, h->kcycle_tail, &prog[k])) { h->tail_refused = true; return false; }
      bytes += sub[k].bytes;
      if (!is_kop(prog[k])) continue;
      const DLevel* C = sub[k].lev;
      size_t at = 0;
      while (at < klev.size() && klev[at] != C) ++at;
      if (at == klev.size()) {
        KTable T = {};
        T.v[KT_R] = C->kr; T.v[KT_Z] = C->kz; T.v[KT_W] = C->kw; T.v[KT_B] = C->b; T.v[KT_X] = C->x;
        T.v[KT_PART] = C->kpart;
        for (int i = 0; i < MAMG_NL_AMLI_MAX; ++i) { T.v[KT_P + i] = C->kp[i]; T.v[KT_Q + i] = C->kq[i]; }
        klev.push_back(C);
        ktabs.push_back(T);
      }
      prog[k].nb = (int64_t)at;
    }
    h->tail_refused = false;
    bool replanned = false;   // a residency plan was made, did not fit the LDS and was discarded
    std::vector<char> img;
    int64_t nov = 0;
    int rrows = 0;
    const std::vector<TOp> plain = prog;
    const std::vector<KTable> kplain = ktabs;
    bool res = tail_res_plan(h, l, &prog, &img, &nov, &rrows);
    int64_t region = 0;   // the resident rows' LDS region, kept free of vectors
    for (const TOp& t : prog)
      if (t.kind == T_RLOAD) region = t.n;
    int64_t lds = tail_lds_plan(h, l, &prog, &ktabs, region + 16);
    // the program itself into the LDS after the vectors when it fits
    // (TAIL_LDS_MAX); the dynamic LDS then covers both
    int prog_lds = -1;
    int64_t pbytes = (int64_t)(prog.size() * sizeof(TOp));
    // default: scalar loads (s_load of a uniform descriptor: 795 vs 1262
    // cycles per empty op)
    if (lds > 0 && h->sw.tail_prog_lds) {
      const int64_t off = (lds + 15) / 16 * 16;
      if (off + pbytes <= TAIL_LDS_MAX) {
        prog_lds = (int)off;
        lds = off + pbytes;
      }
    }
    // the resident rows' LDS region (block inverses, overflow blocks) after
    // both; without room for it (or for the program) the tail keeps its
    // operators in global memory
    if (res) {
      int64_t need = 0;   // the T_RLOAD's LDS region bytes
      for (const TOp& t : prog)
        if (t.kind == T_RLOAD) need = t.n;
      const int64_t off = (lds + 15) / 16 * 16;
      if (lds > 0 && off + need <= TAIL_LDS_MAX) {
        for (TOp& t : prog) {
          if (t.kind == T_RLOAD) { t.r0 = off; t.r1 = nov; }
          if (t.kind == T_GEMV && t.res == 2)   // its matrix in the region: a tagged LDS address
            t.w = reinterpret_cast<const double*>((uintptr_t)(off + (uintptr_t)t.w) | 1);
        }
        lds = off + need;
      } else {
        res = false;
        replanned = true;
        nov = 0;
        rrows = 0;
        img.clear();
        prog = plain;
        ktabs = kplain;
        lds = tail_lds_plan(h, l, &prog, &ktabs);
        prog_lds = -1;
        pbytes = (int64_t)(prog.size() * sizeof(TOp));
        if (lds > 0 && h->sw.tail_prog_lds) {
          const int64_t o2 = (lds + 15) / 16 * 16;
          if (o2 + pbytes <= TAIL_LDS_MAX) {
            prog_lds = (int)o2;
            lds = o2 + pbytes;
          }
        }
      }
    }
    // every gathered x in LDS: the ds_read variant of the kernel (read off
    // the final program: a replan above may have placed the vectors anew)
    bool xl = lds > 0;
    for (const TOp& t : prog)
      if ((t.kind == T_BSR || t.kind == T_GS) && !((uintptr_t)t.x & 1)) xl = false;
    // the plan as the tests read it (before the T_RLOAD's fields become device pointers)
    std::vector<int64_t> info(TAIL_INFO_HEAD, 0);
    info[TI_OPS] = (int64_t)prog.size(); info[TI_LDS] = lds; info[TI_XL] = xl ? 1 : 0; info[TI_RES] = res ? 1 : 0;
    info[TI_PROG_LDS] = prog_lds; info[TI_ROWS] = rrows; info[TI_NOV] = nov; info[TI_REPLANNED] = replanned ? 1 : 0;
    std::vector<int> krd, kwr;
    for (const TOp& t : prog) {
      if (t.kind != T_RLOAD && t.kind != T_COPY)   // a copy in or out is one of each by construction
        for (const double* v : {t.x, t.y, t.b, (const double*)t.out, (const double*)t.part})
          if (v) ++info[((uintptr_t)v & 1) ? TI_VEC_LDS : TI_VEC_GLOBAL];
      if (is_kop(t)) {   // its operands are its table's
        ++info[TI_OPS_K];
        kop_touches(t, &krd, &kwr);
        for (const std::vector<int>* sl : {&krd, &kwr})
          for (int q : *sl) ++info[((uintptr_t)ktabs[(size_t)t.nb].v[q] & 1) ? TI_VEC_LDS : TI_VEC_GLOBAL];
      }
      if (t.kind == T_BSR || t.kind == T_GS) {
        ++info[t.res ? TI_OPS_RES : TI_OPS_BSR];
        if (!t.res) info[TI_MAX_VL] = std::max<int64_t>(info[TI_MAX_VL], t.vl);
      }
      if (t.kind == T_GEMV) {
        ++info[TI_GEMVS];
        info.push_back(t.n);
        info.push_back(((uintptr_t)t.w & 1) ? 1 : 0);
      }
    }
    // one allocation: the ops, the K ops' tables, the resident rows' image
    void* d = nullptr;
    const int64_t koff = (pbytes + 15) / 16 * 16;
    const size_t kbytes = ktabs.size() * sizeof(KTable);
    const int64_t ioff = (koff + (int64_t)kbytes + 15) / 16 * 16;
    const size_t tbytes = img.size();
    if (raw_malloc(&d, (size_t)ioff + tbytes, "long") != hipSuccess) { (void)hipGetLastError(); return false; }
    char* dimg = static_cast<char*>(d) + ioff;
    for (TOp& t : prog)
      if (is_kop(t)) {
        t.ptr = reinterpret_cast<const int64_t*>(static_cast<char*>(d) + koff + (size_t)t.nb * sizeof(KTable));
        t.nb = 0;
      }
    auto fix = [&](auto*& f) {
      if (f) f = reinterpret_cast<std::remove_reference_t<decltype(f)>>(dimg + ((uintptr_t)f - 1));
    };
    for (TOp& t : prog)
      if (t.kind == T_RLOAD) { fix(t.val); fix(t.col); fix(t.ridx); fix(t.b); }
    if (hipMemcpy(d, prog.data(), prog.size() * sizeof(TOp), hipMemcpyHostToDevice) != hipSuccess ||
        (kbytes && hipMemcpy(static_cast<char*>(d) + koff, ktabs.data(), kbytes, hipMemcpyHostToDevice) != hipSuccess) ||
        (tbytes && hipMemcpy(dimg, img.data(), tbytes, hipMemcpyHostToDevice) != hipSuccess)) {
      (void)hipGetLastError();
      (void)raw_free(d);
      return false;
    }
    h->tails.push_back({b, xout, (TOp*)d, (int)prog.size(), bytes, lds, xl, prog_lds, res, !ktabs.empty(), std::move(info)});
    tp = &h->tails.back();
  }
  Op o;
  o.kind = OP_TAIL; o.cls = C_COARSE; o.prog = tp->prog; o.n = tp->n; o.bytes = tp->bytes;
  o.r0 = tp->lds;   // dynamic LDS bytes (0: the program reads global vectors)
  o.r1 = (tp->xl ? 1 : 0) | (tp->res ? 2 : 0) | (tp->kops ? 4 : 0);
  o.tail_pl = tp->prog_lds;
  ops->push_back(o);
  return true;
}

// level l's cycle (launch path) begins with the first sweep X = W b into L.t
// (OP_BD): the restriction into l may then write it (EPI_YBD)
bool starts_with_bd(const DeviceHandle* h, int l) {
  const DLevel& L = h->L[l];
  return l > 0 && l != h->tail_level && !L.coarsest && L.gcs.size() <= 1 && L.pcs.size() <= 1 &&
         L.rcs.size() <= 1;
}

// x1_ready: X = W b is already in L.t (written by the restriction's EPI_YBD)
// A_l as the cycle reads it: level 0's fp32 copy once the handle is narrowed
inline const DBsr& cyc_A(const DLevel& L) { return L.Ac.f32 ? L.Ac : L.Ab; }

// the coarse visit of a BSR2 cycle (coarse_visit_ops_csr restated): ybd: the
// restriction's epilogue has written the first sweep X = W C.b into C.t, which
// the visit's first cycle (V, W: the first visit; nonlinear AMLI: step 0, which
// preconditions C.b itself) then skips
void coarse_visit_ops_bsr(const DeviceHandle* h, int c, std::vector<Op>* ops, bool tail_ok, bool ybd) {
  const DLevel& C = h->L[c];
  const mamg_params& p = h->p;
  if (kcycle(p) && !C.coarsest) {
    for (int j = 0; j < p.amli_degree; ++j) {
      double* z = j == 0 ? C.kp[0] : C.kz;
      cycle_ops_bsr(h, c, j == 0 ? C.b : C.kr, 0, z, 0, ops, tail_ok, j == 0 && ybd);
      ops->push_back(bsr_op(C.Ab, EPI_Y, C_MISC, 1, z, 0, nullptr, nullptr, 0, nullptr, j == 0 ? C.kq[0] : C.kw, 0));
      kstep_ops(h, c, j, ops);
    }
    return;
  }
  cycle_ops_bsr(h, c, C.b, 0, C.x, 0, ops, tail_ok, ybd);
  if (p.cycle_type == MAMG_W_CYCLE && !C.coarsest) {
    ops->push_back(bsr_op(C.Ab, EPI_RESID, C_MISC, 1, C.x, 0, nullptr, C.b, 0, nullptr, C.c, 0));
    cycle_ops_bsr(h, c, C.c, 0, C.e, 0, ops, tail_ok);
    ops->push_back(axpy_op(C.n, C.e, C.x));
  }
}

void cycle_ops_bsr(const DeviceHandle* h, int l, const double* b, int64_t bs, double* xout,
                   int64_t os, std::vector<Op>* ops, bool tail_ok, bool x1_ready) {
  if (tail_ok && l > 0 && l == h->tail_level && bs == 0 && os == 0 && tail_ops(h, l, b, xout, ops)) return;
  const DLevel& L = h->L[l];
  const mamg_params& p = h->p;
  const bool l0 = l == 0;
  if (L.coarsest) { ops->push_back(gemv_op(L, b, xout)); return; }   // l > 0 here
  const DLevel& C = h->L[l + 1];
  const int64_t nv = L.n / 2;
  const int tagA = l0 ? 0 : 1;
  const int clsS = l0 ? C_L0_SMOOTH : C_COARSE;
  const int clsW = l0 ? C_L0_WB : C_COARSE;
  const bool pat = L.pcs.size() > 1;                      // node-patch Schwarz on this level
  const bool rng = L.rcs.size() > 1;                      // seed-ring Schwarz + the rest's GS
  const bool gs = L.gcs.size() > 1 || pat || rng;         // multicolour GS on this level
  const bool sgs = p.smoother == MAMG_SMOOTHER_SGS || pat || rng;
  auto sweep = [&](bool fwd, double* x) {
    if (pat) {
      patch_sweep_ops(L, fwd, x, b, bs, clsS, ops);
    } else if (rng) {   // one symmetric step = rings fwd, rest fwd | rest bwd, rings bwd (mamg_oracle.rings_step)
      if (fwd) { ring_sweep_ops(L, true, x, b, bs, clsS, ops); gs_sweep_ops(L, true, x, b, bs, clsS, ops); }
      else { gs_sweep_ops(L, false, x, b, bs, clsS, ops); ring_sweep_ops(L, false, x, b, bs, clsS, ops); }
    } else {
      gs_sweep_ops(L, fwd, x, b, bs, clsS, ops);
    }
  };
  const int steps = smoother_steps(p);
  const int npre = p.presmooth_iter * steps, npost = p.postsmooth_iter * steps;
  double* X = (gs && os == 0) ? xout : L.t;               // GS sweeps in place
  double* X2 = L.t2;
  if (gs) {   // pre: from x = 0, forward (SGS: then backward) sweeps
    Op z;
    z.kind = OP_ZERO; z.cls = clsW; z.n = L.n; z.out = X; z.bytes = 8.0 * L.n;
    ops->push_back(z);
    for (int s = 0; s < p.presmooth_iter; ++s) {
      sweep(true, X);
      if (sgs) sweep(false, X);
    }
  } else {    // first sweep from x = 0: X = W b (POLY: w_1 W b)
    Op o;
    o.kind = OP_BD; o.cls = clsW; o.n = nv; o.W = step_wd(L, 0, true); o.b = b; o.bs = bs; o.out = X;
    o.bytes = 32.0 * nv + 16.0 * nv + 16.0 * nv;
    if (!x1_ready) ops->push_back(o);
    for (int s = 1; s < npre; ++s) {
      ops->push_back(bsr_op(cyc_A(L), EPI_BJAC, clsS, tagA, X, 0, X, b, bs, step_wd(L, s, true), X2, 0));
      std::swap(X, X2);
    }
  }
  ops->push_back(bsr_op(cyc_A(L), EPI_RESID, l0 ? C_L0_RESID : C_COARSE, tagA, X, 0, nullptr, b, bs,
                        nullptr, L.r, 0));
  ops->push_back(bsr_op(L.Rb, EPI_Y, l0 ? C_L0_R : C_COARSE, tagA, L.r, 0, nullptr, nullptr, 0,
                        nullptr, C.b, 0));
  ops->back().remap = 1;
  // the coarse level's first sweep in the restriction's epilogue (launch path,
  // bsr2_kernel layouts only; the tail programs keep their own T_BD)
  const bool ybd = (h->sw.fuse_rbd == 1 || (h->sw.fuse_rbd == 2 && l > 0)) && tail_ok && starts_with_bd(h, l + 1) &&
                   !L.Rb.sell && !L.Rb.half && !L.Rb.sym && !L.Rb.split;
  if (ybd) {
    Op& r = ops->back();
    r.epi = EPI_YBD;
    r.W = step_wd(C, 0, true);
    r.y = C.t;
    r.bytes += 48.0 * (double)(C.n / 2);   // W_c read, x1_c written
  }
  coarse_visit_ops_bsr(h, l + 1, ops, tail_ok, ybd);
  if (p.coarse_scaling) scale_ops(h, l + 1, ops);
  if (gs) {   // prolongate, then backward (SGS: forward then backward) sweeps
    ops->push_back(bsr_op(L.Pb, EPI_YADD, l0 ? C_L0_P : C_COARSE, tagA, C.x, 0, X, nullptr, 0, nullptr, X, 0));
    for (int s = 0; s < p.postsmooth_iter; ++s) {
      if (sgs) sweep(true, X);
      sweep(false, X);
    }
    if (X != xout) {
      Op o;
      o.kind = OP_ILV; o.epi = 1; o.cls = clsW; o.n = nv; o.b = X; o.out = xout; o.os = os;
      o.bytes = 32.0 * nv;
      ops->push_back(o);
    }
    return;
  }
  int s0 = 0;
  if (L.post_mf && npost >= 1) {
    // matrix-free prolongation (level 0 on the dictionary, DESIGN.md section
    // 4.9): y = T e into L.r (r1 is dead once restricted on this path), then
    // u = x1 + y - Wp (A y); every post sweep is the plain pass below
    Op g;
    g.kind = OP_TGATHER; g.cls = C_L0_P; g.n = nv; g.perm = L.mf_agg; g.x = C.x; g.out = L.r;
    g.bytes = 4.0 * nv + 16.0 * nv + 8.0 * C.n;
    ops->push_back(g);
    ops->push_back(bsr_op(cyc_A(L), EPI_PSM, C_L0_P, tagA, L.r, 0, X, nullptr, 0, L.mf_wp, X2, 0));
    std::swap(X, X2);
  } else if (L.KPb.nr > 0 && npost >= 1) {   // z = x1 + W r1 + K e (one operator, K built with this W)
    const bool last = npost == 1;
    ops->push_back(bsr_op(L.KPb, EPI_KPOST, clsS, tagA, C.x, 0, X, L.r, 0, step_wd(L, 0, false),
                          last ? xout : X2, last ? os : 0));
    if (!last) std::swap(X, X2);
    s0 = 1;
  } else if (L.PAb.nr > 0 && npost >= 1) {   // prolongation + first post sweep
    const bool last = npost == 1;
    ops->push_back(post_op(L.PAb, L.r, step_wd(L, 0, false), clsS, tagA, C.x, X, last ? xout : X2,
                           last ? os : 0));
    if (!last) std::swap(X, X2);
    s0 = 1;
  } else {
    ops->push_back(bsr_op(L.Pb, EPI_YADD, l0 ? C_L0_P : C_COARSE, tagA, C.x, 0, X, nullptr, 0,
                          nullptr, X, 0));
  }
  for (int s = s0; s < npost; ++s) {
    const bool last = s == npost - 1;
    double* out = last ? xout : X2;
    ops->push_back(bsr_op(cyc_A(L), EPI_BJAC, clsS, tagA, X, 0, X, b, bs, step_wd(L, s, false), out,
                          last ? os : 0));
    if (!last) std::swap(X, X2);
  }
}

void apply_ops(const DeviceHandle* h, const double* r, double* z, std::vector<Op>* ops) {
  ops->clear();
  const DLevel& L0 = h->L[0];
  if (h->bsr && !L0.coarsest) {
    const int64_t nv = L0.n / 2;
    cycle_ops_bsr(h, 0, r, nv, z, nv, ops);
    for (int it = 1; it < h->p.maxit; ++it) {   // z += MG(r - A z), field-major
      ops->push_back(bsr_op(cyc_A(L0), EPI_RESID, C_MISC, 1, z, nv, nullptr, r, nv, nullptr, L0.c, nv));
      cycle_ops_bsr(h, 0, L0.c, nv, L0.e, nv, ops);
      ops->push_back(axpy_op(L0.n, L0.e, z));
    }
    return;
  }
  cycle_ops_csr(h, 0, r, z, ops);
  for (int it = 1; it < h->p.maxit; ++it) {
    ops->push_back(csr_op(L0.A, EPI_RESID, C_MISC, 1, z, nullptr, r, nullptr, L0.c));
    cycle_ops_csr(h, 0, L0.c, L0.e, ops);
    ops->push_back(axpy_op(L0.n, L0.e, z));
  }
}

// y = A0 x / r = b - A0 x on caller-layout vectors (PCG, spmv)
Op a0_op(const DeviceHandle* h, int epi, const double* x, const double* b, double* out) {
  const DLevel& L0 = h->L[0];
  if (h->bsr && L0.Ab.nr > 0) {
    const int64_t nv = L0.n / 2;
    return bsr_op(L0.Ab, epi, C_MISC, 1, x, nv, nullptr, b, nv, nullptr, out, nv);
  }
  return csr_op(L0.A, epi, C_MISC, 1, x, nullptr, b, nullptr, out);
}

// ---- the launch ladder: an op's run-time fields become template arguments
// through the with_* helpers (device_int.h), so each kernel family's launch
// statement is written once.  The `if constexpr` guards keep the set of
// instantiated kernels to the combinations the planner builds.

template <int TAG>
void launch_csr_tag(const Op& o, hipStream_t s) {
  const DCsr& M = *o.M;
  const int64_t r0 = o.r1 >= 0 ? o.r0 : 0, r1 = o.r1 >= 0 ? o.r1 : M.n;   // row range (multi-GPU), else all rows
  if (r1 <= r0) return;
  with_lanes(M.lanes, [&](auto vl) {
    constexpr int VL = decltype(vl)::value;
    with_epi<EPI_JACOBI, EPI_Y, EPI_YADD, EPI_RESID>(o.epi, [&](auto epi) {
      csr_kernel<VL, decltype(epi)::value, TAG><<<nblocks((r1 - r0) * (int64_t)VL), 256, 0, s>>>(
          r0, r1, M.ptr, M.col, M.val, o.x, o.y, o.b, o.w, o.out);
    });
  });
}

// the block families' epilogues: anything else is the fused block Jacobi
// sweep.  EPI_KPOST exists for !XFM && !SYM only (K is never symmetric and e
// is node-major), and so does the lane-group kernel's EPI_YBD (restrictions
// only: node-interleaved, never symmetric); elsewhere such an op launches
// nothing.  The half and row-dictionary layouts hold A, never the K operator.
template <class F>
void with_block_epi(int epi, F&& f) { with_epi<EPI_BJAC, EPI_Y, EPI_YADD, EPI_RESID, EPI_KPOST>(epi, f); }
constexpr bool plain_only(int epi) { return epi == EPI_YBD || epi == EPI_KPOST; }

// rows [o.r0, o.r1) when o.r1 >= 0 (the distributed K's overlap split: r0 a
// multiple of 256, r1 too or = nr, so each workgroup's rows lie in the range)
template <int TAG, class VT>
void launch_bsr_vl(const Op& o, hipStream_t s) {
  const DBsr& M = *o.Mb;
  const bool rng = o.r1 >= 0;
  const int64_t r0 = rng ? o.r0 : 0, r1 = rng ? o.r1 : M.nr;
  if (r1 <= r0) return;
  with_lanes(M.lanes, [&](auto vl) {
    constexpr int VL = decltype(vl)::value;
    const int64_t b0 = r0 * VL / 256;
    const unsigned g = (unsigned)(nblocks(r1 * (int64_t)VL) - b0);
    with_bools([&](auto xfm, auto sym) {
      constexpr bool XFM = decltype(xfm)::value, SYM = decltype(sym)::value;
      with_epi<EPI_BJAC, EPI_Y, EPI_YBD, EPI_YADD, EPI_RESID, EPI_KPOST>(o.epi, [&](auto epi) {
        constexpr int E = decltype(epi)::value;
        if constexpr (!plain_only(E) || (!XFM && !SYM))
          bsr2_kernel<VL, E, XFM, SYM, TAG, false, VT><<<g, 256, 0, s>>>(
              r1, M.ptr, M.col, reinterpret_cast<const VT*>(M.val), o.x, o.xs, o.y, o.b, o.bs, o.W, o.out, o.os,
              remap_of(o), (!rng && M.rsched && M.rsched_vl == VL && (int64_t)g == M.nrsched) ? M.rsched : nullptr,
              b0);
      });
    }, o.xfm, M.sym);
  });
}

template <bool XFM, bool SYM, int U, bool NT, int TAG, class VT = double>
void launch_sell_u(const Op& o, hipStream_t s) {
  const DBsr& M = *o.Mb;
  const unsigned g = nblocks(M.nr);
  if (g == 0) return;
  with_block_epi(o.epi, [&](auto epi) {
    constexpr int E = decltype(epi)::value;
    if constexpr (!plain_only(E) || (!XFM && !SYM))
      sell2_kernel<E, XFM, SYM, U, NT, TAG, VT><<<g, 256, 0, s>>>(
          M.nr, M.soff, M.meta, M.col, reinterpret_cast<const VT*>(M.val), M.nbs, o.x, o.xs, o.y, o.b, o.bs, o.W,
          o.out, o.os, 0, ((int64_t)g == M.nsched ? M.sched : nullptr), M.lsort ? 1 : 0);
  });
}

// rows [o.r0, o.r1) when o.r1 >= 0: the bounds are multiples of 256 (or
// r1 = nr), so every workgroup of every LPR covers whole 64-row slices of
// the range (dist K_ROWS_ALIGN)
template <int LPR, int U, bool XFM, bool SYM, int SPL, int TAG, int PROBE = 0, class VT = double>
void launch_msell(const Op& o, hipStream_t s) {
  const DBsr& M = *o.Mb;
  const int64_t rows = 256 / LPR;
  const int64_t r0 = o.r1 < 0 ? 0 : o.r0, r1 = o.r1 < 0 ? M.nr : o.r1;
  if (r1 <= r0) return;
  const int64_t b0 = r0 / rows;
  const unsigned g = (unsigned)((r1 + rows - 1) / rows - b0);
  with_block_epi(o.epi, [&](auto epi) {
    constexpr int E = decltype(epi)::value;
    auto go = [&](auto col16) {
      constexpr bool C16 = decltype(col16)::value;
      msell_kernel<LPR, U, E, XFM, SYM, SPL, TAG, C16 ? 0 : PROBE, C16, VT><<<g, 256, 0, s>>>(
          r1, M.soff, M.meta, M.col, reinterpret_cast<const VT*>(M.val), M.nbs, o.x, o.xs, o.y, o.b, o.bs, o.W,
          o.out, o.os, (TAG == 0 && M.kvar == 3) ? 1 : 0, M.lsort ? 1 : 0, b0, M.col16, M.cbase);
    };
    if constexpr (E != EPI_KPOST) go(std::false_type{});
    // level-0 K with 16-bit columns (compress_sell_cols)
    else if constexpr (!XFM && !SYM) with_bools(go, TAG == 0 && PROBE == 0 && M.col16 != nullptr);
  });
}

// the level-0 K kernel (DBsr::kvar, the diagnosis build's MAMG_K_VARIANT for
// A/Bs): 0 two lanes per row, chunks of 5 (default); 1 one lane
// per row, chunks of 6 (sell2_kernel, round 2); 2 four lanes per row, chunks
// of 3; 4 / 5 the default with non-temporal loads of the columns and values /
// the values only (the K stream kept from evicting the gathered e from L2);
// 9 a probe without the e gathers (wrong results, timing only)
template <int SPL, class VT = double>
bool launch_kvariant(const Op& o, hipStream_t s) {
  // fp32 storage: the product kernel only (the A/B variants stay fp64)
  if constexpr (sizeof(VT) == 4) { launch_msell<2, 5, false, false, SPL, 0, 0, VT>(o, s); return true; }
  else switch (o.Mb->kvar) {
    case 4: launch_msell<2, 5, false, false, SPL, 0, 2>(o, s); return true;
    case 5: launch_msell<2, 5, false, false, SPL, 0, 3>(o, s); return true;
    case 1: return SPL == 2 ? (launch_msell<1, 6, false, false, SPL, 0>(o, s), true) : false;
    case 2: launch_msell<4, 3, false, false, SPL, 0>(o, s); return true;
    case 3: launch_msell<2, 5, false, false, SPL, 0>(o, s); return true;   // XCD-contiguous rows
    case 9: launch_msell<2, 5, false, false, SPL, 0, 1>(o, s); return true;
    default: launch_msell<2, 5, false, false, SPL, 0>(o, s); return true;
  }
}

}  // namespace

// whether the level-0 K launch honours an op's row range [r0, r1) (the
// multi-lane SELL and lane-group kernels do; launch_sell_u, reached only with
// the diagnosis build's MAMG_K_VARIANT=1 on a K not split in two streams,
// does not): the distributed apply splits K around the coarse halo only then
// 
bool k_ranges_ok(const DBsr& K) { return !K.sell || !(K.kvar == 1 && K.split != 2); }

namespace {

template <bool XFM, bool SYM, int TAG, class VT = double>
void launch_sell_x(const Op& o, hipStream_t s) {
  // level-0 K operator: two lanes per row (launch_kvariant); multi-lane SELL
  // coarse operators: lanes per row from the mean row length; everything else
  // one lane, chunks of 8
  if constexpr (TAG == 0 && !XFM && !SYM) {
    if (o.epi == EPI_KPOST && (o.Mb->split == 2   ? launch_kvariant<2, VT>(o, s)
                               : o.Mb->split ? launch_kvariant<1, VT>(o, s)
                                             : launch_kvariant<0, VT>(o, s)))
      return;
  }
  if constexpr (!XFM) {
    if (o.Mb->lpr > 1 && !o.Mb->split) {
      with_lpr(o.Mb->lpr, [&](auto lpr) { launch_msell<decltype(lpr)::value, 5, false, SYM, false, TAG, 0, VT>(o, s); });
      return;
    }
  }
  // a split operator streams non-temporally; chunks of post_u for the tagged-0 K side
  const bool nt = o.Mb->split != 0;
  with_bools([&](auto post, auto ntl) {
    launch_sell_u<XFM, SYM, decltype(post)::value ? post_u : sell_u, decltype(ntl)::value, TAG, VT>(o, s);
  }, TAG == 0 && (nt || o.epi == EPI_KPOST), nt);
}

template <int VL, int TAG>
void launch_post_vl(const Op& o, hipStream_t s) {
  const DBsr& M = *o.Mb;
  const unsigned g = nblocks(M.nr * (int64_t)VL);
  if (g == 0) return;
  bsr2_post_kernel<VL, false, TAG><<<g, 256, 0, s>>>(M.nr, M.ptr, M.col, M.val, o.x, o.y, o.b, o.W,
                                                       o.out, o.os, remap_of(o));
}

template <int TAG>
void launch_post_tag(const Op& o, hipStream_t s) {
  if (o.Mb->sell) {
    const DBsr& M = *o.Mb;
    if (M.nr)
      sell2_post_kernel<TAG><<<nblocks(M.nr), 256, 0, s>>>(M.nr, M.soff, M.meta, M.perm, M.col, M.val,
                                                           o.x, o.y, o.b, o.W, o.out, o.os);
    return;
  }
  with_lanes(o.Mb->lanes, [&](auto vl) { launch_post_vl<decltype(vl)::value, TAG>(o, s); });
}

// half-symmetric A, four entries in flight per lane
template <int TAG, class VT = double>
void launch_half(const Op& o, hipStream_t s) {
  const DBsr& M = *o.Mb;
  const int64_t r0 = o.r1 < 0 ? 0 : o.r0, r1 = o.r1 < 0 ? M.nr : o.r1;
  const unsigned g = nblocks(r1 - r0);
  if (r1 <= r0) return;
  // gh: a rank-local A's ghost part (fp32 storage: gval narrowed with val)
  with_bools([&](auto xfm, auto gh) {
    with_block_epi(o.epi, [&](auto epi) {
      constexpr int E = decltype(epi)::value;
      if constexpr (E != EPI_KPOST)
        hsell2_kernel<E, decltype(xfm)::value, 4, decltype(gh)::value, TAG, VT><<<g, 256, 0, s>>>(
            r0, r1, M.meta, M.col, reinterpret_cast<const VT*>(M.val), M.nbs, M.hwu, M.lptr, M.hwl, M.gsoff, M.gcol,
            reinterpret_cast<const VT*>(M.gval), M.ngs, o.x, o.xs, o.y, o.b, o.bs, o.W, o.out, o.os, 1,
            (r0 == 0 && r1 == M.nr && (int64_t)g == M.nsched)            ? M.sched
            : (r0 == M.sr0 && r1 == M.sr1 && (int64_t)g == M.nsched_r) ? M.sched_r
                                                                       : nullptr);
    });
  }, o.xfm, M.ngs > 0);
}

// row-pattern dictionary (rowdict2_kernel); the band schedule as for the half
// layout.  Entries in flight per lane on the wave-uniform path: build switch
// for A/Bs
#ifndef MAMG_ROWDICT_U
#define MAMG_ROWDICT_U 8
#endif
constexpr int ROWDICT_U = MAMG_ROWDICT_U;

template <int TAG, class VT = double>
void launch_rowdict(const Op& o, hipStream_t s) {
  const DBsr& M = *o.Mb;
  const int64_t r0 = o.r1 < 0 ? 0 : o.r0, r1 = o.r1 < 0 ? M.nr : o.r1;
  const unsigned g = nblocks(r1 - r0);
  if (r1 <= r0) return;
  with_bools([&](auto xfm, auto sym) {
    constexpr bool SYM = decltype(sym)::value;
    const size_t lds = MAMG_ROWDICT_LDS ? (size_t)M.nbs * (4 + (SYM ? 3 : 4) * sizeof(VT)) : 0;
    // the dictionary holds A, never K: EPI_PSM (node-interleaved vectors only) in EPI_KPOST's place
    with_epi<EPI_BJAC, EPI_Y, EPI_YADD, EPI_RESID, EPI_PSM>(o.epi, [&](auto epi) {
      constexpr int E = decltype(epi)::value;
      if constexpr (E != EPI_PSM || !decltype(xfm)::value)
        rowdict2_kernel<E, decltype(xfm)::value, SYM, ROWDICT_U, TAG, VT><<<g, 256, lds, s>>>(
            r0, r1, M.rcode, M.rlen, M.rdelta, reinterpret_cast<const VT*>(M.val), M.nbs, M.rw, o.x, o.xs, o.y, o.b,
            o.bs, o.W, o.out, o.os, 1, (r0 == 0 && r1 == M.nr && (int64_t)g == M.nsched) ? M.sched : nullptr);
    });
  }, o.xfm, M.sym);
}

// DBsr::f32: the operator's values are stored fp32 (dev_set_cycle_storage)
template <int TAG>
void launch_bsr_tag(const Op& o, hipStream_t s) {
  with_value_type(o.Mb->f32, [&](auto vt) {
    using VT = typename decltype(vt)::type;
    if (o.Mb->rowdict) launch_rowdict<TAG, VT>(o, s);
    else if (o.Mb->half) launch_half<TAG, VT>(o, s);
    else if (o.Mb->sell)
      with_bools([&](auto xfm, auto sym) { launch_sell_x<decltype(xfm)::value, decltype(sym)::value, TAG, VT>(o, s); },
                 o.xfm, o.Mb->sym);
    else launch_bsr_vl<TAG, VT>(o, s);
  });
}

void launch_gs(const Op& o, hipStream_t s) {
  const DBsr& M = *o.Mb;
  with_lanes(M.lanes, [&](auto vl) {
    constexpr int VL = decltype(vl)::value;
    with_bools([&](auto sym) {
      gs2_kernel<VL, decltype(sym)::value><<<nblocks(o.n * (int64_t)VL), 256, 0, s>>>(
          o.r0, o.r1, o.perm, M.ptr, M.col, M.val, M.nb, o.W, o.out, o.b, o.bs);
    }, M.sym);
  });
}

void launch_cgs(const Op& o, hipStream_t s) {
  const DCsr& M = *o.M;
  with_lanes(M.lanes, [&](auto vl) {
    constexpr int VL = decltype(vl)::value;
    if (o.kind == OP_CGS) {
      csr_gs_kernel<VL><<<nblocks(o.n * (int64_t)VL), 256, 0, s>>>(o.r0, o.r1, o.perm, M.ptr, M.col, M.val, o.w,
                                                                  o.out, o.b);
      return;
    }
    const DLevel& L = *o.lev;
    auto dir = [](int v) { return v == 1 ? 1 : v == 2 ? -1 : 0; };
    csr_gs_small_kernel<VL><<<1, CSR_GS_SMALL_THREADS, (size_t)M.n * sizeof(double), s>>>(
        M.n, (int)L.gcs.size() - 1, L.gcs_d, o.perm, M.ptr, M.col, M.val, o.w, o.out, o.b, o.epi & 1, (int)o.n,
        dir((o.epi >> 1) & 3), dir((o.epi >> 3) & 3));
  });
}

// nonlinear AMLI: the inner flexible CG's work space of level l (DLevel::kr
// ..), on the levels that can be a Krylov level: 1 .. coarsest - 1
int kcycle_alloc(DeviceHandle* h, int l, std::string* err) {
  DLevel& D = h->L[l];
  if (!kcycle(h->p) || l == 0 || D.coarsest) return MAMG_OK;
  int rc;
  const int m = h->p.amli_degree;
  for (double** v : {&D.kr, &D.kz, &D.kw})
    if ((rc = dalloc(h, v, D.n, err))) return rc;
  for (int i = 0; i < m; ++i)
    if ((rc = dalloc(h, &D.kp[i], D.n, err)) || (rc = dalloc(h, &D.kq[i], D.n, err))) return rc;
  return dalloc(h, &D.kpart, KP_SIZE, err);
}

// one op of a nonlinear AMLI step (kstep_ops): step r0 of r1 on level o.lev
void launch_kstep(const Op& o, hipStream_t s) {
  const DLevel& C = *o.lev;
  const int j = (int)o.r0;
  const bool first = j == 0, last = j == (int)o.r1 - 1;
  const int nb = (int)std::min<int64_t>(SCALE_BLOCKS, nblocks(o.n));
  KDirs D = {};
  for (int i = 0; i < j; ++i) { D.p[i] = C.kp[i]; D.q[i] = C.kq[i]; }
  const double* r = first ? C.b : C.kr;
  if (o.kind == OP_KDOT) {
    switch (j) {
      case 1: kdot_kernel<1><<<nb, 256, 0, s>>>(o.n, C.kz, D, o.part); break;
      case 2: kdot_kernel<2><<<nb, 256, 0, s>>>(o.n, C.kz, D, o.part); break;
      default: kdot_kernel<3><<<nb, 256, 0, s>>>(o.n, C.kz, D, o.part); break;
    }
  } else if (o.kind == OP_KORTH) {
    switch (j) {
      case 0: korth_kernel<0><<<nb, 256, 0, s>>>(o.n, nb, C.kz, C.kw, D, C.kp[0], C.kq[0], r, o.part); break;
      case 1: korth_kernel<1><<<nb, 256, 0, s>>>(o.n, nb, C.kz, C.kw, D, C.kp[1], C.kq[1], r, o.part); break;
      case 2: korth_kernel<2><<<nb, 256, 0, s>>>(o.n, nb, C.kz, C.kw, D, C.kp[2], C.kq[2], r, o.part); break;
      default: korth_kernel<3><<<nb, 256, 0, s>>>(o.n, nb, C.kz, C.kw, D, C.kp[3], C.kq[3], r, o.part); break;
    }
  } else {
    with_bools([&](auto f, auto l) {
      kupd_kernel<decltype(f)::value, decltype(l)::value><<<nb, 256, 0, s>>>(o.n, nb, j, o.part, C.kp[j], C.kq[j],
                                                                            C.x, r, C.kr);
    }, first, last);
  }
}

}  // namespace

void launch(const Op& o, hipStream_t s) {
  switch (o.kind) {
    case OP_CGS:
    case OP_CGSF:
      if (o.n > 0) launch_cgs(o, s);
      break;
    case OP_CSR:
      if (o.tag == 0) launch_csr_tag<0>(o, s); else launch_csr_tag<1>(o, s);
      break;
    case OP_BSR:
      if (o.tag == 0) launch_bsr_tag<0>(o, s); else launch_bsr_tag<1>(o, s);
      break;
    case OP_POST:
      if (o.tag == 0) launch_post_tag<0>(o, s); else launch_post_tag<1>(o, s);
      break;
    case OP_BD:
      if (o.n) bd2_kernel<false><<<nblocks(o.n), 256, 0, s>>>(o.n, o.W, o.b, o.bs, nullptr, o.out, 0);
      break;
    case OP_TGATHER:
      if (o.n) tgather_kernel<<<nblocks(o.n), 256, 0, s>>>(o.n, o.perm, o.x, o.out);
      break;
    case OP_SCALE:
      if (o.n) scale_kernel<<<nblocks(o.n), 256, 0, s>>>(o.n, o.w, o.x, o.out);
      break;
    case OP_AXPY:
      if (o.n) axpy_kernel<<<nblocks(o.n), 256, 0, s>>>(o.n, o.x, o.out);
      break;
    case OP_GEMV:
      if (o.n) gemv_kernel<<<(unsigned)((o.n + 3) / 4), 256, 0, s>>>(o.n, o.w, o.x, o.out);
      break;
    case OP_ILV:
      if (o.n && o.epi == 1) deinterleave2_kernel<<<nblocks(o.n), 256, 0, s>>>(o.n, o.b, o.out, o.os);
      else if (o.n) interleave2_kernel<<<nblocks(o.n), 256, 0, s>>>(o.n, o.b, o.bs, o.out);
      break;
    case OP_GS:
      if (o.n > 0) launch_gs(o, s);
      break;
    case OP_PATCH:
      if (o.n > 0)
        patch_kernel<<<(unsigned)((o.n + 3) / 4), 256, 0, s>>>(o.r0, o.r1, o.lev->pperm, o.lev->Sptr, o.lev->Scol,
                                                                o.lev->Sval, o.lev->pu, o.lev->pus, o.out, o.b, o.bs);
      break;
    case OP_CRING:
      if (o.n > 0)
        ring_csr_kernel<<<(unsigned)o.n, RING_CSR_THREADS, 0, s>>>(o.r0, o.lev->rmo, o.lev->rmem, o.lev->rio,
                                                                  o.lev->rinv, o.M->ptr, o.M->col, o.M->val, o.out,
                                                                  o.b);
      break;
    case OP_RING:
      if (o.n > 0)
        ring_kernel<<<(unsigned)o.n, RING_THREADS, 0, s>>>(o.r0, o.lev->rmo, o.lev->rmem, o.lev->rio, o.lev->rinv,
                                                          o.lev->Sptr, o.lev->Scol, o.lev->Sval, o.out, o.b, o.bs);
      break;
    case OP_ZERO:
      if (o.n) (void)dev_memset(o.out, 0, o.n * sizeof(double), s);
      break;
    case OP_COPY:
      if (o.n) (void)dev_copy(o.out, o.x, o.n * sizeof(double), s);
      break;
    case OP_DOT2:
      if (o.n) dot2_partial_kernel<<<SCALE_BLOCKS, 256, 0, s>>>(o.n, o.b, o.x, o.y, o.part);
      break;
    case OP_KDOT:
    case OP_KORTH:
    case OP_KUPD:
      if (o.n) launch_kstep(o, s);
      break;
    case OP_TAIL:   // r1: bit 0 = every gathered x in LDS, bit 1 = register-resident rows, bit 2 = K ops
      if (o.n) tail_launch<false>((int)o.r1, o.prog, (int)o.n, o.tail_pl, (size_t)o.r0, nullptr, s);
      break;
    case OP_CSCALE:
      if (o.n) cscale_kernel<<<(unsigned)std::min<int64_t>(SCALE_BLOCKS, nblocks(o.n)), 256, 0, s>>>(o.n, SCALE_BLOCKS, o.part, o.out);
      break;
    // distributed PCG: launched even for an empty slice (the partials and
    // the rank's slot must be written on every rank)
    case OP_PDOT:
      dpcg_dot_kernel<<<DOT_BLOCKS, 256, 0, s>>>(o.pcg->n, o.x, o.y, o.pcg->part);
      break;
    case OP_PSLOT:
      dpcg_slot_kernel<<<1, 256, 0, s>>>(DOT_BLOCKS, (int)o.n, o.pcg->part, o.pcg->pv, o.pcg->P, o.pcg->rank);
      break;
    case OP_PR0:
      dpcg_r0_kernel<<<DOT_BLOCKS, 256, 0, s>>>(o.pcg->n, o.pcg->stop, o.pcg->b, o.pcg->q, o.pcg->r, o.pcg->part,
                                                DOT_BLOCKS);
      break;
    case OP_PINIT:
      dpcg_init_kernel<<<1, 64, 0, s>>>(o.pcg->pv, o.pcg->P, o.pcg->st, o.pcg->tol, o.pcg->relconv, o.pcg->maxiter,
                                        o.pcg->stop, o.pcg->res, o.pcg->rn);
      break;
    case OP_PALPHA:
      dpcg_alpha_kernel<<<1, 64, 0, s>>>(o.pcg->pv, o.pcg->P, o.pcg->st);
      break;
    case OP_PXR:
      if (o.pcg->stop)
        dpcg_xr_kernel<true><<<DOT_BLOCKS, 256, 0, s>>>(o.pcg->n, o.pcg->st, o.pcg->d, o.pcg->q, o.pcg->x, o.pcg->r,
                                                        o.pcg->part, DOT_BLOCKS);
      else
        dpcg_xr_kernel<false><<<DOT_BLOCKS, 256, 0, s>>>(o.pcg->n, o.pcg->st, o.pcg->d, o.pcg->q, o.pcg->x, o.pcg->r,
                                                         o.pcg->part, DOT_BLOCKS);
      break;
    case OP_PBETA:
      dpcg_beta_kernel<<<1, 64, 0, s>>>(o.pcg->pv, o.pcg->P, o.pcg->st, o.pcg->res, o.pcg->rn, o.pcg->al, o.pcg->be);
      break;
    case OP_PD:
      if (o.pcg->n) dpcg_d_kernel<<<nblocks(o.pcg->n), 256, 0, s>>>(o.pcg->n, o.pcg->st, o.pcg->z, o.pcg->d, o.pcg->x);
      break;
  }
}

int TimedRun::run(size_t nops, const std::function<int(size_t)>& cls, const std::function<int(size_t)>& op, int reps,
                  int mode, hipStream_t s, const std::function<int()>& queued, double* ms, double* kernel_ms,
                  std::string* err) {
  int rc;
  inst.clear();
  for (size_t k = 0; k < nops; ++k)
    if (mode == 1 || cls(k) == C_L0_RESID || cls(k) == C_L0_SMOOTH) inst.push_back((int)k);
  if ((rc = create(2 * inst.size() * (size_t)reps + 2, err))) return rc;
  HIPCHK(hipEventRecord(ev[0], s));
  size_t q = 2;
  for (int rp = 0; rp < reps; ++rp) {
    size_t ii = 0;
    for (size_t k = 0; k < nops; ++k) {
      const bool timed = ii < inst.size() && inst[ii] == (int)k;
      if (timed) HIPCHK(hipEventRecord(ev[q], s));
      if ((rc = op(k))) return rc;
      if (timed) { HIPCHK(hipEventRecord(ev[q + 1], s)); q += 2; ++ii; }
    }
  }
  HIPCHK(hipEventRecord(ev[1], s));
  if (queued && (rc = queued())) return rc;
  HIPCHK(hipEventSynchronize(ev[1]));
  HIPCHK(hipGetLastError());
  float tot = 0.f;
  HIPCHK(hipEventElapsedTime(&tot, ev[0], ev[1]));
  *ms = tot / reps;
  if (kernel_ms) {
    for (int c = 0; c < 16; ++c) kernel_ms[c] = 0.0;
    for (int rp = 0; rp < reps; ++rp)
      for (size_t ii = 0; ii < inst.size(); ++ii) {
        float t = 0.f;
        if ((rc = op_ms(rp, ii, &t, err))) return rc;
        kernel_ms[cls((size_t)inst[ii])] += t / reps;
      }
  }
  return MAMG_OK;
}

int IterGraph::alloc(size_t hist_doubles, std::string* err) {
  if (raw_malloc((void**)&hist, hist_doubles * sizeof(double), "long") != hipSuccess) {
    (void)hipGetLastError();
    hist = nullptr;
    *err = "PCG history allocation failed";
    return MAMG_ERR_HIP;
  }
  for (hipEvent_t& e : ev) {
    const hipError_t rc = hipEventCreateWithFlags(&e, hipEventDisableTiming);
    if (rc == hipSuccess) continue;
    e = nullptr;
    release();
    *err = std::string("PCG events: ") + hipGetErrorString(rc);
    return MAMG_ERR_HIP;
  }
  return MAMG_OK;
}

int pcg_finish(int status, int it, const PcgHist& d, double* residuals, double* rnorms, double* alphas,
               double* betas, int* niters, std::string* err) {
  if (status == PCG_NOT_POS) {
    *niters = 0;
    residuals[0] = 0.0;
    *err = "Matrix is not positive";
    return MAMG_ERR_BREAKDOWN;
  }
  HIPCHK(hipMemcpy(residuals, d.res, (it + 1) * sizeof(double), hipMemcpyDeviceToHost));
  if (d.rn && rnorms) HIPCHK(hipMemcpy(rnorms, d.rn, (it + 1) * sizeof(double), hipMemcpyDeviceToHost));
  if (it > 0) {
    HIPCHK(hipMemcpy(alphas, d.al, it * sizeof(double), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(betas, d.be, it * sizeof(double), hipMemcpyDeviceToHost));
  }
  *niters = it;
  if (status == PCG_DQ_ZERO) {   // the host loop's breakdown flag (krylov.py): same status here
    *err = "ConjGrad stopped: <d,Ad> = 0";
    return MAMG_ERR_BREAKDOWN;
  }
  if (status == PCG_RZ_NEG) {
    *err = "ConjGrad breakdown (<r,Br> < 0)";
    return MAMG_ERR_BREAKDOWN;
  }
  return MAMG_OK;
}

namespace {

// the apply's graph for (r, z), from the handle's cache or captured now
int get_graph(DeviceHandle* h, const double* r, double* z, hipGraphExec_t* exec, std::string* err) {
  return h->graphs.get(r, z, h->last, [&](CapturedGraph* g) {
    std::vector<Op> ops;
    apply_ops(h, r, z, &ops);
    return capture_graph(&h->cap, [&]() { for (const Op& o : ops) launch(o, h->cap); return (int)MAMG_OK; }, "apply",
                         g, err);
  }, exec, err);
}

// BSR2 layout usable: 2 fields, every level's smoother node-block diagonal
bool bsr_eligible(const Hierarchy& H, const CsrView& A0, const mamg_params& p) {
  if (p.num_functions != 2) return false;
  for (size_t l = 0; l < H.levels.size(); ++l) {
    const HostLevel& hl = H.levels[l];
    if (hl.n % 2) return false;
    if (hl.coarsest) continue;
    if (hl.WB.n == 0) return false;                     // point smoother: CSR path
    std::vector<double> blk;
    if (!node_blocks_of(hl.WB.view(), hl.n / 2, &blk)) return false;
  }
  (void)A0;
  return true;
}

}  // namespace

// ---------------------------------------------------------------------------
// Re-home the level-0 streams -- K values and columns (6.4 GB at nrefs=6),
// A_0's upper values and columns (4.3 GB), R_0's values (2.3 GB) -- and the
// coarser levels' operators into fresh allocations once the setup's
// temporaries are gone.  The kernels' DRAM rate depends on where these arrays
// land, for the same bytes and the same PMC traffic: as built in the
// pre-reserved arena K ran 1.59-1.71 ms; re-homed into plain allocations
// 1.48-1.68 ms (residual 1.06-1.09 vs 1.09-1.10 ms, restriction 0.51 vs
// 0.53 ms) (profiles/r02_rehome_level0.txt).  Same data:
// results are bitwise equal.
// A fresh allocation for a re-homed stream (plain hipMalloc).  Rounds 2-4
// took these from hipExtMallocWithFlags(hipDeviceMallocContiguous); with the
// setup temporaries in the library's own block cache (dmem.h), a setup made
// after a handle with contiguous re-homed arrays faulted in its first
// kernels on every run, so contiguous allocations are
// no longer made.  The K region search (select_k_region) keeps its value:
// distinct plain allocations still differ by a few percent.
void* placement_alloc(size_t b) {
  void* r = nullptr;
  if (dev_malloc(&r, b, "place") != hipSuccess) { (void)hipGetLastError(); r = nullptr; }
  return r;
}

void rehome_array(DeviceHandle* h, void** ptr, size_t b) {
  if (!*ptr || b == 0) return;
  void* r = placement_alloc(b);
  if (!r) return;
  if (dev_copy(r, *ptr, b) != hipSuccess) {
    (void)hipGetLastError();
    (void)raw_free(r);
    return;
  }
  void* old = *ptr;
  h->allocs.push_back(r);
  *ptr = r;
  const bool in_arena = (char*)old >= h->arena0 && (char*)old < h->arena1;
  auto it = std::find(h->allocs.begin(), h->allocs.end(), old);
  if (!in_arena && it != h->allocs.end()) {
    drained_free(old);
    h->allocs.erase(it);
  }
}

// values and columns of one operator (half-symmetric: the upper part)
void rehome_bsr(DeviceHandle* h, DBsr& M) {
  if (M.nr == 0) return;
  if (M.rowdict) return;   // a few KB of table: nothing to place
  const int64_t slots = (M.sell || M.half) ? M.nbs : M.nb;
  rehome_array(h, (void**)&M.val, (size_t)slots * ((M.sym || M.half) ? 3 : 4) * sizeof(double));
  rehome_array(h, (void**)&M.col, (size_t)slots * sizeof(int32_t));
}

// Level-0 K values placed by measurement.  The K
// kernel's time follows the physical memory region its value stream (5.7 GB at
// nrefs=6) lands in: 1.37 vs 1.55 ms for the same bytes, layout and kernel,
// with identical fabric request counts and no TLB misses (bench/kplace.py,
// profiles/r03_k_placement.txt); slice order, split layouts and XCD row order
// do not remove it.  So the values are copied into up to MAMG_KREGION_TRIES
// (4) distinct fresh allocations, K is timed in each (one warm + three launches), and the fastest
// region is kept.  Same bytes: results are bitwise equal.
// Bounded (round 4): candidates are tried one at a time while the search has
// spent less than MAMG_KREGION_BUDGET_MS (200) and a quarter of the HBM stays
// free after the next copy (a co-resident caller keeps its memory); the
// losers are freed at the end (kept until then so that every candidate is a
// distinct region).
void select_k_region(DeviceHandle* h) {
  DLevel& L = h->L[0];
  DBsr& K = L.KPb;
  const size_t bytes = (size_t)K.nbs * 4 * sizeof(double);
  const int tries = h->sw.kregion_tries;
  const double budget = h->sw.kregion_budget_ms;
  if (tries <= 1 || K.sym || !L.r || !L.t || !L.Wd || !h->L[1].x) {
    rehome_array(h, (void**)&K.val, bytes);
    return;
  }
  double* out = nullptr;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  if (raw_malloc((void**)&out, L.n * sizeof(double), "tmp") != hipSuccess || hipEventCreate(&e0) != hipSuccess ||
      hipEventCreate(&e1) != hipSuccess) {
    (void)hipGetLastError();
    if (out) (void)raw_free(out);
    rehome_array(h, (void**)&K.val, bytes);
    return;
  }
  const auto t0 = std::chrono::steady_clock::now();
  void* old = K.val;
  const Op op = bsr_op(K, EPI_KPOST, C_L0_SMOOTH, 0, h->L[1].x, 0, L.t, L.r, 0, L.Wd, out, L.n / 2);
  std::vector<void*> bufs;
  std::vector<float> ms;
  size_t best = 0;
  for (int t = 0; t < tries; ++t) {
    const double spent = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (t > 0 && spent > budget) break;
    size_t fr = 0, tot = 0;
    if (hipMemGetInfo(&fr, &tot) != hipSuccess) { (void)hipGetLastError(); break; }
    if (fr < bytes + tot / 4) break;
    void* r = placement_alloc(bytes);
    if (!r) break;
    bufs.push_back(r);
    (void)dev_copy(r, old, bytes);
    K.val = (double*)r;
    launch(op, nullptr);
    (void)hipEventRecord(e0, nullptr);
    for (int k = 0; k < 3; ++k) launch(op, nullptr);
    (void)hipEventRecord(e1, nullptr);
    (void)hipEventSynchronize(e1);
    float m = 1e30f;
    (void)hipEventElapsedTime(&m, e0, e1);
    ms.push_back(m);
    if (ms.back() < ms[best]) best = bufs.size() - 1;
  }
  if (bufs.empty()) {
    K.val = (double*)old;
    (void)raw_free(out);
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    (void)hipGetLastError();
    return;
  }
  K.val = (double*)bufs[best];
  h->allocs.push_back(bufs[best]);
  for (size_t i = 0; i < bufs.size(); ++i)
    if (i != best) drained_free(bufs[i]);
  const bool in_arena = (char*)old >= h->arena0 && (char*)old < h->arena1;
  auto it = std::find(h->allocs.begin(), h->allocs.end(), old);
  if (!in_arena && it != h->allocs.end()) {
    drained_free(old);
    h->allocs.erase(it);
  }
  drained_free(out);
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  (void)hipGetLastError();
  if (h->p.print_level >= 2) {
    std::fprintf(stderr, "[mamg] K value regions (ms per K launch):");
    for (float m : ms) std::fprintf(stderr, " %.4f", m / 3);
    std::fprintf(stderr, " -> %zu\n", best);
  }
  h->kregion_ms.assign(ms.begin(), ms.end());
  for (auto& m : h->kregion_ms) m /= 3.0;
  h->kregion_best = (int)best;
}

void rehome_operators(DeviceHandle* h) {
  if (!h->sw.rehome) return;   // the operators stay where the layout builder put them (tests)
  if (!h->bsr || h->L.size() < 2) return;
  DLevel& L = h->L[0];
  // a matrix-free level 0 has no K to place; the rest is re-homed as with one
  const bool mf = L.post_mf && L.Ab.nr >= h->sw.sell_min_rows;
  if (!mf && (L.KPb.nr < h->sw.sell_min_rows || !L.KPb.sell)) return;
  auto lap = [t = std::chrono::steady_clock::now()]() mutable {
    const auto n = std::chrono::steady_clock::now();
    const double ms = std::chrono::duration<double, std::milli>(n - t).count();
    t = n;
    return ms;
  };
  if (!mf) {
    select_k_region(h);            // the largest stream first, placed by measurement
    h->layout_ms[LT_KREGION] = lap();
    if (L.KPb.col16) rehome_array(h, (void**)&L.KPb.col16, (size_t)L.KPb.nbs * sizeof(uint16_t));
    else rehome_array(h, (void**)&L.KPb.col, (size_t)L.KPb.nbs * sizeof(int32_t));
  }
  if (L.Ab.half) rehome_bsr(h, L.Ab);
  if (!L.Rb.sell && !L.Rb.sym)
    rehome_array(h, (void**)&L.Rb.val, (size_t)L.Rb.nb * 4 * sizeof(double));
  // the coarser levels' operators too (coarse levels 0.41 -> 0.395 ms per apply)
  for (size_t l = 1; l < h->L.size(); ++l) {
    DLevel& D = h->L[l];
    if (D.coarsest) break;
    for (DBsr* M : {&D.Ab, &D.KPb, &D.Rb, &D.Pb})
      if (!M->half) rehome_bsr(h, *M);
  }
  h->layout_ms[LT_REHOME] = lap();
}

// Block layout of a SELL-stored K's values: one 32-byte block per slot, or two
// 16-byte streams per slot (SPL: each wave load reads contiguous pairs).  The
// arithmetic is the same, so results are bitwise equal either way
// (test_k_block_layouts_bitwise).  Rearranged in place through a temporary.
void set_k_split(DBsr& K, int mode) {
  if (!K.sell || K.sym || K.split == mode || K.nbs == 0 || (K.nbs & 63)) return;
  void* t = nullptr;
  if (raw_malloc((void**)&t, (size_t)K.nbs * sizeof(dv4), "tmp") != hipSuccess) { (void)hipGetLastError(); return; }
  const size_t bytes = (size_t)K.nbs * sizeof(dv4);
  if (K.split) {   // back to one block per slot first
    if (K.split == 2) unsplit_local_kernel<<<nblocks(K.nbs), 256>>>(K.nbs, K.val, (dv4*)t);
    else unsplit_blocks_kernel<<<nblocks(K.nbs), 256>>>(K.nbs, reinterpret_cast<const dv2*>(K.val), (dv4*)t);
    (void)dev_copy(K.val, t, bytes);
    K.split = 0;
  }
  if (mode == 1) split_blocks_kernel<<<nblocks(K.nbs), 256>>>(K.nbs, reinterpret_cast<const dv4*>(K.val), (dv2*)t);
  if (mode == 2) split_local_kernel<<<nblocks(K.nbs), 256>>>(K.nbs, reinterpret_cast<const dv4*>(K.val), (double*)t);
  if (mode) (void)dev_copy(K.val, t, bytes);
  drained_free(t);
  K.split = mode;
}

// Round 2 chose the layout per box by timing both at upload (split 1.57 vs
// 1.71 ms on one box, the opposite on another).  With the two-lanes-per-row
// K kernel (msell_kernel) the one-block layout is kept everywhere
// (DESIGN.md section 4); MAMG_POST_K=2 forces the split layout on every
// SELL-stored K (tests), MAMG_K_LAYOUT=split|block switches level 0 at
// mamg_time_apply (A/Bs on one upload).
// the coarse tail (tail_kernel) takes over from the first level with at most
// MAMG_TAIL_NODES node rows (0 = off).  Default: off for the Jacobi-family
// smoothers and 1024 for the multicolour GS smoothers; a coarsest level alone
// stays a launch.  Measured at nrefs=6 in the bench's timed loop (DESIGN.md
// section 4.2, profiles/r03_ab_tail.txt): the Jacobi V-cycle 276.1-276.3 vs
// 277.5-277.7 applies/s without it (2-D nrefs=6: 4601 vs 4971), because one
// tail op costs ~2 us, more than the kernel boundary it replaces; the
// reference family's W-cycle, whose colour steps are the launches, 196.7 ->
// 182.5 ms per apply with it (PCG graph replay).
void set_tail_level(DeviceHandle* h) {
  h->tail_level = 0;
  const int64_t nodes = h->sw.tail_nodes.set ? h->sw.tail_nodes.v : (gs_smoother(h->p) ? 1024 : 0);
  if (!h->bsr || nodes <= 0) return;
  for (int l = 1; l < (int)h->L.size(); ++l) {
    if (h->L[l].coarsest) return;
    if (h->L[l].n / 2 <= nodes) { h->tail_level = l; return; }
  }
}

void apply_k_layout_knob(DeviceHandle* h) {
  if (!h->bsr || h->L.size() < 2 || h->sw.post_k != 2) return;
  for (DLevel& D : h->L)
    if (!D.coarsest) set_k_split(D.KPb, 1);
}

// MAMG_DEBUG_SUMS=1 (diagnosis): a 64-bit FNV-1a hash of every operator
// array of the handle, per level, printed to stderr at the end of the upload
// and before each apply, so two handles of one problem (which must hold the
// same bytes wherever they live) name the array that differs
void debug_sums(DeviceHandle* h, const char* stage, bool konly) {
#if MAMG_DIAG
  static const bool on = [] {
    const char* e = std::getenv("MAMG_DEBUG_SUMS");
    return e && std::atoi(e) != 0;
  }();
#else
  constexpr bool on = false;   // diagnosis build only
#endif
  if (!on) return;
  // no device-wide sync: the copies below are ordered on the null stream,
  // as every layout-builder step is
  auto hash = [](const void* p, size_t b) -> unsigned long long {
    if (!p || !b) return 0ull;
    std::vector<unsigned char> v(b);
    if (hipMemcpy(v.data(), p, b, hipMemcpyDeviceToHost) != hipSuccess) { (void)hipGetLastError(); return 1ull; }
    unsigned long long x = 1469598103934665603ull;
    for (unsigned char c : v) x = (x ^ c) * 1099511628211ull;
    return x;
  };
  std::string line;
  char buf[160];
  if (konly) {   // level 0's K values and where they live (build-time trace)
    const DBsr& K = h->L[0].KPb;
    const int64_t slots = (K.sell || K.half) ? K.nbs : K.nb;
    const int per = (K.sym || K.half) ? 3 : 4;
    const bool ar = (char*)K.val >= h->arena0 && (char*)K.val < h->arena1;
    std::fprintf(stderr, "[mamg sums] %s L0.K val %016llx at %p (%s, %lld B)\n", stage,
                 hash(K.val, (size_t)slots * per * 8), (void*)K.val, ar ? "arena" : "own", (long long)(slots * per * 8));
    return;
  }
  for (size_t l = 0; l < h->L.size(); ++l) {
    const DLevel& L = h->L[l];
    const std::pair<const char*, const DBsr*> ms[] = {{"A", &L.Ab}, {"K", &L.KPb}, {"PA", &L.PAb}, {"P", &L.Pb},
                                                      {"R", &L.Rb}, {"G", &L.Gb}};
    for (const auto& m : ms) {
      const DBsr& M = *m.second;
      if (!M.nr) continue;
      const int per = (M.sym || M.half) ? 3 : 4;
      const int64_t slots = (M.sell || M.half || M.rowdict) ? M.nbs : M.nb;
      std::snprintf(buf, sizeof buf, " L%zu.%s val %016llx col %016llx", l, m.first,
                    hash(M.val, (size_t)slots * per * (M.f32 ? 4 : 8)),
                    M.rowdict ? hash(M.rdelta, (size_t)slots * 4) : hash(M.col, (size_t)slots * 4));
      line += buf;
    }
    if (L.Wd) {
      std::snprintf(buf, sizeof buf, " L%zu.W %016llx", l, hash(L.Wd, (size_t)(L.n / 2) * 32));
      line += buf;
    }
    if (L.Ainv) {
      std::snprintf(buf, sizeof buf, " L%zu.Ainv %016llx", l, hash(L.Ainv, (size_t)L.n * L.n * 8));
      line += buf;
    }
  }
  std::fprintf(stderr, "[mamg sums] %s%s\n", stage, line.c_str());
}

std::string layout_error(const mamg_params& p) {
  if (patch_schwarz(p))
    return "SCHWARZ_PATCHES needs the BSR2 layout (num_functions 2, node-block smoothers on every level)";
  if (rings_schwarz(p))
    return "SCHWARZ_RINGS with node-block smoothers needs the BSR2 layout (node-block smoothers on every level; "
           "with node_block_smoother 0 it runs on the CSR layout)";
  return "multicolour GS/SGS smoothers need the BSR2 layout (num_functions 2, node-aligned smoother blocks)";
}

int dev_upload(const Hierarchy& H, const CsrView& A0, const mamg_params& p, const Switches& sw,
               DeviceHandle** out, std::string* err) {
  const auto t0 = std::chrono::steady_clock::now();
  std::unique_ptr<DeviceHandle> h(new DeviceHandle(sw));
  h->p = p;
  h->device = p.device;
  int ndev = 0;
  HIPCHK(hipGetDeviceCount(&ndev));
  if (ndev <= 0) { *err = "no HIP device"; return MAMG_ERR_HIP; }
  HIPCHK(hipSetDevice(p.device));
  HIPCHK(hipStreamCreateWithFlags(&h->cap, hipStreamNonBlocking));
  const int nl = (int)H.levels.size();
  h->L.resize(nl);
  h->bsr = !point_gs(p) && bsr_eligible(H, A0, p);   // point-wise GS: the CSR layout, nodal hierarchies too
  if ((gs_smoother(p) || patch_schwarz(p) || (rings_schwarz(p) && !rings_csr(p))) && !h->bsr) {
    *err = layout_error(p);
    return MAMG_ERR_UNSUPPORTED;
  }
  int rc;
  for (int l = 0; l < nl; ++l) {
    const HostLevel& hl = H.levels[l];
    DLevel& D = h->L[l];
    D.n = hl.n;
    D.coarsest = hl.coarsest;
    const CsrView Al = l == 0 ? A0 : H.A(l);
    const int lanesA = l == 0 ? p.spmv_lanes : 0;
    if (h->bsr && !(l == 0 && D.coarsest)) {
      // copy the level's CSRs up once and build the apply layouts on the device
      TmpPool T(h->sw);
      LevelSrc S;
      if ((rc = upload_tmp(&T, Al, &S.A, err))) return rc;
      if (D.coarsest) {
        double* dA = nullptr;
        if ((rc = T.alloc(&dA, D.n * D.n, err))) return rc;
        HIPCHK(hipMemcpy(dA, hl.Ainv.data(), D.n * D.n * sizeof(double), hipMemcpyHostToDevice));
        S.Ainv = dA;
        if ((rc = build_bsr_level(h.get(), l, S, 0, 0, err))) return rc;
      } else {
        const int64_t nv = D.n / 2, nvc = H.levels[l + 1].n / 2;
        if ((rc = upload_tmp(&T, hl.P.view(), &S.P, err))) return rc;
        if ((rc = upload_tmp(&T, hl.R.view(), &S.R, err))) return rc;
        if (p.post_fusion && p.postsmooth_iter >= 1 && hl.AP.n == hl.n)
          if ((rc = upload_tmp(&T, hl.AP.view(), &S.AP, err))) return rc;
        std::vector<double> blk;
        node_blocks_of(hl.WB.view(), nv, &blk);
        double* dW = nullptr;
        if ((rc = T.alloc(&dW, 4 * nv, err))) return rc;
        HIPCHK(hipMemcpy(dW, blk.data(), 4 * nv * sizeof(double), hipMemcpyHostToDevice));
        S.W = dW;
        S.seeds = &H.seeds;
        if (l == 0 && h->sw.post_mf_mode != 0 && (int64_t)hl.agg.size() == nv) {   // try_post_mf's inputs
          int64_t* dagg = nullptr;
          if ((rc = T.alloc(&dagg, nv, err))) return rc;
          HIPCHK(hipMemcpy(dagg, hl.agg.data(), nv * sizeof(int64_t), hipMemcpyHostToDevice));
          S.agg = dagg;
          S.w_sa = hl.w_sa;
        }
        if ((rc = build_bsr_level(h.get(), l, S, nvc, lanesA, err))) return rc;
      }
    } else if (D.coarsest) {     // CSR layout, or a single-level hierarchy
      if ((rc = dalloc(h.get(), &D.Ainv, D.n * D.n, err))) return rc;
      HIPCHK(hipMemcpy(D.Ainv, hl.Ainv.data(), D.n * D.n * sizeof(double), hipMemcpyHostToDevice));
      if ((rc = upload_csr(h.get(), Al, &D.A, lanesA, err))) return rc;
    } else {
      if ((rc = upload_csr(h.get(), Al, &D.A, lanesA, err))) return rc;
      if ((rc = upload_csr(h.get(), hl.P.view(), &D.P, 0, err))) return rc;
      if ((rc = upload_csr(h.get(), hl.R.view(), &D.R, 0, err))) return rc;
      if (hl.WB.n > 0) {
        if ((rc = upload_csr(h.get(), hl.WB.view(), &D.WB, 0, err))) return rc;
      } else {
        if ((rc = dalloc(h.get(), &D.winv, D.n, err))) return rc;
        HIPCHK(hipMemcpy(D.winv, hl.winv.data(), D.n * sizeof(double), hipMemcpyHostToDevice));
      }
      if (l == 0 && rings_schwarz(p) && !H.seeds.empty()) {   // seed rings + point GS on the rest
        TmpPool T(h->sw);
        if ((rc = build_rings_csr(h.get(), &T, H.seeds, p.spmv_lanes, &D, err))) return rc;
      } else if (point_gs(p)) {
        TmpPool T(h->sw);
        if ((rc = build_gs_csr(h.get(), &T, D.A, l, p.spmv_lanes, &D, err))) return rc;
      }
      if (p.smoother == MAMG_SMOOTHER_POLY) {   // step smoothers w_k W (values only)
        std::vector<double*> wk;
        if ((rc = poly_scaled(h.get(), hl.WB.n > 0 ? D.WB.val : D.winv, hl.WB.n > 0 ? D.WB.nnz : D.n, &wk,
                              err)))
          return rc;
        for (double* q : wk) {
          if (hl.WB.n > 0) {
            DCsr c = D.WB;
            c.val = q;
            D.WBk.push_back(c);
          } else {
            D.winvk.push_back(q);
          }
        }
      }
    }
    double** vecs[] = {&D.b, &D.x, &D.t, &D.t2, &D.r, &D.c, &D.e};
    for (double** v : vecs)
      if ((rc = dalloc(h.get(), v, D.n, err))) return rc;
    if (p.coarse_scaling) {
      if ((rc = dalloc(h.get(), &D.q, D.n, err))) return rc;
      if ((rc = dalloc(h.get(), &D.part2, 2 * SCALE_BLOCKS, err))) return rc;
    }
    if ((rc = kcycle_alloc(h.get(), l, err))) return rc;
  }
  const int64_t n0 = h->L[0].n;
  double** v0[] = {&h->hr, &h->hz};
  for (double** v : v0)
    if ((rc = dalloc(h.get(), v, n0, err))) return rc;
  std::vector<Op> ops;
  apply_ops(h.get(), h->hr, h->hz, &ops);
  for (const Op& o : ops) h->apply_bytes += o.bytes;
  HIPCHK(null_sync());
  const auto t1 = std::chrono::steady_clock::now();
  h->layout_ms[LT_BUILD] = std::chrono::duration<double, std::milli>(t1 - t0).count();
  debug_sums(h.get(), "pre-rehome", true);
  rehome_operators(h.get());
  debug_sums(h.get(), "post-rehome", true);
  const auto t2 = std::chrono::steady_clock::now();
  apply_k_layout_knob(h.get());
  set_tail_level(h.get());
  // every layout kernel and device-to-device copy (null stream) ordered
  // before the handle's first use on any stream (HandleOrder::wait waits on it)
  if ((rc = h->mark(nullptr, err))) return rc;
  HIPCHK(hipEventSynchronize(h->last));
  debug_sums(h.get(), "upload", false);
  h->layout_ms[LT_FINISH] =
      std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t2).count();
  *out = h.release();
  return MAMG_OK;
}

// HBM reserved before the GPU setup churns memory: the apply layout is then
// bump-allocated from it (dev_from_ghier / dist_upload adopt it).  Measured at
// nrefs=6, fresh processes: K kernel 1.47-1.50 ms from the reservation vs
// 1.61-1.71 ms from hipMallocs made after the setup's alloc/free churn
// (profiles/r01_bench_prereserve_ab.log).  Bytes per A0
// entry: MAMG_PRERESERVE_B_PER_NNZ (default 20, ~16.5 used at nrefs=6; 0 = off);
// a rank of N reserves 1.25 x that / N + 0.5.
// one pending reservation per host thread (setups in different threads, e.g.
// virtual ranks or several devices, never see each other's), tagged with its
// device: a handle on another device does not adopt it
static thread_local void* g_pre = nullptr;
static thread_local size_t g_pre_bytes = 0;
static thread_local int g_pre_dev = -1;
void dev_prereserve(int device, int64_t nnz, int nranks, const Switches& sw) {
  double b = sw.prereserve_b_per_nnz;
  if (nranks > 1) b = 1.25 * b / nranks + 0.5;
  dev_prereserve_release();
  if (b <= 0 || nnz <= 0) return;
  if (hipSetDevice(device) != hipSuccess) { (void)hipGetLastError(); return; }
  const size_t bytes = ((size_t)(b * (double)nnz) + (1 << 21)) & ~(size_t)((1 << 21) - 1);
  if (raw_malloc(&g_pre, bytes, "pre") == hipSuccess) { g_pre_bytes = bytes; g_pre_dev = device; }
  else { (void)hipGetLastError(); g_pre = nullptr; }
}
void dev_prereserve_release() {
  if (g_pre) {
    int cur = 0;
    (void)hipGetDevice(&cur);
    (void)hipSetDevice(g_pre_dev);
    (void)raw_free(g_pre);
    (void)hipSetDevice(cur);
  }
  g_pre = nullptr;
  g_pre_bytes = 0;
  g_pre_dev = -1;
}
void adopt_prereserve(HandleMem* h, int device) {
  if (!g_pre || g_pre_dev != device) { dev_prereserve_release(); return; }
  h->allocs.push_back(g_pre);
  h->arena = (char*)g_pre;
  h->arena_left = g_pre_bytes;
  g_pre = nullptr;
  g_pre_bytes = 0;
  g_pre_dev = -1;
}
// a DeviceHandle also keeps the adopted range [arena0, arena1) (release_owned,
// rehome_array: arena memory stays with the reservation); none adopted: empty
void adopt_prereserve(DeviceHandle* h) {
  adopt_prereserve(static_cast<HandleMem*>(h), h->device);
  h->arena0 = h->arena;
  h->arena1 = h->arena + h->arena_left;
}

int dev_from_ghier(GHier* G, const DevMat& A0, const mamg_params& p, DeviceHandle** out,
                   std::string* err) {
  const auto t0 = std::chrono::steady_clock::now();
  std::unique_ptr<DeviceHandle> h(new DeviceHandle(G->sw));
  h->p = p;
  h->device = p.device;
  adopt_prereserve(h.get());
  HIPCHK(hipSetDevice(p.device));
  HIPCHK(hipStreamCreateWithFlags(&h->cap, hipStreamNonBlocking));
  h->bsr = !G->generic && !point_gs(p);   // a general block or point smoother: the CSR layout (as dev_upload)
  if ((gs_smoother(p) || patch_schwarz(p) || (rings_schwarz(p) && !rings_csr(p))) && !h->bsr) {
    *err = layout_error(p);
    return MAMG_ERR_UNSUPPORTED;
  }
  const int nl = (int)G->levels.size();
  h->L.resize(nl);
  int rc;
  for (int l = 0; l < nl; ++l) {
    GLevel& g = G->levels[l];
    DLevel& D = h->L[l];
    D.n = g.n;
    D.coarsest = g.coarsest;
    if (!h->bsr) {                       // CSR layout from the device CSRs (dev_upload's CSR branch)
      if ((rc = adopt_csr(h.get(), l == 0 ? A0 : g.A, &D.A, l == 0 ? p.spmv_lanes : 0, err))) return rc;
      if (D.coarsest) {
        if ((rc = dalloc(h.get(), &D.Ainv, D.n * D.n, err))) return rc;
        HIPCHK(dev_copy(D.Ainv, g.Ainv, D.n * D.n * sizeof(double)));
      } else {
        if ((rc = adopt_csr(h.get(), g.P, &D.P, 0, err))) return rc;
        if ((rc = adopt_csr(h.get(), g.R, &D.R, 0, err))) return rc;
        if (g.WB.n > 0) {
          if ((rc = adopt_csr(h.get(), g.WB, &D.WB, 0, err))) return rc;
        } else {
          if ((rc = dalloc(h.get(), &D.winv, D.n, err))) return rc;
          HIPCHK(dev_copy(D.winv, g.winv, D.n * sizeof(double)));
        }
        if (l == 0 && rings_schwarz(p) && !G->seeds.empty()) {   // seed rings + point GS on the rest
          TmpPool T(h->sw);
          if ((rc = build_rings_csr(h.get(), &T, G->seeds, p.spmv_lanes, &D, err))) return rc;
        } else if (point_gs(p)) {
          TmpPool T(h->sw);
          if ((rc = build_gs_csr(h.get(), &T, D.A, l, p.spmv_lanes, &D, err))) return rc;
        }
        if (p.smoother == MAMG_SMOOTHER_POLY) {   // step smoothers w_k W (values only)
          std::vector<double*> wk;
          const bool blk = g.WB.n > 0;
          if ((rc = poly_scaled(h.get(), blk ? D.WB.val : D.winv, blk ? D.WB.nnz : D.n, &wk, err))) return rc;
          for (double* q : wk) {
            if (blk) {
              DCsr c = D.WB;
              c.val = q;
              D.WBk.push_back(c);
            } else {
              D.winvk.push_back(q);
            }
          }
        }
      }
    } else if (l == 0 && D.coarsest) {          // single-level hierarchy: CSR A0 + dense inverse
      if ((rc = dalloc(h.get(), &D.Ainv, D.n * D.n, err))) return rc;
      HIPCHK(dev_copy(D.Ainv, g.Ainv, D.n * D.n * sizeof(double)));
      D.A.n = A0.n; D.A.m = A0.m; D.A.nnz = A0.nnz;
      D.A.lanes = p.spmv_lanes > 0 ? p.spmv_lanes : pick_lanes(A0.n, A0.nnz);
      if ((rc = dalloc(h.get(), &D.A.ptr, A0.n + 1, err))) return rc;
      if ((rc = dalloc(h.get(), &D.A.col, std::max<int64_t>(A0.nnz, 1), err))) return rc;
      if ((rc = dalloc(h.get(), &D.A.val, std::max<int64_t>(A0.nnz, 1), err))) return rc;
      HIPCHK(dev_copy(D.A.ptr, A0.ptr, (A0.n + 1) * sizeof(int64_t)));
      if (A0.nnz) {
        HIPCHK(dev_copy(D.A.col, A0.col, A0.nnz * sizeof(int32_t)));
        HIPCHK(dev_copy(D.A.val, A0.val, A0.nnz * sizeof(double)));
      }
    } else {
      LevelSrc S;
      S.A = l == 0 ? A0 : g.A;
      S.P = g.P; S.R = g.R; S.AP = g.AP; S.W = g.W; S.Ainv = g.Ainv;
      S.seeds = &G->seeds;
      if (l == 0) { S.agg = g.agg; S.w_sa = g.w_sa; }
      const int64_t nvc = D.coarsest ? 0 : G->levels[l + 1].n / 2;
      if ((rc = build_bsr_level(h.get(), l, S, nvc, l == 0 ? p.spmv_lanes : 0, err))) return rc;
    }
    {
      char st[32];
      std::snprintf(st, sizeof st, "built-L%d", l);
      debug_sums(h.get(), st, true);
    }
    // the level's GPU-setup buffers are no longer needed (A_l stays for l+1's
    // Galerkin product only, which is done)
    for (void* q : {(void*)g.P.ptr, (void*)g.P.col, (void*)g.P.val, (void*)g.R.ptr, (void*)g.R.col,
                    (void*)g.R.val, (void*)g.AP.ptr, (void*)g.AP.col, (void*)g.AP.val, (void*)g.W,
                    (void*)g.Ainv, (void*)g.WB.ptr, (void*)g.WB.col, (void*)g.WB.val, (void*)g.winv})
      if (q) G->release(q);
    if (l > 0)
      for (void* q : {(void*)g.A.ptr, (void*)g.A.col, (void*)g.A.val})
        if (q) G->release(q);
    g.P = g.R = g.AP = g.WB = DevMat();
    g.W = g.Ainv = g.winv = nullptr;
    if (l > 0) g.A = DevMat();
    double** vecs[] = {&D.b, &D.x, &D.t, &D.t2, &D.r, &D.c, &D.e};
    for (double** v : vecs)
      if ((rc = dalloc(h.get(), v, D.n, err))) return rc;
    if (p.coarse_scaling) {
      if ((rc = dalloc(h.get(), &D.q, D.n, err))) return rc;
      if ((rc = dalloc(h.get(), &D.part2, 2 * SCALE_BLOCKS, err))) return rc;
    }
    if ((rc = kcycle_alloc(h.get(), l, err))) return rc;
  }
  const int64_t n0 = h->L[0].n;
  double** v0[] = {&h->hr, &h->hz};
  for (double** v : v0)
    if ((rc = dalloc(h.get(), v, n0, err))) return rc;
  std::vector<Op> ops;
  apply_ops(h.get(), h->hr, h->hz, &ops);
  for (const Op& o : ops) h->apply_bytes += o.bytes;
  for (int k = 0; k < 8; ++k) h->setup_ms[k] = G->phase_ms[k];
  HIPCHK(null_sync());
  const auto t1 = std::chrono::steady_clock::now();
  h->layout_ms[LT_BUILD] = std::chrono::duration<double, std::milli>(t1 - t0).count();
  debug_sums(h.get(), "pre-rehome", true);
  rehome_operators(h.get());
  debug_sums(h.get(), "post-rehome", true);
  const auto t2 = std::chrono::steady_clock::now();
  apply_k_layout_knob(h.get());
  set_tail_level(h.get());
  if ((rc = h->mark(nullptr, err))) return rc;   // as in dev_upload
  HIPCHK(hipEventSynchronize(h->last));
  debug_sums(h.get(), "upload", false);
  const auto t3 = std::chrono::steady_clock::now();
  h->layout_ms[LT_FINISH] = std::chrono::duration<double, std::milli>(t3 - t2).count();
  h->setup_ms[GS_LAYOUT] = std::chrono::duration<double, std::milli>(t3 - t0).count();
  *out = h.release();
  return MAMG_OK;
}

void dev_setup_ms(const DeviceHandle* h, double* ms8) {
  for (int k = 0; k < 8; ++k) ms8[k] = h->setup_ms[k];
}
void dev_layout_ms(const DeviceHandle* h, double* ms4) {
  for (int k = 0; k < 4; ++k) ms4[k] = h->layout_ms[k];
}

void dev_tmp_trim() { tmp_trim_all(); }
void dev_tmp_trim_to_limit() { tmp_trim_to_limit_all(); }
void dev_set_cache_limit(int64_t bytes) { set_cache_limit(bytes); }
int64_t dev_cache_limit(int device) { return cache_limit_dev(device); }
int64_t dev_cache_idle_bytes(int device) {
  int64_t b = tmp_idle_bytes(device);
  std::lock_guard<std::mutex> g(detail::stage_mu());
  return b + (int64_t)detail::stage_pools()[device & 63].bytes;
}

void dev_destroy(DeviceHandle* h) {
  if (!h) return;
  (void)hipSetDevice(h->device);
  // every use of the handle (applies, PCG, timing, host applies) recorded
  // h->last on its stream: wait for that, not for the device
  if (h->last) (void)hipEventSynchronize(h->last);
  if (h->cap) (void)hipStreamSynchronize(h->cap);
  delete h;
}

int64_t dev_nrows(const DeviceHandle* h) { return h->L[0].n; }
int dev_num_levels(const DeviceHandle* h) { return (int)h->L.size(); }
double dev_apply_bytes(const DeviceHandle* h) { return h->apply_bytes; }
int dev_layout(const DeviceHandle* h) { return h->bsr ? 1 : 0; }
int dev_level_format(const DeviceHandle* h, int level) {
  const DLevel& L = h->L[level];
  return (L.Ab.sell ? MAMG_FMT_SELL : 0) | (L.Ab.sym ? MAMG_FMT_SYM : 0) | (L.Ab.half ? MAMG_FMT_HALF : 0) |
         (L.Ab.rowdict ? MAMG_FMT_ROWDICT : 0) | (L.post_mf ? MAMG_FMT_POST_MF : 0) |
         (L.PAb.nr > 0 || L.KPb.nr > 0 ? MAMG_FMT_POST_FUSED : 0) | (L.KPb.nr > 0 ? MAMG_FMT_POST_K : 0) |
         (L.KPb.sell ? MAMG_FMT_POST_SELL : 0) | (L.Ab.nsched > 0 || L.Ab.nsched_r > 0 ? MAMG_FMT_BANDS : 0) |
         (L.pcs.size() > 1 ? MAMG_FMT_PATCHES : 0) | (L.gcs.size() > 1 ? MAMG_FMT_GS : 0) |
         (L.rcs.size() > 1 ? MAMG_FMT_RINGS : 0) | (L.Rb.nrsched > 0 ? MAMG_FMT_R_BANDS : 0) |
         (L.KPb.col16 ? MAMG_FMT_K_COL16 : 0);
}

namespace {

// ---------------------------------------------------------------------------
// fp32 storage of the operators the cycle streams (mamg_set_cycle_storage,
// DESIGN.md section 4.7).  The fp32 arrays keep the element layout of the fp64
// ones (blk / blk_split / blk_split_local at VT = float), so one element-wise
// pair of kernels serves every value-array shape: general, SYM, half-symmetric
// upper part, SELL padding and both split layouts.
// ---------------------------------------------------------------------------

constexpr unsigned F32_BLOCKS = 4096;   // grid-stride passes over a value array

// a finite fp64 value whose fp32 rounding is not finite: not representable
__global__ __launch_bounds__(256) void f32_check_kernel(int64_t n, const double* __restrict__ v, int* bad) {
  bool b = false;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const double x = v[i];
    b = b || (isfinite(x) && !isfinite((float)x));
  }
  if (b) atomicOr(bad, 1);
}

// round to nearest even (v_cvt_f32_f64 in the default rounding mode): numpy's
// astype(float32); padding slots are converted like any value
__global__ __launch_bounds__(256) void f32_convert_kernel(int64_t n, const double* __restrict__ v,
                                                         float* __restrict__ out) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
    out[i] = (float)v[i];
}

inline unsigned f32_grid(int64_t n) { return (unsigned)std::min<int64_t>(F32_BLOCKS, (n + 255) / 256); }

}  // namespace

// fp32 copies of the jobs' value arrays (either handle type).  1. every array
// is checked before any is converted: a refusal leaves the handle untouched;
// 2. all copies are made before any operator changes (undone on failure);
// 3. drop_cached(): the caller drops what holds the fp64 op list; 4. the copies
// are swapped in (a dst other than its src first takes src's layout: level 0's
// Ac shares A's index arrays); release() gets each replaced original.
int narrow_values(std::vector<NarrowJob>& jobs, std::vector<void*>* allocs, const std::function<void()>& drop_cached,
                  const std::function<void(void*)>& release, std::string* err) {
  int* bad = nullptr;
  HIPCHK(raw_malloc((void**)&bad, sizeof(int), "tmp"));
  int hbad = 0;
  hipError_t e = dev_memset(bad, 0, sizeof(int));
  if (e == hipSuccess)
    for (const NarrowJob& j : jobs) f32_check_kernel<<<f32_grid(j.count()), 256>>>(j.count(), j.from(), bad);
  if (e == hipSuccess) e = hipGetLastError();
  if (e == hipSuccess) e = hipMemcpy(&hbad, bad, sizeof(int), hipMemcpyDeviceToHost);
  (void)raw_free(bad);
  HIPCHK(e);
  if (hbad) {
    *err = "cycle storage: an operator holds a finite value that is not representable in fp32";
    return MAMG_ERR_UNSUPPORTED;
  }
  for (NarrowJob& j : jobs) {
    e = dev_malloc((void**)&j.val, (size_t)j.count() * sizeof(float));
    if (e != hipSuccess) break;
    f32_convert_kernel<<<f32_grid(j.count()), 256>>>(j.count(), j.from(), j.val);
  }
  if (e == hipSuccess) e = hipGetLastError();
  if (e == hipSuccess) e = null_sync();
  if (e != hipSuccess) {
    (void)hipGetLastError();
    for (NarrowJob& j : jobs)
      if (j.val) (void)raw_free(j.val);
    *err = std::string("cycle storage: ") + hipGetErrorString(e);
    return e == hipErrorOutOfMemory ? MAMG_ERR_NOMEM : MAMG_ERR_HIP;
  }
  drop_cached();
  // job order matters: the first job of a dst that is not its src copies src's layout into it and
  // sets f32; a later job of the same dst (the ghost part) must find f32 set, or it would copy again
  for (NarrowJob& j : jobs) {
    if (j.dst != j.src && !j.dst->f32) *j.dst = *j.src;
    double*& slot = j.ghost ? j.dst->gval : j.dst->val;
    void* old = slot;
    slot = reinterpret_cast<double*>(j.val);
    j.dst->f32 = true;
    allocs->push_back(j.val);
    if (j.dst == j.src) release(old);
  }
  return MAMG_OK;
}

namespace {

// a handle-owned array that nothing reads any more (the caller has waited)
void release_owned(DeviceHandle* h, void* old) {
  if (!old) return;
  const bool in_arena = (char*)old >= h->arena0 && (char*)old < h->arena1;
  auto it = std::find(h->allocs.begin(), h->allocs.end(), old);
  if (in_arena || it == h->allocs.end()) return;   // arena memory stays with the reservation
  (void)raw_free(old);
  h->allocs.erase(it);
}

}  // namespace

int dev_level_storage(const DeviceHandle* h, int level) { return h->L[level].storage; }

int dev_rowdict_info(const DeviceHandle* h, int64_t* info, int cap) {
  const DBsr& A = h->L[0].Ab;
  int64_t v[RD_INFO_N];
  for (int i = 0; i < RD_INFO_N; ++i) v[i] = A.rdinfo[i];
  if (!h->bsr) v[RD_REASON] = RDR_NOT_TRIED;
  for (int i = 0; i < cap && i < RD_INFO_N; ++i) info[i] = v[i];
  return RD_INFO_N;
}

int dev_post_mf_info(const DeviceHandle* h, int64_t* info, int cap) {
  const DLevel& L = h->L[0];
  for (int i = 0; i < cap && i < PM_INFO_N; ++i) info[i] = L.mfinfo[i];
  return PM_INFO_N;
}

int dev_tail_info(const DeviceHandle* h, int index, int64_t* info, int cap) {
  std::lock_guard<std::recursive_mutex> lock(capture_mutex());
  const int np = (int)h->tails.size();
  std::vector<int64_t> v(TAIL_INFO_HEAD, 0);
  if (index < np) v = h->tails[index].info;
  v[TI_PROGS] = np;
  v[TI_LEVEL] = h->tail_level;
  v[TI_REFUSED] = h->tail_refused ? 1 : 0;
  for (int i = 0; i < cap && i < (int)v.size(); ++i) info[i] = v[i];
  return index < np ? (int)v.size() : 0;
}

int dev_set_cycle_storage(DeviceHandle* h, int storage, std::string* err) {
  std::lock_guard<std::recursive_mutex> lock(capture_mutex());
  bool narrowed = false;
  for (const DLevel& L : h->L) narrowed = narrowed || L.storage != 0;
  if (storage == MAMG_STORE_F64) {
    if (!narrowed) return MAMG_OK;
    *err = "cycle storage: the fp64 originals of a narrowed handle are gone (fp32 storage is one way)";
    return MAMG_ERR_UNSUPPORTED;
  }
  if (narrowed) return MAMG_OK;
  if (h->p.cycle_type == MAMG_NL_AMLI_CYCLE) {
    *err = "cycle storage: fp32 is not available with the nonlinear AMLI cycle";
    return MAMG_ERR_UNSUPPORTED;
  }
  if (!h->bsr) {
    *err = "cycle storage: fp32 needs the BSR2 layout (this handle holds the CSR layout)";
    return MAMG_ERR_UNSUPPORTED;
  }
  for (const DLevel& L : h->L) {
    if (L.pcs.size() > 1) { *err = "cycle storage: fp32 is not available with SCHWARZ_PATCHES"; return MAMG_ERR_UNSUPPORTED; }
    if (L.rcs.size() > 1) { *err = "cycle storage: fp32 is not available with SCHWARZ_RINGS"; return MAMG_ERR_UNSUPPORTED; }
    if (L.gcs.size() > 1) { *err = "cycle storage: fp32 is not available with the GS / SGS smoothers"; return MAMG_ERR_UNSUPPORTED; }
  }
  if (gs_smoother(h->p) || patch_schwarz(h->p) || rings_schwarz(h->p)) {
    *err = "cycle storage: fp32 is not available with the GS / SGS smoothers or the Schwarz smoothers";
    return MAMG_ERR_UNSUPPORTED;
  }
  HIPCHK(hipSetDevice(h->device));
  // the launch path's levels: below the coarse tail and above the coarsest
  std::vector<NarrowJob> jobs;
  std::vector<std::pair<int, int>> lev_bit;   // level and mamg_level_storage bit of each job
  auto add = [&](DBsr* src, DBsr* dst, int l, int bit) {
    if (value_count(*src) == 0) return;
    jobs.push_back({src, dst, false});
    lev_bit.push_back({l, bit});
  };
  for (int l = 0; l < (int)h->L.size(); ++l) {
    DLevel& L = h->L[l];
    if (L.coarsest || (h->tail_level > 0 && l >= h->tail_level)) break;
    if (L.Ab.ngs > 0) {   // a rank-local A with ghost columns: the fp32 side is the ghost-free kernel
      *err = "cycle storage: fp32 is not available for a half-symmetric A with a ghost part";
      return MAMG_ERR_UNSUPPORTED;
    }
    add(&L.Ab, l == 0 ? &L.Ac : &L.Ab, l, 1);
    add(&L.KPb, &L.KPb, l, 2);
    add(&L.Pb, &L.Pb, l, 2);
    add(&L.Rb, &L.Rb, l, 4);
    // a merged [P | AP] (PAb, MAMG_POST_K=0) stays fp64: bsr2_post_kernel has no fp32 side
  }
  // wait for the handle's last work; narrow_values' kernels run on the null stream
  if (h->last) HIPCHK(hipEventSynchronize(h->last));
  if (h->cap) HIPCHK(hipStreamSynchronize(h->cap));
  // the cached graphs hold the fp64 op list: dropped, the next apply captures anew
  auto drop_cached = [&]() {
    h->graphs.clear();
    release_all(&h->pcgs);
  };
  // the fp64 originals go back except A_0's (the Krylov operator)
  int rc = narrow_values(jobs, &h->allocs, drop_cached, [&](void* old) { release_owned(h, old); }, err);
  if (rc) return rc;
  for (size_t k = 0; k < jobs.size(); ++k) h->L[lev_bit[k].first].storage |= lev_bit[k].second;
  // a matrix-free level 0 holds no K / P to narrow (its post step reads A's
  // fp32 table, Wp stays fp64): the bit is reported as requested
  if (h->L[0].post_mf && (h->L[0].storage & 1)) h->L[0].storage |= 2;
  std::vector<Op> ops;
  apply_ops(h, h->hr, h->hz, &ops);
  h->apply_bytes = 0.0;
  for (const Op& o : ops) h->apply_bytes += o.bytes;
  return MAMG_OK;
}

// The K ops of the Krylov levels below the tail level join the tail programs
// (on) or stay launches (off, the state after setup).  Everything planned or
// captured with the other state is dropped: the next apply plans again.
int dev_set_kcycle_tail(DeviceHandle* h, int on, std::string* err) {
  std::lock_guard<std::recursive_mutex> lock(capture_mutex());
  if (h->p.cycle_type != MAMG_NL_AMLI_CYCLE) {
    *err = "kcycle tail: the handle's cycle is not the nonlinear AMLI cycle (MAMG_NL_AMLI_CYCLE)";
    return MAMG_ERR_UNSUPPORTED;
  }
  if (!h->bsr) {
    *err = "kcycle tail: the coarse tail needs the BSR2 layout (this handle holds the CSR layout)";
    return MAMG_ERR_UNSUPPORTED;
  }
  if (h->tail_level == 0 || h->kcycle_tail == (on != 0)) {   // no tail to plan, or nothing to change
    h->kcycle_tail = on != 0;
    return MAMG_OK;
  }
  HIPCHK(hipSetDevice(h->device));
  if (h->last) HIPCHK(hipEventSynchronize(h->last));
  if (h->cap) HIPCHK(hipStreamSynchronize(h->cap));
  h->graphs.clear();
  release_all(&h->pcgs);
  for (auto& t : h->tails) (void)raw_free(t.prog);
  h->tails.clear();
  h->tail_refused = false;
  h->kcycle_tail = on != 0;
  return MAMG_OK;
}

int dev_kcycle_tail(const DeviceHandle* h) { return h->kcycle_tail ? 1 : 0; }

// what launch() issues for one apply: every op of the list with work, a tail
// program as one (building the list plans the tail programs, launches nothing)
int dev_apply_launches(const DeviceHandle* h, int64_t* launches, std::string* err) {
  std::lock_guard<std::recursive_mutex> lock(capture_mutex());
  HIPCHK(hipSetDevice(h->device));
  std::vector<Op> ops;
  apply_ops(h, h->hr, h->hz, &ops);
  int64_t c = 0;
  for (const Op& o : ops) c += o.n > 0 ? 1 : 0;
  *launches = c;
  return MAMG_OK;
}

mamg_params dev_params(const DeviceHandle* h) { return h->p; }
const Switches& dev_switches(const DeviceHandle* h) { return h->sw; }
void dev_kregion(const DeviceHandle* h, std::vector<double>* ms, int* kept) {
  *ms = h->kregion_ms;
  *kept = h->kregion_best;
}

int dev_apply(DeviceHandle* h, const double* d_r, double* d_z, void* stream, std::string* err) {
  if (d_r == d_z) { *err = "r and z must not alias"; return MAMG_ERR_ARG; }
  debug_sums(h, "apply", false);
  HIPCHK(hipSetDevice(h->device));
  hipGraphExec_t exec;
  int rc = get_graph(h, d_r, d_z, &exec, err);
  if (rc) return rc;
  if ((rc = h->wait((hipStream_t)stream, err))) return rc;
  HIPCHK(hipGraphLaunch(exec, (hipStream_t)stream));
  return h->mark((hipStream_t)stream, err);
}

int dev_apply_host(DeviceHandle* h, const double* r, double* z, std::string* err) {
  HIPCHK(hipSetDevice(h->device));
  const int64_t n = h->L[0].n;
  hipGraphExec_t exec;
  int rc = get_graph(h, h->hr, h->hz, &exec, err);
  if (rc) return rc;
  if ((rc = h->wait(h->cap, err))) return rc;   // after queued device-pointer applies
  HIPCHK(hipMemcpyAsync(h->hr, r, n * sizeof(double), hipMemcpyHostToDevice, h->cap));
  HIPCHK(hipGraphLaunch(exec, h->cap));
  HIPCHK(hipMemcpyAsync(z, h->hz, n * sizeof(double), hipMemcpyDeviceToHost, h->cap));
  if ((rc = h->mark(h->cap, err))) return rc;
  HIPCHK(hipStreamSynchronize(h->cap));
  return MAMG_OK;
}

int dev_spmv(DeviceHandle* h, const double* d_x, double* d_y, void* stream, std::string* err) {
  HIPCHK(hipSetDevice(h->device));
  int rc = h->wait((hipStream_t)stream, err);
  if (rc) return rc;
  launch(a0_op(h, EPI_Y, d_x, nullptr, d_y), (hipStream_t)stream);
  HIPCHK(hipGetLastError());
  return h->mark((hipStream_t)stream, err);
}

int dev_pcg(DeviceHandle* h, const double* d_b, double* d_x, double tol, int maxiter,
            int relativeconv, double* residuals, double* alphas, double* betas, int* niters,
            void* stream, std::string* err) {
  // cbc.block ConjGrad (mamg_oracle.pcg) with every scalar in HBM: one
  // iteration = one hipGraph (q = A d, <d,q>, alpha, x/r update, z = B r,
  // <r,z>, beta, stop test, d update).  The host keeps one iteration queued
  // ahead and polls the state of the previous one, so the GPU never waits
  // for a host round trip; the queued iteration after the stopping one
  // finds the state inactive and leaves x untouched.
  HIPCHK(hipSetDevice(h->device));
  hipStream_t s = (hipStream_t)stream;
  const int64_t n = h->L[0].n;
  int rc;
  if (maxiter < 0) { *err = "maxiter must be >= 0"; return MAMG_ERR_ARG; }
  if (!h->cr) {
    double** v[] = {&h->cr, &h->cz, &h->cd, &h->cq};
    for (double** q : v)
      if ((rc = dalloc(h, q, n, err))) return rc;
    if ((rc = dalloc(h, &h->part, DOT_BLOCKS, err))) return rc;
    if ((rc = dalloc(h, &h->dres, (int64_t)((sizeof(PcgState) + 7) / 8), err))) return rc;
    HIPCHK(hipHostMalloc((void**)&h->hres, 2 * sizeof(PcgState), hipHostMallocDefault));
  }
  PcgState* st = reinterpret_cast<PcgState*>(h->dres);
  PcgState* hst = reinterpret_cast<PcgState*>(h->hres);
  const unsigned g = nblocks(n);
  if ((rc = h->wait(s, err))) return rc;
  // the iteration graph for (x, maxiter), captured once and kept on the
  // handle (at most 4; the oldest evicted after the handle's work is done)
  PcgGraph* pg = nullptr;
  for (auto& q : h->pcgs)
    if (q.x == d_x && q.maxiter == maxiter) pg = &q;
  if (!pg) {
    if (h->pcgs.size() >= 4) {
      if (h->last) HIPCHK(hipEventSynchronize(h->last));
      HIPCHK(hipStreamSynchronize(s));
      h->pcgs.front().release();
      h->pcgs.erase(h->pcgs.begin());
    }
    PcgGraph q;
    q.x = d_x;
    q.maxiter = maxiter;
    if ((rc = q.alloc(3 * (size_t)maxiter + 1, err))) return rc;
    double *dres = q.hist, *dal = q.hist + maxiter + 1, *dbe = dal + maxiter;
    std::vector<Op> ops;
    apply_ops(h, h->cr, h->cz, &ops);
    rc = capture_graph(&h->cap, [&]() {
      launch(a0_op(h, EPI_Y, h->cd, nullptr, h->cq), h->cap);           // q = A d
      dot_partial_kernel<<<DOT_BLOCKS, 256, 0, h->cap>>>(n, h->cd, h->cq, h->part);
      pcg_alpha_kernel<<<1, 256, 0, h->cap>>>(DOT_BLOCKS, h->part, st);
      pcg_xr_kernel<<<g, 256, 0, h->cap>>>(n, st, h->cd, h->cq, d_x, h->cr);
      for (const Op& o : ops) launch(o, h->cap);                          // z = B r
      dot_partial_kernel<<<DOT_BLOCKS, 256, 0, h->cap>>>(n, h->cr, h->cz, h->part);
      pcg_beta_kernel<<<1, 256, 0, h->cap>>>(DOT_BLOCKS, h->part, st, dres, dal, dbe);
      pcg_d_kernel<<<g, 256, 0, h->cap>>>(n, st, h->cz, h->cd, d_x);
      return (int)MAMG_OK;
    }, "PCG iteration", &q, err);
    if (rc) {
      q.release();
      return rc;
    }
    h->pcgs.push_back(q);
    pg = &h->pcgs.back();
  }
  double *dres = pg->hist, *dal = pg->hist + maxiter + 1, *dbe = dal + maxiter;
  launch(a0_op(h, EPI_RESID, d_x, d_b, h->cr), s);                 // r = b - A x
  if ((rc = dev_apply(h, h->cr, h->cz, s, err))) return rc;         // z = B r
  HIPCHK(dev_copy(h->cd, h->cz, n * sizeof(double), s));
  dot_partial_kernel<<<DOT_BLOCKS, 256, 0, s>>>(n, h->cr, h->cz, h->part);
  pcg_init_kernel<<<1, 256, 0, s>>>(DOT_BLOCKS, h->part, st, tol, relativeconv, maxiter, dres);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(&hst[0], st, sizeof(PcgState), hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  const PcgHist hist{dres, nullptr, dal, dbe};
  if (hst[0].status == PCG_NOT_POS) {
    (void)h->mark(s, err);
    return pcg_finish(PCG_NOT_POS, 0, hist, residuals, nullptr, alphas, betas, niters, err);
  }
  if (hst[0].active) {
    // iteration k's state lands in hst[k & 1]; iteration k + 1 is queued
    // before the host waits for iteration k
    for (int k = 0; k < maxiter; ++k) {
      HIPCHK(hipGraphLaunch(pg->exec, s));
      HIPCHK(hipMemcpyAsync(&hst[k & 1], st, sizeof(PcgState), hipMemcpyDeviceToHost, s));
      HIPCHK(hipEventRecord(pg->ev[k & 1], s));
      if (k == 0) continue;
      HIPCHK(hipEventSynchronize(pg->ev[(k - 1) & 1]));
      if (!hst[(k - 1) & 1].active) break;
    }
  }
  HIPCHK(hipMemcpyAsync(&hst[0], st, sizeof(PcgState), hipMemcpyDeviceToHost, s));
  if ((rc = h->mark(s, err))) return rc;
  HIPCHK(hipStreamSynchronize(s));
  HIPCHK(hipGetLastError());
  return pcg_finish(hst[0].status, hst[0].it, hist, residuals, nullptr, alphas, betas, niters, err);
}

int dev_time_apply(DeviceHandle* h, const double* d_r, double* d_z, int reps, int mode, double* ms,
                   double* kernel_ms, double* class_bytes, void* stream, std::string* err) {
  HIPCHK(hipSetDevice(h->device));
  hipStream_t s = (hipStream_t)stream;
  int rc = h->wait(s, err);
  if (rc) return rc;
  std::vector<Op> ops;
  apply_ops(h, d_r, d_z, &ops);
  if (class_bytes) {
    for (int c = 0; c < 16; ++c) class_bytes[c] = 0.0;
    for (const Op& o : ops) class_bytes[o.cls] += o.bytes;
  }
  if (reps <= 0) { *ms = 0.0; return MAMG_OK; }
  TimedRun tr;
  rc = tr.run(ops.size(), [&](size_t k) { return ops[k].cls; },
              [&](size_t k) { launch(ops[k], s); return (int)MAMG_OK; }, reps, mode, s,
              [&]() { return h->mark(s, err); }, ms, kernel_ms, err);
  if (rc) return rc;
#if MAMG_DIAG
  if (mode == 1 && std::getenv("MAMG_OP_PROFILE")) {
    // diagnosis: event time per (op kind, rows) summed over one apply
    std::map<std::pair<int, int64_t>, std::pair<int, double>> acc;
    for (int rp = 0; rp < reps; ++rp)
      for (size_t ii = 0; ii < tr.inst.size(); ++ii) {
        float t = 0.f;
        if ((rc = tr.op_ms(rp, ii, &t, err))) return rc;
        const Op& o = ops[tr.inst[ii]];
        auto& a = acc[{o.kind, o.Mb ? o.Mb->nr : (o.M ? o.M->n : o.n)}];
        a.first += 1;
        a.second += t;
      }
    for (const auto& kv : acc)
      std::fprintf(stderr, "[mamg op] kind %d rows %lld launches/apply %.1f ms/apply %.4f us/launch %.2f\n",
                   kv.first.first, (long long)kv.first.second, kv.second.first / (double)reps,
                   kv.second.second / reps, 1e3 * kv.second.second / kv.second.first);
  }
  if (std::getenv("MAMG_TAIL_PROFILE")) {
    // diagnosis: the interpreter's cost per op with nothing to do (200 ops
    // with no rows), the program in LDS and in global memory
    {
      const int nn = 200;
      std::vector<TOp> np(nn);
      for (auto& t : np) { t.kind = T_ZERO; t.n = 0; }
      TOp* dp = nullptr;
      uint64_t* dst = nullptr;
      HIPCHK(raw_malloc((void**)&dp, nn * sizeof(TOp), "tmp"));
      HIPCHK(raw_malloc((void**)&dst, 2 * (nn + 1) * sizeof(uint64_t), "tmp"));
      HIPCHK(hipMemcpy(dp, np.data(), nn * sizeof(TOp), hipMemcpyHostToDevice));
      std::vector<uint64_t> st(2 * (nn + 1));
      for (int pl : {0, -1}) {
        for (int rep = 0; rep < 3; ++rep) tail_launch<true>(0, dp, nn, pl, pl == 0 ? nn * sizeof(TOp) : 0, dst, s);
        HIPCHK(hipStreamSynchronize(s));
        HIPCHK(hipMemcpy(st.data(), dst, st.size() * sizeof(uint64_t), hipMemcpyDeviceToHost));
        std::fprintf(stderr, "[mamg tail] %d empty ops, program in %s: %.3f us/op, %.0f cycles/op\n", nn,
                     pl == 0 ? "LDS" : "global", (double)(st[nn] - st[0]) * 0.01 / nn,
                     (double)(st[2 * nn + 1] - st[nn + 1]) / nn);
      }
      // without stamps: event time of 200 vs 2000 empty ops, 512 and 64 threads
      {
        const int nb = 2000;
        std::vector<TOp> nq(nb);
        for (auto& t : nq) { t.kind = T_ZERO; t.n = 0; }
        TOp* dq = nullptr;
        HIPCHK(raw_malloc((void**)&dq, nb * sizeof(TOp), "tmp"));
        HIPCHK(hipMemcpy(dq, nq.data(), nb * sizeof(TOp), hipMemcpyHostToDevice));
        hipEvent_t e0, e1;
        HIPCHK(hipEventCreate(&e0));
        HIPCHK(hipEventCreate(&e1));
        for (int th : {TAIL_THREADS, 64}) {
          float tt[2] = {0.f, 0.f};
          for (int v = 0; v < 2; ++v) {
            const int cnt = v ? nb : nn;
            tail_kernel<false, false, false><<<1, th, 0, s>>>(dq, cnt, -1, nullptr);
            HIPCHK(hipEventRecord(e0, s));
            for (int rep = 0; rep < 10; ++rep) tail_kernel<false, false, false><<<1, th, 0, s>>>(dq, cnt, -1, nullptr);
            HIPCHK(hipEventRecord(e1, s));
            HIPCHK(hipEventSynchronize(e1));
            HIPCHK(hipEventElapsedTime(&tt[v], e0, e1));
          }
          std::fprintf(stderr, "[mamg tail] empty op without stamps, %d threads: %.3f us/op\n", th,
                       1e3 * (tt[1] - tt[0]) / 10.0 / (nb - nn));
        }
        HIPCHK(hipEventDestroy(e0));
        HIPCHK(hipEventDestroy(e1));
        (void)raw_free(dq);
      }
      (void)raw_free(dp);
      (void)raw_free(dst);
    }
    // diagnosis: wall-clock stamps after every op of each coarse-tail program
    for (const auto& tp : h->tails) {
      std::vector<TOp> prog(tp.n);
      std::vector<uint64_t> st(2 * (tp.n + 1));   // 100 MHz stamps, then shader-clock stamps
      uint64_t* dst = nullptr;
      HIPCHK(raw_malloc((void**)&dst, 2 * (tp.n + 1) * sizeof(uint64_t), "tmp"));
      HIPCHK(hipMemcpy(prog.data(), tp.prog, tp.n * sizeof(TOp), hipMemcpyDeviceToHost));
      for (int rep = 0; rep < 2; ++rep)
        tail_launch<true>((tp.xl ? 1 : 0) | (tp.res ? 2 : 0) | (tp.kops ? 4 : 0), tp.prog, tp.n, tp.prog_lds, (size_t)tp.lds, dst, s);
      HIPCHK(hipStreamSynchronize(s));
      HIPCHK(hipMemcpy(st.data(), dst, 2 * (tp.n + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost));
      (void)raw_free(dst);
      std::map<std::pair<int, int64_t>, std::pair<int, double>> acc;
      for (int k = 0; k < tp.n; ++k) {
        auto& a = acc[{prog[k].kind, prog[k].n}];
        a.first += 1;
        a.second += (double)(st[k + 1] - st[k]) * 0.01;   // 100 MHz ticks -> us
      }
      const double us = (double)(st[tp.n] - st[0]) * 0.01, cyc = (double)(st[2 * tp.n + 1] - st[tp.n + 1]);
      std::fprintf(stderr, "[mamg tail] program of %d ops: %.1f us, %.0f shader cycles (%.0f MHz)\n", tp.n, us, cyc,
                   us > 0 ? cyc / us : 0.0);
      if (std::atoi(std::getenv("MAMG_TAIL_PROFILE")) > 1)
        for (int k = 0; k < tp.n; ++k)
          std::fprintf(stderr, "[mamg tail op] %d kind %d n %lld rows [%lld, %lld) vl %d lds %d us %.2f\n", k,
                       prog[k].kind, (long long)prog[k].n, (long long)prog[k].r0, (long long)prog[k].r1,
                       prog[k].vl, (int)(((uintptr_t)prog[k].x | (uintptr_t)prog[k].out) & 1),
                       (double)(st[k + 1] - st[k]) * 0.01);
      for (const auto& kv : acc)
        std::fprintf(stderr, "[mamg tail] kind %d rows %lld ops %d us %.1f us/op %.3f\n", kv.first.first,
                     (long long)kv.first.second, kv.second.first, kv.second.second,
                     kv.second.second / kv.second.first);
    }
  }
#endif  // MAMG_DIAG
  return MAMG_OK;
}

namespace {

__global__ __launch_bounds__(256) void pack2_kernel(int64_t n, const int64_t* __restrict__ idx,
                                                    const double* __restrict__ x,
                                                    double* __restrict__ buf) {
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (k < n) {
    const double2 v = reinterpret_cast<const double2*>(x)[idx[k]];
    reinterpret_cast<double2*>(buf)[k] = v;
  }
}

// ghost slots idx[k] of x (after the nloc owned nodes) <- buf pairs
__global__ __launch_bounds__(256) void unpack2_kernel(int64_t n, const int64_t* __restrict__ idx, int64_t nloc,
                                                      const double* __restrict__ buf, double* x) {
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (k < n) reinterpret_cast<double2*>(x)[nloc + idx[k]] = reinterpret_cast<const double2*>(buf)[k];
}

__global__ __launch_bounds__(256) void addidx2_kernel(int64_t n, const int64_t* __restrict__ idx,
                                                      const double* __restrict__ buf, double* x) {
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (k < n) {
    double2* px = reinterpret_cast<double2*>(x) + idx[k];
    const double2 a = *px, v = reinterpret_cast<const double2*>(buf)[k];
    *px = make_double2(a.x + v.x, a.y + v.y);
  }
}

// width 1 (scalar CSR hierarchies: a node is a dof).  The buffer side is
// contiguous in k, the indexed side one 8-byte access per thread.
__global__ __launch_bounds__(256) void pack1_kernel(int64_t n, const int64_t* __restrict__ idx,
                                                    const double* __restrict__ x,
                                                    double* __restrict__ buf) {
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (k < n) buf[k] = x[idx[k]];
}

__global__ __launch_bounds__(256) void unpack1_kernel(int64_t n, const int64_t* __restrict__ idx, int64_t nloc,
                                                      const double* __restrict__ buf, double* x) {
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (k < n) x[nloc + idx[k]] = buf[k];
}

// idx holds distinct owned rows (one peer's send list): no two threads share a target
__global__ __launch_bounds__(256) void addidx1_kernel(int64_t n, const int64_t* __restrict__ idx,
                                                      const double* __restrict__ buf, double* x) {
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (k < n) {
    const int64_t i = idx[k];
    x[i] = x[i] + buf[k];
  }
}

}  // namespace

// the exchange kernels of a handle with w dofs per node (2: the double2
// kernels of the nodal path, 1: the scalar ones)
void pack_w(int w, int64_t n, const int64_t* idx, const double* x, double* buf, hipStream_t s) {
  if (w == 2) pack2_kernel<<<nblocks(n), 256, 0, s>>>(n, idx, x, buf);
  else pack1_kernel<<<nblocks(n), 256, 0, s>>>(n, idx, x, buf);
}
void unpack_w(int w, int64_t n, const int64_t* idx, int64_t nloc, const double* buf, double* x, hipStream_t s) {
  if (w == 2) unpack2_kernel<<<nblocks(n), 256, 0, s>>>(n, idx, nloc, buf, x);
  else unpack1_kernel<<<nblocks(n), 256, 0, s>>>(n, idx, nloc, buf, x);
}
void addidx_w(int w, int64_t n, const int64_t* idx, const double* buf, double* x, hipStream_t s) {
  if (w == 2) addidx2_kernel<<<nblocks(n), 256, 0, s>>>(n, idx, buf, x);
  else addidx1_kernel<<<nblocks(n), 256, 0, s>>>(n, idx, buf, x);
}

void device_warm(void* stream) {
  warm_kernel<<<1, 64, 0, (hipStream_t)stream>>>();
  dist_layout_warm((hipStream_t)stream);
  (void)hipGetLastError();
}

__global__ __launch_bounds__(256) void vsum_kernel(int64_t n, const double* __restrict__ a,
                                                   double* acc) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) acc[i] = acc[i] + a[i];
}

void vsum(int64_t n, const double* a, double* acc, hipStream_t s) {
  vsum_kernel<<<nblocks(n), 256, 0, s>>>(n, a, acc);
}

}  // namespace mamg
