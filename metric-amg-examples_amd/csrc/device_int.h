// device_int.h -- what the translation units of the device apply path share
// (device.hip, dist_layout.hip, dist_apply.hip): the device structures, the
// two handles and the functions that cross files.  Included by those files
// only; device.h is the interface for the rest of the library (no HIP types).
#pragma once
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <memory>
#include <mutex>
#include <map>
#include <numeric>
#include <vector>

#include "device.h"
#include "dist.h"
#include "dmem.h"
#include "opts.h"
#include "rowstage.h"

namespace mamg {

#define HIPCHK(expr)                                                                 \
  do {                                                                               \
    hipError_t e_ = (expr);                                                          \
    if (e_ != hipSuccess) {                                                          \
      *err = std::string(#expr) + ": " + hipGetErrorString(e_);                      \
      return MAMG_ERR_HIP;                                                           \
    }                                                                                \
  } while (0)

// epilogues: y = s | y = y0 + s | r = b - s | x' = x + w (b - s) (point) |
// x' = x + W_I (b_I - s_I) (2x2 block, BSR only) |
// z = x1_I + W_I r1_I + s_I with s = K e, K = P - W (A P) (BSR only: the
// prolongation fused with the first post sweep through one operator)
enum Epi { EPI_Y = 0, EPI_YADD = 1, EPI_RESID = 2, EPI_JACOBI = 3, EPI_BJAC = 4, EPI_KPOST = 5, EPI_YBD = 6,
           EPI_PSM = 7 };
// EPI_PSM (rowdict2_kernel only): out = y_I + x_I - Wp[type of row I] s_I, the
// smoothed prolongation u = x1 + (I - w D_B^-1 A)(T e) with x = T e, y = x1
// and W the per-type table w D_B^-1
// EPI_YBD (bsr2_kernel only): out = A x as EPI_Y, and the next level's first
// sweep from x = 0 in the same pass, y <- W out (the restriction b_c = R r
// writing x1_c = W_c b_c: one launch and one b_c read fewer per coarse level;
// the same two products as bd2_kernel, so the same bits)

// ---- run-time value -> template argument (the launch ladder, device.hip).
// Each helper hands f a std::integral_constant / std::bool_constant / TypeC
// chosen by a run-time value, so a kernel family's launch statement is
// written once, inside a generic lambda.  The mappings are checked below: a
// wrong one fails the build.
// v if it is one of Vs, else D
template <int D, class F>
constexpr decltype(auto) with_int(int, F&& f) { return f(std::integral_constant<int, D>{}); }
template <int D, int V, int... Vs, class F>
constexpr decltype(auto) with_int(int v, F&& f) {
  if (v == V) return f(std::integral_constant<int, V>{});
  return with_int<D, Vs...>(v, f);
}
// lanes of a lane-group kernel (DCsr / DBsr::lanes): 2, 4, 8, 16, 32, anything else 64
template <class F>
constexpr decltype(auto) with_lanes(int lanes, F&& f) { return with_int<64, 2, 4, 8, 16, 32>(lanes, f); }
// lanes per row of the multi-lane SELL kernel (DBsr::lpr): 2, 4, 8, anything else 16
template <class F>
constexpr decltype(auto) with_lpr(int lpr, F&& f) { return with_int<16, 2, 4, 8>(lpr, f); }
// the epilogue if it is one of Es, else Default
template <int Default, int... Es, class F>
constexpr decltype(auto) with_epi(int epi, F&& f) { return with_int<Default, Es...>(epi, f); }
// f(std::bool_constant<b>...)
template <bool... Bs, class F>
constexpr decltype(auto) with_bools(F&& f) { return f(std::bool_constant<Bs>{}...); }
template <bool... Bs, class F, class... Rest>
constexpr decltype(auto) with_bools(F&& f, bool b, Rest... rest) {
  if (b) return with_bools<Bs..., true>(f, rest...);
  return with_bools<Bs..., false>(f, rest...);
}
// the stored value type of an operator (DBsr::f32)
template <class T> struct TypeC { using type = T; };
template <class F>
constexpr decltype(auto) with_value_type(bool f32, F&& f) {
  if (f32) return f(TypeC<float>{});
  return f(TypeC<double>{});
}

struct DispatchProbe {   // what a helper handed over, as a number
  template <class C> constexpr int operator()(C) const { return C::value; }
  template <class A, class B> constexpr int operator()(A, B) const { return 2 * A::value + B::value; }
  template <class T> constexpr int operator()(TypeC<T>) const { return (int)sizeof(T); }
};
static_assert(with_lanes(2, DispatchProbe{}) == 2 && with_lanes(4, DispatchProbe{}) == 4 &&
              with_lanes(8, DispatchProbe{}) == 8 && with_lanes(16, DispatchProbe{}) == 16 &&
              with_lanes(32, DispatchProbe{}) == 32 && with_lanes(64, DispatchProbe{}) == 64 &&
              with_lanes(3, DispatchProbe{}) == 64 && with_lanes(0, DispatchProbe{}) == 64, "with_lanes");
static_assert(with_lpr(2, DispatchProbe{}) == 2 && with_lpr(4, DispatchProbe{}) == 4 &&
              with_lpr(8, DispatchProbe{}) == 8 && with_lpr(16, DispatchProbe{}) == 16 &&
              with_lpr(5, DispatchProbe{}) == 16 && with_lpr(1, DispatchProbe{}) == 16, "with_lpr");
static_assert(with_epi<EPI_JACOBI, EPI_Y, EPI_YADD, EPI_RESID>(EPI_YADD, DispatchProbe{}) == EPI_YADD &&
              with_epi<EPI_JACOBI, EPI_Y, EPI_YADD, EPI_RESID>(EPI_KPOST, DispatchProbe{}) == EPI_JACOBI &&
              with_epi<EPI_BJAC, EPI_Y, EPI_KPOST>(EPI_KPOST, DispatchProbe{}) == EPI_KPOST &&
              with_epi<EPI_BJAC, EPI_Y, EPI_KPOST>(EPI_YBD, DispatchProbe{}) == EPI_BJAC, "with_epi");
static_assert(with_bools(DispatchProbe{}, true) == 1 && with_bools(DispatchProbe{}, false) == 0 &&
              with_bools(DispatchProbe{}, true, false) == 2 && with_bools(DispatchProbe{}, false, true) == 1 &&
              with_bools(DispatchProbe{}, true, true) == 3, "with_bools keeps the order of its arguments");
static_assert(with_value_type(true, DispatchProbe{}) == 4 && with_value_type(false, DispatchProbe{}) == 8,
              "with_value_type");

typedef double dv4 __attribute__((ext_vector_type(4)));
typedef double dv2 __attribute__((ext_vector_type(2)));

constexpr int SCALE_BLOCKS = 256;   // partial-sum blocks of the coarse-scaling dots

// nonlinear AMLI (K-cycle) work space of a Krylov level, DLevel::kpart: the
// stored d_i = <p_i, q_i> (KP_D), OP_KDOT's block partials of <z, q_i>, slot
// [KP_DOT + i * SCALE_BLOCKS + block], and OP_KORTH's block partials of
// <p_j, q_j> and <p_j, r>, interleaved from KP_PQ
constexpr int KP_D = 0;
constexpr int KP_DOT = 8;
constexpr int KP_PQ = KP_DOT + (MAMG_NL_AMLI_MAX - 1) * SCALE_BLOCKS;
constexpr int KP_SIZE = KP_PQ + 2 * SCALE_BLOCKS;

// partial-sum blocks of the PCG dots
constexpr int DOT_BLOCKS = 1024;

// ---- device-resident PCG state (dev_pcg): the scalars of cbc.block's
// ConjGrad live in HBM, so an iteration is one replayable hipGraph and the
// host only polls the state one iteration behind the GPU
struct PcgState {
  double rz, dq, alpha, beta, tol;
  int it, maxiter, active, run, status;   // status: PCG_* below
};
enum { PCG_RUNNING = 0, PCG_STOPPED = 1, PCG_DQ_ZERO = 2, PCG_RZ_NEG = 3, PCG_NOT_POS = 4 };

// ---- the same loop on N row-partitioned ranks (dist_pcg).  A
// rank's dot is its block partials summed in a fixed order into ONE double,
// written to slot [rank] of a P-vector whose other slots are zero; the
// all-reduce of the P-vector only ever adds zeros to it (exact), so every
// rank and every backend reads the same P doubles, and the alpha / beta
// kernels add them in rank order: the same bits everywhere, whatever the
// reduction tree.  rr / thr: ||r||^2 and stop_type 1's threshold tol ||b||.
struct DPcgState {
  double rz, dq, alpha, beta, tol, rr, thr;
  int it, maxiter, active, run, status, stop;
};

// what the distributed PCG ops of one (x, maxiter, stop_type) plan work on
// (device pointers; the struct itself lives on the host, owned by the plan)
struct DPcgCtx {
  DPcgState* st = nullptr;
  int64_t n = 0;                  // w * nloc owned entries
  int P = 1, rank = 0, stop = 0;
  double *x = nullptr, *r = nullptr, *z = nullptr, *d = nullptr, *q = nullptr;
  double* part = nullptr;         // 3 * DOT_BLOCKS block partials (dot 0, ||r||^2, ||b||^2)
  double* pv = nullptr;           // 3 P-vectors
  double *res = nullptr, *rn = nullptr, *al = nullptr, *be = nullptr;   // histories
  // the solve in flight (start-up ops only; the iteration reads none of them)
  const double* b = nullptr;
  double tol = 0.0;
  int relconv = 0, maxiter = 0;
};

// the coarse tail's ops (tail_kernel, kernels.hip; planned in cycle.hip)
enum TKind { T_BSR = 0, T_BD = 1, T_GEMV = 2, T_AXPY = 3, T_ZERO = 4, T_GS = 5, T_DOT2 = 6, T_CSCALE = 7,
             T_COPY = 8, T_RLOAD = 9,
             // nonlinear AMLI (mamg_set_kcycle_tail): kdot_kernel / korth_kernel / kupd_kernel as one workgroup,
             // step r0 of r1 on a Krylov level whose vectors the op names through a side table (ptr, KT_*)
             T_KDOT = 10, T_KORTH = 11, T_KUPD = 12 };
// A K op's vector operands: one table of tagged addresses per (program, Krylov
// level), in the program's allocation behind the ops; TOp::ptr points at it
// (TOp::nb: its index while the program is planned).  A step names up to
// twelve vectors, more than a TOp has vector fields, and a wider descriptor
// would cost every op of every program.
enum KTab { KT_R = 0, KT_Z = 1, KT_W = 2, KT_B = 3, KT_X = 4, KT_PART = 5, KT_P = 6, KT_Q = KT_P + MAMG_NL_AMLI_MAX,
            KT_SIZE = KT_Q + MAMG_NL_AMLI_MAX };
struct KTable { const double* v[KT_SIZE]; };
// LDS residency (tail_lds_plan): the program itself and every work vector of
// the tail levels live in the workgroup's LDS for the whole launch; a vector
// field of a TOp then holds (byte offset in the dynamic LDS) | 1 instead of a
// global pointer (doubles are 8-aligned, so bit 0 tags it), resolved per op.
// T_COPY ops at the ends move the vectors read before written in, and the
// written ones out.  The colour steps' dependent chain becomes LDS op
// descriptor (scalar loads) -> global (L2) row pointers, columns, values ->
// LDS x gathers.
// Register residency (tail_kernel RES, tail_res_plan): the rows of the tail
// levels' operators are spread over the workgroup's threads, one row per
// thread, and held in registers for the whole launch (T_RLOAD ops at the
// start load them).  An op with res = 1 on such a matrix: thread t computes
// row t - rbase if that lies in the op's (compact) row range [r0, r1), from
// registers; ridx maps compact rows to the matrix's rows (a GS layout pads
// each colour to whole 64-row slices).  A colour step is then LDS descriptor
// -> LDS x gathers -> LDS store, with no global round trip.
struct TOp {
  int kind = 0, epi = 0, vl = 1, sym = 0, res = 0, rbase = 0;
  int64_t n = 0, r0 = 0, r1 = 0, nb = 0;
  const int64_t* ptr = nullptr;
  const int32_t* col = nullptr;
  const double* val = nullptr;
  const double *x = nullptr, *y = nullptr, *b = nullptr, *w = nullptr;
  const dv4* W = nullptr;
  double* out = nullptr;
  const int32_t* perm = nullptr;
  double* part = nullptr;
  const int32_t* ridx = nullptr;
};

// nodes of a patch at most (a row of A_0's node pattern; build_patches checks)
constexpr int PATCH_MAX_NODES = 16;

inline unsigned nblocks(int64_t work) { return (unsigned)((work + 255) / 256); }

// ---------------------------------------------------------------------------
// device structures
// ---------------------------------------------------------------------------
struct DCsr {
  int64_t n = 0, m = 0, nnz = 0;
  int64_t* ptr = nullptr;
  int32_t* col = nullptr;
  double* val = nullptr;
  int lanes = 8;
};

struct DBsr {              // 2x2 blocks, node-major
  int64_t nr = 0, nc = 0, nb = 0;
  int64_t* ptr = nullptr;
  int32_t* col = nullptr;
  double* val = nullptr;   // 4 doubles per block, 3 if sym
  int lanes = 8;
  bool sym = false;        // symmetric-block format (every block has (0,1) == (1,0))
  // SELL-64 storage (sell == true): ptr unused; soff per slice, meta per row,
  // col / val hold nbs (>= nb, padded) slots
  bool sell = false;
  int split = 0;            // SELL general blocks as two 16-byte streams (1: two global streams,
                            // 2: split inside each slot row; sell2_kernel / msell_kernel SPL)
  int lpr = 1;              // SELL lanes per row: 1 sell2_kernel, > 1 msell_kernel
  int64_t nbs = 0;
  int64_t* soff = nullptr;
  int32_t* meta = nullptr;
  int32_t* perm = nullptr;  // SELL-C-sigma: row held by each slot (merged matrices)
  bool lsort = false;       // SELL rows sorted by length inside each slice: meta is per slot,
                            // length | (row - slice start) << 16 (sort_sell_slices)
  // SELL columns as 16-bit offsets from a per-slice base (level-0 K, round
  // 6: compress_sell_cols); col is kept for the layout code, the kernel reads
  // col16 + cbase
  uint16_t* col16 = nullptr;
  int32_t* cbase = nullptr;
  int kvar = 0;             // a K's kernel variant (launch_kvariant; 0 in the product build)
  // half-symmetric ELL-64 (half == true, A symmetric bitwise): col / val hold
  // the upper part I <= J < nr, hwu slots per row; lptr holds,
  // per lower entry J < I, the slot of the mirror block (J, I) in the upper
  // part, hwl slots per row; ghost columns (>= nr, multi-GPU rank-local A)
  // in their own SELL-64 part (gsoff per slice, zero width where a slice has
  // none); meta = upper length | lower length << 8 | ghost length << 16
  bool half = false;
  int hwu = 0, hwl = 0;
  int64_t nlo = 0;          // lower entries (nb = upper + ghost entries + nlo)
  int32_t* lptr = nullptr;
  int64_t ngs = 0;          // ghost-part slots (0: no ghost part)
  int64_t* gsoff = nullptr;
  int32_t* gcol = nullptr;
  double* gval = nullptr;
  // band schedule of the half-symmetric kernel (full-range launches):
  // workgroup b processes 256-row block sched[b] (nullptr: row_block order)
  int32_t* sched = nullptr;
  int64_t nsched = 0;
  int64_t band_stride = 0;  // plane stride S in rows (0: no band schedule)
  // band schedule of one sub-range launch [sr0, sr1) (multi-GPU interior rows)
  int32_t* sched_r = nullptr;
  int64_t nsched_r = 0, sr0 = 0, sr1 = 0;
  // plane-band schedule of a lane-group BSR launch with rsched_vl lanes per
  // row (the level-0 restriction): workgroup b processes row block rsched[b]
  int32_t* rsched = nullptr;
  int64_t nrsched = 0;
  int rsched_vl = 0;
  // values stored fp32 (dev_set_cycle_storage): val then points to a float
  // array of the same element layout, read by the kernels' float side
  bool f32 = false;
  // row-pattern dictionary (rowdict == true, a level-0 A whose node rows
  // repeat; rowdict2_kernel): rcode holds one row-type code per node row;
  // type t has rlen[t] entries, entry j at slot t rw + j of rdelta (column -
  // row, in the row's stored column order) and of val (nbs = types x rw
  // slots of the SYM or general block layout; padding slots are zero).  ptr,
  // col, meta are unused; sched / band_stride as for the half layout.
  bool rowdict = false;
  uint16_t* rcode = nullptr;
  int32_t* rlen = nullptr;
  int32_t* rdelta = nullptr;
  int rw = 0, rtypes = 0;
  // what the builder decided (mamg_test.h mamg_rowdict_info, RD_*)
  int64_t rdinfo[5] = {0, 0, 0, 0, 0};
};

// mamg_rowdict_info's values and refusal reasons (include/mamg_test.h)
enum RowdictInfo { RD_TAKEN = 0, RD_REASON, RD_TYPES, RD_MAXLEN, RD_TABLE_BYTES, RD_INFO_N };
enum RowdictReason { RDR_NONE = 0, RDR_TYPES = 1, RDR_LENGTH = 2, RDR_VERIFY = 3, RDR_THRESHOLD = 4, RDR_NOT_SQUARE = 5,
                     RDR_TABLE = 6, RDR_NOT_TRIED = 7 };

// mamg_post_mf_info's values and refusal reasons (include/mamg_test.h)
enum PostMfInfo { PM_TAKEN = 0, PM_REASON, PM_TABLE_BYTES, PM_INFO_N };
enum PostMfReason { PMR_NONE = 0, PMR_OFF = 1, PMR_THRESHOLD = 2, PMR_NO_DICT = 3, PMR_NOT_SA = 4, PMR_SMOOTHER = 5,
                    PMR_NO_FUSION = 6, PMR_NOT_TRIED = 7, PMR_DIAG = 8 };

struct DLevel {
  int64_t n = 0;           // dofs
  bool coarsest = false;
  DCsr A, P, R, WB;        // CSR layout
  DBsr Ab, Pb, Rb;         // BSR2 layout
  DBsr PAb;                // BSR2 post fusion: merged [P | AP] rows (ptr: 2 nr + 1)
  DBsr KPb;                // BSR2 post fusion: K = P - W (A P), one operator (default)
  // fp32 cycle storage (dev_set_cycle_storage), level 0 only: A_0 as the cycle
  // reads it -- Ab's layout with fp32 copies of its value arrays (Ac.f32), the
  // index arrays shared; Ab itself stays fp64 for the Krylov operator.  On the
  // other narrowed levels Ab's values are replaced in place.
  DBsr Ac;
  int storage = 0;         // mamg_level_storage bits: 1 A, 2 K / P, 4 R stored fp32
  // matrix-free post step of level 0 on the row dictionary (post_mf == true,
  // DESIGN.md section 4.9): P e = (I - w D_B^-1 A)(T e) without a stored K or
  // P.  mf_agg: the aggregate of each node as int32 (-1 isolated: a zero row
  // of T); mf_wp: w D_B^-1 per row type of Ab's dictionary (fp64 always).
  bool post_mf = false;
  int32_t* mf_agg = nullptr;
  dv4* mf_wp = nullptr;
  int64_t mfinfo[3] = {0, 7, 0};   // mamg_post_mf_info, PM_* (not tried until the builder ran)
  dv4* Wd = nullptr;       // BSR2 layout: 2x2 smoother block per node
  double* winv = nullptr;
  // SMOOTHER_POLY: the step smoothers w_k W, k = 1..m (BSR2: Wk; CSR: WBk
  // sharing WB's pattern, or winvk); empty for the Jacobi smoothers
  std::vector<dv4*> Wk;
  std::vector<DCsr> WBk;
  std::vector<double*> winvk;
  double* Ainv = nullptr;
  double *b = nullptr, *x = nullptr, *t = nullptr, *t2 = nullptr, *r = nullptr,
         *c = nullptr, *e = nullptr;
  // multicolour Gauss-Seidel (SMOOTHER_SGS / SMOOTHER_GS, BSR2 layout): A_l's
  // node rows permuted colour by colour (Gb, lane groups), the node of each
  // permuted row (gperm), the unscaled smoother-block inverses in that order
  // (Gd), colour c = permuted rows [gcs[c], gcs[c + 1])
  DBsr Gb;
  int32_t* gperm = nullptr;
  dv4* Gd = nullptr;
  std::vector<int64_t> gcs, gbk;     // colour row starts / block starts (+ end)
  // point-wise multicolour GS (SMOOTHER_GS_POINT / SGS_POINT, CSR layout):
  // A_l's rows permuted colour by colour (Gc; gperm = the row of each
  // permuted row, gcs / gbk as above, unpadded), 1 / a_ii in that order
  // (gdinv), the colour row starts on the device (gcs_d: the one-launch
  // smoothing call of a small level, gsmall)
  DCsr Gc;
  double* gdinv = nullptr;
  int64_t* gcs_d = nullptr;
  bool gsmall = false;
  // level-0 node-patch Schwarz (Schwarz_type PATCHES): A_0 as plain BSR2 in
  // node order (Sptr, Scol, Sval: the patch rows), the patch centres colour by
  // colour (pperm), colour c = patches [pcs[c], pcs[c + 1]), the packed upper
  // triangles of the patch inverses (pu, stride pus doubles per patch)
  int64_t* Sptr = nullptr;
  int32_t* Scol = nullptr;
  dv4* Sval = nullptr;
  int64_t Snb = 0;
  int32_t* pperm = nullptr;
  double* pu = nullptr;
  int64_t pus = 0;
  std::vector<int64_t> pcs;
  // level-0 seed-ring Schwarz (Schwarz_type RINGS): the blocks colour by
  // colour (colour c = blocks [rcs[c], rcs[c + 1])), block k's members as
  // node-interleaved dof indices 2 I + f at rmem[rmo[k] .. rmo[k + 1]), its
  // Gauss-Jordan inverse transposed (column-major d x d) at rinv + rio[k];
  // A_0's rows in Sptr / Scol / Sval; the rest's GS in Gb / gperm / Gd / gcs
  // (covered dofs masked out of Gd)
  int64_t* rmo = nullptr;
  int32_t* rmem = nullptr;
  int64_t* rio = nullptr;
  double* rinv = nullptr;
  std::vector<int64_t> rcs;
  int64_t rnm = 0;          // members of all blocks
  double rinv_n = 0.0;      // inverse entries of all blocks
  // ... on the CSR layout (scalar systems, point smoothers): rmem holds plain
  // dof indices, the member rows are A's, the rest's point-wise GS over the
  // uncovered rows is in Gc / gperm / gdinv / gcs; per colour c the members,
  // inverse entries and member-row entries of its blocks, as prefix sums
  // (the byte count of a colour step)
  std::vector<int64_t> rcm, rci, rce;
  // coarse-grid correction scaling of the correction computed ON this level:
  // q = A_l e, partial sums of <b, e>, <q, e>
  double* q = nullptr;
  double* part2 = nullptr;
  // nonlinear AMLI (K-cycle handles, levels 1 .. coarsest - 1): the inner
  // flexible CG's residual, preconditioned residual and A z, its amli_degree
  // directions p_i and q_i = A p_i, and the scalar / partials block (KP_*).
  // The level's cycle scribbles on t / t2 / r / c / e / q: these are their own.
  double *kr = nullptr, *kz = nullptr, *kw = nullptr;
  double *kp[MAMG_NL_AMLI_MAX] = {}, *kq[MAMG_NL_AMLI_MAX] = {};
  double* kpart = nullptr;
};

enum OpKind { OP_CSR = 0, OP_SCALE = 1, OP_GEMV = 2, OP_AXPY = 3, OP_BSR = 4, OP_BD = 5, OP_POST = 6, OP_ILV = 7,
              OP_GS = 8, OP_ZERO = 9, OP_DOT2 = 10, OP_CSCALE = 11, OP_PATCH = 12, OP_TAIL = 13, OP_RING = 14,
              OP_CGS = 15,     // point-wise GS, one colour of a CSR level (csr_gs_kernel)
              OP_CGSF = 16,    // point-wise GS, a small level's whole smoothing call (csr_gs_small_kernel)
              OP_CRING = 17,   // one colour of a seed-ring sweep on the CSR layout (ring_csr_kernel)
              OP_COPY = 18,    // out = x (n doubles): a rank's plain slice into its [owned | ghost] buffer
              // the distributed PCG's kernels on Op::pcg (dpcg_*_kernel)
              OP_PDOT = 19,    // block partials of <x, y> over the owned entries
              OP_PSLOT = 20,   // n dots' partials -> slot [rank] of their P-vectors
              OP_PR0 = 21,     // r = b - q (start-up)
              OP_PINIT = 22, OP_PALPHA = 23, OP_PXR = 24, OP_PBETA = 25, OP_PD = 26,
              // nonlinear AMLI: step r0 of r1 of the inner flexible CG on level Op::lev (kdot_kernel,
              // korth_kernel, kupd_kernel)
              OP_KDOT = 27,    // block partials of <z, q_i>, i < r0
              OP_KORTH = 28,   // beta_i from them; p_j, q_j; block partials of <p_j, q_j>, <p_j, r>
              OP_KUPD = 29,    // d_j stored, alpha; e (+)= alpha p_j, r -= alpha q_j
              OP_TGATHER = 30 };   // out(I) = perm[I] < 0 ? 0 : x(perm[I]), n nodes: y = T e (tgather_kernel)
// kernel classes (kernel_ms / class_bytes slots)
enum Cls {
  C_L0_RESID = 0,   // dominant: r = b - A0 x (once per apply)
  C_L0_SMOOTH = 1,  // post-smooth SpMV on A0 (fused Jacobi / block Jacobi)
  C_L0_WB = 2,      // level-0 smoother application outside an SpMV
  C_L0_R = 3,       // level-0 restriction
  C_L0_P = 4,       // level-0 prolongation
  C_COARSE = 5,     // all SpMV-class launches on levels >= 1
  C_DENSE = 6,      // coarsest dense solve
  C_MISC = 7,       // W-cycle / maxit corrections
  C_COMM = 8,       // multi-GPU: halo pack/unpack + RCCL exchanges
  NCLS = 8
};

struct Op {
  int kind = OP_CSR, epi = EPI_Y, cls = 0, tag = 1;
  const DCsr* M = nullptr;
  const DBsr* Mb = nullptr;
  int64_t n = 0;
  const double *x = nullptr, *y = nullptr, *b = nullptr, *w = nullptr;
  const dv4* W = nullptr;
  double* out = nullptr;
  int64_t xs = 0, bs = 0, os = 0;   // BSR2 field strides (0 = node-major)
  bool xfm = false;
  int remap = 0;                    // XCD-contiguous row order (restriction ops)
  int64_t r0 = 0, r1 = -1;          // row range [r0, r1) (half-symmetric ops, GS colours; r1 < 0: all rows)
  const int32_t* perm = nullptr;    // GS: node of each permuted row
  double* part = nullptr;           // DOT2 / CSCALE partial sums
  const struct DLevel* lev = nullptr;   // PATCH: the level's patch data
  const TOp* prog = nullptr;        // TAIL: the device op list (n ops)
  int tail_pl = -1;                 // TAIL: the program's LDS byte offset (-1: read from global memory)
  const DPcgCtx* pcg = nullptr;     // OP_P*: the distributed PCG plan's pointers
  double bytes = 0.0;
};

inline int remap_of(const Op& o) { return o.remap; }

// a captured stream as graph + exec (capture_graph, device.hip), owned by
// whoever holds it: drop() destroys both
struct CapturedGraph {
  hipGraph_t graph = nullptr;
  hipGraphExec_t exec = nullptr;
  void drop() {
    if (exec) (void)hipGraphExecDestroy(exec);
    if (graph) (void)hipGraphDestroy(graph);
    exec = nullptr; graph = nullptr;
  }
};

// `body` captured on *cap (created on first use) and instantiated: *out holds
// graph and exec, or nothing is left behind -- on every failure what was made
// is destroyed and the sticky HIP error cleared.  body's own code is returned
// as it is; a HIP failure is MAMG_ERR_HIP with "stream capture of the <what>:
// ..." or "hipGraphInstantiate of the <what>: ...".  The capture mutex is held
// from before the begin until after the instantiate.
int capture_graph(hipStream_t* cap, const std::function<int()>& body, const char* what, CapturedGraph* out,
                  std::string* err);

// A handle's apply graphs, one per (r, z) pair, at most 16: the oldest goes
// once every launch on the handle has finished (`last`, HandleOrder below).
struct GraphCache {
  struct Entry { const double* r; double* z; CapturedGraph g; };
  std::vector<Entry> v;
  // the exec for (r, z): cached, or captured now by capture(CapturedGraph*)
  template <class Capture>
  int get(const double* r, double* z, hipEvent_t last, Capture&& capture, hipGraphExec_t* exec, std::string* err) {
    for (Entry& e : v)
      if (e.r == r && e.z == z) { *exec = e.g.exec; return MAMG_OK; }
    if (v.size() >= 16) {   // evict the oldest, after every launch on the handle finished
      if (last) HIPCHK(hipEventSynchronize(last));
      v.front().g.drop();
      v.erase(v.begin());
    }
    Entry e{r, z, {}};
    const int rc = capture(&e.g);
    if (rc) return rc;
    v.push_back(e);
    *exec = e.g.exec;
    return MAMG_OK;
  }
  void clear() {
    for (Entry& e : v) e.g.drop();
    v.clear();
  }
};

// one PCG iteration as a graph (none: the iteration runs eagerly), with the
// device histories of a solve and the two events the host polls behind
struct IterGraph : CapturedGraph {
  double* hist = nullptr;
  hipEvent_t ev[2] = {nullptr, nullptr};
  int alloc(size_t hist_doubles, std::string* err);   // hist and ev; nothing left behind on failure
  void release() {
    drop();
    for (hipEvent_t& e : ev) { if (e) (void)hipEventDestroy(e); e = nullptr; }
    if (hist) (void)raw_free(hist);
    hist = nullptr;
  }
};
// a handle's iteration graphs or plans, all of them (destructor, set_cycle_storage)
template <class V>
void release_all(V* v) {
  for (auto& q : *v) q.release();
  v->clear();
}

// the iteration graph of a solution vector x and a history length (dev_pcg):
// reused by later solves into the same x (drivers, gamma sweeps); hist holds
// residuals[maxiter + 1], alphas[maxiter], betas[maxiter]
struct PcgGraph : IterGraph {
  double* x = nullptr;
  int maxiter = 0;
};

// The memory side of a handle, single-GPU or rank: all that dalloc and the
// layout builders need of either.  The handle's destructor frees allocs.
struct HandleMem {
  const Switches sw;               // the switches the handle was built with (opts.h)
  std::vector<void*> allocs;
  char* arena = nullptr;           // pre-reserved HBM, bump-allocated (dev_prereserve)
  size_t arena_left = 0;
};

// The ordering side of a handle, single-GPU or rank.  Every piece of work on
// the handle's scratch, ghost, send, receive and level work buffers (apply,
// host apply, spmv, PCG, timing) makes its stream wait for the handle's last
// mark, whatever stream that was recorded on, and leaves its own mark behind:
// work on one handle is serialized across streams (include/mamg.h).  A base
// beside HandleMem and not part of it: the layout builders take a HandleMem
// and order nothing, they run on the null stream before the handle's first
// mark.  The handle's destructor owns `last` (a rank waits for it first).
struct HandleOrder {
  hipEvent_t last = nullptr;
  int wait(hipStream_t s, std::string* err) {
    if (last) HIPCHK(hipStreamWaitEvent(s, last, 0));   // never marked: nothing to wait for
    return MAMG_OK;
  }
  int mark(hipStream_t s, std::string* err) {
    if (!last) HIPCHK(hipEventCreateWithFlags(&last, hipEventDisableTiming));
    HIPCHK(hipEventRecord(last, s));
    return MAMG_OK;
  }
};

// `reps` runs of a list of ops on one stream between two events, with an
// event pair around every op of the level-0 residual and smoothing classes
// (mode 0) or around every op (mode 1).  The object owns the events: they go
// with it on every path.
struct TimedRun {
  std::vector<int> inst;           // the instrumented ops
  std::vector<hipEvent_t> ev;      // [0], [1]: the whole run; then per rep, per instrumented op, (start, end)
  ~TimedRun() {
    for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e);
  }
  int create(size_t n, std::string* err) {
    ev.assign(n, nullptr);
    for (auto& e : ev) HIPCHK(hipEventCreate(&e));
    return MAMG_OK;
  }
  // cls(k): the class of op k; op(k): queue it on s (the project's code);
  // queued(): between the last record and the host's wait (may be empty).
  // ms: per rep; kernel_ms (16 slots, may be null): per class and rep
  int run(size_t nops, const std::function<int(size_t)>& cls, const std::function<int(size_t)>& op, int reps, int mode,
          hipStream_t s, const std::function<int()>& queued, double* ms, double* kernel_ms, std::string* err);
  // the time of instrumented op ii in rep rp
  int op_ms(int rp, size_t ii, float* t, std::string* err) const {
    const size_t q = 2 + 2 * ((size_t)rp * inst.size() + ii);
    HIPCHK(hipEventElapsedTime(t, ev[q], ev[q + 1]));
    return MAMG_OK;
  }
};

// The end of a PCG solve, single-GPU or distributed, from the final state's
// status and iteration count: "Matrix is not positive" (no iteration ran), or
// the device histories (rn: nullptr without stop_type 1's ||r||) copied out,
// niters set, and the two breakdown messages.
struct PcgHist { const double *res, *rn, *al, *be; };
int pcg_finish(int status, int it, const PcgHist& d, double* residuals, double* rnorms, double* alphas,
               double* betas, int* niters, std::string* err);

struct DeviceHandle : HandleMem, HandleOrder {
  mamg_params p;
  explicit DeviceHandle(const Switches& s) : HandleMem{s, {}, nullptr, 0} {}
  int device = 0;
  bool bsr = false;
  std::vector<DLevel> L;
  char* arena0 = nullptr;          // the reservation's range [arena0, arena1)
  char* arena1 = nullptr;
  hipStream_t cap = nullptr;
  GraphCache graphs;
  std::vector<PcgGraph> pcgs;
  // coarse tail (tail_kernel): first level run by it (0 = off) and the
  // device op lists built so far, one per (b, x) entry of that level
  int tail_level = 0;
  std::vector<double> kregion_ms;  // select_k_region: K ms per candidate region, the one kept
  int kregion_best = -1;
  struct TailProg {
    const double* b; double* x; TOp* prog; int n; double bytes; int64_t lds; bool xl; int prog_lds; bool res;
    bool kops;                     // it holds nonlinear AMLI steps (tail_kernel KOPS)
    std::vector<int64_t> info;     // what the planner decided (dev_tail_info; mamg_test.h mamg_tail_info)
  };
  mutable std::vector<TailProg> tails;
  mutable bool tail_refused = false;   // the last plan attempt met an op the tail cannot express (to_tail)
  bool kcycle_tail = false;            // nonlinear AMLI: the K ops run inside the tail (dev_set_kcycle_tail)
  double* hr = nullptr;            // host-apply staging (device)
  double* hz = nullptr;
  double *cr = nullptr, *cz = nullptr, *cd = nullptr, *cq = nullptr;  // PCG
  double* part = nullptr;
  double* dres = nullptr;
  double* hres = nullptr;          // pinned host scalar
  double apply_bytes = 0.0;
  double setup_ms[8] = {};         // GPU setup phase timings (dev_from_ghier)
  double layout_ms[4] = {};        // apply-layout phases: build, K region trials, re-homing, finish (LT_*)
  ~DeviceHandle() {
    if (last) (void)hipEventDestroy(last);
    graphs.clear();
    release_all(&pcgs);
    for (auto& t : tails) (void)raw_free(t.prog);
    for (void* a : allocs) (void)raw_free(a);
    if (hres) (void)hipHostFree(hres);
    if (cap) (void)hipStreamDestroy(cap);
  }
};

enum { LT_BUILD = 0, LT_KREGION = 1, LT_REHOME = 2, LT_FINISH = 3 };

// MAMG_POISON=1 (tests): every double array a handle or the layout builder
// allocates starts as NaN bytes instead of whatever the memory held, so a
// read of a value nothing wrote shows in the result (index arrays are left
// alone: a poisoned index would fault instead of showing)
template <class T>
void poison_doubles(const Switches& sw, T* p, size_t bytes) {
  if constexpr (std::is_same<T, double>::value) {
    if (sw.poison) (void)dev_memset(p, 0xff, bytes);
  }
}

// free a handle-owned (hipMalloc) array replaced during the upload, behind
// its last reader on the null stream (dmem.h ordered_free)
inline void drained_free(void* p) { ordered_free(p); }

// wait for the layout builder's queued work (all of it on the null stream)
inline hipError_t null_sync() { return hipStreamSynchronize(nullptr); }

// device allocation owned by a handle (single-GPU or multi-GPU: HandleMem)
template <class T>
int dalloc(HandleMem* h, T** p, int64_t count, std::string* err) {
  *p = nullptr;
  if (count <= 0) return MAMG_OK;
  const size_t bytes = ((size_t)count * sizeof(T) + 4095) & ~(size_t)4095;
  if (h->arena && bytes <= h->arena_left) {
    *p = (T*)h->arena;
    h->arena += bytes;
    h->arena_left -= bytes;
    poison_doubles(h->sw, *p, bytes);
    return MAMG_OK;
  }
  void* q = nullptr;
  // a very large long-lived array (the node patches' inverses: 63 GB at
  // nrefs=6) is placed after the idle setup cache is released, so it is not
  // laid out around the cached blocks (with them kept, the patch layout build
  // took 2.2-2.8 s instead of 0.68 s, BENCH_r05 / profiles/r05_bench_g.json)
  if ((size_t)count * sizeof(T) >= ((size_t)8 << 30)) tmp_trim();
  HIPCHK(dev_malloc(&q, (size_t)count * sizeof(T)));
  h->allocs.push_back(q);
  *p = (T*)q;
  poison_doubles(h->sw, *p, (size_t)count * sizeof(T));
  return MAMG_OK;
}

// raw device BSR2 (4 doubles per block); merged: ptr has 2 nr + 1 entries
struct TBsr {
  int64_t nr = 0, nc = 0, nb = 0;
  bool merged = false;
  int64_t* ptr = nullptr;
  int32_t* col = nullptr;
  dv4* val = nullptr;
};

// scoped temporaries of the layout builder, null-stream ordered (dmem.h):
// the layout kernels that read them are queued on the null stream, and a
// block handed out again is used only by work queued behind them
struct TmpPool {
  const Switches& sw;   // the owning handle's
  std::vector<void*> v;
  explicit TmpPool(const Switches& s) : sw(s) {}
  ~TmpPool() {
    for (void* p : v) tmp_free(p);
  }
  template <class T>
  int alloc(T** p, int64_t count, std::string* err) {
    void* q = nullptr;
    HIPCHK(tmp_malloc(&q, (size_t)std::max<int64_t>(count, 1) * sizeof(T)));
    v.push_back(q);
    *p = (T*)q;
    poison_doubles(sw, *p, (size_t)std::max<int64_t>(count, 1) * sizeof(T));
    return MAMG_OK;
  }
  void release(void* p) {
    for (auto& q : v)
      if (q == p) {
        tmp_free(q);
        q = nullptr;
      }
  }
};

// one BSR2 level from device-resident field-major CSRs (AP.n == 0: no fusion)
struct LevelSrc {
  DevMat A, P, AP, R;
  const double* W = nullptr;      // 4 nv node blocks (device)
  const double* Ainv = nullptr;   // coarsest: n x n dof order (device)
  const std::vector<int32_t>* seeds = nullptr;   // level 0, SCHWARZ_RINGS
  // level 0: the aggregate of each node (device, -1 isolated; nullptr: not
  // handed over) and w = sa_omega / rho_B of P = (I - w D_B^-1 A) T
  const int64_t* agg = nullptr;
  double w_sa = 0.0;
};

inline bool gs_smoother(const mamg_params& p) {
  return p.smoother == MAMG_SMOOTHER_SGS || p.smoother == MAMG_SMOOTHER_GS;
}

// smoothing step s of a sweep sequence: the Jacobi smoothers take W every
// step; SMOOTHER_POLY takes w_1 W .. w_m W before the coarse correction and
// w_m W .. w_1 W after it (mamg_oracle.Hierarchy.cycle), repeated per sweep
inline int step_index(int m, int s, bool pre) {
  const int k = s % m;
  return pre ? k : m - 1 - k;
}

inline bool patch_schwarz(const mamg_params& p) {
  return p.Schwarz_levels >= 1 && p.Schwarz_type == MAMG_SCHWARZ_PATCHES;
}

inline bool rings_schwarz(const mamg_params& p) {
  return p.Schwarz_levels >= 1 && p.Schwarz_type == MAMG_SCHWARZ_RINGS;
}

// one multicolour GS sweep (colours ascending if fwd, else descending) in place on x
template <class LV>
Op gs_op(const LV& L, int c, double* x, const double* b, int64_t bs, int cls) {
  Op o;
  o.kind = OP_GS; o.cls = cls; o.Mb = &L.Gb; o.perm = L.gperm; o.W = L.Gd;
  o.x = x; o.out = x; o.b = b; o.bs = bs;
  o.r0 = L.gcs[c]; o.r1 = L.gcs[c + 1]; o.n = o.r1 - o.r0;
  const double rows = (double)o.n, ncol = (double)(L.gcs.size() - 1);
  // blocks + pointers + perm + D + b + own x read/write + the gathered x
  // (every node's pair once per sweep, spread over the colours)
  o.bytes = (L.Gb.sym ? 28.0 : 36.0) * (double)(L.gbk[c + 1] - L.gbk[c]) + 8.0 * (rows + 1) + 4.0 * rows +
            32.0 * rows + 16.0 * rows + 32.0 * rows + 16.0 * (double)L.Gb.nc / ncol;
  return o;
}
// mamg_tail_info's values (include/mamg_test.h): the header, then (n, matrix in LDS) per T_GEMV
enum TailInfo { TI_PROGS = 0, TI_LEVEL, TI_OPS, TI_LDS, TI_XL, TI_RES, TI_PROG_LDS, TI_ROWS, TI_NOV, TI_VEC_LDS,
                TI_VEC_GLOBAL, TI_REFUSED, TI_GEMVS, TI_OPS_RES, TI_OPS_BSR, TI_MAX_VL, TI_REPLANNED, TI_OPS_K, TAIL_INFO_HEAD };

// stored values of an operator's main array (rehome_bsr's count)
inline int64_t value_count(const DBsr& M) {
  if (M.nr == 0 || !M.val) return 0;
  const int64_t slots = (M.sell || M.half || M.rowdict) ? M.nbs : M.nb;
  return slots * ((M.sym || M.half) ? 3 : 4);
}
// stored values of a half-symmetric operator's ghost part (gval: the diagonal
// pairs of its ngs slots, then their off-diagonals)
inline int64_t ghost_value_count(const DBsr& M) { return (M.half && M.gval) ? 3 * M.ngs : 0; }

// one value array to store fp32 (narrow_values)
struct NarrowJob {
  DBsr* src;        // the operator whose fp64 values are read
  DBsr* dst;        // the operator that reads the fp32 copy (src itself, or level 0's Ac)
  bool ghost;       // the half-symmetric ghost part (gval) instead of the main array
  float* val = nullptr;
  const double* from() const { return ghost ? src->gval : src->val; }
  int64_t count() const { return ghost ? ghost_value_count(*src) : value_count(*src); }
};

#define NCCLCHK(expr)                                                                \
  do {                                                                               \
    ncclResult_t r_ = (expr);                                                        \
    if (r_ != ncclSuccess) {                                                         \
      *err = std::string(#expr) + ": " + ncclGetErrorString(r_);                     \
      return MAMG_ERR_HIP;                                                           \
    }                                                                                \
  } while (0)

struct DDLevel {
  int64_t nv = 0, nloc = 0, ng = 0;
  bool replicated = false, coarsest = false;
  DBsr A, P, R;
  // fp32 cycle storage (dist_set_cycle_storage), level 0 only: A_loc as the
  // cycle reads it -- A's layout with fp32 copies of val and, half-symmetric,
  // gval (Ac.f32), the index arrays shared; A itself stays fp64 for the Krylov
  // operator (dspmv_ops).  On the other narrowed levels A's values are
  // replaced in place.
  DBsr Ac;
  int storage = 0;         // mamg_dist_level_storage bits: 1 A, 2 K / P, 4 R stored fp32
  // scalar (CSR) level: A_loc, P_loc, Rp_loc, on level 0 with seed blocks the
  // owned rows of WB (else the winv slice); POLY: the step smoothers w_k WB
  // (sharing WB's pattern) or w_k winv; vectors hold nloc + ng doubles
  DCsr cA, cP, cR, cWB;
  std::vector<DCsr> cWBk;
  double* winv = nullptr;
  std::vector<double*> winvk;
  double* gb = nullptr;    // level 0 with WB: b over [owned | ghost] (X = WB_loc b reads b's ghosts)
  DBsr PA;                 // post fusion: merged [P_loc | AP_loc]
  DBsr K;                  // post fusion: K_loc = P_loc - W (AP)_loc (default)
  dv4* W = nullptr;
  std::vector<dv4*> Wk;    // SMOOTHER_POLY step smoothers w_k W (empty: Jacobi)
  double* Ainv = nullptr;
  double *b = nullptr, *x = nullptr, *t = nullptr, *t2 = nullptr, *r = nullptr;
  double *c = nullptr, *e = nullptr;     // W-cycle: second visit's right-hand side / correction
  double *q = nullptr, *part2 = nullptr; // coarse scaling of this level's correction: A e, dot partials
  double* spx = nullptr;   // level 0: [owned | ghost] operand of the standalone SpMV
  int64_t ib0 = 0, ib1 = 0;  // longest run of A_loc rows without ghost columns
  int64_t kb0 = 0, kb1 = 0;  // the same for K (coarse ghost columns), bounds multiples of K_ROWS_ALIGN or nloc
  int64_t* send_idx = nullptr;
  double *sendbuf = nullptr, *recvbuf = nullptr;
  std::vector<int64_t> send_off, ghost_off;
  // multicolour GS (SMOOTHER_GS / SGS): the owned rows permuted colour by
  // colour (gs_layout; the level's global colouring, so every rank has the
  // same colours), and each colour's halo: its send nodes and ghost slots per
  // peer, offsets cs_off / cg_off[c (P + 1) + q]
  DBsr Gb;
  int32_t* gperm = nullptr;
  dv4* Gd = nullptr;
  std::vector<int64_t> gcs, gbk;
  int64_t *csend_idx = nullptr, *cghost_idx = nullptr;
  std::vector<int64_t> cs_off, cg_off;
  // level-0 node-patch Schwarz on N ranks (dist_patches): the ghost region is
  // the 3-hop ball of the owned nodes; the rank computes every patch centred
  // within 1 hop of its nodes (pl: the patch rows of the nodes within 2 hops,
  // columns local in the global column order, centres colour by colour,
  // inverses); cs_off / cg_off above hold each colour's halo of the nodes
  // its patches write; pb = b interleaved over [owned | ghost]
  bool patches = false;
  DLevel pl;
  int32_t* Sgcol = nullptr;
  double* pb = nullptr;
  // level-0 seed-ring Schwarz on N ranks (dist_rings): the rank's blocks
  // (rl: rcs, rmo, rmem, rio, rinv; the block rows Sptr / Scol / Sval over
  // the local nodes), the ring colours' halos at cs_off / cg_off indices
  // [0, nrc), the rest GS's colours at [nrc, nrc + gcs.size() - 1)
  bool rings = false;
  int nrc = 0;
  DLevel rl;
  uint8_t* rcov = nullptr;   // covered dofs of the owned nodes (bit f)
};

// D_CHALO: the forward halo of one colour's nodes (after that colour's GS step)
enum DKind { D_OP = 0, D_HALO = 1, D_REVERSE = 2, D_ALLREDUCE = 3, D_OVERLAP = 4, D_CHALO = 5 };

struct DOp {
  int dk = D_OP;
  Op op;
  int level = 0;
  int colour = 0;            // D_CHALO
  double* buf = nullptr;
  int64_t count = 0;
  double bytes = 0.0;
  int cls = 0;
};

// A_loc as the cycle reads it: level 0's fp32 copy once the rank is narrowed
inline const DBsr& dcyc_A(const DDLevel& D) { return D.Ac.f32 ? D.Ac : D.A; }

struct DistHandle : HandleMem, HandleOrder {   // last: marked after every apply / spmv / PCG (dist_destroy waits)
  mamg_params p;
  explicit DistHandle(const Switches& s) : HandleMem{s, {}, nullptr, 0} {}
  int rank = 0, nranks = 1, device = 0;
  int w = 2;                           // dofs per node: 2 nodal (BSR2), 1 scalar (CSR)
  ncclComm_t comm = nullptr;
  std::vector<DDLevel> L;
  double apply_bytes = 0.0;
  int64_t nv0 = 0, o0 = 0, o1 = 0;
  bool dry = false;                    // MAMG_DIST_TEST=dry: virtual rank skips its exchanges (timing only)
  hipStream_t side = nullptr;          // stream of the interior rows
  hipEvent_t ev_in = nullptr, ev_out = nullptr;
  // host-staged exchange backend (mamg_dist_set_exchange): pinned staging
  // per level (sends, ghost payloads, receives of the reverse-add) and one
  // all-reduce buffer
  bool host_ex = false;
  mamg_exchange ex{};
  std::vector<double*> hsend, hghost, hrecv;
  double* hred = nullptr;
  std::vector<void*> pinned;
  // the apply replayed as a hipGraph (dist_apply_graph): one per (r, z) pair,
  // captured on `cap` with the RCCL calls inside; graph_err set when a
  // capture failed (the handle then stays eager)
  GraphCache graphs;
  hipStream_t cap = nullptr;
  std::string graph_err;
  // device-resident PCG (dist_pcg): r, z, d, q of w * nloc
  // doubles, the dots' block partials and P-vectors, the state with its
  // pinned mirror (two slots per rank whose state is read here), and one
  // plan per (x, maxiter, stop_type): histories, the ops' context and, on
  // an RCCL or single-rank handle, the captured iteration
  double *cr = nullptr, *cz = nullptr, *cd = nullptr, *cq = nullptr, *ppart = nullptr, *pv = nullptr;
  DPcgState* pst = nullptr;
  DPcgState* hst = nullptr;
  int hst_ranks = 0;
  struct PcgPlan : IterGraph {         // hist: residuals, ||r||, alphas, betas
    std::unique_ptr<DPcgCtx> c;
  };
  std::vector<PcgPlan> pcgs;
  std::string pcg_graph_err;           // why the iteration runs eagerly on this handle
  ~DistHandle() {
    if (last) (void)hipEventSynchronize(last);
    graphs.clear();
    release_all(&pcgs);
    if (hst) (void)hipHostFree(hst);
    if (cap) (void)hipStreamDestroy(cap);
    for (void* q : pinned) (void)hipHostFree(q);
    if (ev_in) (void)hipEventDestroy(ev_in);
    if (ev_out) (void)hipEventDestroy(ev_out);
    if (last) (void)hipEventDestroy(last);
    if (side) (void)hipStreamDestroy(side);
    for (void* a : allocs) (void)raw_free(a);
    if (comm) (void)ncclCommDestroy(comm);
  }
};

template <class T>
int ddalloc(DistHandle* h, T** p, int64_t count, std::string* err) {
  *p = nullptr;
  if (count <= 0) return MAMG_OK;
  void* q = nullptr;
  HIPCHK(dev_malloc(&q, (size_t)count * sizeof(T)));
  HIPCHK(dev_memset(q, 0, (size_t)count * sizeof(T)));
  h->allocs.push_back(q);
  *p = (T*)q;
  return MAMG_OK;
}

// ---- device.hip (and capture_graph, TimedRun::run, IterGraph::alloc, pcg_finish above)
void wscale(int64_t n, double w, const double* in, double* out);
void launch_patch_inv(int version, int64_t np, const int32_t* perm, const int64_t* ptr, const int32_t* col,
                      const int32_t* gcol, const dv4* val, int64_t ustride, double* U, int* bad);
void ring_perm_inv(int64_t nb, const int32_t* ord, const int64_t* blen, const int64_t* sq, const double* inv,
                   const int64_t* rio, double* rinv);
void rest_w(int64_t nv, const dv4* W, const uint8_t* cov, dv4* Wp);
void rest_mask(int64_t nr, const int32_t* perm, const uint8_t* cov, dv4* D);
int pick_lanes(int64_t n, int64_t nnz);
int pick_lanes_bsr(int64_t nr, int64_t nb);
int upload_bsr(HandleMem* h, const HBsr& B, DBsr* D, int lanes, std::string* err,
               bool sym = false);
void sym_check(int64_t nb, const dv4* v, int* bad);
int dev_csr_to_bsr(TmpPool* T, const DevMat& M, int64_t nr, int64_t nc, TBsr* B, std::string* err);
int dev_merge_rows(TmpPool* T, const TBsr& P, const TBsr& Q, TBsr* M, std::string* err);
int dev_kmerge(TmpPool* T, const TBsr& P, const TBsr& Q, const double* W, TBsr* K, std::string* err);
int build_band_sched_range(HandleMem* h, DBsr* D, int64_t r0, int64_t r1, std::string* err);
int try_half(HandleMem* h, TmpPool* T, const TBsr& B, DBsr* D, std::string* err);
int upload_half_or_bsr(HandleMem* h, const HBsr& B, DBsr* D, std::string* err);
int finalize_bsr(HandleMem* h, TmpPool* T, TBsr& B, DBsr* D, int lanes, bool sym_ok, std::string* err,
                 bool allow_sell = true, bool allow_half = false, bool allow_msell = false);
int sort_sell_slices(HandleMem* h, TmpPool* T, DBsr* D, std::string* err);
int gs_colour(TmpPool* T, const TBsr& B, int level, int8_t** ca_out, int* ncol_out, std::string* err);
int gs_layout(HandleMem* h, TmpPool* T, const TBsr& B, const double* W, const int8_t* ca, int ncol, int level,
              DBsr* Gb, int32_t** gperm, dv4** Gd, std::vector<int64_t>* gcs_out, std::vector<int64_t>* gbk,
              std::string* err);
int patch_colour(TmpPool* T, const TBsr& B, int16_t** cout, int* maxlen, std::string* err);
Op csr_op(const DCsr& M, int epi, int cls, int tag, const double* x, const double* y,
          const double* b, const double* w, double* out);
Op bsr_op(const DBsr& M, int epi, int cls, int tag, const double* x, int64_t xs, const double* y,
          const double* b, int64_t bs, const dv4* W, double* out, int64_t os);
Op post_op(const DBsr& M, const double* r1, const dv4* W, int cls, int tag, const double* e,
           const double* x1, double* out, int64_t os);
Op axpy_op(int64_t n, const double* e, double* x);
Op patch_op(const DLevel& L, int c, double* x, const double* b, int64_t bs, int cls);
Op ring_op(const DLevel& L, int c, double* x, const double* b, int64_t bs, int cls);
bool k_ranges_ok(const DBsr& K);
void launch(const Op& o, hipStream_t s);
void adopt_prereserve(HandleMem* h, int device);
void adopt_prereserve(DeviceHandle* h);
int narrow_values(std::vector<NarrowJob>& jobs, std::vector<void*>* allocs, const std::function<void()>& drop_cached,
                  const std::function<void(void*)>& release, std::string* err);
void pack_w(int w, int64_t n, const int64_t* idx, const double* x, double* buf, hipStream_t s);
void unpack_w(int w, int64_t n, const int64_t* idx, int64_t nloc, const double* buf, double* x, hipStream_t s);
void addidx_w(int w, int64_t n, const int64_t* idx, const double* buf, double* x, hipStream_t s);
void vsum(int64_t n, const double* a, double* acc, hipStream_t s);

// ---- dist_layout.hip
void dist_layout_warm(hipStream_t s);

// ---- dist_apply.hip
void dapply_ops(const DistHandle* h, const double* r, double* z, std::vector<DOp>* ops);

}  // namespace mamg
