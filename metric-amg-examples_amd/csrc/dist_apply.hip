// dist_apply.hip -- the multi-GPU V-cycle (row-partitioned, RCCL over xGMI):
// the DOp lists, their eager and captured execution, the virtual ranks and
// the distributed PCG.  Plan: dist.cpp.
#include "device_int.h"

namespace mamg {

namespace {

DOp wrap(const Op& o) {
  DOp d;
  d.dk = D_OP; d.op = o; d.bytes = o.bytes; d.cls = o.cls;
  return d;
}

DOp halo_op(int level, double* x, const DDLevel& D, int cls) {
  DOp d;
  d.dk = D_HALO; d.level = level; d.buf = x; d.cls = cls;
  const int64_t ns = D.send_off.empty() ? 0 : D.send_off.back();
  d.bytes = 8.0 * ns + 16.0 * ns * 2 + 16.0 * D.ng;   // idx, pack r/w, ghost writes
  return d;
}

// forward halo of x followed by the SpMV `op` on A_loc: with the
// half-symmetric A, the ghost-free row run [ib0, ib1) (maybe empty) runs on the
// side stream while the halo is in flight (one D_OVERLAP), the rest after it.
// Every row is computed by the same kernel code either way (same bits).
void halo_residual(const DistHandle* h, int l, double* x, const Op& op, std::vector<DOp>* ops) {
  const DDLevel& D = h->L[l];
  if (!(h->sw.overlap && D.A.half)) {
    ops->push_back(halo_op(l, x, D, C_COMM));
    ops->push_back(wrap(op));
    return;
  }
  const double f = (double)(D.ib1 - D.ib0) / (double)std::max<int64_t>(D.nloc, 1);
  DOp ov = halo_op(l, x, D, op.cls);   // timed and counted with the SpMV's class
  ov.dk = D_OVERLAP;
  ov.op = op;
  ov.op.r0 = D.ib0;
  ov.op.r1 = D.ib1;
  ov.op.bytes = op.bytes * f;
  ov.bytes += ov.op.bytes;
  ops->push_back(ov);
  const int64_t lo[2] = {0, D.ib1}, hi[2] = {D.ib0, D.nloc};
  for (int k = 0; k < 2; ++k) {   // both always emitted (possibly empty): one schedule on every rank
    Op b = op;
    b.r0 = lo[k];
    b.r1 = hi[k];
    b.bytes = op.bytes * (double)std::max<int64_t>(hi[k] - lo[k], 0) / (double)std::max<int64_t>(D.nloc, 1);
    ops->push_back(wrap(b));
  }
}

// coarse-grid correction scaling of level lc's correction C.x against C.b on
// N ranks: halo of C.x (distributed level), q = A_c x on the owned rows,
// partial sums of <b, x>, <q, x> over the owned rows, one all-reduce of the
// partials (distributed level), alpha = num / den on every rank, x <- alpha x
// on the owned rows and the ghosts (so the post step needs no second halo)
void dscale_ops(const DistHandle* h, int lc, std::vector<DOp>* ops) {
  const DDLevel& C = h->L[lc];
  const Op q = bsr_op(C.A, EPI_Y, C_MISC, 1, C.x, 0, nullptr, nullptr, 0, nullptr, C.q, 0);
  if (C.replicated) ops->push_back(wrap(q)); else halo_residual(h, lc, C.x, q, ops);
  Op d;
  d.kind = OP_DOT2; d.cls = C_MISC; d.n = 2 * C.nloc; d.b = C.b; d.x = C.x; d.y = C.q; d.part = C.part2;
  d.bytes = 24.0 * d.n;
  ops->push_back(wrap(d));
  if (!C.replicated) {
    DOp a;
    a.dk = D_ALLREDUCE; a.cls = C_COMM; a.buf = C.part2; a.count = 2 * SCALE_BLOCKS; a.bytes = 16.0 * SCALE_BLOCKS;
    ops->push_back(a);
  }
  Op sc;
  sc.kind = OP_CSCALE; sc.cls = C_MISC; sc.n = 2 * (C.nloc + C.ng); sc.part = C.part2; sc.out = C.x;
  sc.bytes = 16.0 * sc.n;
  ops->push_back(wrap(sc));
}

void dcycle_ops(const DistHandle* h, int l, const double* b, int64_t bs, double* xout, int64_t os,
                std::vector<DOp>* ops);

// coarse-grid correction of level l from its residual D.r: partial
// restriction, reverse-add (or all-reduce into a replicated level), the
// coarse cycle (W: twice), scaling, and the halo of the correction C.x
// (left to the caller when defer_halo: it overlaps that halo with K)
void dcoarse_ops(const DistHandle* h, int l, std::vector<DOp>* ops, bool defer_halo = false) {
  const DDLevel& D = h->L[l];
  const DDLevel& C = h->L[l + 1];
  const bool l0 = l == 0;
  const int tagA = l0 ? 0 : 1;
  ops->push_back(wrap(bsr_op(D.R, EPI_Y, l0 ? C_L0_R : C_COARSE, tagA, D.r, 0, nullptr, nullptr, 0,
                             nullptr, C.b, 0)));
  ops->back().op.remap = 1;
  if (!D.replicated) {
    DOp d;
    d.cls = C_COMM;
    if (C.replicated) {
      d.dk = D_ALLREDUCE; d.buf = C.b; d.count = 2 * C.nv; d.bytes = 16.0 * C.nv * 2;
    } else {
      d.dk = D_REVERSE; d.level = l + 1; d.buf = C.b;
      const int64_t ns = C.send_off.back();
      d.bytes = 16.0 * C.ng + 16.0 * ns * 3 + 8.0 * ns;
    }
    ops->push_back(d);
  }
  dcycle_ops(h, l + 1, C.b, 0, C.x, 0, ops);
  if (h->p.cycle_type == MAMG_W_CYCLE && !C.coarsest) {   // second visit on the updated residual
    const Op res = bsr_op(C.A, EPI_RESID, C_MISC, 1, C.x, 0, nullptr, C.b, 0, nullptr, C.c, 0);
    if (C.replicated) ops->push_back(wrap(res)); else halo_residual(h, l + 1, C.x, res, ops);
    dcycle_ops(h, l + 1, C.c, 0, C.e, 0, ops);
    ops->push_back(wrap(axpy_op(2 * C.nloc, C.e, C.x)));
  }
  if (h->p.coarse_scaling) dscale_ops(h, l + 1, ops);      // ghosts of C.x scaled too
  else if (!C.replicated && !defer_halo) ops->push_back(halo_op(l + 1, C.x, C, C_COMM));
}

// level 0's K with the coarse-e halo in flight: rows [kb0, kb1) (no coarse
// ghost columns) on the side stream during the halo (one D_OVERLAP), the
// rest after it; the same kernel code computes every row either way
void k_overlap(const DistHandle* h, const Op& k, std::vector<DOp>* ops) {
  const DDLevel& D = h->L[0];
  const DDLevel& C = h->L[1];
  const double n = (double)std::max<int64_t>(D.nloc, 1);
  DOp ov = halo_op(1, C.x, C, k.cls);   // timed and counted with K's class
  ov.dk = D_OVERLAP;
  ov.op = k;
  ov.op.r0 = D.kb0;
  ov.op.r1 = D.kb1;
  ov.op.bytes = k.bytes * (double)(D.kb1 - D.kb0) / n;
  ov.bytes += ov.op.bytes;
  ops->push_back(ov);
  const int64_t lo[2] = {0, D.kb1}, hi[2] = {D.kb0, D.nloc};
  for (int q = 0; q < 2; ++q) {   // both always emitted (possibly empty): one schedule on every rank
    Op b = k;
    b.r0 = lo[q];
    b.r1 = hi[q];
    b.bytes = k.bytes * (double)std::max<int64_t>(hi[q] - lo[q], 0) / n;
    ops->push_back(wrap(b));
  }
}

DOp chalo_op(int level, int c, double* x, const DDLevel& D, int P) {
  DOp d;
  d.dk = D_CHALO; d.level = level; d.colour = c; d.buf = x; d.cls = C_COMM;
  const int64_t ns = D.cs_off[(size_t)(c + 1) * (P + 1) - 1] - D.cs_off[(size_t)c * (P + 1)];
  const int64_t ng = D.cg_off[(size_t)(c + 1) * (P + 1) - 1] - D.cg_off[(size_t)c * (P + 1)];
  d.bytes = 8.0 * ns + 32.0 * ns + 8.0 * ng + 32.0 * ng;   // indices, pack, unpack
  return d;
}

// one multicolour GS sweep on the owned rows, each colour's step followed by
// that colour's halo so the next colour reads current ghosts; every rank
// emits the same exchanges, also for colours it has no rows of
void dgs_sweep(const DistHandle* h, int l, bool fwd, double* x, const double* b, int64_t bs, int cls,
               std::vector<DOp>* ops) {
  const DDLevel& D = h->L[l];
  const int nc = (int)D.gcs.size() - 1;
  for (int k = 0; k < nc; ++k) {
    const int c = fwd ? k : nc - 1 - k;
    ops->push_back(wrap(gs_op(D, c, x, b, bs, cls)));   // empty here: not launched (same schedule on every rank)
    if (!D.replicated) ops->push_back(chalo_op(l, c, x, D, h->nranks));
  }
}

// multi-GPU cycle with multicolour GS / SGS (cycle_ops_bsr's GS branch): from
// x = 0, pre sweeps, residual (ghosts current), coarse correction, x += P e,
// halo, post sweeps; X holds [owned | ghost]
void dcycle_gs(const DistHandle* h, int l, const double* b, int64_t bs, double* xout, int64_t os,
               std::vector<DOp>* ops) {
  const DDLevel& D = h->L[l];
  const DDLevel& C = h->L[l + 1];
  const bool l0 = l == 0;
  const int tagA = l0 ? 0 : 1;
  const int clsS = l0 ? C_L0_SMOOTH : C_COARSE;
  const int clsW = l0 ? C_L0_WB : C_COARSE;
  const bool sgs = h->p.smoother == MAMG_SMOOTHER_SGS;
  double* X = os == 0 ? xout : D.t;
  {
    Op z;
    z.kind = OP_ZERO; z.cls = clsW; z.n = 2 * (D.nloc + D.ng); z.out = X; z.bytes = 8.0 * z.n;
    ops->push_back(wrap(z));
  }
  for (int s = 0; s < h->p.presmooth_iter; ++s) {
    dgs_sweep(h, l, true, X, b, bs, clsS, ops);
    if (sgs) dgs_sweep(h, l, false, X, b, bs, clsS, ops);
  }
  ops->push_back(wrap(bsr_op(D.A, EPI_RESID, l0 ? C_L0_RESID : C_COARSE, tagA, X, 0, nullptr, b, bs, nullptr,
                             D.r, 0)));
  dcoarse_ops(h, l, ops);
  ops->push_back(wrap(bsr_op(D.P, EPI_YADD, l0 ? C_L0_P : C_COARSE, tagA, C.x, 0, X, nullptr, 0, nullptr, X, 0)));
  if (!D.replicated) ops->push_back(halo_op(l, X, D, C_COMM));
  for (int s = 0; s < h->p.postsmooth_iter; ++s) {
    if (sgs) dgs_sweep(h, l, true, X, b, bs, clsS, ops);
    dgs_sweep(h, l, false, X, b, bs, clsS, ops);
  }
  if (X != xout) {
    Op o;
    o.kind = OP_ILV; o.epi = 1; o.cls = clsW; o.n = D.nloc; o.b = X; o.out = xout; o.os = os;
    o.bytes = 32.0 * D.nloc;
    ops->push_back(wrap(o));
  }
}

// one node-patch sweep of level 0 on N ranks: per colour the rank's patches
// of that colour, then that colour's halo (the written nodes within 3 hops);
// every rank emits every colour's exchange, also without patches of its own
void dpatch_sweep(const DistHandle* h, bool fwd, double* x, std::vector<DOp>* ops) {
  const DDLevel& D = h->L[0];
  const int nc = (int)D.pl.pcs.size() - 1;
  for (int k = 0; k < nc; ++k) {
    const int c = fwd ? k : nc - 1 - k;
    ops->push_back(wrap(patch_op(D.pl, c, x, D.pb, 0, C_L0_SMOOTH)));   // empty: not launched
    ops->push_back(chalo_op(0, c, x, D, h->nranks));
  }
}

// multi-GPU level-0 cycle with the node-patch Schwarz (cycle_ops_bsr's
// patch branch): b interleaved over [owned | ghost] + its halo; x = 0; pre
// sweeps forward then backward; residual (ghosts current); the coarse
// correction; x += P e and its halo; post sweeps forward then backward
void dcycle_patch(const DistHandle* h, const double* b, int64_t bs, double* xout, int64_t os,
                  std::vector<DOp>* ops) {
  const DDLevel& D = h->L[0];
  const DDLevel& C = h->L[1];
  double* X = D.t;
  {
    Op o;
    o.kind = OP_ILV; o.cls = C_L0_WB; o.n = D.nloc; o.b = b; o.bs = bs; o.out = D.pb;
    o.bytes = 32.0 * D.nloc;
    ops->push_back(wrap(o));
    ops->push_back(halo_op(0, D.pb, D, C_COMM));
    Op z;
    z.kind = OP_ZERO; z.cls = C_L0_WB; z.n = 2 * (D.nloc + D.ng); z.out = X; z.bytes = 8.0 * z.n;
    ops->push_back(wrap(z));
  }
  for (int s = 0; s < h->p.presmooth_iter; ++s) {
    dpatch_sweep(h, true, X, ops);
    dpatch_sweep(h, false, X, ops);
  }
  ops->push_back(wrap(bsr_op(D.A, EPI_RESID, C_L0_RESID, 0, X, 0, nullptr, b, bs, nullptr, D.r, 0)));
  dcoarse_ops(h, 0, ops);
  ops->push_back(wrap(bsr_op(D.P, EPI_YADD, C_L0_P, 0, C.x, 0, X, nullptr, 0, nullptr, X, 0)));
  ops->push_back(halo_op(0, X, D, C_COMM));
  for (int s = 0; s < h->p.postsmooth_iter; ++s) {
    dpatch_sweep(h, true, X, ops);
    dpatch_sweep(h, false, X, ops);
  }
  Op o;
  o.kind = OP_ILV; o.epi = 1; o.cls = C_L0_WB; o.n = D.nloc; o.b = X; o.out = xout; o.os = os;
  o.bytes = 32.0 * D.nloc;
  ops->push_back(wrap(o));
}

// one symmetric level-0 seed-ring step on N ranks (the single-GPU sweep of
// cycle_ops_bsr, mamg_oracle.rings_step): forward = ring colours ascending,
// then the rest's GS colours ascending; backward = the rest descending, then
// the rings descending; each colour's step followed by its halo (every rank
// emits every exchange, also for colours it has no work in)
void dring_sweep(const DistHandle* h, bool fwd, double* x, std::vector<DOp>* ops) {
  const DDLevel& D = h->L[0];
  const int nrc = D.nrc, ngc = (int)D.gcs.size() - 1, P = h->nranks;
  auto rings = [&](bool f) {
    for (int k = 0; k < nrc; ++k) {
      const int c = f ? k : nrc - 1 - k;
      ops->push_back(wrap(ring_op(D.rl, c, x, D.pb, 0, C_L0_SMOOTH)));   // empty: not launched
      ops->push_back(chalo_op(0, c, x, D, P));
    }
  };
  auto rest = [&](bool f) {
    for (int k = 0; k < ngc; ++k) {
      const int c = f ? k : ngc - 1 - k;
      ops->push_back(wrap(gs_op(D, c, x, D.pb, 0, C_L0_SMOOTH)));
      ops->push_back(chalo_op(0, nrc + c, x, D, P));
    }
  };
  if (fwd) { rings(true); rest(true); } else { rest(false); rings(false); }
}

// multi-GPU level-0 cycle with the seed-ring Schwarz (cycle_ops_bsr's ring
// branch): b interleaved over [owned | ghost] + its halo; x = 0; pre steps
// forward then backward; residual; the coarse correction; x += P e and its
// halo; post steps forward then backward
void dcycle_rings(const DistHandle* h, const double* b, int64_t bs, double* xout, int64_t os,
                  std::vector<DOp>* ops) {
  const DDLevel& D = h->L[0];
  const DDLevel& C = h->L[1];
  double* X = D.t;
  {
    Op o;
    o.kind = OP_ILV; o.cls = C_L0_WB; o.n = D.nloc; o.b = b; o.bs = bs; o.out = D.pb;
    o.bytes = 32.0 * D.nloc;
    ops->push_back(wrap(o));
    ops->push_back(halo_op(0, D.pb, D, C_COMM));
    Op z;
    z.kind = OP_ZERO; z.cls = C_L0_WB; z.n = 2 * (D.nloc + D.ng); z.out = X; z.bytes = 8.0 * z.n;
    ops->push_back(wrap(z));
  }
  for (int s = 0; s < h->p.presmooth_iter; ++s) {
    dring_sweep(h, true, X, ops);
    dring_sweep(h, false, X, ops);
  }
  ops->push_back(wrap(bsr_op(D.A, EPI_RESID, C_L0_RESID, 0, X, 0, nullptr, b, bs, nullptr, D.r, 0)));
  dcoarse_ops(h, 0, ops);
  ops->push_back(wrap(bsr_op(D.P, EPI_YADD, C_L0_P, 0, C.x, 0, X, nullptr, 0, nullptr, X, 0)));
  ops->push_back(halo_op(0, X, D, C_COMM));
  for (int s = 0; s < h->p.postsmooth_iter; ++s) {
    dring_sweep(h, true, X, ops);
    dring_sweep(h, false, X, ops);
  }
  Op o;
  o.kind = OP_ILV; o.epi = 1; o.cls = C_L0_WB; o.n = D.nloc; o.b = X; o.out = xout; o.os = os;
  o.bytes = 32.0 * D.nloc;
  ops->push_back(wrap(o));
}

// ---- scalar (CSR) hierarchies on N ranks: cycle_ops_csr restated with
// exchanges.  Vectors are [owned | ghost] doubles;
// every rank emits the same schedule whatever it owns.
DOp halo_op1(int level, double* x, const DDLevel& D, int cls) {
  DOp d;
  d.dk = D_HALO; d.level = level; d.buf = x; d.cls = cls;
  const int64_t ns = D.send_off.empty() ? 0 : D.send_off.back();
  d.bytes = 8.0 * ns + 8.0 * ns * 2 + 8.0 * D.ng;   // idx, pack r/w, ghost writes
  return d;
}

// forward halo of x, then the SpMV `op` on the rank-local operator.  With
// `split` (the level-0 residual and the standalone SpMV) the longest run of
// rows without ghost columns [ib0, ib1) (maybe empty) runs on the side stream
// while the halo is in flight (one D_OVERLAP) and the rest after it; the same
// kernel computes every row either way (same bits).
void halo_csr(const DistHandle* h, int l, double* x, const Op& op, bool split, std::vector<DOp>* ops) {
  const DDLevel& D = h->L[l];
  if (D.replicated) { ops->push_back(wrap(op)); return; }
  if (!(split && h->sw.overlap)) {
    ops->push_back(halo_op1(l, x, D, C_COMM));
    ops->push_back(wrap(op));
    return;
  }
  const double n = (double)std::max<int64_t>(D.nloc, 1);
  DOp ov = halo_op1(l, x, D, op.cls);   // timed and counted with the SpMV's class
  ov.dk = D_OVERLAP;
  ov.op = op;
  ov.op.r0 = D.ib0;
  ov.op.r1 = D.ib1;
  ov.op.bytes = op.bytes * (double)(D.ib1 - D.ib0) / n;
  ov.bytes += ov.op.bytes;
  ops->push_back(ov);
  const int64_t lo[2] = {0, D.ib1}, hi[2] = {D.ib0, D.nloc};
  for (int k = 0; k < 2; ++k) {   // both always emitted (possibly empty): one schedule on every rank
    Op b = op;
    b.r0 = lo[k];
    b.r1 = hi[k];
    b.bytes = op.bytes * (double)std::max<int64_t>(hi[k] - lo[k], 0) / n;
    ops->push_back(wrap(b));
  }
}

// as dscale_ops: the dots over the owned rows, the scale over [owned | ghost]
void dscale_csr(const DistHandle* h, int lc, std::vector<DOp>* ops) {
  const DDLevel& C = h->L[lc];
  halo_csr(h, lc, C.x, csr_op(C.cA, EPI_Y, C_MISC, 1, C.x, nullptr, nullptr, nullptr, C.q), false, ops);
  Op d;
  d.kind = OP_DOT2; d.cls = C_MISC; d.n = C.nloc; d.b = C.b; d.x = C.x; d.y = C.q; d.part = C.part2;
  d.bytes = 24.0 * d.n;
  ops->push_back(wrap(d));
  if (!C.replicated) {
    DOp a;
    a.dk = D_ALLREDUCE; a.cls = C_COMM; a.buf = C.part2; a.count = 2 * SCALE_BLOCKS; a.bytes = 16.0 * SCALE_BLOCKS;
    ops->push_back(a);
  }
  Op sc;
  sc.kind = OP_CSCALE; sc.cls = C_MISC; sc.n = C.nloc + C.ng; sc.part = C.part2; sc.out = C.x;
  sc.bytes = 16.0 * sc.n;
  ops->push_back(wrap(sc));
}

// one smoothing step of a scalar level from the iterate X (not the first from
// x = 0): halo of X, then x + w_s winv (b - A X) in one pass, or with the
// sparse block smoother r = b - A X, halo of r, x + w_s WB_loc r
void dsmooth_csr(const DistHandle* h, int l, const double* b, double* X, double* out, int s, bool pre,
                 std::vector<DOp>* ops) {
  const DDLevel& D = h->L[l];
  const bool l0 = l == 0;
  const int tagA = l0 ? 0 : 1, clsS = l0 ? C_L0_SMOOTH : C_COARSE, clsW = l0 ? C_L0_WB : C_COARSE;
  const int m = smoother_steps(h->p);
  if (D.cWB.n > 0) {
    const DCsr& wb = D.cWBk.empty() ? D.cWB : D.cWBk[step_index(m, s, pre)];
    halo_csr(h, l, X, csr_op(D.cA, EPI_RESID, clsS, tagA, X, nullptr, b, nullptr, D.r), false, ops);
    halo_csr(h, l, D.r, csr_op(wb, EPI_YADD, clsW, tagA, D.r, X, nullptr, nullptr, out), false, ops);
  } else {
    const double* wv = D.winvk.empty() ? D.winv : D.winvk[step_index(m, s, pre)];
    halo_csr(h, l, X, csr_op(D.cA, EPI_JACOBI, clsS, tagA, X, X, b, wv, out), false, ops);
  }
}

void dcycle_csr(const DistHandle* h, int l, const double* b, double* xout, std::vector<DOp>* ops) {
  const DDLevel& D = h->L[l];
  const mamg_params& p = h->p;
  const bool l0 = l == 0;
  if (D.coarsest) {
    Op o;
    o.kind = OP_GEMV; o.cls = C_DENSE; o.n = D.nv; o.x = b; o.w = D.Ainv; o.out = xout;
    o.bytes = 8.0 * o.n * o.n + 16.0 * o.n;
    ops->push_back(wrap(o));
    return;
  }
  const DDLevel& C = h->L[l + 1];
  const int tagA = l0 ? 0 : 1, clsW = l0 ? C_L0_WB : C_COARSE;
  const int m = smoother_steps(p);
  const int npre = p.presmooth_iter * m, npost = p.postsmooth_iter * m;
  double* X = D.t;
  double* X2 = D.t2;
  if (D.cWB.n > 0) {   // X = WB_loc b: b's ghosts first (b copied into its [owned | ghost] buffer)
    const DCsr& wb = D.cWBk.empty() ? D.cWB : D.cWBk[step_index(m, 0, true)];
    Op c;
    c.kind = OP_COPY; c.cls = clsW; c.n = D.nloc; c.x = b; c.out = D.gb; c.bytes = 16.0 * D.nloc;
    ops->push_back(wrap(c));
    halo_csr(h, l, D.gb, csr_op(wb, EPI_Y, clsW, tagA, D.gb, nullptr, nullptr, nullptr, X), false, ops);
  } else {
    Op o;
    o.kind = OP_SCALE; o.cls = clsW; o.n = D.nloc; o.w = D.winvk.empty() ? D.winv : D.winvk[step_index(m, 0, true)];
    o.x = b; o.out = X; o.bytes = 24.0 * D.nloc;
    ops->push_back(wrap(o));
  }
  for (int s = 1; s < npre; ++s) {
    dsmooth_csr(h, l, b, X, X2, s, true, ops);
    std::swap(X, X2);
  }
  halo_csr(h, l, X, csr_op(D.cA, EPI_RESID, l0 ? C_L0_RESID : C_COARSE, tagA, X, nullptr, b, nullptr, D.r), l0, ops);
  // partial restriction, then the ghost partials to their owners (added in
  // rank order) or the sum over the ranks into a replicated level
  ops->push_back(wrap(csr_op(D.cR, EPI_Y, l0 ? C_L0_R : C_COARSE, tagA, D.r, nullptr, nullptr, nullptr, C.b)));
  if (!D.replicated) {
    DOp d;
    d.cls = C_COMM;
    if (C.replicated) {
      d.dk = D_ALLREDUCE; d.buf = C.b; d.count = C.nv; d.bytes = 16.0 * C.nv;
    } else {
      d.dk = D_REVERSE; d.level = l + 1; d.buf = C.b;
      const int64_t ns = C.send_off.back();
      d.bytes = 8.0 * C.ng + 8.0 * ns * 3 + 8.0 * ns;
    }
    ops->push_back(d);
  }
  dcycle_csr(h, l + 1, C.b, C.x, ops);
  if (p.cycle_type == MAMG_W_CYCLE && !C.coarsest) {   // second visit on the updated residual
    halo_csr(h, l + 1, C.x, csr_op(C.cA, EPI_RESID, C_MISC, 1, C.x, nullptr, C.b, nullptr, C.c), false, ops);
    dcycle_csr(h, l + 1, C.c, C.e, ops);
    ops->push_back(wrap(axpy_op(C.nloc, C.e, C.x)));
  }
  if (p.coarse_scaling) dscale_csr(h, l + 1, ops);      // ghosts of C.x scaled too
  else if (!C.replicated) ops->push_back(halo_op1(l + 1, C.x, C, C_COMM));
  ops->push_back(wrap(csr_op(D.cP, EPI_YADD, l0 ? C_L0_P : C_COARSE, tagA, C.x, X, nullptr, nullptr, X)));
  for (int s = 0; s < npost; ++s) {
    double* out = s == npost - 1 ? xout : X2;
    dsmooth_csr(h, l, b, X, out, s, false, ops);
    if (out == X2) std::swap(X, X2);
  }
}

// multi-GPU cycle from x = 0 (V or W, nu1 / nu2 sweeps, optional coarse-grid
// scaling): see dist.cpp / dist_ref.py
void dcycle_ops(const DistHandle* h, int l, const double* b, int64_t bs, double* xout, int64_t os,
                std::vector<DOp>* ops) {
  if (l == 0 && h->L[0].patches) { dcycle_patch(h, b, bs, xout, os, ops); return; }
  if (l == 0 && h->L[0].rings) { dcycle_rings(h, b, bs, xout, os, ops); return; }
  if (!h->L[l].coarsest && h->L[l].gcs.size() > 1) { dcycle_gs(h, l, b, bs, xout, os, ops); return; }
  const DDLevel& D = h->L[l];
  const bool l0 = l == 0;
  const int tagA = l0 ? 0 : 1;
  if (D.coarsest) {
    Op o;
    o.kind = OP_GEMV; o.cls = C_DENSE; o.n = 2 * D.nv; o.x = b; o.w = D.Ainv; o.out = xout;
    o.bytes = 8.0 * o.n * o.n + 16.0 * o.n;
    ops->push_back(wrap(o));
    return;
  }
  const DDLevel& C = h->L[l + 1];
  const int m = smoother_steps(h->p);   // steps per smoothing (POLY: Chebyshev degree)
  const int npre = h->p.presmooth_iter * m, npost = h->p.postsmooth_iter * m;
  auto wk = [&](int s, bool pre) -> const dv4* { return D.Wk.empty() ? D.W : D.Wk[step_index(m, s, pre)]; };
  const int clsS = l0 ? C_L0_SMOOTH : C_COARSE;
  double* X = D.t;
  double* X2 = D.t2;
  {
    Op o;
    o.kind = OP_BD; o.cls = l0 ? C_L0_WB : C_COARSE; o.n = D.nloc; o.W = wk(0, true); o.b = b; o.bs = bs;
    o.out = X; o.bytes = 64.0 * D.nloc;
    ops->push_back(wrap(o));
  }
  for (int s = 1; s < npre; ++s) {   // further pre steps: halo of X, then x + w_s W (b - A x)
    const Op bj = bsr_op(dcyc_A(D), EPI_BJAC, clsS, tagA, X, 0, X, b, bs, wk(s, true), X2, 0);
    if (D.replicated) ops->push_back(wrap(bj)); else halo_residual(h, l, X, bj, ops);
    std::swap(X, X2);
  }
  {
    const Op res = bsr_op(dcyc_A(D), EPI_RESID, l0 ? C_L0_RESID : C_COARSE, tagA, X, 0, nullptr, b, bs, nullptr, D.r, 0);
    if (D.replicated) {
      ops->push_back(wrap(res));
    } else {
      halo_residual(h, l, X, res, ops);
    }
  }
  // K on its ghost-free rows while the coarse-e halo is in flight (level 0,
  // no coarse scaling); the schedule's shape is the same on every rank (the
  // overlap and both remainder launches are emitted, maybe empty)
  const bool kov = l == 0 && h->sw.overlap && D.K.nr > 0 && !C.replicated && !h->p.coarse_scaling && npost >= 1 &&
                   k_ranges_ok(D.K);
  dcoarse_ops(h, l, ops, kov);
  int s0 = 0;
  if (D.K.nr > 0 || D.PA.nr > 0) {   // fused first post step (K built with its smoother), operands local
    const bool last = npost == 1;
    if (D.K.nr > 0) { // X + W r + K e
      const Op k = bsr_op(D.K, EPI_KPOST, clsS, tagA, C.x, 0, X, D.r, 0, wk(0, false), last ? xout : X2,
                          last ? os : 0);
      if (kov) k_overlap(h, k, ops); else ops->push_back(wrap(k));
    } else            // X + P e + W (r - AP e)
      ops->push_back(wrap(post_op(D.PA, D.r, wk(0, false), clsS, tagA, C.x, X, last ? xout : X2,
                                  last ? os : 0)));
    if (last) return;
    std::swap(X, X2);
    s0 = 1;
  } else {
    ops->push_back(wrap(bsr_op(D.P, EPI_YADD, l0 ? C_L0_P : C_COARSE, tagA, C.x, 0, X, nullptr, 0,
                               nullptr, X, 0)));
  }
  for (int s = s0; s < npost; ++s) {   // halo of the iterate, then x + w W (b - A x)
    const bool last = s == npost - 1;
    const Op bj = bsr_op(dcyc_A(D), EPI_BJAC, clsS, tagA, X, 0, X, b, bs, wk(s, false), last ? xout : X2,
                         last ? os : 0);
    if (D.replicated) ops->push_back(wrap(bj)); else halo_residual(h, l, X, bj, ops);
    std::swap(X, X2);
  }
}

// one exchange through the host callbacks: device payloads staged in pinned
// memory around the callback (stream synchronised first), the same pack /
// unpack / rank-ordered reverse-add kernels as the RCCL branch of run_dop
int run_dop_host(DistHandle* h, const DOp& d, hipStream_t s, std::string* err) {
  const int P = h->nranks, w = h->w;
  std::vector<double*> snd(P, nullptr), rcv(P, nullptr);
  std::vector<int64_t> sc(P, 0), rc(P, 0);
  if (d.dk == D_ALLREDUCE) {
    HIPCHK(hipMemcpyAsync(h->hred, d.buf, d.count * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (h->ex.allreduce(h->ex.ctx, h->hred, d.count)) { *err = "exchange allreduce callback failed"; return MAMG_ERR_HIP; }
    HIPCHK(hipMemcpyAsync(d.buf, h->hred, d.count * sizeof(double), hipMemcpyHostToDevice, s));
    return MAMG_OK;
  }
  const DDLevel& D = h->L[d.level];
  const int64_t ns = D.send_off.back();
  if (d.dk == D_OVERLAP) {   // interior rows on the side stream, host halo on s, join
    HIPCHK(hipEventRecord(h->ev_in, s));
    HIPCHK(hipStreamWaitEvent(h->side, h->ev_in, 0));
    launch(d.op, h->side);
    HIPCHK(hipEventRecord(h->ev_out, h->side));
    DOp hd = d;
    hd.dk = D_HALO;
    int r = run_dop_host(h, hd, s, err);
    HIPCHK(hipStreamWaitEvent(s, h->ev_out, 0));
    return r;
  }
  double* hs = h->hsend[d.level];
  double* hg = h->hghost[d.level];
  double* hr = h->hrecv[d.level];
  if (d.dk == D_CHALO) {
    const size_t b0 = (size_t)d.colour * (P + 1);
    const int64_t s0 = D.cs_off[b0], s1 = D.cs_off[b0 + P], g0 = D.cg_off[b0], g1 = D.cg_off[b0 + P];
    for (int q = 0; q < P; ++q) {
      if (q == h->rank) continue;
      snd[q] = hs + w * D.cs_off[b0 + q]; sc[q] = w * (D.cs_off[b0 + q + 1] - D.cs_off[b0 + q]);
      rcv[q] = hg + w * D.cg_off[b0 + q]; rc[q] = w * (D.cg_off[b0 + q + 1] - D.cg_off[b0 + q]);
    }
    if (s1 > s0) {
      pack_w(w, s1 - s0, D.csend_idx + s0, d.buf, D.sendbuf + w * s0, s);
      HIPCHK(hipMemcpyAsync(hs + w * s0, D.sendbuf + w * s0, w * (s1 - s0) * sizeof(double), hipMemcpyDeviceToHost, s));
    }
    HIPCHK(hipStreamSynchronize(s));
    if (h->ex.sendrecv(h->ex.ctx, P, snd.data(), sc.data(), rcv.data(), rc.data())) {
      *err = "exchange sendrecv callback failed";
      return MAMG_ERR_HIP;
    }
    if (g1 > g0) {
      HIPCHK(hipMemcpyAsync(D.recvbuf + w * g0, hg + w * g0, w * (g1 - g0) * sizeof(double), hipMemcpyHostToDevice, s));
      unpack_w(w, g1 - g0, D.cghost_idx + g0, D.nloc, D.recvbuf + w * g0, d.buf, s);
    }
    return MAMG_OK;
  }
  for (int q = 0; q < P; ++q) {
    if (q == h->rank) continue;
    const int64_t sq = D.send_off[q + 1] - D.send_off[q], gq = D.ghost_off[q + 1] - D.ghost_off[q];
    if (d.dk == D_HALO) {   // my owned values they ghost -> their ghosts of mine
      snd[q] = hs + w * D.send_off[q]; sc[q] = w * sq;
      rcv[q] = hg + w * D.ghost_off[q]; rc[q] = w * gq;
    } else {                // D_REVERSE: my ghost partials -> their owned rows
      snd[q] = hg + w * D.ghost_off[q]; sc[q] = w * gq;
      rcv[q] = hr + w * D.send_off[q]; rc[q] = w * sq;
    }
  }
  if (d.dk == D_HALO) {
    if (ns) {
      pack_w(w, ns, D.send_idx, d.buf, D.sendbuf, s);
      HIPCHK(hipMemcpyAsync(hs, D.sendbuf, w * ns * sizeof(double), hipMemcpyDeviceToHost, s));
    }
    HIPCHK(hipStreamSynchronize(s));
    if (h->ex.sendrecv(h->ex.ctx, P, snd.data(), sc.data(), rcv.data(), rc.data())) {
      *err = "exchange sendrecv callback failed";
      return MAMG_ERR_HIP;
    }
    if (D.ng)
      HIPCHK(hipMemcpyAsync(d.buf + w * D.nloc, hg, w * D.ng * sizeof(double), hipMemcpyHostToDevice, s));
    return MAMG_OK;
  }
  // D_REVERSE
  if (D.ng) HIPCHK(hipMemcpyAsync(hg, d.buf + w * D.nloc, w * D.ng * sizeof(double), hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  if (h->ex.sendrecv(h->ex.ctx, P, snd.data(), sc.data(), rcv.data(), rc.data())) {
    *err = "exchange sendrecv callback failed";
    return MAMG_ERR_HIP;
  }
  if (ns) HIPCHK(hipMemcpyAsync(D.recvbuf, hr, w * ns * sizeof(double), hipMemcpyHostToDevice, s));
  for (int q = 0; q < P; ++q) {
    const int64_t sq = D.send_off[q + 1] - D.send_off[q];
    if (q == h->rank || !sq) continue;
    addidx_w(w, sq, D.send_idx + D.send_off[q], D.recvbuf + w * D.send_off[q], d.buf, s);
  }
  return MAMG_OK;
}

int run_dop(DistHandle* h, const DOp& d, hipStream_t s, std::string* err) {
  if (d.dk == D_OP) {
    launch(d.op, s);
    return MAMG_OK;
  }
  const int w = h->w;
  if (h->nranks == 1 && !h->comm) {     // no peers: halos empty, sums over one rank
    if (d.dk == D_OVERLAP) launch(d.op, s);
    return MAMG_OK;
  }
  // (a 1-rank RCCL communicator takes the RCCL path below: empty send /
  // receive groups, an all-reduce over one rank, the side-stream fork; the
  // one-GPU tests exercise those calls, eager and inside a graph capture)
  if (!h->comm && h->dry) {            // compute-only timing of one rank (results meaningless)
    if (d.dk == D_OVERLAP) launch(d.op, s);
    return MAMG_OK;
  }
  if (!h->comm && h->host_ex) return run_dop_host(h, d, s, err);
  if (!h->comm) {
    *err = "virtual rank handle (no communicator): use mamg_dist_virtual_apply / _spmv";
    return MAMG_ERR_ARG;
  }
  if (d.dk == D_ALLREDUCE) {
    NCCLCHK(ncclAllReduce(d.buf, d.buf, d.count, ncclDouble, ncclSum, h->comm, s));
    return MAMG_OK;
  }
  const DDLevel& D = h->L[d.level];
  const int64_t ns = D.send_off.back();
  if (d.dk == D_OVERLAP) {   // interior rows on the side stream, halo on s, join
    HIPCHK(hipEventRecord(h->ev_in, s));
    HIPCHK(hipStreamWaitEvent(h->side, h->ev_in, 0));
    launch(d.op, h->side);
    HIPCHK(hipEventRecord(h->ev_out, h->side));
    DOp hd = d;
    hd.dk = D_HALO;
    int rc = run_dop(h, hd, s, err);
    HIPCHK(hipStreamWaitEvent(s, h->ev_out, 0));
    return rc;
  }
  if (d.dk == D_CHALO) {      // one colour's nodes: pack, send / receive, unpack into the ghost slots
    const int P = h->nranks;
    const size_t b0 = (size_t)d.colour * (P + 1);
    const int64_t s0 = D.cs_off[b0], s1 = D.cs_off[b0 + P], g0 = D.cg_off[b0], g1 = D.cg_off[b0 + P];
    if (s1 > s0) pack_w(w, s1 - s0, D.csend_idx + s0, d.buf, D.sendbuf + w * s0, s);
    NCCLCHK(ncclGroupStart());
    for (int q = 0; q < P; ++q) {
      if (q == h->rank) continue;
      const int64_t sc = D.cs_off[b0 + q + 1] - D.cs_off[b0 + q], gc = D.cg_off[b0 + q + 1] - D.cg_off[b0 + q];
      if (sc) NCCLCHK(ncclSend(D.sendbuf + w * D.cs_off[b0 + q], w * sc, ncclDouble, q, h->comm, s));
      if (gc) NCCLCHK(ncclRecv(D.recvbuf + w * D.cg_off[b0 + q], w * gc, ncclDouble, q, h->comm, s));
    }
    NCCLCHK(ncclGroupEnd());
    if (g1 > g0) unpack_w(w, g1 - g0, D.cghost_idx + g0, D.nloc, D.recvbuf + w * g0, d.buf, s);
    return MAMG_OK;
  }
  if (d.dk == D_HALO) {
    if (ns) pack_w(w, ns, D.send_idx, d.buf, D.sendbuf, s);
    NCCLCHK(ncclGroupStart());
    for (int q = 0; q < h->nranks; ++q) {
      if (q == h->rank) continue;
      const int64_t sc = D.send_off[q + 1] - D.send_off[q];
      const int64_t gc = D.ghost_off[q + 1] - D.ghost_off[q];
      if (sc) NCCLCHK(ncclSend(D.sendbuf + w * D.send_off[q], w * sc, ncclDouble, q, h->comm, s));
      if (gc) NCCLCHK(ncclRecv(d.buf + w * (D.nloc + D.ghost_off[q]), w * gc, ncclDouble, q, h->comm, s));
    }
    NCCLCHK(ncclGroupEnd());
    return MAMG_OK;
  }
  // D_REVERSE: ghost partials -> owners; owners add in rank order
  NCCLCHK(ncclGroupStart());
  for (int q = 0; q < h->nranks; ++q) {
    if (q == h->rank) continue;
    const int64_t sc = D.send_off[q + 1] - D.send_off[q];
    const int64_t gc = D.ghost_off[q + 1] - D.ghost_off[q];
    if (gc) NCCLCHK(ncclSend(d.buf + w * (D.nloc + D.ghost_off[q]), w * gc, ncclDouble, q, h->comm, s));
    if (sc) NCCLCHK(ncclRecv(D.recvbuf + w * D.send_off[q], w * sc, ncclDouble, q, h->comm, s));
  }
  NCCLCHK(ncclGroupEnd());
  for (int q = 0; q < h->nranks; ++q) {
    const int64_t sc = D.send_off[q + 1] - D.send_off[q];
    if (q == h->rank || !sc) continue;
    addidx_w(w, sc, D.send_idx + D.send_off[q], D.recvbuf + w * D.send_off[q], d.buf, s);
  }
  return MAMG_OK;
}

}  // namespace

void dapply_ops(const DistHandle* h, const double* r, double* z, std::vector<DOp>* ops) {
  ops->clear();
  const int64_t nloc = h->L[0].nloc;
  if (h->w == 1) { dcycle_csr(h, 0, r, z, ops); return; }   // scalar: the rank's plain slices
  dcycle_ops(h, 0, r, nloc, z, nloc, ops);
}

namespace {

// y = A x on the rank's rows (field-major local slices): interleave x into
// the [owned | ghost] buffer, forward halo, SpMV with A_loc (PCG operator)
void dspmv_ops(const DistHandle* h, const double* x, double* y, std::vector<DOp>* ops) {
  ops->clear();
  const DDLevel& D = h->L[0];
  if (h->w == 1) {   // scalar: x copied into the [owned | ghost] buffer, halo, A_loc (interior rows meanwhile)
    Op c;
    c.kind = OP_COPY; c.cls = C_MISC; c.n = D.nloc; c.x = x; c.out = D.spx; c.bytes = 16.0 * D.nloc;
    ops->push_back(wrap(c));
    halo_csr(h, 0, D.spx, csr_op(D.cA, EPI_Y, C_L0_RESID, 0, D.spx, nullptr, nullptr, nullptr, y), true, ops);
    return;
  }
  Op o;
  o.kind = OP_ILV; o.cls = C_MISC; o.n = D.nloc; o.b = x; o.bs = D.nloc; o.out = D.spx;
  o.bytes = 32.0 * D.nloc;
  ops->push_back(wrap(o));
  const Op mv = bsr_op(D.A, EPI_Y, C_L0_RESID, 0, D.spx, 0, nullptr, nullptr, 0, nullptr, y, D.nloc);
  if (D.replicated) ops->push_back(wrap(mv)); else halo_residual(h, 0, D.spx, mv, ops);
}

}  // namespace

int dist_get_unique_id(void* id, std::string* err) {
  ncclUniqueId u;
  NCCLCHK(ncclGetUniqueId(&u));
  std::memcpy(id, &u, sizeof(u));
  return MAMG_OK;
}

void dist_destroy(DistHandle* h) {
  if (!h) return;
  (void)hipSetDevice(h->device);
  if (h->last) (void)hipEventSynchronize(h->last);   // the last apply / spmv / timing on any stream
  if (h->side) (void)hipStreamSynchronize(h->side);
  delete h;
}

int dist_dofs(const DistHandle* h) { return h->w; }
const Switches& dist_switches(const DistHandle* h) { return h->sw; }

void dist_range(const DistHandle* h, int64_t* o0, int64_t* o1, int64_t* nv) {
  *o0 = h->o0; *o1 = h->o1; *nv = h->nv0;
}

double dist_apply_bytes(const DistHandle* h) { return h->apply_bytes; }

int dist_num_levels(const DistHandle* h) { return (int)h->L.size(); }

// mamg_level_format's bits for the rank-local operators of a nodal level (0
// on a scalar handle: its levels are plain CSR)
int dist_level_format(const DistHandle* h, int level) {
  const DDLevel& D = h->L[level];
  if (h->w != 2) return 0;
  return (D.A.sell ? MAMG_FMT_SELL : 0) | (D.A.sym ? MAMG_FMT_SYM : 0) | (D.A.half ? MAMG_FMT_HALF : 0) |
         (D.PA.nr > 0 || D.K.nr > 0 ? MAMG_FMT_POST_FUSED : 0) | (D.K.nr > 0 ? MAMG_FMT_POST_K : 0) |
         (D.K.sell ? MAMG_FMT_POST_SELL : 0) | (D.A.nsched > 0 || D.A.nsched_r > 0 ? MAMG_FMT_BANDS : 0) |
         (D.patches ? MAMG_FMT_PATCHES : 0) | (D.gcs.size() > 1 ? MAMG_FMT_GS : 0) |
         (D.rings ? MAMG_FMT_RINGS : 0) | (D.R.nrsched > 0 ? MAMG_FMT_R_BANDS : 0) |
         (D.K.col16 ? MAMG_FMT_K_COL16 : 0);
}

// ---------------------------------------------------------------------------
// fp32 storage of the operators a rank's cycle streams
// (mamg_dist_set_cycle_storage): dev_set_cycle_storage
// on the rank-local operators.  A_loc (level 0: both value arrays of the
// half-symmetric form, owned part and ghost part), K_loc or plain P_loc and
// the partial restriction of every level above the coarsest become fp32
// copies in the same layout; W / Wk, the coarsest inverse, the merged
// [P_loc | AP_loc], every vector and every exchange buffer stay fp64, and so
// does level 0's A_loc itself (dspmv_ops: the Krylov operator), whose index
// arrays the fp32 copy Ac shares.  No communication: every rank calls it.
// ---------------------------------------------------------------------------
int dist_level_storage(const DistHandle* h, int level) { return h->L[level].storage; }

int dist_cycle_storage(const DistHandle* h) {
  for (const DDLevel& D : h->L)
    if (D.storage != 0) return MAMG_STORE_F32;
  return MAMG_STORE_F64;
}

int dist_set_cycle_storage(DistHandle* h, int storage, std::string* err) {
  std::lock_guard<std::recursive_mutex> lock(capture_mutex());
  const bool narrowed = dist_cycle_storage(h) == MAMG_STORE_F32;
  if (storage == MAMG_STORE_F64) {
    if (!narrowed) return MAMG_OK;
    *err = "cycle storage: the fp64 originals of a narrowed handle are gone (fp32 storage is one way)";
    return MAMG_ERR_UNSUPPORTED;
  }
  if (narrowed) return MAMG_OK;
  if (h->w != 2) {
    *err = "cycle storage: fp32 needs the BSR2 layout (this rank handle holds a scalar hierarchy in the CSR layout)";
    return MAMG_ERR_UNSUPPORTED;
  }
  for (const DDLevel& D : h->L) {
    if (D.patches) { *err = "cycle storage: fp32 is not available with SCHWARZ_PATCHES"; return MAMG_ERR_UNSUPPORTED; }
    if (D.rings) { *err = "cycle storage: fp32 is not available with SCHWARZ_RINGS"; return MAMG_ERR_UNSUPPORTED; }
    if (D.gcs.size() > 1) { *err = "cycle storage: fp32 is not available with the GS / SGS smoothers"; return MAMG_ERR_UNSUPPORTED; }
  }
  if (gs_smoother(h->p) || patch_schwarz(h->p) || rings_schwarz(h->p)) {
    *err = "cycle storage: fp32 is not available with the GS / SGS smoothers or the Schwarz smoothers";
    return MAMG_ERR_UNSUPPORTED;
  }
  HIPCHK(hipSetDevice(h->device));
  std::vector<NarrowJob> jobs;
  auto add = [&](DBsr* src, DBsr* dst) {
    if (value_count(*src) > 0) jobs.push_back({src, dst, false});
    if (ghost_value_count(*src) > 0) jobs.push_back({src, dst, true});
  };
  std::vector<int> bits(h->L.size(), 0);
  for (size_t l = 0; l < h->L.size(); ++l) {
    DDLevel& D = h->L[l];
    if (D.coarsest) break;
    add(&D.A, l == 0 ? &D.Ac : &D.A);
    add(&D.K, &D.K);
    add(&D.P, &D.P);
    add(&D.R, &D.R);
    // a merged [P_loc | AP_loc] (PA, MAMG_POST_K=0) stays fp64: bsr2_post_kernel has no fp32 side
    bits[l] = 1 | (D.PA.nr > 0 ? 0 : 2) | 4;
  }
  // wait for the rank's last work; the kernels below run on the null stream
  if (h->last) HIPCHK(hipEventSynchronize(h->last));
  if (h->side) HIPCHK(hipStreamSynchronize(h->side));
  if (h->cap) HIPCHK(hipStreamSynchronize(h->cap));
  // the cached graphs and PCG plans hold the fp64 op list: dropped, the next use captures anew
  auto drop_cached = [&]() {
    h->graphs.clear();
    release_all(&h->pcgs);
  };
  // the fp64 originals go back except level 0's A_loc (the Krylov operator)
  auto release = [&](void* old) {
    auto it = std::find(h->allocs.begin(), h->allocs.end(), old);
    if (!old || it == h->allocs.end()) return;
    (void)raw_free(old);
    h->allocs.erase(it);
  };
  int rc = narrow_values(jobs, &h->allocs, drop_cached, release, err);
  if (rc) return rc;
  for (size_t l = 0; l < h->L.size(); ++l) h->L[l].storage = bits[l];
  std::vector<DOp> ops;
  dapply_ops(h, nullptr, nullptr, &ops);
  h->apply_bytes = 0.0;
  for (const DOp& d : ops) h->apply_bytes += d.bytes;
  return MAMG_OK;
}

// What one distributed apply issues on a rank with P > 1 peers over RCCL
// (the same walk as run_dop, nothing launched): c[0] kernels, c[1] RCCL
// send / receive groups, c[2] point-to-point messages, c[3] all-reduces,
// c[4] stream forks (interior rows on the side stream).  With P == 1 only
// the kernels remain.
static void count_launches(const DistHandle* h, const std::vector<DOp>& ops, int64_t c[5]) {
  for (int k = 0; k < 5; ++k) c[k] = 0;
  const int P = h->nranks;
  for (const DOp& d : ops) {
    if (d.dk == D_OP || (P == 1 && d.dk == D_OVERLAP)) { ++c[0]; continue; }
    if (P == 1) continue;
    if (d.dk == D_ALLREDUCE) { ++c[3]; continue; }
    const DDLevel& D = h->L[d.level];
    const int64_t ns = D.send_off.back();
    if (d.dk == D_OVERLAP) { ++c[0]; ++c[4]; }
    if (d.dk == D_OVERLAP || d.dk == D_HALO) {
      if (ns) ++c[0];
      ++c[1];
      for (int q = 0; q < P; ++q) {
        if (q == h->rank) continue;
        c[2] += (D.send_off[q + 1] > D.send_off[q]) + (D.ghost_off[q + 1] > D.ghost_off[q]);
      }
    } else if (d.dk == D_CHALO) {
      const size_t b0 = (size_t)d.colour * (P + 1);
      c[0] += (D.cs_off[b0 + P] > D.cs_off[b0]) + (D.cg_off[b0 + P] > D.cg_off[b0]);
      ++c[1];
      for (int q = 0; q < P; ++q) {
        if (q == h->rank) continue;
        c[2] += (D.cs_off[b0 + q + 1] > D.cs_off[b0 + q]) + (D.cg_off[b0 + q + 1] > D.cg_off[b0 + q]);
      }
    } else {   // D_REVERSE
      ++c[1];
      for (int q = 0; q < P; ++q) {
        if (q == h->rank) continue;
        const bool sc = D.send_off[q + 1] > D.send_off[q], gc = D.ghost_off[q + 1] > D.ghost_off[q];
        c[2] += sc + gc;
        c[0] += sc;
      }
    }
  }
}

void dist_apply_launches(const DistHandle* h, int64_t c[5]) {
  std::vector<DOp> ops;
  dapply_ops(h, nullptr, nullptr, &ops);
  count_launches(h, ops, c);
}

int dist_apply(DistHandle* h, const double* d_r, double* d_z, void* stream, std::string* err) {
  HIPCHK(hipSetDevice(h->device));
  std::vector<DOp> ops;
  dapply_ops(h, d_r, d_z, &ops);
  int rc = h->wait((hipStream_t)stream, err);
  if (rc) return rc;
  for (const DOp& d : ops) {
    if ((rc = run_dop(h, d, (hipStream_t)stream, err))) return rc;
  }
  HIPCHK(hipGetLastError());
  return h->mark((hipStream_t)stream, err);
}

int dist_spmv(DistHandle* h, const double* d_x, double* d_y, void* stream, std::string* err) {
  HIPCHK(hipSetDevice(h->device));
  if (h->L.empty() || h->L[0].coarsest) { *err = "single-level hierarchy: no distributed operator"; return MAMG_ERR_ARG; }
  std::vector<DOp> ops;
  dspmv_ops(h, d_x, d_y, &ops);
  int rc = h->wait((hipStream_t)stream, err);
  if (rc) return rc;
  for (const DOp& d : ops) {
    if ((rc = run_dop(h, d, (hipStream_t)stream, err))) return rc;
  }
  HIPCHK(hipGetLastError());
  return h->mark((hipStream_t)stream, err);
}

// The op list of one apply captured into a hipGraph on the handle's capture
// stream: kernels, the side-stream fork of the interior rows (events), and
// the RCCL send / receive groups and all-reduces inside the capture.  A
// failed capture leaves nothing behind and is reported (the caller stays
// eager).
int dist_capture(DistHandle* h, const std::vector<DOp>& ops, CapturedGraph* g, std::string* err) {
  return capture_graph(&h->cap, [&]() {
    int rc = MAMG_OK;
    for (const DOp& d : ops)
      if ((rc = run_dop(h, d, h->cap, err))) break;
    return rc;
  }, "distributed apply", g, err);
}

int dist_graph_exec(DistHandle* h, const double* d_r, double* d_z, hipGraphExec_t* ex, std::string* err) {
  if (!h->comm && h->nranks > 1 && !h->dry) {
    *err = "graph replay needs an RCCL communicator (or one rank): host-staged and virtual exchanges run eagerly";
    return MAMG_ERR_UNSUPPORTED;
  }
  if (!h->graph_err.empty()) { *err = "graph capture failed on this handle: " + h->graph_err; return MAMG_ERR_UNSUPPORTED; }
  return h->graphs.get(d_r, d_z, h->last, [&](CapturedGraph* g) {
    std::vector<DOp> ops;
    dapply_ops(h, d_r, d_z, &ops);
    const int rc = dist_capture(h, ops, g, err);
    if (rc) h->graph_err = *err;
    return rc;
  }, ex, err);
}

int dist_graph_prepare(DistHandle* h, const double* d_r, double* d_z, std::string* err) {
  HIPCHK(hipSetDevice(h->device));
  hipGraphExec_t ex = nullptr;
  return dist_graph_exec(h, d_r, d_z, &ex, err);
}

int dist_apply_graph(DistHandle* h, const double* d_r, double* d_z, void* stream, std::string* err) {
  HIPCHK(hipSetDevice(h->device));
  hipGraphExec_t ex = nullptr;
  int rc = dist_graph_exec(h, d_r, d_z, &ex, err);
  if (rc) return rc;
  if ((rc = h->wait((hipStream_t)stream, err))) return rc;
  HIPCHK(hipGraphLaunch(ex, (hipStream_t)stream));
  return h->mark((hipStream_t)stream, err);
}

int dist_time_apply(DistHandle* h, const double* d_r, double* d_z, int reps, int mode, double* ms,
                    double* kernel_ms, double* class_bytes, void* stream, std::string* err) {
  HIPCHK(hipSetDevice(h->device));
  hipStream_t s = (hipStream_t)stream;
  std::vector<DOp> ops;
  dapply_ops(h, d_r, d_z, &ops);
  if (class_bytes) {
    for (int c = 0; c < 16; ++c) class_bytes[c] = 0.0;
    for (const DOp& d : ops) class_bytes[d.cls] += d.bytes;
  }
  if (reps <= 0) { *ms = 0.0; return MAMG_OK; }
  if (mode == 2) {   // graph replays, events around the whole run only
    hipGraphExec_t ex = nullptr;
    int rc = dist_graph_exec(h, d_r, d_z, &ex, err);
    if (rc) return rc;
    if ((rc = h->wait(s, err))) return rc;
    TimedRun tr;
    if ((rc = tr.create(2, err))) return rc;
    HIPCHK(hipEventRecord(tr.ev[0], s));
    for (int rp = 0; rp < reps; ++rp) HIPCHK(hipGraphLaunch(ex, s));
    HIPCHK(hipEventRecord(tr.ev[1], s));
    HIPCHK(hipEventSynchronize(tr.ev[1]));
    float t = 0.f;
    HIPCHK(hipEventElapsedTime(&t, tr.ev[0], tr.ev[1]));
    *ms = t / reps;
    if (kernel_ms)
      for (int c = 0; c < 16; ++c) kernel_ms[c] = 0.0;
    return h->mark(s, err);
  }
  int rc;
  if ((rc = h->wait(s, err))) return rc;
  TimedRun tr;
  return tr.run(ops.size(), [&](size_t k) { return ops[k].cls; }, [&](size_t k) { return run_dop(h, ops[k], s, err); },
                reps, mode, s, nullptr, ms, kernel_ms, err);
}

// ---------------------------------------------------------------------------
// Virtual communicator (tests on a single GPU): P rank handles on one device,
// executed in lockstep on one stream; exchanges are device copies between the
// ranks' buffers with exactly the counts/offsets the RCCL path uses.
// ---------------------------------------------------------------------------

// P ranks' op lists in lockstep on one stream
int virtual_run(const std::vector<DistHandle*>& hs, const std::vector<std::vector<DOp>>& ops, hipStream_t s,
                std::string* err, bool mark = true) {
  const int P = (int)hs.size(), w = hs[0]->w;
  for (int p = 1; p < P; ++p)
    if (hs[p]->w != w) { *err = "rank handles of different layouts"; return MAMG_ERR_ARG; }
  for (int p = 1; p < P; ++p)
    if (ops[p].size() != ops[0].size()) { *err = "rank schedules differ"; return MAMG_ERR_SETUP; }
  for (size_t k = 0; k < ops[0].size(); ++k) {
    const int dk = ops[0][k].dk;
    if (dk == D_OP) {
      for (int p = 0; p < P; ++p) launch(ops[p][k].op, s);
    } else if (dk == D_HALO || dk == D_OVERLAP) {
      if (dk == D_OVERLAP)
        for (int p = 0; p < P; ++p) launch(ops[p][k].op, s);
      for (int p = 0; p < P; ++p) {
        const DDLevel& D = hs[p]->L[ops[p][k].level];
        const int64_t ns = D.send_off.back();
        if (ns) pack_w(w, ns, D.send_idx, ops[p][k].buf, D.sendbuf, s);
      }
      for (int p = 0; p < P; ++p) {          // p receives from q
        const DDLevel& D = hs[p]->L[ops[p][k].level];
        for (int q = 0; q < P; ++q) {
          if (q == p) continue;
          const int64_t gc = D.ghost_off[q + 1] - D.ghost_off[q];
          if (!gc) continue;
          const DDLevel& Q = hs[q]->L[ops[q][k].level];
          const int64_t sc = Q.send_off[p + 1] - Q.send_off[p];
          if (sc != gc) { *err = "halo count mismatch"; return MAMG_ERR_SETUP; }
          HIPCHK(dev_copy(ops[p][k].buf + w * (D.nloc + D.ghost_off[q]), Q.sendbuf + w * Q.send_off[p], w * gc * sizeof(double), s));
        }
      }
    } else if (dk == D_CHALO) {
      const int c = ops[0][k].colour;
      const size_t b0 = (size_t)c * (P + 1);
      for (int p = 0; p < P; ++p) {
        const DDLevel& D = hs[p]->L[ops[p][k].level];
        const int64_t s0 = D.cs_off[b0], s1 = D.cs_off[b0 + P];
        if (s1 > s0)
          pack_w(w, s1 - s0, D.csend_idx + s0, ops[p][k].buf, D.sendbuf + w * s0, s);
      }
      for (int p = 0; p < P; ++p) {          // p receives colour c's ghosts from q
        const DDLevel& D = hs[p]->L[ops[p][k].level];
        for (int q = 0; q < P; ++q) {
          if (q == p) continue;
          const int64_t gc = D.cg_off[b0 + q + 1] - D.cg_off[b0 + q];
          const DDLevel& Q = hs[q]->L[ops[q][k].level];
          const int64_t sc = Q.cs_off[b0 + p + 1] - Q.cs_off[b0 + p];
          if (sc != gc) { *err = "colour halo count mismatch"; return MAMG_ERR_SETUP; }
          if (!gc) continue;
          HIPCHK(dev_copy(D.recvbuf + w * D.cg_off[b0 + q], Q.sendbuf + w * Q.cs_off[b0 + p], w * gc * sizeof(double), s));
        }
      }
      for (int p = 0; p < P; ++p) {
        const DDLevel& D = hs[p]->L[ops[p][k].level];
        const int64_t g0 = D.cg_off[b0], g1 = D.cg_off[b0 + P];
        if (g1 > g0)
          unpack_w(w, g1 - g0, D.cghost_idx + g0, D.nloc, D.recvbuf + w * g0, ops[p][k].buf, s);
      }
    } else if (dk == D_REVERSE) {
      for (int q = 0; q < P; ++q) {          // owner q receives partials from p
        const DDLevel& Q = hs[q]->L[ops[q][k].level];
        for (int p = 0; p < P; ++p) {
          if (p == q) continue;
          const int64_t sc = Q.send_off[p + 1] - Q.send_off[p];
          if (!sc) continue;
          const DDLevel& D = hs[p]->L[ops[p][k].level];
          const int64_t gc = D.ghost_off[q + 1] - D.ghost_off[q];
          if (sc != gc) { *err = "reverse count mismatch"; return MAMG_ERR_SETUP; }
          HIPCHK(dev_copy(Q.recvbuf + w * Q.send_off[p], ops[p][k].buf + w * (D.nloc + D.ghost_off[q]), w * sc * sizeof(double), s));
        }
      }
      for (int q = 0; q < P; ++q) {
        const DDLevel& Q = hs[q]->L[ops[q][k].level];
        for (int p = 0; p < P; ++p) {
          const int64_t sc = Q.send_off[p + 1] - Q.send_off[p];
          if (p == q || !sc) continue;
          addidx_w(w, sc, Q.send_idx + Q.send_off[p], Q.recvbuf + w * Q.send_off[p], ops[q][k].buf, s);
        }
      }
    } else {                                 // D_ALLREDUCE: sum in rank order
      const int64_t n = ops[0][k].count;
      for (int p = 1; p < P; ++p)
        vsum(n, ops[p][k].buf, ops[0][k].buf, s);
      for (int p = 1; p < P; ++p)
        HIPCHK(dev_copy(ops[p][k].buf, ops[0][k].buf, n * sizeof(double), s));
    }
  }
  HIPCHK(hipGetLastError());
  if (mark)
    for (DistHandle* h : hs) {
      const int rc = h->mark(s, err);
      if (rc) return rc;
    }
  return MAMG_OK;
}

int dist_set_exchange(DistHandle* h, const mamg_exchange& ex, std::string* err) {
  if (h->comm) { *err = "handle has an RCCL communicator; the host exchange is for comm_id == NULL"; return MAMG_ERR_ARG; }
  HIPCHK(hipSetDevice(h->device));
  auto pin = [&](double** p, int64_t n) -> int {
    *p = nullptr;
    if (n <= 0) return MAMG_OK;
    void* q = nullptr;
    HIPCHK(hipHostMalloc(&q, n * sizeof(double), hipHostMallocDefault));
    h->pinned.push_back(q);
    *p = (double*)q;
    return MAMG_OK;
  };
  if (!h->host_ex) {
    int64_t red = 0;
    const int w = h->w;
    const int nl = (int)h->L.size();
    h->hsend.assign(nl, nullptr);
    h->hghost.assign(nl, nullptr);
    h->hrecv.assign(nl, nullptr);
    for (int l = 0; l < nl; ++l) {
      const DDLevel& D = h->L[l];
      const int64_t ns = D.send_off.empty() ? 0 : D.send_off.back();
      const int64_t tcs = D.cs_off.empty() ? 0 : D.cs_off.back(), tcg = D.cg_off.empty() ? 0 : D.cg_off.back();
      int rc;
      if ((rc = pin(&h->hsend[l], w * std::max(ns, tcs))) || (rc = pin(&h->hghost[l], w * std::max(D.ng, tcg))) ||
          (rc = pin(&h->hrecv[l], w * ns)))
        return rc;
      red = std::max(red, w * D.nv);
    }
    red = std::max<int64_t>(red, 2 * SCALE_BLOCKS);   // coarse scaling partials
    red = std::max<int64_t>(red, 3 * (int64_t)h->nranks);   // the PCG dots' P-vectors (dist_pcg)
    int rc = pin(&h->hred, red);
    if (rc) return rc;
  }
  h->ex = ex;
  h->host_ex = true;
  return MAMG_OK;
}

int dist_virtual_apply(const std::vector<DistHandle*>& hs, const std::vector<const double*>& r,
                       const std::vector<double*>& z, void* stream, std::string* err) {
  const int P = (int)hs.size();
  HIPCHK(hipSetDevice(hs[0]->device));
  std::vector<std::vector<DOp>> ops(P);
  for (int p = 0; p < P; ++p) dapply_ops(hs[p], r[p], z[p], &ops[p]);
  int rc;
  for (DistHandle* h : hs)
    if ((rc = h->wait((hipStream_t)stream, err))) return rc;
  return virtual_run(hs, ops, (hipStream_t)stream, err);
}

// the virtual ranks' lockstep apply captured into one hipGraph (rank 0's
// capture stream), launched once and destroyed: the graph path's kernels,
// forks and exchange order, checked bitwise against the eager lockstep run
int dist_virtual_apply_graph(const std::vector<DistHandle*>& hs, const std::vector<const double*>& r,
                             const std::vector<double*>& z, void* stream, std::string* err) {
  const int P = (int)hs.size();
  HIPCHK(hipSetDevice(hs[0]->device));
  std::vector<std::vector<DOp>> ops(P);
  for (int p = 0; p < P; ++p) dapply_ops(hs[p], r[p], z[p], &ops[p]);
  DistHandle* h0 = hs[0];
  CapturedGraph g;
  int rc = capture_graph(&h0->cap, [&]() { return virtual_run(hs, ops, h0->cap, err, false); }, "virtual apply", &g,
                         err);
  if (rc) return rc;
  for (DistHandle* h : hs)
    if ((rc = h->wait((hipStream_t)stream, err))) { g.drop(); return rc; }
  const hipError_t el = hipGraphLaunch(g.exec, (hipStream_t)stream);
  const hipError_t es = hipStreamSynchronize((hipStream_t)stream);
  g.drop();
  if (el != hipSuccess || es != hipSuccess) {
    *err = std::string("virtual apply graph launch: ") + hipGetErrorString(el != hipSuccess ? el : es);
    return MAMG_ERR_HIP;
  }
  for (DistHandle* h : hs)
    if ((rc = h->mark((hipStream_t)stream, err))) return rc;
  return MAMG_OK;
}

int dist_virtual_spmv(const std::vector<DistHandle*>& hs, const std::vector<const double*>& x,
                      const std::vector<double*>& y, void* stream, std::string* err) {
  const int P = (int)hs.size();
  HIPCHK(hipSetDevice(hs[0]->device));
  std::vector<std::vector<DOp>> ops(P);
  for (int p = 0; p < P; ++p) {
    if (hs[p]->L.empty() || hs[p]->L[0].coarsest) { *err = "single-level hierarchy"; return MAMG_ERR_ARG; }
    dspmv_ops(hs[p], x[p], y[p], &ops[p]);
  }
  int rc;
  for (DistHandle* h : hs)
    if ((rc = h->wait((hipStream_t)stream, err))) return rc;
  return virtual_run(hs, ops, (hipStream_t)stream, err);
}

namespace {

// ---------------------------------------------------------------------------
// Device-resident PCG on row-partitioned ranks: dev_pcg's loop
// with the operator, the preconditioner and the dots as one DOp list per
// iteration, so the RCCL, captured-graph, host-staged and virtual backends
// all execute the same schedule.
// ---------------------------------------------------------------------------

void append(std::vector<DOp>* ops, const std::vector<DOp>& more) { ops->insert(ops->end(), more.begin(), more.end()); }

DOp pcg_op(int kind, const DPcgCtx* c, double bytes, int64_t n = 0) {
  Op o;
  o.kind = kind; o.cls = C_MISC; o.pcg = c; o.n = n; o.bytes = bytes;
  return wrap(o);
}

// the rank's partials of <a, b> (dot 0), its slot in each of the nd
// P-vectors (dots 1, 2: partials already written by the pass before), and
// the all-reduce of the nd P-vectors
void dpcg_dot_ops(const DPcgCtx* c, const double* a, const double* b, int nd, std::vector<DOp>* ops) {
  DOp d = pcg_op(OP_PDOT, c, 16.0 * c->n);
  d.op.x = a; d.op.y = b;
  ops->push_back(d);
  ops->push_back(pcg_op(OP_PSLOT, c, 8.0 * nd * DOT_BLOCKS, nd));
  DOp r;
  r.dk = D_ALLREDUCE; r.cls = C_COMM; r.buf = c->pv; r.count = (int64_t)nd * c->P; r.bytes = 16.0 * r.count;
  ops->push_back(r);
}

// one iteration: q = A d, <d,q>, alpha, x / r update (+ ||r||^2 partials),
// z = B r, <r,z> (and ||r||^2), beta + histories + stop test, d update.  An
// inactive iteration issues every op and every exchange; the state's flags
// mask the x, r and d updates only.
void dpcg_iter_ops(const DistHandle* h, const DPcgCtx* c, std::vector<DOp>* ops) {
  ops->clear();
  std::vector<DOp> part;
  dspmv_ops(h, c->d, c->q, &part);
  append(ops, part);
  dpcg_dot_ops(c, c->d, c->q, 1, ops);
  ops->push_back(pcg_op(OP_PALPHA, c, 0.0));
  ops->push_back(pcg_op(OP_PXR, c, 48.0 * c->n));
  dapply_ops(h, c->r, c->z, &part);
  append(ops, part);
  dpcg_dot_ops(c, c->r, c->z, c->stop ? 2 : 1, ops);
  ops->push_back(pcg_op(OP_PBETA, c, 0.0));
  ops->push_back(pcg_op(OP_PD, c, 24.0 * c->n));
}

// start-up: r = b - A x0, z = B r, d = z, <r,z> (and ||r||^2, ||b||^2), first state
void dpcg_start_ops(const DistHandle* h, const DPcgCtx* c, std::vector<DOp>* ops) {
  ops->clear();
  std::vector<DOp> part;
  dspmv_ops(h, c->x, c->q, &part);
  append(ops, part);
  ops->push_back(pcg_op(OP_PR0, c, 24.0 * c->n));
  dapply_ops(h, c->r, c->z, &part);
  append(ops, part);
  Op cp;
  cp.kind = OP_COPY; cp.cls = C_MISC; cp.n = c->n; cp.x = c->z; cp.out = c->d; cp.bytes = 16.0 * c->n;
  ops->push_back(wrap(cp));
  dpcg_dot_ops(c, c->r, c->z, c->stop ? 3 : 1, ops);
  ops->push_back(pcg_op(OP_PINIT, c, 0.0));
}

int dpcg_check(const DistHandle* h, int maxiter, int stop, const double* rnorms, std::string* err) {
  if (stop != 0 && stop != 1) { *err = "stop_type must be 0 (cbc.block) or 1 (||r|| <= tol ||b||)"; return MAMG_ERR_ARG; }
  if (maxiter < 0) { *err = "maxiter must be >= 0"; return MAMG_ERR_ARG; }
  if (stop == 1 && !rnorms) { *err = "stop_type 1 needs the rnorms history"; return MAMG_ERR_ARG; }
  if (h->L.empty() || h->L[0].coarsest) { *err = "single-level hierarchy: no distributed operator"; return MAMG_ERR_ARG; }
  return MAMG_OK;
}

// the handle's plan for (x, maxiter, stop): work buffers on first use,
// histories and the ops' context per plan (at most 4, the oldest evicted
// once the handle's work is done); slots: host mirrors of the state wanted
int dpcg_plan(DistHandle* h, double* x, int maxiter, int stop, int slots, DistHandle::PcgPlan** out,
              std::string* err) {
  int rc;
  const int64_t n = (int64_t)h->w * h->L[0].nloc;
  if (!h->pst) {
    double** v[] = {&h->cr, &h->cz, &h->cd, &h->cq};
    for (double** q : v)
      if ((rc = ddalloc(h, q, std::max<int64_t>(n, 1), err))) return rc;
    if ((rc = ddalloc(h, &h->ppart, 3 * DOT_BLOCKS, err))) return rc;
    if ((rc = ddalloc(h, &h->pv, 3 * (int64_t)h->nranks, err))) return rc;
    if ((rc = ddalloc(h, &h->pst, 1, err))) return rc;
  }
  if (h->hst_ranks < slots) {
    if (h->last) HIPCHK(hipEventSynchronize(h->last));
    if (h->hst) HIPCHK(hipHostFree(h->hst));
    h->hst = nullptr;
    h->hst_ranks = 0;
    HIPCHK(hipHostMalloc((void**)&h->hst, 2 * (size_t)slots * sizeof(DPcgState), hipHostMallocDefault));
    h->hst_ranks = slots;
  }
  for (auto& q : h->pcgs)
    if (q.c->x == x && q.c->maxiter == maxiter && q.c->stop == stop) { *out = &q; return MAMG_OK; }
  if (h->pcgs.size() >= 4) {
    if (h->last) HIPCHK(hipEventSynchronize(h->last));
    h->pcgs.front().release();
    h->pcgs.erase(h->pcgs.begin());
  }
  DistHandle::PcgPlan q;
  if ((rc = q.alloc(4 * (size_t)maxiter + 2, err))) return rc;
  q.c.reset(new DPcgCtx());
  DPcgCtx& c = *q.c;
  c.st = h->pst; c.n = n; c.P = h->nranks; c.rank = h->rank; c.stop = stop; c.maxiter = maxiter;
  c.x = x; c.r = h->cr; c.z = h->cz; c.d = h->cd; c.q = h->cq; c.part = h->ppart; c.pv = h->pv;
  c.res = q.hist; c.rn = c.res + maxiter + 1; c.al = c.rn + maxiter + 1; c.be = c.al + maxiter;
  h->pcgs.push_back(std::move(q));
  *out = &h->pcgs.back();
  return MAMG_OK;
}

// histories and the return code from the final state (pcg_finish, device.hip)
int dpcg_finish(const DPcgCtx& c, const DPcgState& fin, double* residuals, double* rnorms, double* alphas,
                double* betas, int* niters, std::string* err) {
  return pcg_finish(fin.status, fin.it, {c.res, c.stop ? c.rn : nullptr, c.al, c.be}, residuals, rnorms, alphas, betas,
                    niters, err);
}

}  // namespace

void dist_pcg_launches(const DistHandle* h, int stop, int64_t c[5]) {
  DPcgCtx ctx;
  ctx.P = h->nranks; ctx.rank = h->rank; ctx.stop = stop; ctx.n = (int64_t)h->w * h->L[0].nloc;
  std::vector<DOp> ops;
  dpcg_iter_ops(h, &ctx, &ops);
  count_launches(h, ops, c);
}

int dist_pcg(DistHandle* h, const double* d_b, double* d_x, double tol, int maxiter, int relativeconv,
             int stop, double* residuals, double* rnorms, double* alphas, double* betas, int* niters,
             void* stream, std::string* err) {
  int rc;
  if ((rc = dpcg_check(h, maxiter, stop, rnorms, err))) return rc;
  if (!h->comm && h->nranks > 1 && !h->host_ex && !h->dry) {
    *err = "virtual rank handle (no communicator): use mamg_dist_virtual_pcg";
    return MAMG_ERR_ARG;
  }
  HIPCHK(hipSetDevice(h->device));
  hipStream_t s = (hipStream_t)stream;
  DistHandle::PcgPlan* pl = nullptr;
  if ((rc = dpcg_plan(h, d_x, maxiter, stop, 1, &pl, err))) return rc;
  DPcgCtx& c = *pl->c;
  c.b = d_b; c.tol = tol; c.relconv = relativeconv;
  DPcgState* st = h->pst;
  DPcgState* hst = h->hst;
  std::vector<DOp> ops;
  dpcg_iter_ops(h, &c, &ops);
  // one iteration as one hipGraph (RCCL calls inside) on an RCCL or
  // single-rank handle; a failed capture is recorded and the same op list
  // runs eagerly -- the RCCL sequence of a rank is the same either way
  const bool graphable = (h->comm || h->nranks == 1) && h->graph_err.empty() && h->pcg_graph_err.empty();
  if (graphable && !pl->exec) {
    std::string cerr;
    if (dist_capture(h, ops, pl, &cerr)) h->pcg_graph_err = cerr;
  }
  if ((rc = h->wait(s, err))) return rc;   // the work buffers are the handle's
  std::vector<DOp> start;
  dpcg_start_ops(h, &c, &start);
  for (const DOp& d : start)
    if ((rc = run_dop(h, d, s, err))) return rc;
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(&hst[0], st, sizeof(DPcgState), hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  if (hst[0].status == PCG_NOT_POS) {
    (void)h->mark(s, err);
    return dpcg_finish(c, hst[0], residuals, rnorms, alphas, betas, niters, err);
  }
  if (hst[0].active) {
    // iteration k's state lands in hst[k & 1].  The host-staged exchange
    // synchronises at every exchange, so its state is read after each
    // iteration; otherwise iteration k + 1 is queued before the host waits
    // for iteration k.  Either way the number of iterations a rank issues
    // depends on all-reduced state only: the same on every rank.
    const bool ahead = !(h->host_ex && !h->comm);
    for (int k = 0; k < maxiter; ++k) {
      if (pl->exec) {
        HIPCHK(hipGraphLaunch(pl->exec, s));
      } else {
        for (const DOp& d : ops)
          if ((rc = run_dop(h, d, s, err))) return rc;
      }
      HIPCHK(hipMemcpyAsync(&hst[k & 1], st, sizeof(DPcgState), hipMemcpyDeviceToHost, s));
      HIPCHK(hipEventRecord(pl->ev[k & 1], s));
      if (ahead && k == 0) continue;
      const int w = ahead ? (k - 1) & 1 : k & 1;
      HIPCHK(hipEventSynchronize(pl->ev[w]));
      if (!hst[w].active) break;
    }
  }
  HIPCHK(hipMemcpyAsync(&hst[0], st, sizeof(DPcgState), hipMemcpyDeviceToHost, s));
  if ((rc = h->mark(s, err))) return rc;
  HIPCHK(hipStreamSynchronize(s));
  HIPCHK(hipGetLastError());
  return dpcg_finish(c, hst[0], residuals, rnorms, alphas, betas, niters, err);
}

// test mode: the ranks' op lists in lockstep (virtual_run), eager or as one
// captured lockstep iteration replayed; every rank's state is compared with
// rank 0's, byte for byte, whenever it is read back
int dist_virtual_pcg(const std::vector<DistHandle*>& hs, const std::vector<const double*>& b,
                     const std::vector<double*>& x, double tol, int maxiter, int relativeconv, int stop,
                     int graph, double* residuals, double* rnorms, double* alphas, double* betas, int* niters,
                     void* stream, std::string* err) {
  const int P = (int)hs.size();
  int rc;
  for (int p = 0; p < P; ++p) {
    if ((rc = dpcg_check(hs[p], maxiter, stop, rnorms, err))) return rc;
    if (hs[p]->nranks != P || hs[p]->rank != p) { *err = "rank handles do not form ranks 0..n-1 of n"; return MAMG_ERR_ARG; }
  }
  DistHandle* h0 = hs[0];
  HIPCHK(hipSetDevice(h0->device));
  hipStream_t s = (hipStream_t)stream;
  std::vector<DistHandle::PcgPlan*> pl(P, nullptr);
  std::vector<std::vector<DOp>> start(P), ops(P);
  for (int p = 0; p < P; ++p) {
    if ((rc = dpcg_plan(hs[p], x[p], maxiter, stop, p == 0 ? P : 1, &pl[p], err))) return rc;
    DPcgCtx& c = *pl[p]->c;
    c.b = b[p]; c.tol = tol; c.relconv = relativeconv;
    dpcg_start_ops(hs[p], &c, &start[p]);
    dpcg_iter_ops(hs[p], &c, &ops[p]);
    if ((rc = hs[p]->wait(s, err))) return rc;
  }
  DPcgState* hst = h0->hst;                    // [2][P]
  auto read_states = [&](int slot) -> int {
    for (int p = 0; p < P; ++p)
      HIPCHK(hipMemcpyAsync(&hst[(size_t)slot * P + p], hs[p]->pst, sizeof(DPcgState), hipMemcpyDeviceToHost, s));
    return MAMG_OK;
  };
  auto same_states = [&](int slot, int k) -> int {
    for (int p = 1; p < P; ++p)
      if (std::memcmp(&hst[(size_t)slot * P + p], &hst[(size_t)slot * P], sizeof(DPcgState))) {
        *err = "virtual PCG: rank " + std::to_string(p) + "'s state differs from rank 0's after iteration " +
               std::to_string(k);
        return MAMG_ERR_SETUP;
      }
    return MAMG_OK;
  };
  CapturedGraph g;
  if (graph && maxiter > 0 &&
      (rc = capture_graph(&h0->cap, [&]() { return virtual_run(hs, ops, h0->cap, err, false); },
                          "virtual PCG iteration", &g, err)))
    return rc;
  // from here on every exit drains the stream and drops the graph
  auto body = [&]() -> int {
    int r;
    if ((r = virtual_run(hs, start, s, err, false))) return r;
    if ((r = read_states(0))) return r;
    HIPCHK(hipStreamSynchronize(s));
    if ((r = same_states(0, 0))) return r;
    if (hst[0].status == PCG_NOT_POS || !hst[0].active) return MAMG_OK;
    for (int k = 0; k < maxiter; ++k) {
      if (g.exec) HIPCHK(hipGraphLaunch(g.exec, s));
      else if ((r = virtual_run(hs, ops, s, err, false))) return r;
      if ((r = read_states(k & 1))) return r;
      HIPCHK(hipEventRecord(pl[0]->ev[k & 1], s));
      if (k == 0) continue;
      const int w = (k - 1) & 1;
      HIPCHK(hipEventSynchronize(pl[0]->ev[w]));
      if ((r = same_states(w, k))) return r;
      if (!hst[(size_t)w * P].active) break;
    }
    if ((r = read_states(0))) return r;
    HIPCHK(hipStreamSynchronize(s));
    return same_states(0, hst[0].it);
  };
  rc = body();
  for (DistHandle* h : hs) {
    std::string merr;
    (void)h->mark(s, &merr);
  }
  (void)hipStreamSynchronize(s);
  g.drop();
  if (rc) return rc;
  HIPCHK(hipGetLastError());
  return dpcg_finish(*pl[0]->c, hst[0], residuals, rnorms, alphas, betas, niters, err);
}

}  // namespace mamg
