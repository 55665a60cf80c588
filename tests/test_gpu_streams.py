"""Every stream-taking entry point of the C-ABI on a stream the caller created.

Everywhere else in the suite the stream is None or torch's current stream,
which is the legacy null stream: there a launch that forgets its stream
argument, a graph launched on the wrong stream, a fork event recorded on the
wrong stream and a missing wait on the handle's last event all give the right
answer.  Here every call runs on a torch.cuda.Stream() behind pending work
(tests/stream_cases.py): the inputs sit in buffers that hold NaN until a copy
queued on the user stream behind a delay fills them, and the library call is
issued at once, so anything the library runs off the caller's stream reads
NaN or stale vectors.  Each call of a test uses a right-hand side the handle
has not seen, so stale work vectors cannot pass for right ones.

What every parity case compares:
  (i)  the same handle's result for the same input in the same buffers on the
       null stream, bit for bit (replays are deterministic);
  (ii) the oracle's apply within APPLY_TOL = 1e-10, the SpMV within the per-row
       rounding bound of tests/test_gpu_sizes.py part b, a PCG against the
       oracle's iteration count, its residual history to rtol 1e-6 and its
       solution to 1e-6 (the existing PCG tests' comparison).
No tolerance of its own.

  a  one handle, one user stream: each launch site of launch() and of the PCG
  b  rank handles: virtual ranks, the one-rank RCCL handle, a scalar plan
  c  one handle used on two streams in turn: the handle orders the calls
  d  two handles on two streams, enqueued alternately

Every id asserts the control (stream_cases.streams) and, per call, that the
delay was still pending when the call returned (asynchronous calls) or
immediately before it (calls that synchronise inside).  The contract under
test: include/mamg.h, "Streams and ordering"; DESIGN.md section 2.3.3.
"""
import contextlib
import functools
import itertools

import numpy as np
import pytest

import dist_csr_ref as dc
import mamg_oracle as mo
import size_cases as sc
import stream_cases as st
import tail_cases as tc
import test_gpu_point_rings as tpr
import test_gpu_rings as tgr
import test_gpu_sizes as gs
import test_gpu_tail as tgt
from conftest import set_opt
from cycle_storage_ref import ALL, StorageRef
from test_gpu import APPLY_TOL, rel
from test_gpu_cycle_storage import bits

pytestmark = pytest.mark.gpu

CD = sc.COARSE_DOF
PATCHES = 6
PCG_TOL, PCG_MAXIT = 1e-8, 500
_seed = itertools.count(20000)      # every vector of this file from a seed of its own


def _mamg():
    import metric_amg_examples_amd as M
    return M


def _torch():
    import torch
    return torch


def fresh(n):
    """(host vector, its device copy) from a seed no call has used before."""
    torch = _torch()
    v = mo.seeded_rhs(n, next(_seed))
    return v, torch.as_tensor(v).cuda()


def nan(n):
    torch = _torch()
    return torch.full((n,), float('nan'), dtype=torch.float64, device='cuda')


def host(t):
    _torch().cuda.synchronize()
    return t.cpu().numpy()


class Errors:
    """Collects the failed calls of one id, so that an id names every call
    that went wrong and not only the first."""

    def __init__(self):
        self.msgs = []

    @contextlib.contextmanager
    def call(self, label):
        try:
            yield
        except AssertionError as e:
            self.msgs.append('%s: %s' % (label, str(e).splitlines()[0] if str(e) else type(e).__name__))
            _torch().cuda.synchronize()

    def check(self):
        assert not self.msgs, '%d call(s) failed:\n  ' % len(self.msgs) + '\n  '.join(self.msgs)


@pytest.fixture
def user_streams(lib_built):
    """(s1, s2) with the control asserted for this id."""
    return st.streams()


def spmv_bound_ok(A, x, y):
    """tests/test_gpu_sizes.py part b: |y_i - ref_i| <= (len_i + 2) 2^-53 sum_j |a_ij x_j|."""
    prod = A.data.astype(np.longdouble) * x[A.indices].astype(np.longdouble)
    ref = np.add.reduceat(prod, A.indptr[:-1])
    mag = np.add.reduceat(np.abs(prod), A.indptr[:-1])
    bound = (np.diff(A.indptr) + 2) * np.longdouble(2.0) ** -53 * mag
    err = np.abs(y.astype(np.longdouble) - ref)
    assert np.isfinite(y).all(), 'non-finite SpMV result'
    worst = int(np.argmax(err - bound))
    assert np.all(err <= bound), 'SpMV row %d off by %.3e (bound %.3e)' % (worst, float(err[worst]),
                                                                          float(bound[worst]))


def assert_pcg(res, x, ref):
    gs.assert_history(res, ref.residuals)
    assert rel(x, ref.x) < 1e-6, 'PCG solution off by %.3e' % rel(x, ref.x)


# ---------------------------------------------------------------------------
# a. one handle, one user stream
# ---------------------------------------------------------------------------
class Case:
    """build() -> a fresh MetricAMG (called twice: the handle under test and
    its twin, which only times the calls on the idle null stream, in the same
    state); check(B) asserts the branch; ref(B) -> the reference apply;
    after(B, class_bytes) asserts what only shows after the applies."""

    def __init__(self, build, check, ref, after=None, tol=APPLY_TOL):
        self.build, self.check, self.ref, self.after, self.tol = build, check, ref, after, tol


def _half_build():
    return gs.build('stencil3d', 257, 'sell', 'gpu')


def _half_check(B):
    gs.check_mode(B, 'sell')            # half-symmetric A_0, SELL K with 16-bit columns
    print('level 0 format', B.level_format(0))


def _bsr2_check(B):
    gs.check_mode(B, 'default')
    assert B.num_levels == len(sc.HIER[('slice', 257)])


def _poly_build():
    set_opt('MAMG_TAIL_NODES', '0')     # the launch path on every level: dot2_partial_kernel, cscale_kernel
    return gs.build('slice', 257, 'default', 'gpu', cycle_type='W', smoother='POLY', poly_degree=3, coarse_scaling=1)


def _poly_check(B):
    p = B.effective_params
    assert (p['smoother'], p['poly_degree'], p['cycle_type'], p['coarse_scaling']) == (12, 3, 2, 1), p
    assert B.num_levels == 4


def _poly_after(B, cb):
    info = B.tail_info()
    assert info['tail_level'] == 0 and info['programs'] == [], info


SGS_W = dict(tc.SGS, cycle_type='W')


def _sgs_tail_check(B):
    assert B.level_format(0)['gs'] and B.effective_params['cycle_type'] == 2


def _sgs_tail_after(B, cb):
    info = B.tail_info()
    print('tail', info)
    assert info['tail_level'] == 1 and not info['refused'] and len(info['programs']) == 2, info


@functools.lru_cache(maxsize=None)
def _grid16():
    return sc.truncated(2, 16, 1e3, 289)            # the whole 2-D n = 16 grid


@functools.lru_cache(maxsize=None)
def _grid16_patches():
    A, nv, idofs = _grid16()
    return mo.setup(A, mo.Params(num_functions=2, coarse_dof=CD, Schwarz_type=PATCHES), idofs=idofs)


def _patches_build():
    A, nv, idofs = _grid16()
    return _mamg().MetricAMG(A, [nv, nv], idofs=idofs, num_functions=2, coarse_dof=CD, setup='gpu',
                             Schwarz_type=PATCHES)


def _patches_check(B):
    assert B.layout == 'bsr2' and B.level_format(0)['patches'], B.level_format(0)


@functools.lru_cache(maxsize=None)
def _emi():
    s = _mamg().problems.emi(3, 8, 1e6)
    A = s.scipy()
    return s, A, mo.setup(A, mo.Params(**tgr.REF_DEFAULT), idofs=s.idofs)


def _rings_build():
    s, A, _ = _emi()
    return _mamg().precond.get_hazmath_metric_precond_mono(A, s.W, interface_dofs=s.idofs, setup='gpu')


def _rings_check(B):
    assert B.layout == 'bsr2' and B.level_format(0)['rings'] and B.level_format(1)['gs']


def _scalar_build():
    return _mamg().MetricAMG(sc.scalar(1025), None, num_functions=1, coarse_dof=CD, setup='gpu')


def _scalar_check(B):
    assert B.layout == 'csr' and B.num_levels == len(sc.HIER_SCALAR[1025])


def _point_check(B):
    assert B.layout == 'csr' and all(B.level_format(l)['gs'] for l in range(B.num_levels - 1))


def _point_after(k):
    def after(B, cb):       # test_point_gs_side_of_the_small_level_boundary's criterion
        assert cb[1] > 0 and (cb[2] > 0) == (k > sc.GS_SMALL_MAX_ROWS), (k, cb[2])
    return after


def _prings_check(B):
    f = B.level_format(0)
    assert B.layout == 'csr' and f['rings'] and f['gs']


def _maxit_check(B):
    assert B.effective_params['maxit'] == 2
    gs.check_mode(B, 'default')


def _f32_build():
    B = _half_build()
    B.set_cycle_storage('f32')
    return B


def _f32_check(B):
    gs.check_mode(B, 'sell')
    assert bits(B, 0) == ALL and bits(B, B.num_levels - 1) == 0, B.level_storage(0)


def _f32_ref(B):
    n = B.num_levels
    return StorageRef(sc.oracle('stencil3d', 257), masks=[bits(B, l) for l in range(n)],
                      kform=[bool(B.level_format(l)['post_fused']) for l in range(n)]).apply


CASES = {
    'half-sell-col16': Case(_half_build, _half_check, lambda B: sc.oracle('stencil3d', 257).apply),
    'lane-group-bsr2': Case(lambda: gs.build('slice', 257, 'default', 'gpu'), _bsr2_check,
                            lambda B: sc.oracle('slice', 257).apply),
    'poly3-w-scaling': Case(_poly_build, _poly_check,
                            lambda B: sc.oracle('slice', 257, 'W', 'POLY', poly_degree=3, coarse_scaling=1).apply,
                            _poly_after),
    'sgs-w-tail': Case(lambda: tgt.build('ua3d12c40', SGS_W), _sgs_tail_check,
                       lambda B: tc.oracle('ua3d12c40', **SGS_W).apply, _sgs_tail_after),
    'patches-2d16': Case(_patches_build, _patches_check, lambda B: _grid16_patches().apply),
    'rings-emi': Case(_rings_build, _rings_check, lambda B: _emi()[2].apply),
    'scalar-jacobi-1025': Case(_scalar_build, _scalar_check, lambda B: sc.oracle_scalar(1025).apply),
    'point-sgs-4096': Case(lambda: gs.pointgs_handle(4096, 'SGS'), _point_check,
                           lambda B: gs.pointgs(4096, 'SGS')[0].apply, _point_after(4096)),
    'point-sgs-4097': Case(lambda: gs.pointgs_handle(4097, 'SGS'), _point_check,
                           lambda B: gs.pointgs(4097, 'SGS')[0].apply, _point_after(4097)),
    'point-rings-3d1d16': Case(lambda: tpr.handle(1), _prings_check, lambda B: tpr.reference(1)[0].apply),
    'maxit2': Case(lambda: gs.build('slice', 257, 'default', 'gpu', maxit=2), _maxit_check,
                   lambda B: sc.oracle('slice', 257, maxit=2).apply),
    'half-sell-f32': Case(_f32_build, _f32_check, _f32_ref),
}


def apply_call(E, label, s, B, T, ref, tol, bufs, tbufs):
    """apply_device on `s` behind a delay of FACTOR x the twin's time for the
    same kind of call; (i) and (ii)."""
    torch = _torch()
    (rb, zb), (tr, tz) = bufs, tbufs
    n = rb.numel()
    tr.copy_(fresh(n)[1])
    call_ms = st.host_ms(lambda: T.apply_device(tr, tz))
    r, src = fresh(n)
    rb.fill_(float('nan'))
    zb.fill_(float('nan'))
    with E.call(label):
        st.behind_delay(label, s, call_ms, lambda: rb.copy_(src), lambda: B.apply_device(rb, zb, s))
        zu = zb.clone()
        zb.fill_(float('nan'))
        B.apply_device(rb, zb)
        torch.cuda.synchronize()
        assert torch.equal(zu, zb), 'differs from the null-stream result of the same handle and buffers'
        e = rel(host(zu), ref(r))
        assert e < tol, 'apply off the reference by %.3e' % e


def pcg_call(E, label, s, B, T, ref, xb, bb, tx, tb):
    """mamg_pcg_device under `with torch.cuda.stream(s)`; b and x0 produced late."""
    torch = _torch()
    M = _mamg()
    A = B._Aop
    n = xb.numel()

    def solver(P):
        return M.ConjGrad(P._Aop, precond=P, tolerance=PCG_TOL, maxiter=PCG_MAXIT, device=True)

    tb.copy_(fresh(n)[1])
    tx.zero_()
    call_ms = st.host_ms(lambda: solver(T).solve_device(tb, tx))
    b, src = fresh(n)
    x0 = torch.zeros_like(src)
    cg = solver(B)

    def run():
        with torch.cuda.stream(s):
            cg.solve_device(bb, xb)

    def fill():
        bb.copy_(src)
        xb.copy_(x0)

    bb.fill_(float('nan'))
    xb.fill_(float('nan'))
    with E.call(label):
        st.behind_delay(label, s, call_ms, fill, run, sync_inside=True)
        xu, resu = xb.clone(), list(cg.residuals)
        xb.copy_(x0)
        cg.solve_device(bb, xb)
        torch.cuda.synchronize()
        assert torch.equal(xu, xb) and resu == list(cg.residuals), \
            'differs from the null-stream solve of the same handle and buffers'
        assert_pcg(resu, host(xu), mo.pcg(A, ref, b, PCG_TOL, PCG_MAXIT))


@pytest.mark.parametrize('name', list(CASES))
def test_one_handle_one_user_stream(user_streams, name):
    """apply_device (first call on a fresh handle, replay on the same buffers,
    a new (r, z) pair), spmv_device, time_apply(mode=1) -- the eager op-by-op
    path -- and mamg_pcg_device (first solve, second solve on the cached
    iteration graph), each on a user stream behind a delay."""
    torch = _torch()
    s1, _ = user_streams
    c = CASES[name]
    B, T = c.build(), c.build()
    E = Errors()
    try:
        c.check(B)
        ref = c.ref(B)
        n = B.shape[0]
        A = B._Aop
        bufs, tbufs = (nan(n), nan(n)), (nan(n), nan(n))
        apply_call(E, 'a %s apply first' % name, s1, B, T, ref, c.tol, bufs, tbufs)
        apply_call(E, 'a %s apply replay' % name, s1, B, T, ref, c.tol, bufs, tbufs)
        apply_call(E, 'a %s apply new pair' % name, s1, B, T, ref, c.tol, (nan(n), nan(n)), (nan(n), nan(n)))

        # y = A_0 x
        (xb, yb), (tx, ty) = bufs, tbufs
        tx.copy_(fresh(n)[1])
        call_ms = st.host_ms(lambda: T.spmv_device(tx, ty))
        x, src = fresh(n)
        xb.fill_(float('nan'))
        yb.fill_(float('nan'))
        with E.call('spmv'):
            st.behind_delay('a %s spmv' % name, s1, call_ms, lambda: xb.copy_(src), lambda: B.spmv_device(xb, yb, s1))
            yu = yb.clone()
            yb.fill_(float('nan'))
            B.spmv_device(xb, yb)
            torch.cuda.synchronize()
            assert torch.equal(yu, yb), 'differs from the null-stream result of the same handle and buffers'
            spmv_bound_ok(A, x, host(yu))

        # the eager op list
        (rb, zb) = bufs
        tx.copy_(fresh(n)[1])
        call_ms = st.host_ms(lambda: T.time_apply(tx, ty, 1, mode=1))
        r, src = fresh(n)
        rb.fill_(float('nan'))
        zb.fill_(float('nan'))
        out = {}
        with E.call('time_apply'):
            st.behind_delay('a %s time_apply' % name, s1, call_ms, lambda: rb.copy_(src),
                            lambda: out.update(t=B.time_apply(rb, zb, 1, mode=1, stream=s1)), sync_inside=True)
            zu = zb.clone()
            zb.fill_(float('nan'))
            B.time_apply(rb, zb, 1, mode=1)
            torch.cuda.synchronize()
            assert out['t'][0] > 0
            assert torch.equal(zu, zb), 'differs from the null-stream result of the same handle and buffers'
            e = rel(host(zu), ref(r))
            assert e < c.tol, 'eager apply off the reference by %.3e' % e
            if c.after:
                c.after(B, out['t'][2])

        xb2, bb2, tx2, tb2 = nan(n), nan(n), nan(n), nan(n)
        pcg_call(E, 'a %s pcg first' % name, s1, B, T, ref, xb2, bb2, tx2, tb2)
        pcg_call(E, 'a %s pcg second' % name, s1, B, T, ref, xb2, bb2, tx2, tb2)
        torch.cuda.synchronize()
    finally:
        torch.cuda.synchronize()
        B.close()
        T.close()
    E.check()


def test_matvec_and_conjgrad_under_stream_context(user_streams):
    """MetricAMG.matvec and ConjGrad(device=True) `*` under
    `with torch.cuda.stream(s)`: the wrappers pass torch's current stream."""
    torch = _torch()
    M = _mamg()
    s1, _ = user_streams
    A = sc.nodal('slice', 257)[0]
    B, T = (gs.build('slice', 257, 'default', 'gpu') for _ in range(2))
    E = Errors()
    try:
        n = B.shape[0]
        ref = sc.oracle('slice', 257).apply
        warm = fresh(n)[1]
        call_ms = st.host_ms(lambda: T.matvec(warm))
        r, src = fresh(n)
        rb = nan(n)
        out = {}

        def mv():
            with torch.cuda.stream(s1):
                out['z'] = B.matvec(rb)

        with E.call('matvec'):
            st.behind_delay('a matvec', s1, call_ms, lambda: rb.copy_(src), mv)
            z0 = B.matvec(rb)
            torch.cuda.synchronize()
            assert torch.equal(out['z'], z0), 'differs from the null-stream matvec of the same handle'
            e = rel(host(out['z']), ref(r))
            assert e < APPLY_TOL, 'matvec off the oracle by %.3e' % e

        tb = fresh(n)[1]
        call_ms = st.host_ms(lambda: M.ConjGrad(A, precond=T, tolerance=PCG_TOL, maxiter=PCG_MAXIT, device=True) * tb)
        b, src = fresh(n)
        bb = nan(n)
        cg = M.ConjGrad(A, precond=B, tolerance=PCG_TOL, maxiter=PCG_MAXIT, device=True)

        def solve():
            with torch.cuda.stream(s1):
                out['x'] = cg * bb

        with E.call('ConjGrad'):
            st.behind_delay('a ConjGrad *', s1, call_ms, lambda: bb.copy_(src), solve, sync_inside=True)
            assert_pcg(cg.residuals, host(out['x']), mo.pcg(A, ref, b, PCG_TOL, PCG_MAXIT))
    finally:
        torch.cuda.synchronize()
        B.close()
        T.close()
    E.check()


# ---------------------------------------------------------------------------
# b. rank handles
# ---------------------------------------------------------------------------
SMOOTHERS = {
    'jacobi': (dict(), dict()),
    'sgs': (dict(smoother=11, Schwarz_type=7), dict(smoother='SGS')),
    'patches': (dict(Schwarz_type=PATCHES), dict(Schwarz_type=PATCHES)),
}
RANK_M = 129


def rank_oracle(smo):
    okw = dict(SMOOTHERS[smo][1])
    return sc.oracle('slice', RANK_M, 'V', okw.pop('smoother', 'JACOBI_RHO'), **okw)


def nodal_ranks(P, smo, comm=False):
    """P rank handles of ('slice', 129), every level above the coarsest
    partitioned (rep_nodes 1), half-symmetric A_loc (the interior-row fork)."""
    M = _mamg()
    set_opt('MAMG_SELL_MIN_ROWS', '1')
    A, nv, idofs = sc.nodal('slice', RANK_M)
    return [M.DistMetricAMG(A, [nv, nv], idofs=idofs, rank=p, nranks=P, rep_nodes=1, num_functions=2, coarse_dof=CD,
                            comm_id=M.DistMetricAMG.unique_id() if comm else None, **SMOOTHERS[smo][0])
            for p in range(P)]


def gather(hs, zs, nv):
    z = np.zeros(hs[0].dofs_per_node * nv)
    for h, zl in zip(hs, zs):
        zl = zl.cpu().numpy()
        if h.dofs_per_node == 1:
            z[h.o0:h.o1] = zl
        else:
            z[h.o0:h.o1] = zl[:h.nloc]
            z[nv + h.o0:nv + h.o1] = zl[h.nloc:]
    return z


def slices(hs, v):
    torch = _torch()
    return [torch.as_tensor(np.ascontiguousarray(h.local_slice(v), dtype=np.float64)).cuda() for h in hs]


def nans(hs):
    return [nan(h.local_size) for h in hs]


def refill(bufs, srcs):
    for b, s_ in zip(bufs, srcs):
        b.copy_(s_)


def poison(*lists):
    for bufs in lists:
        for b in bufs:
            b.fill_(float('nan'))


def equal_lists(a, b):
    torch = _torch()
    return all(torch.equal(x, y) for x, y in zip(a, b))


def rank_call(E, label, s, hs, N, run, check, sync_inside=False):
    """One call on the rank handles hs: timed on the idle null stream with a
    vector of its own (the handles are warm), then on `s` behind the delay with
    a fresh one, then again on the null stream in the same buffers (i);
    check(v, gathered result) is (ii).  run(inb, outb, stream)."""
    torch = _torch()
    nv = hs[0].nv
    inb, outb = nans(hs), nans(hs)
    refill(inb, slices(hs, fresh(N)[0]))
    call_ms = st.host_ms(lambda: run(inb, outb, None))
    v, _ = fresh(N)
    src = slices(hs, v)
    poison(inb, outb)
    with E.call(label):
        st.behind_delay(label, s, call_ms, lambda: refill(inb, src), lambda: run(inb, outb, s), sync_inside=sync_inside)
        user = [o.clone() for o in outb]
        poison(outb)
        run(inb, outb, None)
        torch.cuda.synchronize()
        assert equal_lists(user, outb), 'differs from the null-stream result of the same handles and buffers'
        check(v, gather(hs, user, nv))


def rank_pcg_call(E, label, s, hs, A, ref, **kw):
    """mamg_dist_pcg_device (one handle) / mamg_dist_virtual_pcg (a list)."""
    torch = _torch()
    M = _mamg()
    N = A.shape[0]
    nv = hs[0].nv
    single = kw.pop('single', False)

    def solver(stream):
        return M.DistConjGrad.for_handles(hs[0] if single else hs, stream=stream, device=True, tolerance=PCG_TOL,
                                          maxiter=PCG_MAXIT, **kw)

    bb, xb = nans(hs), nans(hs)
    refill(bb, slices(hs, fresh(N)[0]))
    for x in xb:
        x.zero_()
    call_ms = st.host_ms(lambda: solver(None).solve(bb, xb))
    b, _ = fresh(N)
    src = slices(hs, b)
    zero = [torch.zeros_like(x) for x in xb]
    poison(bb, xb)
    cg, cg0 = solver(s), solver(None)
    with E.call(label):
        st.behind_delay(label, s, call_ms, lambda: (refill(bb, src), refill(xb, zero)), lambda: cg.solve(bb, xb),
                        sync_inside=True)
        user = [x.clone() for x in xb]
        refill(xb, zero)
        cg0.solve(bb, xb)
        torch.cuda.synchronize()
        assert equal_lists(user, xb) and list(cg.residuals) == list(cg0.residuals), \
            'differs from the null-stream solve of the same handles and buffers'
        assert_pcg(cg.residuals, gather(hs, user, nv), mo.pcg(A, ref, b, PCG_TOL, PCG_MAXIT))


def apply_check(ref, tol=APPLY_TOL):
    def check(r, z):
        e = rel(z, ref(r))
        assert e < tol, 'apply off the oracle by %.3e' % e
    return check


def close_all(hs):
    _torch().cuda.synchronize()
    for h in hs:
        h.close()


@pytest.mark.parametrize('smo', list(SMOOTHERS))
@pytest.mark.parametrize('P', [2, 3])
def test_virtual_ranks_on_user_stream(user_streams, P, smo):
    """mamg_dist_virtual_apply, _apply_graph, _spmv and _virtual_pcg (eager
    and one captured lockstep iteration) on P virtual ranks of ('slice', 129),
    rep_nodes 1: nodal Jacobi, SGS (colour halos) and the node patches."""
    M = _mamg()
    s1, _ = user_streams
    A = sc.nodal('slice', RANK_M)[0]
    ref = rank_oracle(smo).apply
    hs = nodal_ranks(P, smo)
    E = Errors()
    try:
        N = A.shape[0]
        assert hs[0].o0 == 0 and hs[-1].o1 == RANK_M and all(h.nloc >= 1 for h in hs)
        forks = [h.apply_launches['stream_forks'] for h in hs]
        print('stream forks per apply', forks)
        if smo == 'jacobi':
            assert all(h.level_format(0)['half'] for h in hs) and all(f > 0 for f in forks), forks
        V = M.DistMetricAMG
        rank_call(E, 'b virtual_apply P%d %s' % (P, smo), s1, hs, N,
                  lambda i, o, s: V.virtual_apply(hs, i, o, s), apply_check(ref))
        rank_call(E, 'b virtual_apply_graph P%d %s' % (P, smo), s1, hs, N,
                  lambda i, o, s: V.virtual_apply(hs, i, o, s, graph=True), apply_check(ref), sync_inside=True)
        rank_call(E, 'b virtual_spmv P%d %s' % (P, smo), s1, hs, N,
                  lambda i, o, s: V.virtual_spmv(hs, i, o, s), lambda x, y: spmv_bound_ok(A, x, y))
        for g in (0, 1):
            rank_pcg_call(E, 'b virtual_pcg graph=%d P%d %s' % (g, P, smo), s1, hs, A, ref, graph=bool(g))
    finally:
        close_all(hs)
    E.check()


def one_rank_calls(E, tag, s, d, A, ref):
    """Every stream-taking call of a communicator handle."""
    hs = [d]
    N = A.shape[0]
    rank_call(E, 'b %s dist_apply_device' % tag, s, hs, N, lambda i, o, q: d.apply_device(i[0], o[0], q),
              apply_check(ref))
    rank_call(E, 'b %s dist_apply_graph' % tag, s, hs, N, lambda i, o, q: d.apply_graph(i[0], o[0], q),
              apply_check(ref))
    rank_call(E, 'b %s dist_spmv_device' % tag, s, hs, N, lambda i, o, q: d.spmv_device(i[0], o[0], q),
              lambda x, y: spmv_bound_ok(A, x, y))
    for mode in (1, 2):
        rank_call(E, 'b %s dist_time_apply mode %d' % (tag, mode), s, hs, N,
                  lambda i, o, q: d.time_apply(i[0], o[0], 1, mode, q), apply_check(ref), sync_inside=True)
    rank_pcg_call(E, 'b %s dist_pcg_device first' % tag, s, hs, A, ref, single=True)
    rank_pcg_call(E, 'b %s dist_pcg_device second' % tag, s, hs, A, ref, single=True)


@pytest.mark.parametrize('smo', ['jacobi', 'sgs'])
def test_one_rank_rccl_on_user_stream(user_streams, smo):
    """The one-rank RCCL handle: empty send / receive groups and all-reduces
    over one rank on the caller's stream, the interior rows of the
    half-symmetric A_loc forked to the handle's side stream and joined back,
    eager, inside the captured apply and inside the captured PCG iteration."""
    s1, _ = user_streams
    A = sc.nodal('slice', RANK_M)[0]
    d = nodal_ranks(1, smo, comm=True)[0]
    E = Errors()
    try:
        assert d.nloc == RANK_M
        if smo == 'jacobi':          # halo_residual splits the half-symmetric A: D_OVERLAP ops, run through h->side
            assert d.level_format(0)['half'], d.level_format(0)
        else:
            assert d.level_format(0)['gs'], d.level_format(0)
        one_rank_calls(E, 'rccl-%s' % smo, s1, d, A, rank_oracle(smo).apply)
    finally:
        close_all([d])
    E.check()


@functools.lru_cache(maxsize=None)
def _csr_oracle():
    key, seeds, (_, okw), _ = dc._case_table()['bidomain2d']
    A, idofs = dc._matrix(key)
    return mo.setup(A, mo.Params(num_functions=1, **okw), idofs=idofs if seeds else None)


def test_scalar_plan_on_user_stream(user_streams):
    """The scalar CSR plan (tests/test_gpu_dist_csr.py's smallest case,
    'bidomain2d'): two virtual ranks and the one-rank RCCL handle."""
    M = _mamg()
    s1, _ = user_streams
    A, idofs, kw, _ = dc.case('bidomain2d')
    ref = _csr_oracle().apply
    N = A.shape[0]
    hs = [M.DistMetricAMG(A, None, idofs=idofs, rank=p, nranks=2, comm_id=None, rep_nodes=100, **kw) for p in range(2)]
    d = M.DistMetricAMG(A, None, idofs=idofs, rank=0, nranks=1, comm_id=M.DistMetricAMG.unique_id(), rep_nodes=1, **kw)
    E = Errors()
    try:
        assert all(h.dofs_per_node == 1 for h in hs + [d])
        V = M.DistMetricAMG
        rank_call(E, 'b csr virtual_apply', s1, hs, N, lambda i, o, s: V.virtual_apply(hs, i, o, s), apply_check(ref))
        rank_call(E, 'b csr virtual_apply_graph', s1, hs, N, lambda i, o, s: V.virtual_apply(hs, i, o, s, graph=True),
                  apply_check(ref), sync_inside=True)
        rank_call(E, 'b csr virtual_spmv', s1, hs, N, lambda i, o, s: V.virtual_spmv(hs, i, o, s),
                  lambda x, y: spmv_bound_ok(A, x, y))
        rank_pcg_call(E, 'b csr virtual_pcg graph=1', s1, hs, A, ref, graph=True)
        one_rank_calls(E, 'csr-rccl', s1, d, A, ref)
    finally:
        close_all(hs + [d])
    E.check()


# ---------------------------------------------------------------------------
# c. one handle on two streams in turn: the handle orders the calls
# ---------------------------------------------------------------------------
def ordered_pair(E, label, streams_, call_ms, first, second, second_syncs, results):
    """first(s1) behind a delay, an event e1 recorded on s1 behind it; then
    second(s2) at once, on buffers of its own that are already filled.  After
    s2.synchronize() e1 must have completed: the handle put call 2 behind
    call 1, whose work vectors it shares.  The delay must still be pending
    when call 2 is issued (second_syncs) or has returned, or the order would
    hold by itself.  results(): both results right."""
    torch = _torch()
    s1, s2 = streams_
    with E.call(label):
        fill, call = first
        e1 = torch.cuda.Event()

        def call1():
            call(s1)
            e1.record(s1)

        ev = st.behind_delay(label + ' (call 1)', s1, call_ms, fill, call1, wait=False)
        if second_syncs:
            pending = not ev.query()
            second(s2)
        else:
            second(s2)
            pending = not ev.query()
        s2.synchronize()
        done = e1.query()
        torch.cuda.synchronize()
        if not pending:
            raise st.Inconclusive(label + ': the delay on s1 was over before call 2 was under way')
        assert done, 'call 2 on s2 finished while call 1 on s1 was still pending: the handle did not order them'
        results()


def test_one_handle_two_streams(user_streams):
    """apply / apply, spmv / apply, apply / pcg on a single-GPU handle, and a
    host-pointer mamg_apply right after a delayed device apply."""
    torch = _torch()
    M = _mamg()
    A = sc.nodal('slice', 257)[0]
    ref = sc.oracle('slice', 257).apply
    B = gs.build('slice', 257, 'default', 'gpu')
    E = Errors()
    try:
        n = B.shape[0]
        r1b, z1b, r2, z2 = nan(n), nan(n), nan(n), nan(n)
        r1b.copy_(fresh(n)[1])
        r2.copy_(fresh(n)[1])
        B.spmv_device(r1b, z1b)                              # warm: both graphs captured, PCG vectors allocated
        B.apply_device(r1b, z1b)
        B.apply_device(r2, z2)
        cg = M.ConjGrad(A, precond=B, tolerance=PCG_TOL, maxiter=PCG_MAXIT, device=True)
        xb = torch.zeros(n, dtype=torch.float64, device='cuda')
        cg.solve_device(fresh(n)[1], xb)
        t_apply = st.host_ms(lambda: B.apply_device(r2, z2))
        t_pcg = st.host_ms(lambda: (xb.zero_(), cg.solve_device(r2, xb)))

        def first_apply(v1):
            return (lambda: r1b.copy_(v1[1])), (lambda s: B.apply_device(r1b, z1b, s))

        def both_right(v1, v2, out2=None):
            def results():
                e1 = rel(host(z1b), ref(v1[0]))
                assert e1 < APPLY_TOL, 'call 1 off the oracle by %.3e' % e1
                if out2 is None:
                    e2 = rel(host(z2), ref(v2[0]))
                    assert e2 < APPLY_TOL, 'call 2 off the oracle by %.3e' % e2
                else:
                    out2()
            return results

        # apply / apply
        v1, v2 = fresh(n), fresh(n)
        poison([r1b, z1b, z2])
        r2.copy_(v2[1])
        ordered_pair(E, 'c apply/apply', user_streams, t_apply, first_apply(v1),
                     lambda s: B.apply_device(r2, z2, s), False, both_right(v1, v2))

        # spmv / apply
        v1, v2 = fresh(n), fresh(n)
        poison([r1b, z1b, z2])
        r2.copy_(v2[1])

        def spmv_right():
            spmv_bound_ok(A, v1[0], host(z1b))
            e2 = rel(host(z2), ref(v2[0]))
            assert e2 < APPLY_TOL, 'call 2 off the oracle by %.3e' % e2

        ordered_pair(E, 'c spmv/apply', user_streams, t_apply,
                     ((lambda: r1b.copy_(v1[1])), (lambda s: B.spmv_device(r1b, z1b, s))),
                     lambda s: B.apply_device(r2, z2, s), False, spmv_right)

        # apply / pcg
        v1, v2 = fresh(n), fresh(n)
        poison([r1b, z1b])
        r2.copy_(v2[1])
        xb.zero_()

        def solve(s):
            with torch.cuda.stream(s):
                cg.solve_device(r2, xb)

        ordered_pair(E, 'c apply/pcg', user_streams, t_pcg, first_apply(v1), solve, True,
                     both_right(v1, v2, lambda: assert_pcg(cg.residuals, host(xb),
                                                           mo.pcg(A, ref, v2[0], PCG_TOL, PCG_MAXIT))))

        # device apply / host-pointer apply
        v1, v2 = fresh(n), fresh(n)
        poison([r1b, z1b])
        out = {}
        t_host = st.host_ms(lambda: B * v2[0])

        def host_right():
            e2 = rel(out['z'], ref(v2[0]))
            assert e2 < APPLY_TOL, 'host-pointer apply off the oracle by %.3e' % e2

        ordered_pair(E, 'c apply/host apply', user_streams, t_host, first_apply(v1),
                     lambda s: out.update(z=B * v2[0]), True, both_right(v1, v2, host_right))
    finally:
        torch.cuda.synchronize()
        B.close()
    E.check()


@pytest.mark.parametrize('comm', [True, False], ids=['rccl', 'no-comm'])
def test_one_rank_handle_two_streams(user_streams, comm):
    """spmv / apply, apply / apply, apply / apply_graph and apply / pcg on a
    rank handle: its ghost, send and level work buffers are shared by all of
    its calls, so it orders them across streams as a single-GPU handle does.
    On the handle without a communicator nothing but the handle's own event
    can order the two calls; on the RCCL handle the communicator serialises
    its own operations across streams, which covers everything behind call
    2's first exchange even without the handle's wait."""
    torch = _torch()
    M = _mamg()
    A = sc.nodal('slice', RANK_M)[0]
    ref = rank_oracle('jacobi').apply
    d = nodal_ranks(1, 'jacobi', comm=comm)[0]
    E = Errors()
    try:
        n = d.local_size
        r1b, z1b, r2, z2 = nan(n), nan(n), nan(n), nan(n)
        r2.copy_(fresh(n)[1])
        d.apply_device(r2, z2)                               # warm: graph of (r2, z2), PCG plan
        d.apply_graph(r2, z2)
        d.spmv_device(r2, z1b)
        cg = M.DistConjGrad.for_handles(d, stream=None, device=True, tolerance=PCG_TOL, maxiter=PCG_MAXIT)
        xb = torch.zeros(n, dtype=torch.float64, device='cuda')
        cg.solve([r2], [xb])
        t_apply = st.host_ms(lambda: d.apply_device(r2, z2))
        t_pcg = st.host_ms(lambda: (xb.zero_(), cg.solve([r2], [xb])))

        def full(t):
            return gather([d], [t], d.nv)

        def first(v1, spmv=False):
            f = d.spmv_device if spmv else d.apply_device
            src = slices([d], v1)[0]
            return (lambda: r1b.copy_(src)), (lambda s: f(r1b, z1b, s))

        def right(v1, v2, spmv=False, out2=None):
            def results():
                if spmv:
                    spmv_bound_ok(A, v1, full(z1b))
                else:
                    e1 = rel(full(z1b), ref(v1))
                    assert e1 < APPLY_TOL, 'call 1 off the oracle by %.3e' % e1
                if out2 is None:
                    e2 = rel(full(z2), ref(v2))
                    assert e2 < APPLY_TOL, 'call 2 off the oracle by %.3e' % e2
                else:
                    out2()
            return results

        N = A.shape[0]
        for label, spmv, second in (('c rank spmv/apply', True, lambda s: d.apply_device(r2, z2, s)),
                                    ('c rank apply/apply', False, lambda s: d.apply_device(r2, z2, s)),
                                    ('c rank apply/apply_graph', False, lambda s: d.apply_graph(r2, z2, s))):
            v1, v2 = fresh(N)[0], fresh(N)[0]
            poison([r1b, z1b, z2])
            r2.copy_(slices([d], v2)[0])
            ordered_pair(E, label, user_streams, t_apply, first(v1, spmv), second, False, right(v1, v2, spmv))

        v1, v2 = fresh(N)[0], fresh(N)[0]
        poison([r1b, z1b])
        r2.copy_(slices([d], v2)[0])
        xb.zero_()
        cg2 = M.DistConjGrad.for_handles(d, stream=user_streams[1], device=True, tolerance=PCG_TOL, maxiter=PCG_MAXIT)
        ordered_pair(E, 'c rank apply/pcg', user_streams, t_pcg, first(v1), lambda s: cg2.solve([r2], [xb]), True,
                     right(v1, v2, out2=lambda: assert_pcg(cg2.residuals, full(xb),
                                                           mo.pcg(A, ref, v2, PCG_TOL, PCG_MAXIT))))
    finally:
        close_all([d])
    E.check()


def test_virtual_ranks_two_streams(user_streams):
    """virtual_spmv / virtual_apply and virtual_apply / virtual_apply on two
    virtual ranks: the lockstep calls order against every handle of the list."""
    M = _mamg()
    V = M.DistMetricAMG
    A = sc.nodal('slice', RANK_M)[0]
    ref = rank_oracle('jacobi').apply
    hs = nodal_ranks(2, 'jacobi')
    E = Errors()
    try:
        N, nv = A.shape[0], hs[0].nv
        in1, out1, in2, out2 = nans(hs), nans(hs), nans(hs), nans(hs)
        refill(in2, slices(hs, fresh(N)[0]))
        V.virtual_spmv(hs, in2, out2)                      # warm
        V.virtual_apply(hs, in2, out2)
        t_apply = st.host_ms(lambda: V.virtual_apply(hs, in2, out2))
        for label, spmv in (('c virtual spmv/apply', True), ('c virtual apply/apply', False)):
            v1, v2 = fresh(N)[0], fresh(N)[0]
            src1 = slices(hs, v1)
            poison(in1, out1, out2)
            refill(in2, slices(hs, v2))
            f = V.virtual_spmv if spmv else V.virtual_apply

            def results(v1=v1, v2=v2, spmv=spmv):
                z1, z2 = gather(hs, out1, nv), gather(hs, out2, nv)
                if spmv:
                    spmv_bound_ok(A, v1, z1)
                else:
                    e1 = rel(z1, ref(v1))
                    assert e1 < APPLY_TOL, 'call 1 off the oracle by %.3e' % e1
                e2 = rel(z2, ref(v2))
                assert e2 < APPLY_TOL, 'call 2 off the oracle by %.3e' % e2

            ordered_pair(E, label, user_streams, t_apply,
                         ((lambda src1=src1: refill(in1, src1)), (lambda s, f=f: f(hs, in1, out1, s))),
                         lambda s: V.virtual_apply(hs, in2, out2, s), False, results)
    finally:
        close_all(hs)
    E.check()


# ---------------------------------------------------------------------------
# d. two handles on two user streams, enqueued alternately
# ---------------------------------------------------------------------------
def test_two_handles_two_streams_alternating(user_streams):
    """Five rounds of apply_device on two handles, each on its own stream,
    enqueued alternately behind a delay on both streams: every result is
    bitwise the serial one on the null stream (and the oracle's to APPLY_TOL)."""
    torch = _torch()
    s1, s2 = user_streams
    B1 = gs.build('slice', 257, 'default', 'gpu')
    B2 = gs.build('stencil3d', 257, 'sell', 'gpu')
    refs = (sc.oracle('slice', 257).apply, sc.oracle('stencil3d', 257).apply)
    rounds = 5
    try:
        n1, n2 = B1.shape[0], B2.shape[0]
        vs = [(fresh(n1), fresh(n2)) for _ in range(rounds)]
        rb = [(nan(n1), nan(n2)) for _ in range(rounds)]
        zb = [(nan(n1), nan(n2)) for _ in range(rounds)]
        for k in range(rounds):                                   # warm: every graph captured
            B1.apply_device(rb[k][0], zb[k][0])
            B2.apply_device(rb[k][1], zb[k][1])

        def enqueue(q1, q2):
            for k in range(rounds):
                B1.apply_device(rb[k][0], zb[k][0], q1)
                B2.apply_device(rb[k][1], zb[k][1], q2)

        for k in range(rounds):
            rb[k][0].copy_(fresh(n1)[1])
            rb[k][1].copy_(fresh(n2)[1])
        call_ms = st.host_ms(lambda: enqueue(None, None))
        poison([t for p in rb + zb for t in p])

        def fill2():
            for k in range(rounds):
                rb[k][1].copy_(vs[k][1][1])

        other = {}

        def fill():                     # s2 gets a delay and late inputs of its own, then s1's inputs
            other['ev'] = st.delayed(s2, st.delay_for(call_ms))
            with torch.cuda.stream(s2):
                fill2()
            for k in range(rounds):
                rb[k][0].copy_(vs[k][0][1])

        ev1 = st.behind_delay('d alternating x5', s1, call_ms, fill, lambda: enqueue(s1, s2), wait=False)
        pending2 = not other['ev'].query()
        torch.cuda.synchronize()
        assert ev1.query()
        if not pending2:
            raise st.Inconclusive('d: the delay on s2 was over when the calls returned')
        user = [(a.clone(), b.clone()) for a, b in zb]
        poison([t for p in zb for t in p])
        enqueue(None, None)
        torch.cuda.synchronize()
        for k in range(rounds):
            for j in range(2):
                assert torch.equal(user[k][j], zb[k][j]), 'round %d handle %d differs from the serial run' % (k, j + 1)
                e = rel(host(user[k][j]), refs[j](vs[k][j][0]))
                assert e < APPLY_TOL, (k, j, e)
    finally:
        torch.cuda.synchronize()
        B1.close()
        B2.close()
