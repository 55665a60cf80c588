"""The device PCG loops off the healthy x0 = 0 path: nonzero x0, relative
tolerance, maxiter 0, b = 0, <r,Br> < 0 inside the loop (x restored) and at
the start ("Matrix is not positive") -- mamg_pcg_device on one GPU,
mamg_dist_virtual_pcg on virtual ranks (eager and as a captured lockstep
iteration), mamg_dist_pcg_device over a one-rank RCCL communicator (cached
graph) and in two processes through the host-staged gloo exchange.

Inputs and references: tests/pcg_edges_ref.py (mamg_oracle.pcg, and the host
loop around the oracle's apply for stop type 1; never the code under test);
tests/test_pcg_edges_ref.py pins on the CPU that each input breaks where
stated, by margins that make the checks here decisive.  The project's PCG
contract: as many residuals as the reference, every residual
(and alpha, beta) within 1e-6 relative, the solution within 1e-6; "bitwise"
is np.array_equal.  Measured deviations: DESIGN 6.6 "Tests"."""
import ctypes as C
import warnings

import numpy as np
import pytest

import mamg_oracle as mo
import pcg_edges_ref as pe
from conftest import set_opt

pytestmark = pytest.mark.gpu

BREAKS = ['neg2', 'neg1x', 'neg0', 'neg0_x7', 'neg1', 'neg1_x7']
# the partitions of tests/test_gpu_dist_pcg.py: system -> (P, rep_nodes)
PART = {'b3': (3, 100), 'b2': (8, 10 ** 6)}


def _M():
    import metric_amg_examples_amd as M
    return M


def _cuda(v):
    import torch
    return torch.as_tensor(np.array(v, dtype=np.float64)).cuda()


def _rel(a, b):
    return float(np.max(np.abs(np.asarray(a) / np.asarray(b) - 1.0))) if len(b) else 0.0


def _contract(case, res, al, be, x, norms=None, what=''):
    """histories and solution against the reference of `case`"""
    outcome, k, xr, rres, ral, rbe = pe.reference(case)
    x0 = pe.vectors(case)[1]
    assert len(res) == len(rres) == k + 1, (len(res), len(rres))
    assert len(al) == len(be) == k
    step = pe.margins(case)[2] if outcome == 'rz_neg' else 0.0
    dx = np.linalg.norm(x - xr)
    print('%s %s: %d iterations; residuals %.2e alphas %.2e betas %.2e; ||x - x_ref|| / ||x_ref|| %.2e%s'
          % (case, what, k, _rel(res, rres), _rel(al, ral), _rel(be, rbe),
             dx / max(np.linalg.norm(xr), 1e-300), '; / ||alpha d|| %.2e' % (dx / step) if step else ''))
    assert np.allclose(res, rres, rtol=1e-6, atol=0)
    assert np.allclose(al, ral, rtol=1e-6, atol=0) and np.allclose(be, rbe, rtol=1e-6, atol=0)
    if norms is not None:
        rn = pe.reference_norms(case)
        assert len(norms) == len(rn) and np.allclose(norms, rn, rtol=1e-6, atol=0)
    if pe.CASES[case]['b'] == 'zero':         # the solution is 0: measured against where the solve started
        assert dx <= 1e-6 * np.linalg.norm(x0)
    elif outcome == 'rz_neg' and k == 0:      # restored to x0, to round-off of the step that was undone
        assert np.linalg.norm(x - x0) <= 1e-6 * step
        assert dx <= 1e-6 * max(np.linalg.norm(xr), step)
    else:
        assert dx <= 1e-6 * np.linalg.norm(xr)


# ---------------------------------------------------------------------------
# one GPU: ConjGrad -> mamg_pcg_device
# ---------------------------------------------------------------------------
def _precond(case):
    A, s = pe.system(pe.CASES[case]['system'])
    return A, _M().MetricAMG(A, s.W, idofs=s.idofs, **pe.param_kw(case))


def _solver(case, A, B, **kw):
    c = pe.CASES[case]
    kw.setdefault('maxiter', pe.MAXITER)
    return _M().ConjGrad(A, precond=B, tolerance=c['tol'], relativeconv=c['relativeconv'], **kw)


def _both_entries(case, A, B, warns=False):
    """the case through `initial_guess=` with solver * b and through
    solve_device(b, xt): [(solver, x)] of the two"""
    import torch
    b, x0 = pe.vectors(case)
    guess = np.array(x0)
    out = []
    for entry in ('initial_guess', 'solve_device'):
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter('always')
            if entry == 'initial_guess':
                cg = _solver(case, A, B, initial_guess=guess)
                assert cg._device_ok()
                x = cg * np.array(b)
                assert np.array_equal(guess, x0)          # initial_guess is left unmodified
            else:
                cg = _solver(case, A, B)
                assert cg._device_ok()
                xt = _cuda(x0)
                assert cg.solve_device(_cuda(b), xt) is xt
                torch.cuda.synchronize()
                x = xt.cpu().numpy()
        assert bool([v for v in w if 'breakdown' in str(v.message)]) == warns
        out.append((cg, x))
    return out


@pytest.mark.parametrize('case', ['h3_x7', 'h2_x7', 'c3_x7', 'h3_rel', 'h2_rel', 'h3_b0', 'h2_b0'])
def test_one_gpu_x0(lib_built, case):
    """x0 = x7 through both entries: the start-up r = b - A x0 on caller-layout
    vectors (BSR2 and CSR layouts), the relative tolerance without a callback
    (so the device loop runs) and b = 0, against the reference from the same x0"""
    A, B = _precond(case)
    assert B.layout == ('csr' if case == 'c3_x7' else 'bsr2')
    runs = _both_entries(case, A, B)
    B.close()
    for cg, x in runs:
        assert not cg.breakdown
        _contract(case, cg.residuals, cg.alphas, cg.betas, x)
        if pe.CASES[case]['relativeconv']:
            assert cg.residuals[-1] <= 1e-6 * cg.residuals[0]


def test_one_gpu_x0_level0_storages(lib_built):
    """the same x0 = x7 solve under each level-0 storage the switches give at
    3-D n=16: CSR-style rows (default), half-symmetric ELL-64 and full SELL-64;
    the last two bitwise each other, all three within contract"""
    M = _M()
    A, s = pe.system('b3')
    b, x0 = pe.vectors('h3_x7')
    runs = []
    for sell_min, half in ((None, None), ('1', '1'), ('1', '0')):
        if sell_min:
            set_opt('MAMG_SELL_MIN_ROWS', sell_min)
            set_opt('MAMG_HALF', half)
        B = M.MetricAMG(A, s.W, idofs=s.idofs, **pe.param_kw('h3_x7'))
        f = B.level_format(0)
        if sell_min:
            assert f['sell'] != (half == '1') and f['half'] == (half == '1') and f['sym']
        else:
            assert not f['sell'] and not f['half']
        cg = M.ConjGrad(A, precond=B, tolerance=1e-8, maxiter=pe.MAXITER, initial_guess=np.array(x0))
        x = cg * np.array(b)
        B.close()
        _contract('h3_x7', cg.residuals, cg.alphas, cg.betas, x, what=str((sell_min, half)))
        runs.append((x, cg.residuals, cg.alphas, cg.betas))
    for u, v in zip(runs[1], runs[2]):
        assert np.array_equal(u, v)


@pytest.mark.parametrize('case', ['h3_x7', 'h2_x7'])
def test_one_gpu_maxiter_0(lib_built, case):
    """maxiter = 0 from x0 = x7: one residual, <r0,Br0>^1/2 of the reference, x bitwise x0"""
    A, B = _precond(case)
    b, x0 = pe.vectors(case)
    cg = _solver(case, A, B, maxiter=0, initial_guess=np.array(x0))
    x = cg * np.array(b)
    B.close()
    r0 = pe.reference(case)[3][0]
    assert len(cg.residuals) == 1 and cg.alphas == [] and cg.betas == [] and not cg.breakdown
    assert abs(cg.residuals[0] / r0 - 1.0) <= 1e-6
    assert np.array_equal(x, x0)


@pytest.mark.parametrize('case', BREAKS + ['csr0'])
def test_one_gpu_breakdown(lib_built, case):
    """<r,Br> < 0 in iteration k: the warning, the flag, k + 1 residuals, k
    alphas / betas, x restored to the reference's x_k (the un-restored iterate
    is >= 1e-2 away, test_pcg_edges_ref) -- so the iteration queued after the
    breaking one restored nothing a second time"""
    A, B = _precond(case)
    assert B.layout == ('csr' if case == 'csr0' else 'bsr2')
    runs = _both_entries(case, A, B, warns=True)
    B.close()
    k = pe.CASES[case]['k']
    for cg, x in runs:
        assert cg.breakdown is True
        assert len(cg.residuals) == k + 1 and len(cg.alphas) == len(cg.betas) == k
        _contract(case, cg.residuals, cg.alphas, cg.betas, x)


@pytest.mark.parametrize('case', ['notpos', 'notpos_x7'])
def test_one_gpu_not_positive(lib_built, case):
    """<r0,Br0> < 0: ValueError('Matrix is not positive'), x left as x0.  Through
    the C entry with NaN-filled histories: MAMG_ERR_BREAKDOWN, the message,
    *niters = 0, residuals[0] = 0.0 and nothing else written (include/mamg.h)"""
    import torch
    M = _M()
    A, B = _precond(case)
    b, x0 = pe.vectors(case)
    cg = _solver(case, A, B, initial_guess=np.array(x0))
    with pytest.raises(ValueError, match='Matrix is not positive'):
        cg * np.array(b)
    assert cg.breakdown
    xt = _cuda(x0)
    with pytest.raises(ValueError, match='Matrix is not positive'):
        _solver(case, A, B).solve_device(_cuda(b), xt)
    assert np.array_equal(xt.cpu().numpy(), x0)
    res, al, be = (np.full(n, np.nan) for n in (6, 5, 5))
    it = C.c_int(-1)
    bt = _cuda(b)
    rc = B._L.mamg_pcg_device(B.handle, C.c_void_p(bt.data_ptr()), C.c_void_p(xt.data_ptr()), 1e-8, 5, 0,
                              M._lib.ptr(res, C.c_double), M._lib.ptr(al, C.c_double), M._lib.ptr(be, C.c_double),
                              C.byref(it), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    msg = B._L.mamg_last_error().decode()
    torch.cuda.synchronize()
    x = xt.cpu().numpy()
    B.close()
    assert rc == M._lib.ERR_BREAKDOWN and 'not positive' in msg and it.value == 0
    assert res[0] == 0.0 and np.isnan(res[1:]).all() and np.isnan(al).all() and np.isnan(be).all()
    assert np.array_equal(x, x0)


def test_one_gpu_state_reset(lib_built):
    """One indefinite handle (3-D n=16, relaxation 3.0), one x tensor: neg2,
    then the healthy ok3, then neg2 again.  The state in HBM and the cached
    (x, maxiter) iteration graph -- the third solve passes the first's x
    pointer and maxiter, so it replays that graph -- carry nothing over: the
    first and third are bitwise equal, ok3 converges with the reference's count"""
    import torch
    A, B = _precond('neg2')
    assert pe.param_kw('ok3') == pe.param_kw('neg2')
    cg = _solver('neg2', A, B)
    xt = _cuda(pe.vectors('neg2')[1])
    ptr = xt.data_ptr()
    runs = []
    for case in ('neg2', 'ok3', 'neg2'):
        b, x0 = pe.vectors(case)
        xt.copy_(_cuda(x0))
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter('always')
            assert cg.solve_device(_cuda(b), xt) is xt and xt.data_ptr() == ptr
        torch.cuda.synchronize()
        assert bool(w) == (case == 'neg2')
        runs.append((xt.cpu().numpy().copy(), list(cg.residuals), list(cg.alphas), list(cg.betas), cg.breakdown))
    B.close()
    for case, (x, res, al, be, broke) in zip(('neg2', 'ok3', 'neg2'), runs):
        assert broke == (case == 'neg2')
        _contract(case, res, al, be, x)
    assert len(runs[1][1]) - 1 == 11
    for u, v in zip(runs[0], runs[2]):
        assert np.array_equal(u, v)


# ---------------------------------------------------------------------------
# virtual ranks: DistConjGrad.for_handles(list, device=True) -> mamg_dist_virtual_pcg
# ---------------------------------------------------------------------------
def _ranks(case, P=None, comm_id=None):
    M = _M()
    name = pe.CASES[case]['system']
    s = pe.system(name)[1]
    Pd, rep = PART[name]
    P = P or Pd
    return [M.DistMetricAMG(s, s.W, idofs=s.idofs, rank=p, nranks=P, comm_id=comm_id, rep_nodes=rep,
                            **pe.param_kw(case)) for p in range(P)]


def _slices(hs, v):
    return [_cuda(h.local_slice(v)) for h in hs]


def _gather(case, hs, xs):
    s = pe.system(pe.CASES[case]['system'])[1]
    out = np.zeros(s.N)
    for h, xl in zip(hs, xs):
        xl = xl.cpu().numpy()
        out[h.o0:h.o1] = xl[:h.nloc]
        out[s.nv + h.o0:s.nv + h.o1] = xl[h.nloc:]
    return out


def _close(hs):
    for h in hs:
        h.close()


def _dsolve(case, hs, graph=False, maxiter=pe.MAXITER, relativeconv=None, virtual=True, stream=None, xs=None):
    """(solver, x slices, ValueError or None) of the device-resident solve of the case from its x0"""
    import torch
    c = pe.CASES[case]
    b, x0 = pe.vectors(case)
    cg = _M().DistConjGrad.for_handles(list(hs) if virtual else hs[0], device=True, graph=graph, stream=stream,
                                       tolerance=c['tol'], maxiter=maxiter, stop_type=1 if c['stop'] else None,
                                       relativeconv=c['relativeconv'] if relativeconv is None else relativeconv)
    if xs is None:
        xs = _slices(hs, x0)
    err = None
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter('always')
        try:
            assert all(u is v for u, v in zip(cg.solve(_slices(hs, b), xs), xs))
        except ValueError as e:       # a state that differs between ranks is a RuntimeError: not caught
            err = e
    torch.cuda.synchronize()
    cg.warned = bool([v for v in w if 'breakdown' in str(v.message)])
    return cg, xs, err


def _history(cg):
    return [np.array(cg.residuals), np.array(cg.alphas), np.array(cg.betas), np.array(cg.residual_norms)]


def _dcontract(case, hs, cg, xs):
    _contract(case, cg.residuals, cg.alphas, cg.betas, _gather(case, hs, xs),
              norms=cg.residual_norms if pe.CASES[case]['stop'] else None, what='P=%d' % len(hs))
    if not pe.CASES[case]['stop']:
        assert cg.residual_norms == []


def _same(a, b):
    (ca, xa), (cb, xb) = a, b
    assert ca.breakdown == cb.breakdown
    for u, v in zip(_history(ca), _history(cb)):
        assert np.array_equal(u, v)
    for u, v in zip(xa, xb):
        assert np.array_equal(u.cpu().numpy(), v.cpu().numpy())


@pytest.mark.parametrize('case', ['h3_x7', 'h2_x7', 'h3_x7_s1', 'h2_x7_s1', 'h3_rel', 'h2_rel', 'h3_b0_s1',
                                  'h2_b0_s1'])
def test_virtual_x0(lib_built, case):
    """x0 = x7 sliced into xs: dspmv_ops(x -> q) with the halo of x and
    dpcg_r0_kernel, under both stopping rules; the relative tolerance; stop
    type 1 with b = 0 (threshold tol * 1, ||r0|| from dpcg_r0_kernel)"""
    hs = _ranks(case)
    cg, xs, err = _dsolve(case, hs)
    assert err is None and not cg.breakdown and not cg.warned
    _dcontract(case, hs, cg, xs)
    if pe.CASES[case]['stop']:        # the rule ignores relativeconv
        _same((cg, xs), _dsolve(case, hs, relativeconv=True)[:2])
    _close(hs)


@pytest.mark.parametrize('case', BREAKS + ['neg2_s1'])
def test_virtual_breakdown(lib_built, case):
    """<r,Br> < 0 in iteration k on P ranks, eager and as the captured
    lockstep iteration: the graph run bitwise the eager one, x restored to
    the reference's x_k on every rank, the ranks' states equal whenever read
    (the library's memcmp raises otherwise)"""
    hs = _ranks(case)
    eager = _dsolve(case, hs)
    graph = _dsolve(case, hs, graph=True)
    again = _dsolve(case, hs, graph=True)
    _close(hs)
    k = pe.CASES[case]['k']
    for cg, xs, err in (eager, graph, again):
        assert err is None and cg.breakdown is True and cg.warned
        assert len(cg.residuals) == k + 1 and len(cg.alphas) == len(cg.betas) == k
        if pe.CASES[case]['stop']:
            assert len(cg.residual_norms) == k + 1
    _dcontract(case, hs, eager[0], eager[1])
    _same(eager[:2], graph[:2])
    _same(eager[:2], again[:2])


@pytest.mark.parametrize('case', ['notpos', 'notpos_x7'])
def test_virtual_not_positive(lib_built, case):
    """ValueError, eager and captured, and every x slice bitwise untouched"""
    hs = _ranks(case)
    x0s = [x.cpu().numpy() for x in _slices(hs, pe.vectors(case)[1])]
    for graph in (False, True):
        cg, xs, err = _dsolve(case, hs, graph=graph)
        assert err is not None and 'Matrix is not positive' in str(err) and cg.breakdown
        for x, x0 in zip(xs, x0s):
            assert np.array_equal(x.cpu().numpy(), x0)
    _close(hs)


@pytest.mark.parametrize('case', ['h3_x7', 'h2_x7_s1'])
def test_virtual_maxiter_0(lib_built, case):
    """maxiter = 0 from x0 = x7: x slices bitwise untouched, one residual"""
    hs = _ranks(case)
    x0s = [x.cpu().numpy() for x in _slices(hs, pe.vectors(case)[1])]
    cg, xs, err = _dsolve(case, hs, maxiter=0)
    _close(hs)
    assert err is None and not cg.breakdown
    assert len(cg.residuals) == 1 and cg.alphas == [] and cg.betas == []
    assert abs(cg.residuals[0] / pe.reference(case)[3][0] - 1.0) <= 1e-6
    if pe.CASES[case]['stop']:
        assert len(cg.residual_norms) == 1
        assert abs(cg.residual_norms[0] / pe.reference_norms(case)[0] - 1.0) <= 1e-6
    for x, x0 in zip(xs, x0s):
        assert np.array_equal(x.cpu().numpy(), x0)


# ---------------------------------------------------------------------------
# one rank over a real RCCL communicator: mamg_dist_pcg_device, cached graph
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('case', ['neg2', 'h3_x7'])
def test_single_rank_rccl(lib_built, case):
    """called twice into the same x (reset to x0 in between), so the second
    solve replays the cached graph: both bitwise the P = 1 virtual run"""
    import torch
    M = _M()
    hv = _ranks(case, P=1)
    virt = _dsolve(case, hv)
    _close(hv)
    d = _ranks(case, P=1, comm_id=M.DistMetricAMG.unique_id())
    x0 = _slices(d, pe.vectors(case)[1])[0]
    xt = [x0.clone()]
    runs = []
    for _ in range(2):
        xt[0].copy_(x0)
        cg, xs, err = _dsolve(case, d, virtual=False, stream=torch.cuda.current_stream(), xs=xt)
        assert err is None and xs[0] is xt[0]
        runs.append((cg, [xt[0].clone()]))
    _close(d)
    broke = pe.CASES[case]['outcome'] == 'rz_neg'
    assert virt[2] is None and virt[0].breakdown == broke and virt[0].warned == broke
    _dcontract(case, hv, virt[0], virt[1])
    for run in runs:
        assert run[0].warned == broke
        _same(virt[:2], run)


# ---------------------------------------------------------------------------
# two processes through gloo: the loop that reads the state after every iteration
# ---------------------------------------------------------------------------
GLOO_CASES = ('h3_x7', 'neg2')


def _free_port():
    import socket
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _gloo_worker(rank, world, port, q):
    """one rank process: both cases on one rank-local handle per relaxation"""
    import os
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for p in (root, os.path.join(root, 'oracle'), os.path.join(root, 'tests')):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    import torch
    import torch.distributed as dist
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        import metric_amg_examples_amd as M
        import pcg_edges_ref as ref
        out = []
        for case in GLOO_CASES:
            c = ref.CASES[case]
            s = ref.system(c['system'])[1]
            h = M.DistMetricAMG(s, s.W, idofs=s.idofs, rank=rank, nranks=world, comm_id=None, rep_nodes=100,
                                exchange='gloo', **ref.param_kw(case))
            b, x0 = ref.vectors(case)
            bt = torch.as_tensor(h.local_slice(np.array(b))).cuda()
            xt = torch.as_tensor(h.local_slice(np.array(x0))).cuda()
            cg = M.DistConjGrad.for_handles(h, device=True, tolerance=c['tol'], maxiter=ref.MAXITER)
            with warnings.catch_warnings():
                warnings.simplefilter('ignore')
                cg.solve([bt], [xt])
            torch.cuda.synchronize()
            out.append((h.o0, h.o1, xt.cpu().numpy(), list(cg.residuals), list(cg.alphas), list(cg.betas),
                        bool(cg.breakdown)))
            h.close()
        q.put((rank, out))
    finally:
        dist.destroy_process_group()


def test_two_processes_host_exchange(lib_built):
    """the healthy x0 = x7 solve and neg2 in one pair of rank processes, every
    exchange and all-reduce through gloo: identical histories and the same
    breakdown flag on the two ranks, within contract of the reference"""
    import torch.multiprocessing as mp
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_gloo_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = dict(q.get(timeout=200) for _ in range(2))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for i, case in enumerate(GLOO_CASES):
        s = pe.system(pe.CASES[case]['system'])[1]
        r0, r1 = got[0][i], got[1][i]
        assert r0[3:] == r1[3:]
        assert r0[6] == (pe.CASES[case]['outcome'] == 'rz_neg')
        x = np.zeros(s.N)
        for o0, o1, xl, *_ in (r0, r1):
            x[o0:o1], x[s.nv + o0:s.nv + o1] = xl[:o1 - o0], xl[o1 - o0:]
        _contract(case, r0[3], r0[4], r0[5], x, what='gloo')
