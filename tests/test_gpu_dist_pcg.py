"""Device-resident PCG on row-partitioned ranks:
mamg_dist_virtual_pcg on virtual ranks (eager and as one captured lockstep
iteration), mamg_dist_pcg_device over a one-rank RCCL communicator (the
cached iteration graph) and in two processes through the host-staged gloo
exchange.

The reference is never the code under test: mamg_oracle.pcg around the
oracle's apply for the cbc.block rule, and for stop type 1 the host loop
krylov.ConjGrad(device=False, stop_type=1) around the oracle's apply.  The
project's PCG contract: equal iteration count, every residual
within 1e-6 relative, the solution within 1e-6.  The systems are those of
tests/test_gpu_dist.py and tests/dist_csr_ref.py."""
import numpy as np
import pytest

import dist_csr_ref as dc
import mamg_oracle as mo

pytestmark = pytest.mark.gpu

# name -> (kind, arguments): nodal bidomain systems (dim, n, gamma) and the scalar cases of dist_csr_ref
SYSTEMS = {'b3': ('nodal', (3, 16, 1e4)), 'b2': ('nodal', (2, 32, 1e4)),
           'uahemw': ('scalar', 'bidomain3d_ua_hem_w'), '3d1d': ('scalar', '3d1d')}
_cache = {}


def _M():
    import metric_amg_examples_amd as M
    return M


def _system(name):
    """(A, b, oracle handle, nodal system or None): built once per system, shared, read-only"""
    if name not in _cache:
        kind, arg = SYSTEMS[name]
        if kind == 'nodal':
            s = _M().problems.bidomain(*arg)
            A = s.scipy()
            h = mo.setup(A, mo.Params(num_functions=2), idofs=s.idofs)
        else:
            s = None
            A, idofs, _, _ = dc.case(arg)
            okw = dc._case_table()[arg][2][1]
            h = mo.setup(A, mo.Params(num_functions=1, **okw), idofs=idofs)
        b = mo.seeded_rhs(A.shape[0])
        b.setflags(write=False)
        _cache[name] = (A, b, h, s)
    return _cache[name]


class _OracleB:
    """the oracle's apply behind the `B * r` the host ConjGrad calls"""

    def __init__(self, h):
        self.h = h

    def __mul__(self, r):
        return self.h.apply(r)


def _reference(name, stop, tol):
    """(x, residuals, ||r|| history or None) of the reference solve, once per (system, rule)"""
    k = ('ref', name, stop, tol)
    if k not in _cache:
        A, b, h, _ = _system(name)
        if stop == 0:
            ref = mo.pcg(A, h.apply, np.array(b), tol, 500)
            out = (np.array(ref.x), np.array(ref.residuals), None)
        else:
            cg = _M().ConjGrad(A, precond=_OracleB(h), tolerance=tol, maxiter=500, device=False, stop_type=1)
            x = cg * np.array(b)
            out = (np.array(x), np.array(cg.residuals), np.array(cg.residual_norms))
        for a in out:
            if a is not None:
                a.setflags(write=False)
        _cache[k] = out
    return _cache[k]


def _ranks(name, P, rep, comm_id=None):
    M = _M()
    kind, arg = SYSTEMS[name]
    if kind == 'nodal':
        s = _system(name)[3]
        return [M.DistMetricAMG(s, s.W, idofs=s.idofs, rank=p, nranks=P, comm_id=comm_id, rep_nodes=rep,
                                num_functions=2) for p in range(P)]
    A, idofs, kw, _ = dc.case(arg)
    return [M.DistMetricAMG(A, None, idofs=idofs, rank=p, nranks=P, comm_id=comm_id, rep_nodes=rep, **kw)
            for p in range(P)]


def _slices(hs, v):
    import torch
    return [torch.as_tensor(np.array(h.local_slice(v), dtype=np.float64)).cuda() for h in hs]


def _gather(name, hs, xs):
    s = _system(name)[3]
    if s is None:
        return np.concatenate([x.cpu().numpy() for x in xs])
    out = np.zeros(s.N)
    for h, xl in zip(hs, xs):
        xl = xl.cpu().numpy()
        out[h.o0:h.o1] = xl[:h.nloc]
        out[s.nv + h.o0:s.nv + h.o1] = xl[h.nloc:]
    return out


def _close(hs):
    for h in hs:
        h.close()


def _solve(hs, b, stop, tol, maxiter=500, graph=False, xs=None):
    """device-resident solve on virtual ranks: (solver, list of solution slices)"""
    import torch
    M = _M()
    cg = M.DistConjGrad.for_handles(list(hs), device=True, graph=graph, tolerance=tol, maxiter=maxiter,
                                    stop_type=1 if stop else None)
    xs = cg.solve(_slices(hs, b), xs)
    torch.cuda.synchronize()
    return cg, xs


def _history(cg):
    return [np.array(cg.residuals), np.array(cg.alphas), np.array(cg.betas), np.array(cg.residual_norms)]


def _check_against_reference(name, stop, tol, cg, x):
    xr, res, norms = _reference(name, stop, tol)
    assert len(cg.residuals) == len(res), (len(cg.residuals), len(res))
    assert len(cg.alphas) == len(cg.betas) == len(res) - 1
    assert np.allclose(cg.residuals, res, rtol=1e-6, atol=0)
    if stop:
        assert len(cg.residual_norms) == len(norms)
        assert np.allclose(cg.residual_norms, norms, rtol=1e-6, atol=0)
    else:
        assert cg.residual_norms == []
    assert np.linalg.norm(x - xr) / np.linalg.norm(xr) < 1e-6


VIRTUAL = [('b3', 1, 100, 0, 1e-8), ('b3', 3, 100, 0, 1e-8), ('b2', 8, 10 ** 6, 0, 1e-8),
           ('uahemw', 3, 1, 0, 1e-8), ('3d1d', 3, 1, 0, 1e-8), ('3d1d', 3, 1, 1, 1e-6)]


@pytest.mark.parametrize('name,P,rep,stop,tol', VIRTUAL)
def test_virtual_ranks_eager(lib_built, name, P, rep, stop, tol):
    """P virtual ranks in lockstep against the reference; the host-loop
    DistConjGrad on the same handles is printed for comparison only"""
    import torch
    M = _M()
    b = _system(name)[1]
    hs = _ranks(name, P, rep)
    cg, xs = _solve(hs, b, stop, tol)
    x = _gather(name, hs, xs)
    host = M.DistConjGrad.for_handles(hs if P > 1 else hs[0], tolerance=tol, maxiter=500,
                                      stop_type=1 if stop else None)
    host.solve(_slices(hs, b))
    torch.cuda.synchronize()
    _close(hs)
    m = min(len(host.residuals), len(cg.residuals))
    dev = np.max(np.abs(np.array(cg.residuals[:m]) / np.array(host.residuals[:m]) - 1.0))
    print('%s P=%d stop %d: %d iterations (host loop %d, reference %d); history vs host loop %.3e'
          % (name, P, stop, len(cg.residuals) - 1, len(host.residuals) - 1,
             len(_reference(name, stop, tol)[1]) - 1, dev))
    assert not cg.breakdown
    _check_against_reference(name, stop, tol, cg, x)


@pytest.mark.parametrize('name,rep,stop,tol', [('b3', 100, 0, 1e-8), ('3d1d', 1, 0, 1e-8), ('3d1d', 1, 1, 1e-6)])
def test_virtual_graph_equals_eager_bitwise(lib_built, name, rep, stop, tol):
    """one captured lockstep iteration replayed = the eager lockstep run, bit
    for bit (x and all four histories); a second solve into a fresh x
    repeats the first"""
    b = _system(name)[1]
    hs = _ranks(name, 3, rep)
    ce, xe = _solve(hs, b, stop, tol)
    cgr, xg = _solve(hs, b, stop, tol, graph=True)
    cg2, xg2 = _solve(hs, b, stop, tol, graph=True)
    ce2, xe2 = _solve(hs, b, stop, tol)
    _close(hs)
    assert len(ce.residuals) > 3
    for other, xo in ((cgr, xg), (cg2, xg2), (ce2, xe2)):
        for u, v in zip(_history(ce), _history(other)):
            assert np.array_equal(u, v)
        for u, v in zip(xe, xo):
            assert np.array_equal(u.cpu().numpy(), v.cpu().numpy())


@pytest.mark.parametrize('name,rep,stop,tol', [('b3', 100, 0, 1e-8), ('3d1d', 1, 1, 1e-6)])
def test_queued_extra_iteration_does_nothing(lib_built, name, rep, stop, tol):
    """The host stays one iteration ahead, so a solve that stops on the
    tolerance has one more iteration queued than one that stops on maxiter:
    the same x, bit for bit.  maxiter = 3 is exactly the first three
    iterations; b = 0 is no iteration and an untouched x."""
    import torch
    b = _system(name)[1]
    hs = _ranks(name, 3, rep)
    full, xf = _solve(hs, b, stop, tol)
    n = len(full.residuals) - 1
    exact, xe = _solve(hs, b, stop, tol, maxiter=n)
    three, _ = _solve(hs, b, stop, tol, maxiter=3)
    x0 = [torch.zeros_like(x) for x in xf]
    zero, xz = _solve(hs, np.zeros_like(b), stop, tol, xs=x0)
    _close(hs)
    assert 3 < n < 500
    assert len(exact.residuals) - 1 == n
    for u, v in zip(_history(full), _history(exact)):
        assert np.array_equal(u, v)
    for u, v in zip(xf, xe):
        assert np.array_equal(u.cpu().numpy(), v.cpu().numpy())
    assert len(three.residuals) == 4 and len(three.alphas) == 3 and len(three.betas) == 3
    assert np.array_equal(three.residuals, full.residuals[:4])
    assert np.array_equal(three.alphas, full.alphas[:3]) and np.array_equal(three.betas, full.betas[:3])
    if stop:
        assert np.array_equal(three.residual_norms, full.residual_norms[:4])
    assert len(zero.residuals) == 1 and zero.residuals[0] == 0.0 and zero.alphas == []
    assert all(x is y and not bool(x.any()) for x, y in zip(x0, xz))


@pytest.mark.parametrize('name,rep,stop,tol', [('b3', 100, 0, 1e-8), ('3d1d', 1, 1, 1e-6)])
def test_single_rank_rccl(lib_built, name, rep, stop, tol):
    """one rank over a real RCCL communicator (empty send / receive groups and
    one-rank all-reduces inside the captured iteration), called twice so the
    second solve replays the cached graph: the history of the P = 1 virtual
    run bit for bit, the reference's iteration count"""
    import torch
    M = _M()
    b = _system(name)[1]
    hv = _ranks(name, 1, rep)
    cv, xv = _solve(hv, b, stop, tol)
    _close(hv)
    d = _ranks(name, 1, rep, comm_id=M.DistMetricAMG.unique_id())[0]
    cg = M.DistConjGrad.for_handles(d, device=True, stream=torch.cuda.current_stream(), tolerance=tol,
                                    maxiter=500, stop_type=1 if stop else None)
    bt = _slices([d], b)
    xt = [torch.zeros_like(bt[0])]
    runs = []
    for _ in range(2):
        xt[0].zero_()
        cg.solve(bt, xt)
        torch.cuda.synchronize()
        runs.append((_history(cg), xt[0].cpu().numpy().copy()))
    d.close()
    for hist, x in runs:
        for u, v in zip(hist, _history(cv)):
            assert np.array_equal(u, v)
        assert np.array_equal(x, xv[0].cpu().numpy())
    assert len(cg.residuals) == len(_reference(name, stop, tol)[1])
    _check_against_reference(name, stop, tol, cg, _gather(name, [d], xt))


def _free_port():
    import socket
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _host_exchange_worker(rank, world, port, q):
    """one rank process: the rank-local handle on the (shared) GPU, the
    device-resident loop's exchanges through the host-staged gloo transport"""
    import os
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for p in (root, os.path.join(root, 'oracle')):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    import torch
    import torch.distributed as dist
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        import metric_amg_examples_amd as M
        import mamg_oracle
        s = M.problems.bidomain(3, 16, 1e4)
        h = M.DistMetricAMG(s, s.W, idofs=s.idofs, rank=rank, nranks=world, comm_id=None, rep_nodes=100,
                            exchange='gloo', num_functions=2)
        b = torch.as_tensor(h.local_slice(mamg_oracle.seeded_rhs(s.N))).cuda()
        cg = M.DistConjGrad.for_handles(h, device=True, tolerance=1e-8, maxiter=500)
        x = cg.solve([b])[0]
        torch.cuda.synchronize()
        q.put((rank, h.o0, h.o1, x.cpu().numpy(), list(cg.residuals), list(cg.alphas), list(cg.betas)))
        h.close()
    finally:
        dist.destroy_process_group()


def test_two_processes_host_exchange(lib_built):
    """two rank processes on one GPU, device=True in each, every exchange and
    both all-reduces of an iteration through gloo: the reference's iteration
    count and residuals, and identical histories on the two ranks"""
    import torch.multiprocessing as mp
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_host_exchange_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=200) for _ in range(2)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    xr, ref, _ = _reference('b3', 0, 1e-8)
    s = _system('b3')[3]
    x = np.zeros(s.N)
    for rank, o0, o1, xl, resid, al, be in res:
        nloc = o1 - o0
        x[o0:o1], x[s.nv + o0:s.nv + o1] = xl[:nloc], xl[nloc:]
        assert len(resid) == len(ref)
        assert np.allclose(resid, ref, rtol=1e-6, atol=0)
    assert res[0][4:] == res[1][4:]
    assert np.linalg.norm(x - xr) / np.linalg.norm(xr) < 1e-6


def test_pcg_launches(lib_built):
    """what one iteration issues: only kernels on one rank; on three, the
    apply's all-reduces plus the two of the dots, for either stopping rule"""
    for name, rep in (('b3', 100), ('uahemw', 1)):
        h1 = _ranks(name, 1, rep)[0]
        for stop in (None, 1):
            c = h1.pcg_launches(stop)
            assert c['kernels'] > h1.apply_launches['kernels']
            assert all(v == 0 for k, v in c.items() if k != 'kernels')
        h1.close()
        hs = _ranks(name, 3, rep)
        for h in hs:
            a, c0, c1 = h.apply_launches, h.pcg_launches(), h.pcg_launches(1)
            print(name, 'rank', h.rank, 'apply', a, 'PCG iteration', c0)
            assert c0['allreduces'] == c1['allreduces'] == a['allreduces'] + 2
            assert c0['kernels'] == c1['kernels'] > a['kernels']
            assert c0['p2p_groups'] > a['p2p_groups'] and c0['p2p_messages'] > a['p2p_messages']
        _close(hs)
