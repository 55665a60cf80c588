"""Scalar (CSR) hierarchies on N ranks on the GPU: the
row-partitioned cycle of num_functions 1 systems -- Jacobi-family / POLY
smoothers and the additive seed blocks of the 3D-1D preset -- on virtual
ranks (eager and as one hipGraph), over a one-rank RCCL communicator and in
two processes through the host-staged exchange, against the one-GPU apply and
the oracle.  The systems are those of tests/test_dist_csr.py
(tests/dist_csr_ref.py)."""
import numpy as np
import pytest

import dist_csr_ref as dc
from conftest import set_opt

pytestmark = pytest.mark.gpu


def _M():
    import metric_amg_examples_amd as M
    return M


def _rel(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def _ranks(name, P, rep):
    M = _M()
    A, idofs, kw, _ = dc.case(name)
    hs = [M.DistMetricAMG(A, None, idofs=idofs, rank=p, nranks=P, comm_id=None, rep_nodes=rep, **kw)
          for p in range(P)]
    assert all(h.dofs_per_node == 1 and h.nv == A.shape[0] for h in hs)
    assert hs[0].o0 == 0 and hs[-1].o1 == A.shape[0]
    return hs


def _slices(hs, v):
    import torch
    return [torch.as_tensor(np.array(h.local_slice(v), dtype=np.float64)).cuda() for h in hs]


def _gather(zs):
    return np.concatenate([z.cpu().numpy() for z in zs])


def _close(hs):
    for h in hs:
        h.close()


_one_gpu = {}


def _one_gpu_apply(name):
    """the one-GPU MetricAMG apply to the case's right-hand side (once per case)"""
    if name not in _one_gpu:
        M = _M()
        A, idofs, kw, levels = dc.case(name)
        B = M.MetricAMG(A, None, idofs=idofs, **kw)
        assert B.num_levels == len(levels)
        z = np.array(B * dc.oracle_apply(name)[0])
        B.close()
        z.setflags(write=False)
        _one_gpu[name] = z
    return _one_gpu[name]


VIRTUAL = [('bidomain2d', 2, 100), ('bidomain2d', 3, 10 ** 6), ('bidomain2d_seeds', 3, 1),
           ('bidomain3d_ua_hem', 3, 1), ('bidomain3d_ua_hem_w', 3, 1), ('bidomain3d_poly3', 8, 100),
           ('permuted2d', 3, 100), ('3d1d', 2, 1), ('3d1d', 3, 1), ('3d1d', 8, 1)]


@pytest.mark.parametrize('name,P,rep', VIRTUAL)
def test_virtual_ranks(lib_built, name, P, rep):
    """The gathered apply of P virtual ranks equals the one-GPU apply to 1e-12
    and the oracle's to 1e-10 (summation order only: local column order,
    partial restriction sums); a second apply repeats the first bit for bit."""
    import torch
    M = _M()
    r, zo = dc.oracle_apply(name)
    z1 = _one_gpu_apply(name)
    hs = _ranks(name, P, rep)
    rs = _slices(hs, r)
    zs = [torch.full_like(x, float('nan')) for x in rs]
    z2 = [torch.full_like(x, float('nan')) for x in rs]
    M.DistMetricAMG.virtual_apply(hs, rs, zs)
    M.DistMetricAMG.virtual_apply(hs, rs, z2)
    torch.cuda.synchronize()
    z = _gather(zs)
    e1, eo = _rel(z, z1), _rel(z, zo)
    print('%s P=%d rep_nodes=%d: vs one GPU %.3e, vs oracle %.3e; rank 0 issues %s'
          % (name, P, rep, e1, eo, hs[0].apply_launches))
    assert all(torch.equal(a, b) for a, b in zip(zs, z2))
    assert hs[0].apply_bytes > 0
    _close(hs)
    assert e1 < 1e-12
    assert eo < 1e-10


@pytest.mark.parametrize('name,P', [('3d1d', 3), ('bidomain3d_ua_hem_w', 3)])
def test_virtual_ranks_graph_bitwise(lib_built, name, P):
    """the lockstep apply captured into one hipGraph is the eager one bit for bit"""
    import torch
    M = _M()
    r, _ = dc.oracle_apply(name)
    hs = _ranks(name, P, 1)
    rs = _slices(hs, r)
    ze = [torch.zeros_like(x) for x in rs]
    zg = [torch.full_like(x, float('nan')) for x in rs]
    M.DistMetricAMG.virtual_apply(hs, rs, ze)
    M.DistMetricAMG.virtual_apply(hs, rs, zg, graph=True)
    torch.cuda.synchronize()
    same = all(torch.equal(a, b) for a, b in zip(ze, zg))
    _close(hs)
    assert same


@pytest.mark.parametrize('name,P', [('3d1d', 3), ('bidomain2d', 2)])
def test_virtual_ranks_overlap_bitwise(lib_built, name, P):
    """The level-0 residual and the rank SpMV split into the ghost-free row
    run (on the side stream during the halo) and the rest: bitwise the unsplit
    launches.  3D-1D at P = 3 has a long interior run; the field-major
    bidomain at P = 2 has none worth the name (every coupled row has a ghost
    column)."""
    import torch
    M = _M()
    r, _ = dc.oracle_apply(name)
    out, forks = [], []
    for ov in ('1', '0'):
        set_opt('MAMG_OVERLAP', ov)
        hs = _ranks(name, P, 1)
        rs = _slices(hs, r)
        zs = [torch.zeros_like(x) for x in rs]
        ys = [torch.zeros_like(x) for x in rs]
        M.DistMetricAMG.virtual_apply(hs, rs, zs)
        M.DistMetricAMG.virtual_spmv(hs, rs, ys)
        torch.cuda.synchronize()
        out.append([z.cpu().numpy() for z in zs] + [y.cpu().numpy() for y in ys])
        forks.append([h.apply_launches['stream_forks'] for h in hs])
        _close(hs)
    print(name, 'stream forks per apply with / without the overlap', forks)
    assert all(np.array_equal(a, b) for a, b in zip(out[0], out[1]))
    assert all(f == 1 for f in forks[0]) and all(f == 0 for f in forks[1])


@pytest.mark.parametrize('name,P', [('permuted2d', 3), ('3d1d', 8)])
def test_virtual_spmv_within_row_bound(lib_built, name, P):
    """the rank SpMV against A x accumulated in long double: per row
    |y_i - ref_i| <= (len_i + 2) 2^-53 sum_j |a_ij x_j| (any summation order)"""
    import torch
    M = _M()
    A = dc.case(name)[0]
    x = np.random.default_rng(3).standard_normal(A.shape[0])
    hs = _ranks(name, P, 1)
    xs = _slices(hs, x)
    ys = [torch.full_like(v, float('nan')) for v in xs]
    M.DistMetricAMG.virtual_spmv(hs, xs, ys)
    torch.cuda.synchronize()
    y = _gather(ys)
    _close(hs)
    prod = A.data.astype(np.longdouble) * x[A.indices].astype(np.longdouble)
    ref = np.add.reduceat(prod, A.indptr[:-1])
    mag = np.add.reduceat(np.abs(prod), A.indptr[:-1])
    ln = np.diff(A.indptr)
    assert ln.min() >= 1
    bound = (ln + 2) * np.longdouble(2.0) ** -53 * mag
    err = np.abs(y.astype(np.longdouble) - ref)
    worst = int(np.argmax(err / bound))
    print(name, 'P', P, 'worst err / bound %.3f at row %d (len %d)' % (float(err[worst] / bound[worst]), worst,
                                                                    int(ln[worst])))
    assert np.all(err <= bound), (worst, float(err[worst]), float(bound[worst]))


_pcg_ref = {}


def _one_gpu_pcg():
    if not _pcg_ref:
        M = _M()
        A, idofs, kw, _ = dc.case('3d1d')
        b = dc.oracle_apply('3d1d')[0]
        B = M.MetricAMG(A, None, idofs=idofs, **kw)
        cg = M.ConjGrad(A, precond=B, tolerance=1e-8, maxiter=500)
        x = cg * b
        x = x.cpu().numpy() if hasattr(x, 'cpu') else np.asarray(x)
        _pcg_ref.update(x=np.array(x), n=len(cg.residuals))
        B.close()
    return _pcg_ref['x'], _pcg_ref['n']


@pytest.mark.parametrize('P', [1, 3])
def test_dist_pcg(lib_built, P):
    """DistConjGrad.for_handles on scalar handles (rank SpMV with halo, the
    distributed cycle, dots summed over the ranks): the iteration count of
    ConjGrad with the one-GPU preconditioner, the same solution to 1e-6"""
    M = _M()
    xo, n = _one_gpu_pcg()
    b = dc.oracle_apply('3d1d')[0]
    hs = _ranks('3d1d', P, 1)
    cg = M.DistConjGrad.for_handles(hs if P > 1 else hs[0], tolerance=1e-8, maxiter=500)
    x = _gather(cg.solve(_slices(hs, b)))
    _close(hs)
    print('3d1d P=%d: %d PCG iterations (one GPU %d), solutions differ by %.3e'
          % (P, len(cg.residuals) - 1, n - 1, _rel(x, xo)))
    assert len(cg.residuals) == n
    assert _rel(x, xo) < 1e-6


def test_single_rank_rccl(lib_built):
    """one rank over a real RCCL communicator (empty send / receive groups,
    all-reduces over one rank, the side-stream fork), eager and replayed from
    a hipGraph: the oracle's apply, graph bitwise the eager run"""
    import torch
    M = _M()
    for name in ('3d1d', 'bidomain3d_ua_hem_w'):
        A, idofs, kw, _ = dc.case(name)
        r, zo = dc.oracle_apply(name)
        d = M.DistMetricAMG(A, None, idofs=idofs, rank=0, nranks=1, comm_id=M.DistMetricAMG.unique_id(),
                            rep_nodes=1, **kw)
        st = torch.cuda.current_stream()
        rt = _slices([d], r)[0]
        ze, zg = torch.zeros_like(rt), torch.full_like(rt, float('nan'))
        d.apply_device(rt, ze, st)
        d.apply_graph(rt, zg, st)
        torch.cuda.synchronize()
        assert torch.equal(ze, zg)
        zg.fill_(float('nan'))
        ms, _, _ = d.time_apply(rt, zg, 3, 2, st)       # graph replays
        ms1, _, cb = d.time_apply(rt, zg, 3, 1, st)
        torch.cuda.synchronize()
        e = _rel(ze.cpu().numpy(), zo)
        print(name, 'one RCCL rank vs oracle %.3e' % e)
        assert ms > 0 and ms1 > 0 and torch.equal(ze, zg) and abs(sum(cb) - d.apply_bytes) <= 1e-9 * d.apply_bytes
        d.close()
        assert e < 1e-10


def _free_port():
    import socket
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _host_exchange_worker(rank, world, port, q):
    """one rank process: the rank-local scalar handle on the (shared) GPU, its
    exchanges through the host-staged gloo transport"""
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
        s = M.problems.emi_3d1d(12, 1e4, 1.0)
        h = M.DistMetricAMG(s.scipy(), None, idofs=s.idofs, rank=rank, nranks=world, comm_id=None, rep_nodes=1,
                            exchange='gloo', parameters=dict(M.parameters.parameters_metric_3d1d, coarse_dof=100))
        r = torch.as_tensor(np.ascontiguousarray(h.local_slice(mamg_oracle.seeded_rhs(s.N)))).cuda()
        z = torch.zeros_like(r)
        h.apply_device(r, z)
        torch.cuda.synchronize()
        q.put((rank, h.o0, h.o1, z.cpu().numpy(), h.apply_launches))
        h.close()
    finally:
        dist.destroy_process_group()


def test_two_processes_host_exchange(lib_built):
    """Two rank processes on one GPU through the host-staged gloo exchange
    (3D-1D, n = 12, every level above the coarsest distributed): the
    width-1 pack / reverse-add kernels around pinned staging; the gathered
    apply equals the oracle's"""
    import mamg_oracle as mo
    import torch.multiprocessing as mp
    M = _M()
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
    s = M.problems.emi_3d1d(12, 1e4, 1.0)
    h = mo.setup(s.scipy(), mo.Params(num_functions=1, Schwarz_type=5, Schwarz_maxlvl=2, Schwarz_mmsize=200,
                                      coarse_dof=100, max_levels=30), idofs=s.idofs)
    r = mo.seeded_rhs(s.N)
    zo = h.apply(r)
    z = np.zeros(s.N)
    for rank, o0, o1, zl, launches in res:
        print('rank', rank, launches)
        assert launches['p2p_groups'] > 0 and launches['p2p_messages'] > 0
        z[o0:o1] = zl
    e = _rel(z, zo)
    print('two processes, host exchange, vs oracle %.3e' % e)
    assert e < 1e-10
