"""The host plumbing both handles share: the (r, z)
graph cache of a rank handle across its cap of 16, the PCG plan caches across
their cap of 4, and the timed run on both handles.  Everything is compared
bit for bit with another path of the same library (eager against graph, a
later solve against the first), so these tests pin behaviour, not accuracy:
the accuracy of every path here is the subject of test_gpu_dist.py,
test_gpu_dist_pcg.py and test_gpu_pcg_edges.py.

The system is the 2-D bidomain generator at n = 16 (N = 578), the smallest on
which a multi-level BSR2 hierarchy, the graph paths and a PCG of several
iterations all engage."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TOL, MAXITER = 1e-8, 60
_cache = {}


def _M():
    import metric_amg_examples_amd as M
    return M


def _system():
    """(system, scipy A, right-hand side): built once, shared, read-only"""
    if 'sys' not in _cache:
        s = _M().problems.bidomain(2, 16, 1e4)
        b = _M().problems.seeded_rhs(s.N)
        b.setflags(write=False)
        _cache['sys'] = (s, s.scipy(), b)
    return _cache['sys']


def _ranks(P):
    s = _system()[0]
    return [_M().DistMetricAMG(s, s.W, idofs=s.idofs, rank=p, nranks=P, comm_id=None, num_functions=2)
            for p in range(P)]


def _single():
    s, A, _ = _system()
    return _M().MetricAMG(A, [s.nv, s.nv], idofs=s.idofs, num_functions=2)


def _slices(hs, v):
    import torch
    return [torch.as_tensor(np.array(h.local_slice(v), dtype=np.float64)).cuda() for h in hs]


def test_rank_graph_cache_across_its_cap(lib_built):
    """20 distinct (r, z) pairs through mamg_dist_apply_graph on a one-rank
    handle (cap 16: the first four are evicted), each the eager apply's bits;
    then the first pair again, captured anew."""
    import torch
    h = _ranks(1)[0]
    try:
        n = h.local_size
        rng = np.random.default_rng(7)
        rs = [torch.as_tensor(rng.standard_normal(n)).cuda() for _ in range(20)]
        zs = [torch.full((n,), float('nan'), dtype=torch.float64, device='cuda') for _ in range(20)]
        ze = [torch.empty(n, dtype=torch.float64, device='cuda') for _ in range(20)]
        for r, z, e in zip(rs, zs, ze):
            h.apply_device(r, e)
            h.apply_graph(r, z)
        torch.cuda.synchronize()
        for i in range(20):
            assert torch.equal(zs[i], ze[i]), i
        assert len({(r.data_ptr(), z.data_ptr()) for r, z in zip(rs, zs)}) == 20
        zs[0].fill_(float('nan'))
        h.apply_graph(rs[0], zs[0])
        torch.cuda.synchronize()
        assert torch.equal(zs[0], ze[0])
    finally:
        h.close()


def _same_solves(solve, new_x):
    """six solves into six x buffers, then one more into the first: all equal the first, bit for bit"""
    import torch
    xs = [new_x() for _ in range(6)]
    first = solve(xs[0])
    assert first[3] >= 3, first[3]                      # the loop ran: there is a history to compare
    keep = [t.clone() for t in xs[0]]
    for x in xs[1:] + [None]:
        if x is None:                                   # the evicted first plan again, from x0 = 0
            x = xs[0]
            for t in x:
                t.zero_()
        got = solve(x)
        assert got[3] == first[3]
        for a, b in zip(got[:3], first[:3]):
            assert np.array_equal(np.array(a), np.array(b))
        torch.cuda.synchronize()
        for t, k in zip(x, keep):
            assert torch.equal(t, k)
    assert len({x[0].data_ptr() for x in xs}) == 6


def test_pcg_graph_cache_across_its_cap(lib_built):
    """mamg_pcg_device: (x, maxiter) iteration graphs, at most 4 kept"""
    import torch
    _, A, b = _system()
    B = _single()
    try:
        bt = torch.as_tensor(np.array(b)).cuda()
        cg = _M().ConjGrad(A, precond=B, tolerance=TOL, maxiter=MAXITER)

        def solve(x):
            cg.solve_device(bt, x[0])
            return cg.residuals, cg.alphas, cg.betas, len(cg.residuals) - 1
        _same_solves(solve, lambda: [torch.zeros_like(bt)])
    finally:
        B.close()


@pytest.mark.parametrize('mode', ['rank', 'virtual', 'virtual-graph'])
def test_dist_pcg_plan_cache_across_its_cap(lib_built, mode):
    """mamg_dist_pcg_device on a one-rank handle (cached iteration graph) and
    mamg_dist_virtual_pcg on two virtual ranks, eager and as a captured
    lockstep iteration: (x, maxiter, stop_type) plans, at most 4 kept per rank"""
    import torch
    b = _system()[2]
    hs = _ranks(1 if mode == 'rank' else 2)
    try:
        bs = _slices(hs, b)
        cg = _M().DistConjGrad.for_handles(hs[0] if mode == 'rank' else hs, device=True,
                                            graph=mode == 'virtual-graph', tolerance=TOL, maxiter=MAXITER)

        def solve(x):
            cg.solve(bs, x)
            return cg.residuals, cg.alphas, cg.betas, len(cg.residuals) - 1
        _same_solves(solve, lambda: [torch.zeros_like(t) for t in bs])
    finally:
        for h in hs:
            h.close()


@pytest.mark.parametrize('kind', ['single', 'rank'])
def test_timed_run(lib_built, kind):
    """mamg_time_apply / mamg_dist_time_apply, reps = 2, modes 0 and 1: z is
    the graph apply's, class_bytes sums to apply_bytes, in mode 1 every class
    with bytes has a time; reps = 0 gives 0 ms and leaves z alone.

    class_bytes and apply_bytes add the same op bytes (integers below 2^53
    held in doubles) in two orders: the sums may differ by rounding only,
    bounded by (number of ops) x 2^-53 relative, far below the 1e-12 asked."""
    import torch
    b = _system()[2]
    h = _single() if kind == 'single' else _ranks(1)[0]
    try:
        r = torch.as_tensor(np.array(b)).cuda()
        zg = torch.empty_like(r)
        if kind == 'single':
            h.apply_device(r, zg)
        else:
            h.apply_graph(r, zg)
        for mode in (0, 1):
            z = torch.full_like(r, float('nan'))
            ms, kms, cb = h.time_apply(r, z, 2, mode)
            torch.cuda.synchronize()
            assert ms > 0
            assert torch.equal(z, zg), mode
            assert abs(sum(cb) - h.apply_bytes) <= 1e-12 * h.apply_bytes
            assert all(c >= 0 for c in cb) and all(t >= 0 for t in kms)
            if mode == 1:
                for c in range(16):
                    assert (kms[c] > 0) or cb[c] == 0, (c, kms[c], cb[c])
        z = torch.full_like(r, 3.0)
        ms, kms, cb = h.time_apply(r, z, 0, 1)
        torch.cuda.synchronize()
        assert ms == 0.0
        assert bool((z == 3.0).all())
        assert abs(sum(cb) - h.apply_bytes) <= 1e-12 * h.apply_bytes
    finally:
        h.close()
