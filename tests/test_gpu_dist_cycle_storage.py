"""fp32 storage of the cycle's operators on row-partitioned ranks
(mamg_dist_set_cycle_storage).

The contract is section 4.7's on every rank: the rounding is element-wise and
A_loc, K_loc, P_loc, Rp_loc are rows of the global operators (K_loc formed in
fp64 first), so one apply of N narrowed ranks is the narrowed one-GPU apply up
to summation order.  The references are never the code under test:

  * tests/cycle_storage_ref.StorageRef on the oracle's hierarchy, under the
    masks and the K form the ranks themselves report (bound: the suite's
    APPLY_TOL = 1e-10);
  * the one-GPU narrowed MetricAMG of the same hierarchy (bound 1e-12, the one
    the project uses where only the summation order differs).

That the result is more than 1e-8 away from the fp64 oracle apply shows the
rounding happened (the CPU restatement alone measures 1.5e-7 .. 2.4e-6 on
these systems).  The systems are those of tests/test_gpu_dist.py: 3-D n = 16
(a rank of 8 owns two z-planes: no ghost-free interior run; P = 3: uneven
ranges; rep_nodes 1: level 1's 199 nodes spread 25 to a rank, less than one
64-row slice), 2-D n = 32 and the EMI system.  Every case names its mode:
'sell' is MAMG_SELL_MIN_ROWS=1 (the benchmark's layouts: half-symmetric
level-0 A_loc with its ghost part, SELL K split around the coarse halo, SELL
coarse operators), 'default' the lane-group BSR2 kernels these sizes get.

Measured on the MI355X over the parity cases: 1.5e-15 .. 3.4e-13 against the
restatement, 1.2e-16 .. 3.8e-14 against the one-GPU narrowed apply, 1.5e-7 ..
3.7e-5 against the fp64 oracle apply; PCG solutions within 4.5e-14 of the
one-GPU narrowed solve.
"""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import mamg_oracle as mo
from conftest import set_opt
from cycle_storage_ref import ALL, BIT_A, BIT_KP, BIT_R, StorageRef
from test_gpu import APPLY_TOL, rel

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_UNSUPPORTED = -1, -4
ONE_GPU_TOL = 1e-12          # summation order only (tests/test_gpu_dist.py: N ranks against one GPU)
ROUNDED_MIN = 1e-8           # the narrowed apply is further than this from the fp64 oracle apply
CODES = {'smoother': {'POLY': 12, 'SGS': 11}, 'cycle_type': {'V': 1, 'W': 2}, 'AMG_type': {'UA': 1},
         'aggregation_type': {'HEM': 5}}

POLY2 = dict(smoother='POLY', poly_degree=2)
POLY3 = dict(smoother='POLY', poly_degree=3)
W22 = dict(cycle_type='W', coarse_scaling=1, presmooth_iter=2, postsmooth_iter=2)
UAHEM = dict(AMG_type='UA', aggregation_type='HEM', cycle_type='W', coarse_scaling=1)


def _M():
    import metric_amg_examples_amd as M
    return M


def to_c(kw):
    c = dict(kw)
    for key, names in CODES.items():
        if key in c:
            c[key] = names[c[key]]
    return c


@functools.lru_cache(maxsize=None)
def system(name):
    M = _M()
    if name == 'b3':
        return M.problems.bidomain(3, 16, 1e6), {}
    if name == 'b2':
        return M.problems.bidomain(2, 32, 1e6), {}
    assert name == 'emi'
    return M.problems.emi(3, 16, 1e6), dict(Schwarz_maxlvl=0)


@functools.lru_cache(maxsize=None)
def _oracle(name, kwt):
    s, extra = system(name)
    kw = dict(kwt)
    kw.pop('post_fusion', None)
    return mo.setup(s.scipy(), mo.Params(num_functions=2, **dict(extra, **kw)), idofs=s.idofs)


def oracle(name, kw):
    return _oracle(name, tuple(sorted(kw.items())))


@functools.lru_cache(maxsize=None)
def rhs(name, seed):
    r = mo.seeded_rhs(system(name)[0].N, seed)
    r.setflags(write=False)
    return r


def mode_opts(mode):
    if mode == 'sell':
        set_opt('MAMG_SELL_MIN_ROWS', '1')


def ranks(name, kw, P, rep, narrow=True, **more):
    M = _M()
    s, extra = system(name)
    A = s.tocsr() if name == 'emi' else s
    hs = [M.DistMetricAMG(A, s.W, idofs=s.idofs, rank=p, nranks=P, comm_id=None, rep_nodes=rep,
                          num_functions=2, **dict(to_c(dict(extra, **kw)), **more)) for p in range(P)]
    if narrow:
        for h in hs:
            h.set_cycle_storage('f32')
    return hs


def one_gpu(name, kw, narrow=True):
    M = _M()
    s, extra = system(name)
    B = M.MetricAMG(s.scipy(), s.W, idofs=s.idofs, num_functions=2, **to_c(dict(extra, **kw)))
    if narrow:
        B.set_cycle_storage('f32')
    return B


def close(hs):
    for h in hs:
        h.close()


def bits(h, l):
    s = h.level_storage(l)
    return (BIT_A if s['A'] else 0) | (BIT_KP if s['KP'] else 0) | (BIT_R if s['R'] else 0)


def reported(h):
    n = h.num_levels
    return [bits(h, l) for l in range(n)], [bool(h.level_format(l)['post_fused']) for l in range(n)]


def restatement(name, kw, masks, kform):
    return StorageRef(oracle(name, kw), masks=masks, kform=kform)


def slices(hs, v):
    import torch
    return [torch.as_tensor(np.array(h.local_slice(v), dtype=np.float64)).cuda() for h in hs]


def gather(name, hs, zs):
    s = system(name)[0]
    z = np.zeros(s.N)
    for h, zl in zip(hs, zs):
        zl = zl.cpu().numpy()
        z[h.o0:h.o1] = zl[:h.nloc]
        z[s.nv + h.o0:s.nv + h.o1] = zl[h.nloc:]
    return z


def vapply(name, hs, r, graph=False, zs=None):
    import torch
    M = _M()
    rs = slices(hs, r)
    zs = zs if zs is not None else [torch.full_like(x, float('nan')) for x in rs]
    M.DistMetricAMG.virtual_apply(hs, rs, zs, graph=graph)
    torch.cuda.synchronize()
    return zs


def check_report(hs, expect=ALL):
    """1d: every rank reports the same storage on every level: all three bits
    (expect) above the coarsest, 0 on it."""
    n = hs[0].num_levels
    for h in hs:
        assert h.num_levels == n
        assert [bits(h, l) for l in range(n)] == [expect] * (n - 1) + [0], (h.rank, [h.level_storage(l) for l in range(n)])


# ---------------------------------------------------------------------------
# 1. parity
# ---------------------------------------------------------------------------
PARITY = [
    ('b3', {}, 2, 100, 'sell'), ('b3', {}, 3, 1, 'sell'), ('b3', {}, 8, 32768, 'sell'), ('b3', {}, 8, 1, 'sell'),
    ('b3', {}, 3, 100, 'default'), ('b3', {}, 8, 1, 'default'),
    ('b3', POLY2, 3, 100, 'sell'), ('b3', POLY3, 8, 1, 'sell'), ('b3', POLY2, 2, 32768, 'default'),
    ('b3', W22, 3, 1, 'sell'), ('b3', W22, 8, 100, 'sell'), ('b3', W22, 2, 32768, 'default'),
    ('b3', UAHEM, 2, 1, 'sell'), ('b3', UAHEM, 8, 100, 'default'), ('b3', UAHEM, 3, 32768, 'sell'),
    ('b3', dict(post_fusion=0), 3, 100, 'sell'),
    ('b2', {}, 3, 100, 'sell'), ('b2', {}, 8, 1, 'sell'), ('b2', W22, 2, 32768, 'default'),
    ('emi', {}, 3, 100, 'sell'), ('emi', {}, 2, 1, 'default'), ('emi', POLY2, 8, 32768, 'sell'),
]


def pid(v):
    return '-'.join('%s=%s' % kv for kv in v.items()) or 'defaults' if isinstance(v, dict) else str(v)


@pytest.mark.parametrize('name,kw,P,rep,mode', PARITY, ids=pid)
def test_parity(lib_built, name, kw, P, rep, mode):
    """1a: within 1e-10 of StorageRef under the reported masks for two
    right-hand sides; 1b: within 1e-12 of the one-GPU narrowed apply; 1c: more
    than 1e-8 from the fp64 oracle apply; 1d: the report."""
    mode_opts(mode)
    hs = ranks(name, kw, P, rep)
    B = one_gpu(name, kw)
    try:
        check_report(hs)
        f = hs[0].level_format(0)
        if mode == 'sell' and name != 'emi':
            assert f['half'] and f['post_sell'] == bool(kw.get('post_fusion', 1)), f   # the ghost part is really taken
        masks, kform = reported(hs[0])
        assert kform[0] == bool(kw.get('post_fusion', 1))
        assert reported(B) == (masks, kform)
        ref = restatement(name, kw, masks, kform)
        h64 = oracle(name, kw)
        for seed in (1234, 7):
            r = rhs(name, seed)
            z = gather(name, hs, vapply(name, hs, r))
            e, d1, d64 = rel(z, ref.apply(r)), rel(z, B * np.array(r)), rel(z, h64.apply(np.array(r)))
            print(name, kw, 'P', P, 'rep', rep, mode, 'seed', seed,
                  'vs restatement %.2e, vs one GPU narrowed %.2e, vs fp64 oracle %.2e' % (e, d1, d64))
            assert e < APPLY_TOL, e
            assert d1 < ONE_GPU_TOL, d1
            assert d64 > ROUNDED_MIN, d64
    finally:
        close(hs)
        B.close()


def test_merged_post_operator_stays_fp64(lib_built):
    """MAMG_POST_K=0 stores [P_loc | AP_loc]: that operator keeps fp64 (bits 1
    and 4 only, as on one GPU); A_loc and Rp_loc narrow."""
    set_opt('MAMG_POST_K', '0')
    mode_opts('sell')
    hs = ranks('b3', {}, 3, 100)
    try:
        f = hs[0].level_format(0)
        assert f['post_fused'] and not f['post_k'], f
        check_report(hs, BIT_A | BIT_R)
        masks, kform = reported(hs[0])
        ref = restatement('b3', {}, masks, kform)
        r = rhs('b3', 1234)
        e = rel(gather('b3', hs, vapply('b3', hs, r)), ref.apply(r))
        print('merged [P | AP]: vs restatement %.2e' % e)
        assert e < APPLY_TOL, e
    finally:
        close(hs)


# ---------------------------------------------------------------------------
# 2. the same op list on every path
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('kw,P,rep,mode', [({}, 3, 100, 'sell'), ({}, 8, 1, 'sell'), (POLY2, 2, 100, 'default')], ids=pid)
def test_paths_bitwise(lib_built, kw, P, rep, mode):
    """Overlap split on and off, eager against the captured lockstep graph and
    a repeated apply: bitwise equal on narrowed ranks."""
    import torch
    mode_opts(mode)
    r = rhs('b3', 1234)
    out, forks = [], []
    for ov in ('1', '0'):
        set_opt('MAMG_OVERLAP', ov)
        hs = ranks('b3', kw, P, rep)
        try:
            check_report(hs)
            ze = vapply('b3', hs, r)
            zg = vapply('b3', hs, r, graph=True)
            z2 = vapply('b3', hs, r)
            for a, b, c in zip(ze, zg, z2):
                assert torch.equal(a, b) and torch.equal(a, c)
            out.append([z.cpu().numpy() for z in ze])
            forks.append(sum(h.apply_launches['stream_forks'] for h in hs))
        finally:
            close(hs)
    for a, b in zip(out[0], out[1]):
        assert np.array_equal(a, b)
    assert forks[0] > 0 and forks[1] == 0, forks


# ---------------------------------------------------------------------------
# 3. graphs dropped
# ---------------------------------------------------------------------------
def test_narrowing_drops_cached_graphs(lib_built):
    """A one-rank RCCL handle caches its apply graph per (r, z) and its PCG
    iteration graph per plan: apply and solve, narrow, apply and solve again
    into the same tensors.  The second apply obeys 1a and differs from the
    first; the second solve takes the restatement's iteration count."""
    import torch
    M = _M()
    mode_opts('sell')
    s = system('b3')[0]
    A = s.scipy()
    r = rhs('b3', 1234)
    d = M.DistMetricAMG(s, s.W, idofs=s.idofs, rank=0, nranks=1, comm_id=M.DistMetricAMG.unique_id(),
                        rep_nodes=100, num_functions=2)
    try:
        st = torch.cuda.current_stream()
        rt = torch.as_tensor(np.array(d.local_slice(r))).cuda()
        z, x = torch.zeros_like(rt), torch.zeros_like(rt)
        d.apply_graph(rt, z, st)
        cg = M.DistConjGrad.for_handles(d, device=True, tolerance=1e-8, maxiter=500)
        cg.solve([rt.clone()], [x])
        torch.cuda.synchronize()
        z64, it64 = z.clone(), len(cg.residuals)
        d.set_cycle_storage('f32')
        check_report([d])
        d.apply_graph(rt, z, st)
        x.zero_()
        cg.solve([rt.clone()], [x])
        torch.cuda.synchronize()
        masks, kform = reported(d)
        ref = restatement('b3', {}, masks, kform)
        e = rel(z.cpu().numpy(), ref.apply(r))
        assert e < APPLY_TOL, e
        assert not torch.equal(z, z64)
        pr = mo.pcg(A, ref, np.array(r), 1e-8, 500)
        print('one-rank graph: vs restatement %.2e, PCG iterations fp64 %d, fp32 %d, restatement %d'
              % (e, it64 - 1, len(cg.residuals) - 1, pr.niters))
        assert len(cg.residuals) == len(pr.residuals)
        assert np.allclose(cg.residuals, pr.residuals, rtol=1e-6, atol=0)
    finally:
        d.close()


def test_narrowing_between_virtual_applies(lib_built):
    """Each virtual rank: apply, narrow, apply into the same tensors."""
    import torch
    mode_opts('sell')
    r = rhs('b3', 7)
    hs = ranks('b3', {}, 3, 100, narrow=False)
    try:
        zs = vapply('b3', hs, r, graph=True)
        z64 = [z.clone() for z in zs]
        assert rel(gather('b3', hs, zs), oracle('b3', {}).apply(np.array(r))) < APPLY_TOL
        for h in hs:
            h.set_cycle_storage('f32')
        check_report(hs)
        vapply('b3', hs, r, graph=True, zs=zs)
        masks, kform = reported(hs[0])
        e = rel(gather('b3', hs, zs), restatement('b3', {}, masks, kform).apply(r))
        assert e < APPLY_TOL, e
        for a, b in zip(zs, z64):
            assert not torch.equal(a, b)
    finally:
        close(hs)


# ---------------------------------------------------------------------------
# 4. bytes
# ---------------------------------------------------------------------------
def node_blocks(M, o0=0):
    """(blocks, blocks left of the diagonal among the owned columns) of the 2x2
    node-block pattern of a field-major matrix whose row I is node o0 + I."""
    M = sp.csr_matrix(M)
    nr, nc = M.shape[0] // 2, M.shape[1] // 2
    C = M.tocoo()
    G = sp.csr_matrix((np.ones(C.nnz), (C.row % nr, C.col % nc)), shape=(nr, nc))
    G.sum_duplicates()
    G = G.tocoo()
    return G.nnz, int(np.sum((G.col >= o0) & (G.col < G.row + o0)))


def pattern(M):
    M = sp.csr_matrix(M, copy=True)
    M.data[:] = 1.0
    return M


def node_rows(M, o0, o1):
    """rows of the nodes [o0, o1) of a field-major matrix, field-major"""
    nr = M.shape[0] // 2
    return sp.csr_matrix(M)[np.r_[o0:o1, nr + o0:nr + o1], :]


def level_ranges(levels, P, rep):
    """The partition of DESIGN.md section 6: level l's nodes split nv q / P,
    replicated from the first level l > 0 of at most rep nodes (and the
    coarsest) on."""
    out, r = [], False
    for l, lev in enumerate(levels):
        nv = lev.A.shape[0] // 2
        r = r or (l > 0 and (nv <= rep or lev.Ainv is not None))
        out.append([(0, nv)] * P if r else [(nv * q // P, nv * (q + 1) // P) for q in range(P)])
    return out


@pytest.mark.parametrize('P,rep,mode', [(3, 100, 'sell'), (8, 1, 'sell'), (3, 1, 'default'), (2, 32768, 'default')])
def test_bytes(lib_built, P, rep, mode):
    """apply_bytes of each rank drops by 4 bytes per narrowed stored value
    (V cycle, nu = 1: each of A_loc, K_loc, Rp_loc is read once per apply; the
    half-symmetric A_loc stores its upper and ghost blocks, three values
    each).  The count comes from the oracle's matrices, the partition rule and
    the formats the rank reports.  The overlap split prices its three
    launches by row fractions, so the sums agree to fp64 rounding: 1e-12."""
    mode_opts(mode)
    h = oracle('b3', {})
    rng = level_ranges(h.levels, P, rep)
    hs = ranks('b3', {}, P, rep, narrow=False)
    try:
        before = [x.apply_bytes for x in hs]
        for x in hs:
            x.set_cycle_storage('f32')
        check_report(hs)
        for p, x in enumerate(hs):
            assert (x.o0, x.o1) == rng[0][p]
            saved = 0.0
            for l, lev in enumerate(h.levels[:-1]):
                f = x.level_format(l)
                o0, o1 = rng[l][p]
                nbA, nloA = node_blocks(node_rows(lev.A, o0, o1), o0)
                nbK, _ = node_blocks(node_rows(pattern(lev.A) @ pattern(lev.P), o0, o1))
                nbR, _ = node_blocks(node_rows(lev.P, o0, o1))
                assert f['post_k'], f
                saved += 4.0 * ((3 * (nbA - nloA) if f['half'] else 3 * nbA if f['sym'] else 4 * nbA) + 4 * nbK + 4 * nbR)
            after = x.apply_bytes
            print('rank', p, 'of', P, mode, 'apply bytes %.0f -> %.0f (derived saving %.0f)' % (before[p], after, saved))
            assert after < before[p]
            assert abs(after - (before[p] - saved)) <= 1e-12 * before[p], (after, before[p] - saved)
    finally:
        close(hs)


# ---------------------------------------------------------------------------
# 5. the Krylov operator stays fp64
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('P,mode', [(3, 'sell'), (8, 'default')])
def test_krylov_operator_stays_fp64(lib_built, P, mode):
    import torch
    M = _M()
    mode_opts(mode)
    s = system('b3')[0]
    x = rhs('b3', 7)
    hs = ranks('b3', {}, P, 100, narrow=False)
    try:
        xs = slices(hs, x)
        y0 = [torch.zeros_like(v) for v in xs]
        y1 = [torch.zeros_like(v) for v in xs]
        M.DistMetricAMG.virtual_spmv(hs, xs, y0)
        for h in hs:
            h.set_cycle_storage('f32')
        M.DistMetricAMG.virtual_spmv(hs, xs, y1)
        torch.cuda.synchronize()
        for a, b in zip(y0, y1):
            assert torch.equal(a, b)
        assert rel(gather('b3', hs, y1), s.scipy() @ np.array(x)) < 1e-13
    finally:
        close(hs)


# ---------------------------------------------------------------------------
# 6. device PCG
# ---------------------------------------------------------------------------
class _Times:
    """a callable behind the `B * r` the host ConjGrad calls"""

    def __init__(self, f):
        self.f = f

    def __mul__(self, r):
        return self.f(r)


def host_reference(A, B, b, stop, tol):
    """(x, residuals, ||r|| history) of the host loop ConjGrad(device=False) around the apply B"""
    cg = _M().ConjGrad(A, precond=_Times(B), tolerance=tol, maxiter=500, device=False, stop_type=1 if stop else None)
    x = cg * np.array(b)
    return np.array(x), np.array(cg.residuals), np.array(cg.residual_norms) if stop else None


def one_gpu_solution(A, B, b, stop, tol):
    """The one-GPU narrowed solve: its device PCG under the cbc.block rule; the
    one-GPU device PCG has no ||r|| / ||b|| rule, so there the host loop
    around the one-GPU narrowed apply."""
    M = _M()
    if stop:
        return host_reference(A, lambda r: B * r, b, 1, tol)[0]
    B._Aop = A
    return np.asarray(M.ConjGrad(A, precond=B, tolerance=tol, maxiter=500, device=True) * np.array(b))


def check_pcg(cg, x, ref, x1, stop):
    xr, res, norms = ref
    assert len(cg.residuals) == len(res), (len(cg.residuals), len(res))
    assert np.allclose(cg.residuals, res, rtol=1e-6, atol=0)
    if stop:
        assert len(cg.residual_norms) == len(norms)
        assert np.allclose(cg.residual_norms, norms, rtol=1e-6, atol=0)
    dx = rel(x, x1)
    print('PCG stop', stop, 'iterations %d (reference %d), solution vs one GPU narrowed %.2e, vs host reference %.2e'
          % (len(cg.residuals) - 1, len(res) - 1, dx, rel(x, xr)))
    assert dx < 1e-10, dx


@pytest.mark.parametrize('P,rep,mode,graph', [(3, 100, 'sell', False), (8, 1, 'sell', True), (3, 1, 'default', True),
                                              (8, 100, 'default', False)])
def test_device_pcg(lib_built, P, rep, mode, graph):
    import torch
    M = _M()
    mode_opts(mode)
    s = system('b3')[0]
    A = s.scipy()
    b = rhs('b3', 1234)
    hs = ranks('b3', {}, P, rep)
    B = one_gpu('b3', {})
    try:
        check_report(hs)
        masks, kform = reported(hs[0])
        ref = restatement('b3', {}, masks, kform)
        for stop, tol in ((0, 1e-8), (1, 1e-6)):
            cg = M.DistConjGrad.for_handles(list(hs), device=True, graph=graph, tolerance=tol, maxiter=500,
                                            stop_type=1 if stop else None)
            xs = cg.solve(slices(hs, b))
            torch.cuda.synchronize()
            check_pcg(cg, gather('b3', hs, xs), host_reference(A, ref.apply, b, stop, tol),
                      one_gpu_solution(A, B, b, stop, tol), stop)
    finally:
        close(hs)
        B.close()


# ---------------------------------------------------------------------------
# 7. two processes over the host-staged exchange
# ---------------------------------------------------------------------------
def _free_port():
    import socket
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _worker(rank, world, port, q, sell):
    """one rank process: its handle narrowed, one apply, one device PCG per stopping rule"""
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
        if sell:
            M._lib.set_option('MAMG_SELL_MIN_ROWS', '1')
        s = M.problems.bidomain(3, 16, 1e6)
        h = M.DistMetricAMG(s, s.W, idofs=s.idofs, rank=rank, nranks=world, comm_id=None, rep_nodes=100,
                            exchange='gloo', num_functions=2)
        h.set_cycle_storage('f32')
        n = h.num_levels
        rep = ([h._L.mamg_dist_level_storage(h._h, l) for l in range(n)],
               [bool(h.level_format(l)['post_fused']) for l in range(n)], h.level_format(0)['half'])
        r = torch.as_tensor(h.local_slice(mamg_oracle.seeded_rhs(s.N))).cuda()
        z = torch.zeros_like(r)
        h.apply_device(r, z)
        torch.cuda.synchronize()
        sol = []
        for stop, tol in ((None, 1e-8), (1, 1e-6)):
            cg = M.DistConjGrad.for_handles(h, device=True, tolerance=tol, maxiter=500, stop_type=stop)
            x = cg.solve([r.clone()])[0]
            torch.cuda.synchronize()
            sol.append((x.cpu().numpy(), list(cg.residuals), list(cg.residual_norms)))
        q.put((rank, h.o0, h.o1, rep, z.cpu().numpy(), sol))
        h.close()
    finally:
        dist.destroy_process_group()


def test_two_processes_host_exchange(lib_built):
    import queue
    import torch.multiprocessing as mp
    s = system('b3')[0]
    A = s.scipy()
    r = rhs('b3', 1234)
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(k, 2, port, q, True)) for k in range(2)]
    for p in procs:
        p.start()
    res = []
    try:
        for _ in range(2):
            res.append(q.get(timeout=240))
    except queue.Empty:
        pass
    for p in procs:
        p.join(timeout=60)
        if p.is_alive():
            p.kill()
            p.join()
    assert [p.exitcode for p in procs] == [0, 0] and len(res) == 2, ([p.exitcode for p in procs], len(res))
    masks, kform, half = res[0][3]
    assert all(x[3] == (masks, kform, half) for x in res) and half
    assert masks == [ALL] * (len(masks) - 1) + [0], masks
    ref = restatement('b3', {}, masks, kform)
    mode_opts('sell')
    B = one_gpu('b3', {})
    try:
        z = np.zeros(s.N)
        xs = [np.zeros(s.N), np.zeros(s.N)]
        for rank, o0, o1, _, zl, sol in res:
            nloc = o1 - o0
            z[o0:o1], z[s.nv + o0:s.nv + o1] = zl[:nloc], zl[nloc:]
            for k in range(2):
                xs[k][o0:o1], xs[k][s.nv + o0:s.nv + o1] = sol[k][0][:nloc], sol[k][0][nloc:]
        e = rel(z, ref.apply(r))
        print('two processes: apply vs restatement %.2e' % e)
        assert e < APPLY_TOL, e
        for k, (stop, tol) in enumerate(((0, 1e-8), (1, 1e-6))):
            xr, rr, nn = host_reference(A, ref.apply, r, stop, tol)
            x1 = one_gpu_solution(A, B, r, stop, tol)
            for rank, _, _, _, _, sol in res:
                assert len(sol[k][1]) == len(rr), (rank, stop, len(sol[k][1]), len(rr))
                assert np.allclose(sol[k][1], rr, rtol=1e-6, atol=0)
                if stop:
                    assert np.allclose(sol[k][2], nn, rtol=1e-6, atol=0)
            dx = rel(xs[k], x1)
            print('two processes: PCG stop', stop, 'iterations', len(rr) - 1, 'solution vs one GPU narrowed %.2e' % dx)
            assert dx < 1e-10, dx
    finally:
        B.close()


# ---------------------------------------------------------------------------
# 8. refusals: the reason named, the handle untouched (bitwise the same apply)
# ---------------------------------------------------------------------------
def refused(hs, r, storage, word):
    import torch
    M = _M()
    z0 = [z.clone() for z in vapply(None, hs, r)]
    for h in hs:
        with pytest.raises(M._lib.MamgError) as ei:
            h.set_cycle_storage(storage)
        assert ei.value.code == ERR_UNSUPPORTED and word in str(ei.value), str(ei.value)
    z1 = vapply(None, hs, r)
    for a, b in zip(z0, z1):
        assert torch.equal(a, b)


def test_refusals(lib_built):
    import dist_csr_ref as dc
    M = _M()
    s = system('b3')[0]
    r = rhs('b3', 1234)
    P = 2
    Ac, idofs, ckw, _ = dc.case('bidomain3d_poly3')
    big = sp.csr_matrix(s.scipy() * 1e40)

    def nodal(A=s, **kw):
        return [M.DistMetricAMG(A, s.W, idofs=s.idofs, rank=p, nranks=P, comm_id=None, rep_nodes=100, **kw)
                for p in range(P)]
    cases = [
        (lambda: [M.DistMetricAMG(Ac, None, idofs=idofs, rank=p, nranks=P, comm_id=None, rep_nodes=100, **ckw)
                  for p in range(P)], 'CSR'),
        (lambda: nodal(num_functions=2, smoother=11, Schwarz_type=7), 'SGS'),
        (lambda: nodal(parameters=M.parameters.parameters_metric_schwarz), 'SCHWARZ_PATCHES'),
        (lambda: nodal(A=big, num_functions=2), 'not representable'),
    ]
    for make, word in cases:
        hs = make()
        try:
            refused(hs, r, 'f32', word)
            for h in hs:
                for l in range(h.num_levels):
                    assert bits(h, l) == 0
                h.set_cycle_storage('f64')          # un-narrowed: MAMG_OK
        finally:
            close(hs)


def test_one_way_and_mixed_lists(lib_built):
    """F32 twice is a no-op; F64 after F32 is refused; a list whose handles
    disagree in storage is refused by the virtual entries before a kernel
    runs; NULL and unknown codes through ctypes."""
    import ctypes as C
    import torch
    M = _M()
    L = M._lib.lib()
    r = rhs('b3', 1234)
    hs = ranks('b3', {}, 2, 100, narrow=False)
    try:
        hs[0].set_cycle_storage('f32')
        rs = slices(hs, r)
        zs = [torch.full_like(x, 3.0) for x in rs]
        for call in (lambda: M.DistMetricAMG.virtual_apply(hs, rs, zs),
                     lambda: M.DistMetricAMG.virtual_apply(hs, rs, zs, graph=True),
                     lambda: M.DistMetricAMG.virtual_spmv(hs, rs, zs),
                     lambda: M.DistConjGrad.for_handles(list(hs), device=True, tolerance=1e-8, maxiter=5).solve(
                         [x.clone() for x in rs], zs)):
            with pytest.raises(M._lib.MamgError) as ei:
                call()
            assert ei.value.code == ERR_ARG and 'storage' in str(ei.value), str(ei.value)
        torch.cuda.synchronize()
        assert all(bool((z == 3.0).all()) for z in zs)       # nothing ran
        hs[1].set_cycle_storage('f32')
        check_report(hs)
        z0 = [z.clone() for z in vapply('b3', hs, r)]
        nbytes = [h.apply_bytes for h in hs]
        for h in hs:
            h.set_cycle_storage('f32')
        assert [h.apply_bytes for h in hs] == nbytes
        for a, b in zip(z0, vapply('b3', hs, r)):
            assert torch.equal(a, b)
        refused(hs, r, 'f64', 'one way')
        check_report(hs)
        assert L.mamg_dist_set_cycle_storage(hs[0]._h, 7) == ERR_ARG
        assert L.mamg_dist_set_cycle_storage(hs[0]._h, -1) == ERR_ARG
        assert L.mamg_dist_level_storage(hs[0]._h, 99) == ERR_ARG
        assert L.mamg_dist_level_storage(hs[0]._h, -1) == ERR_ARG
        check_report(hs)
    finally:
        close(hs)
    assert L.mamg_dist_set_cycle_storage(C.c_void_p(None), 1) == ERR_ARG
    assert L.mamg_dist_level_storage(C.c_void_p(None), 0) == ERR_ARG
