"""Matrix-free level-0 prolongation through the row dictionary of A (DESIGN.md
section 4.9): P e = (I - w D_B^-1 A)(T e) from the aggregate index and the
dictionary, no stored K or P.  The post step is then tgather_kernel (y = T e),
rowdict2_kernel's EPI_PSM pass (u = x1 + y - Wp (A y), Wp = w D_B^-1 per row
type) and the plain block-Jacobi sweeps.

The result is not bitwise the stored-K path's (the stored P sums A's entries
per aggregate before it multiplies e); tests/test_post_mf_identity.py bounds
that difference on the CPU, and here the GPU's own matrix-free-vs-K difference
is held to ten times the CPU restatement's for the same case.

Grids (tests/rowdict_cases.py): 3-D n = 6 (343 rows: two workgroups and a
23-lane tail wave, 98 isolated Dirichlet nodes), 3-D n = 10 (1331 rows,
aggregates that straddle workgroups), 2-D n = 32, and 2-D n = 128 (16641
rows: the smallest grid here where whole 64-row runs of interior rows share
one type, so the wave-uniform scalar path runs on nonzero y).

Every case sets the dictionary's and the post step's row thresholds to 1 and
MAMG_SELL_MIN_ROWS=1."""
import dataclasses
import functools

import numpy as np
import pytest

import kcycle_ref
import mamg_oracle as mo
import post_mf_ref as pm
import rowdict_cases as rc
from conftest import set_opt
from cycle_storage_ref import BIT_A, BIT_KP, BIT_R, StorageRef
from test_gpu import APPLY_TOL, rel

pytestmark = pytest.mark.gpu

SEEDS = (1234, 7)
GRIDS = {'grid3d-6': (3, 6), 'grid3d-10': (3, 10), 'grid2d-32': (2, 32), 'grid2d-128': (2, 128)}
AMLI_DEGREE = 2
FAMILIES = {
    'default': dict(),
    'poly': dict(smoother='POLY'),
    'sweeps2-maxit2': dict(presmooth_iter=2, postsmooth_iter=2, maxit=2),
    'wcycle': dict(cycle_type='W'),
    'kcycle': dict(cycle_type='K'),
    'coarse-scaling': dict(coarse_scaling=1),
    # the smoother's W = (relaxation / rho) D^-1 and the prolongator's w D_B^-1 differ: catches a Wp taken from W
    'omega1-relax1.2': dict(sa_omega=1.0, relaxation=1.2),
}
SETUP_KEYS = ('smoother', 'sa_omega', 'relaxation', 'AMG_type')   # the others are read by the apply only
SMOOTHERS = {'JACOBI_RHO': 3, 'SGS': 11, 'POLY': 12}


def _mamg():
    import metric_amg_examples_amd as M
    return M


@pytest.fixture(autouse=True)
def _reset_hooks():
    yield
    L = _mamg()._lib
    L.set_rowdict(-1, -1, -1)
    L.set_post_mf(-1, -1)


def to_c(kw):
    c = dict(kw)
    if 'smoother' in c:
        c['smoother'] = SMOOTHERS[c['smoother']]
        if kw['smoother'] == 'SGS':
            c['Schwarz_type'] = 7        # the level-0 seed blocks take the level smoother
    if 'AMG_type' in c:
        c['AMG_type'] = {'SA': 2, 'UA': 1}[c['AMG_type']]
    if 'cycle_type' in c:
        c['cycle_type'] = {'V': 1, 'W': 2, 'K': 4}[c['cycle_type']]
        if kw['cycle_type'] == 'K':
            c['amli_degree'] = AMLI_DEGREE
    return c


def build(system, mf=(1, 1), setup='gpu', **kw):
    """A handle with the dictionary's threshold at 1; mf: mamg_test_set_post_mf's
    (mode, min_rows): (1, 1) takes the matrix-free post step wherever it is
    eligible, (0, -1) never (the stored K), (-1, -1) the defaults."""
    M = _mamg()
    set_opt('MAMG_SELL_MIN_ROWS', '1')
    M._lib.set_rowdict(1, -1, -1)
    M._lib.set_post_mf(*mf)
    A, nv, idofs = system
    B = M.MetricAMG(A, [nv, nv], idofs=idofs, num_functions=2, setup=setup, **to_c(kw))
    assert B.layout == 'bsr2' and B.setup_path == setup
    return B


def taken(B):
    f, info = B.level_format(0), B.post_mf_info()
    assert f['post_mf'] and f['rowdict'] and not f['post_fused'] and not f['post_k'] and not f['post_sell'], f
    assert info['taken'] and info['reason'] is None, info
    assert 0 < info['table_bytes'] <= 32 * 256
    for l in range(1, B.num_levels):
        assert not B.level_format(l)['post_mf']
    return info


def stored_k(B, reason='off'):
    f, info = B.level_format(0), B.post_mf_info()
    assert not f['post_mf'] and not info['taken'] and info['reason'] == reason, (f, info)
    return f


def applies(B, A):
    return [B * mo.seeded_rhs(A.shape[0], s) for s in SEEDS]


def results(B, A):
    """B r for both seeds and the device PCG's solution and residual history."""
    M = _mamg()
    out = applies(B, A)
    solver = M.ConjGrad(A, precond=B, tolerance=1e-8, maxiter=500)
    x = solver * mo.seeded_rhs(A.shape[0], SEEDS[0])
    return out + [x, np.array(solver.residuals)]


def same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


# ---------------------------------------------------------------------------
# CPU references, computed once per (grid, family) and left unchanged
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def oracle_setup(name, items):
    A, nv, idofs = rc.grid(*GRIDS[name])
    return mo.setup(A, mo.Params(num_functions=2, **dict(items)), idofs=idofs)


def oracle(name, family, matrix_free=False):
    """The oracle's cycle of a family (the K-cycle: its restatement,
    tests/kcycle_ref.py), with the stored P or the matrix-free one."""
    kw = dict(FAMILIES[family])
    h = oracle_setup(name, tuple(sorted((k, kw.pop(k)) for k in SETUP_KEYS if k in kw)))
    k = kw.get('cycle_type') == 'K'
    if k:
        del kw['cycle_type']
    h = mo.Hierarchy(h.levels, dataclasses.replace(h.params, **kw))
    if matrix_free:
        h = pm.matrix_free(h)
    return kcycle_ref.KCycle(h, AMLI_DEGREE) if k else h


@functools.lru_cache(maxsize=None)
def reference(name, family):
    """{seed: (oracle's B r, the CPU restatement's own difference d to it)}"""
    h, hm = oracle(name, family), oracle(name, family, True)
    out = {}
    for seed in SEEDS:
        r = mo.seeded_rhs(rc.grid(*GRIDS[name])[0].shape[0], seed)
        z = h.apply(r)
        z.setflags(write=False)
        out[seed] = (z, rel(hm.apply(r), z))
    return out


@functools.lru_cache(maxsize=None)
def reference_pcg(name, family):
    A = rc.grid(*GRIDS[name])[0]
    ref = mo.pcg(A, oracle(name, family), mo.seeded_rhs(A.shape[0], SEEDS[0]), 1e-8, 500)
    res = np.array(ref.residuals)
    res.setflags(write=False)
    return res


# ---------------------------------------------------------------------------
# taken and right
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('family', list(FAMILIES))
@pytest.mark.parametrize('name', list(GRIDS))
def test_taken_matches_oracle(lib_built, name, family):
    system = rc.grid(*GRIDS[name])
    A = system[0]
    B = build(system, **FAMILIES[family])
    taken(B)
    got = results(B, A)
    B.close()
    ref = reference(name, family)
    for seed, z in zip(SEEDS, got):
        e = rel(z, ref[seed][0])
        print('%s %s seed %d: vs oracle %.2e' % (name, family, seed, e))
        assert e < APPLY_TOL, e
    res, cres = got[3], reference_pcg(name, family)
    print('%s %s: PCG iterations %d (oracle %d)' % (name, family, len(res) - 1, len(cres) - 1))
    assert len(res) == len(cres)
    assert np.allclose(res, cres, rtol=1e-6, atol=0)


@pytest.mark.parametrize('family', list(FAMILIES))
@pytest.mark.parametrize('name', list(GRIDS))
def test_against_the_stored_k_of_the_same_build(lib_built, name, family):
    """The matrix-free handle against the stored-K handle (hook mode 0): at
    most ten times the difference d the CPU restatement of the same case has
    to the oracle (the factor is for the kernels' different summation order),
    and never above APPLY_TOL."""
    system = rc.grid(*GRIDS[name])
    A = system[0]
    B = build(system, **FAMILIES[family])
    taken(B)
    got = applies(B, A)
    B.close()
    Bk = build(system, mf=(0, -1), **FAMILIES[family])
    f = stored_k(Bk)
    assert f['rowdict'] and f['post_fused'] and f['post_k'], f
    want = applies(Bk, A)
    Bk.close()
    ref = reference(name, family)
    for seed, z, zk in zip(SEEDS, got, want):
        g, d = rel(z, zk), ref[seed][1]
        print('%s %s seed %d: matrix-free vs K %.2e, CPU restatement vs oracle d = %.2e' % (name, family, seed, g, d))
        assert g <= 10 * d, (g, d)
        assert g <= APPLY_TOL


# ---------------------------------------------------------------------------
# same ops, same bits
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['grid3d-6', 'grid2d-128'])
def test_host_setup_equals_gpu_setup(lib_built, name):
    system = rc.grid(*GRIDS[name])
    A = system[0]
    Bg = build(system, setup='gpu')
    Bh = build(system, setup='host')
    assert taken(Bg) == taken(Bh)
    for l in range(Bg.num_levels):
        assert Bg.level_format(l) == Bh.level_format(l)
    assert same(results(Bg, A), results(Bh, A))
    Bg.close()
    Bh.close()


@pytest.mark.parametrize('name', ['grid3d-10', 'grid2d-128'])
def test_poison_graph_and_user_stream(lib_built, name):
    """MAMG_POISON=1 (every double array starts as NaN bytes), graph replay
    against the eager op list, and a caller-created stream against the default."""
    import torch
    set_opt('MAMG_POISON', '1')
    system = rc.grid(*GRIDS[name])
    A = system[0]
    B = build(system)
    taken(B)
    r = mo.seeded_rhs(A.shape[0], 7)
    ref = B * r
    assert np.all(np.isfinite(ref))
    rt = torch.as_tensor(r).cuda()
    zg, ze, zs = torch.zeros_like(rt), torch.zeros_like(rt), torch.zeros_like(rt)
    B.apply_device(rt, zg)                     # captured graph
    B.apply_device(rt, zg)                     # its replay
    B.time_apply(rt, ze, 1, mode=1)            # eager, op by op
    s1 = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s1):
        B.apply_device(rt, zs, s1)
    s1.synchronize()
    torch.cuda.synchronize()
    assert np.array_equal(zg.cpu().numpy(), ref)
    assert np.array_equal(ze.cpu().numpy(), ref)
    assert np.array_equal(zs.cpu().numpy(), ref)
    B.close()


# ---------------------------------------------------------------------------
# symmetry
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('family', ['default', 'poly', 'sweeps2-maxit2'])
@pytest.mark.parametrize('name', list(GRIDS))
def test_symmetric(lib_built, name, family):
    system = rc.grid(*GRIDS[name])
    A = system[0]
    B = build(system, **FAMILIES[family])
    taken(B)
    r1, r2 = (mo.seeded_rhs(A.shape[0], s) for s in SEEDS)
    a, b = float(np.dot(r2, B * r1)), float(np.dot(r1, B * r2))
    B.close()
    assert abs(a - b) <= 1e-9 * (abs(a) + abs(b)), (a, b)


# ---------------------------------------------------------------------------
# fp32 cycle storage
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('family', ['default', 'poly'])
@pytest.mark.parametrize('name', ['grid3d-10', 'grid2d-128'])
def test_fp32_cycle_storage(lib_built, name, family):
    """A narrowed matrix-free handle reads A's fp32 table in both dictionary
    passes; Wp = w D_B^-1 stays fp64 (it is built from the fp64 table).  The
    reference is tests/test_gpu_cycle_storage.py's: the numpy restatement under
    the masks the handle reports, with level 0's P the matrix-free map over the
    rounded A, at that file's bound for level-0 narrowing, APPLY_TOL."""
    system = rc.grid(*GRIDS[name])
    A = system[0]
    B = build(system, **FAMILIES[family])
    taken(B)
    b64 = B.apply_bytes
    B.set_cycle_storage('f32')
    taken(B)
    n = B.num_levels
    s0 = B.level_storage(0)
    assert s0['A'] and s0['KP'] and s0['R'], s0        # K / P: nothing left to narrow, reported as requested
    assert B.apply_bytes < b64
    masks = []
    for l in range(n):
        s = B.level_storage(l)
        masks.append((BIT_A if s['A'] else 0) | (BIT_KP if s['KP'] else 0) | (BIT_R if s['R'] else 0))
    kform = [bool(B.level_format(l)['post_fused']) for l in range(n)]
    assert not kform[0]
    h = oracle(name, family)
    ref = StorageRef(h, masks=masks, kform=kform)
    ref.P[0] = pm.MatrixFreeP(h.levels[0], ref.A[0])
    ref64 = StorageRef(h, masks=0, kform=kform)
    ref64.P[0] = pm.MatrixFreeP(h.levels[0])
    for seed in SEEDS:
        r = mo.seeded_rhs(A.shape[0], seed)
        z = B * r
        e, d = rel(z, ref.apply(r)), rel(z, ref64.apply(r))
        print('%s %s seed %d: vs rounded restatement %.2e, vs unrounded %.2e' % (name, family, seed, e, d))
        assert e < APPLY_TOL, e
        assert d > APPLY_TOL, d
    B.close()


# ---------------------------------------------------------------------------
# refused means untouched
# ---------------------------------------------------------------------------
REFUSALS = {
    'threshold': (lambda: rc.grid(3, 10), dict(), (-1, -1), 'threshold'),
    'sgs': (lambda: rc.grid(3, 10), dict(smoother='SGS'), (1, 1), 'smoother'),
    'ua': (lambda: rc.grid(3, 10), dict(AMG_type='UA'), (1, 1), 'not SA'),
    'unfused': (lambda: rc.grid(3, 10), dict(post_fusion=0), (1, 1), 'no fusion'),
    'no-dictionary': (rc.REFUSED['permuted2d-32'], dict(), (1, 1), 'no dictionary'),
}


@pytest.mark.parametrize('case', list(REFUSALS))
def test_refused_means_untouched(lib_built, case):
    gen, kw, mf, reason = REFUSALS[case]
    system = gen()
    A = system[0]
    B = build(system, mf=mf, **kw)
    f = stored_k(B, reason)
    assert B.post_mf_info()['table_bytes'] == 0
    assert f['rowdict'] == (case != 'no-dictionary'), f
    got = results(B, A)
    B.close()
    B0 = build(system, mf=(0, -1), **kw)
    assert stored_k(B0) == f
    assert same(got, results(B0, A))
    B0.close()
