"""Row-pattern dictionary of a level-0 A: one 16-bit
row-type code per node row plus a table of the distinct rows, read by
rowdict2_kernel.  The layout is exact, so wherever it is taken the apply and
the device PCG are bitwise those of the half-symmetric and SELL-64 layouts,
and wherever it is refused the handle is exactly the one built without the
attempt.  Inputs are the smallest that reach each path (3-D n = 6: 343 rows,
two workgroups and a 23-lane tail wave; n = 10: 1331 = 5 * 256 + 51; 2-D
n = 32: 1089); tests/test_rowdict_cases.py pins their row-type counts.

Every case sets the hook's row threshold to 1 and MAMG_SELL_MIN_ROWS=1."""
import functools

import numpy as np
import pytest

import mamg_oracle as mo
import rowdict_cases as rc
from conftest import set_opt
from test_gpu import APPLY_TOL, oracle_kw, rel, to_c

pytestmark = pytest.mark.gpu

SEEDS = (1234, 7)
GRIDS = {'grid3d-6': (3, 6, 28), 'grid3d-10': (3, 10, 28), 'grid2d-32': (2, 32, 10)}
FAMILIES = {
    'default': dict(),
    'poly': dict(smoother='POLY'),
    'sweeps2-maxit2': dict(presmooth_iter=2, postsmooth_iter=2, maxit=2),
    'unfused': dict(post_fusion=0),
}


def _mamg():
    import metric_amg_examples_amd as M
    return M


@pytest.fixture(autouse=True)
def _reset_hook():
    yield
    _mamg()._lib.set_rowdict(-1, -1, -1)


def build(system, hook=(1, -1, -1), setup='gpu', **kw):
    """A handle under MAMG_SELL_MIN_ROWS=1; hook: mamg_test_set_rowdict's
    arguments, None for the defaults (the dictionary is then out of reach of
    these sizes)."""
    M = _mamg()
    set_opt('MAMG_SELL_MIN_ROWS', '1')
    M._lib.set_rowdict(*(hook or (-1, -1, -1)))
    A, nv, idofs = system
    B = M.MetricAMG(A, [nv, nv], idofs=idofs, num_functions=2, setup=setup, **to_c(kw))
    assert B.layout == 'bsr2' and B.setup_path == setup
    return B


def results(B, A, pcg=True):
    """B r for both seeds and the device PCG's residual history."""
    M = _mamg()
    out = [B * mo.seeded_rhs(A.shape[0], s) for s in SEEDS]
    if pcg:
        solver = M.ConjGrad(A, precond=B, tolerance=1e-8, maxiter=200)   # EPI_Y on A_0, field-major x
        x = solver * mo.seeded_rhs(A.shape[0], SEEDS[0])
        out += [x, np.array(solver.residuals)]
    return out


def same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


@functools.lru_cache(maxsize=None)
def oracle(name, smoother):
    A, nv, idofs = rc.grid(*GRIDS[name][:2])
    return mo.setup(A, mo.Params(num_functions=2, smoother=smoother), idofs=idofs)


def oracle_apply(name, kw, r):
    import dataclasses
    kw = oracle_kw(kw)
    h = oracle(name, kw.pop('smoother', 'JACOBI_RHO'))
    return mo.Hierarchy(h.levels, dataclasses.replace(h.params, **kw)).apply(r)


def taken(B, types=None):
    f, info = B.level_format(0), B.rowdict_info()
    assert f['rowdict'] and not f['half'] and not f['sell'], f
    assert info['taken'] and info['reason'] is None, info
    if types is not None:
        assert info['types'] == types, info
    assert 0 < info['table_bytes'] <= 64 << 10
    return info


# ---------------------------------------------------------------------------
# taken: exact
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('family', list(FAMILIES))
@pytest.mark.parametrize('name', list(GRIDS))
def test_taken_bitwise_half_and_sell(lib_built, name, family):
    dim, n, types = GRIDS[name]
    kw = FAMILIES[family]
    system = rc.grid(dim, n)
    A = system[0]
    B = build(system, **kw)
    info = taken(B, types)
    assert info['maxlen'] == (15 if dim == 3 else 7)
    got = results(B, A)
    B.close()
    Bh = build(system, hook=None, **kw)                 # half-symmetric ELL-64
    fh = Bh.level_format(0)
    assert fh['half'] and not fh['rowdict'] and Bh.rowdict_info()['reason'] == 'threshold'
    half = results(Bh, A)
    Bh.close()
    set_opt('MAMG_HALF', '0')
    Bs = build(system, hook=None, **kw)                 # SELL-64
    fs = Bs.level_format(0)
    assert fs['sell'] and not fs['half'] and not fs['rowdict']
    sell = results(Bs, A)
    Bs.close()
    assert same(got, half), [int(np.sum(x != y)) for x, y in zip(got, half)]
    assert same(got, sell)
    for seed, z in zip(SEEDS, got):
        assert rel(z, oracle_apply(name, kw, mo.seeded_rhs(A.shape[0], seed))) < APPLY_TOL


def test_type_cap_boundary(lib_built):
    system = rc.grid(3, 6)
    A = system[0]
    B = build(system, hook=(1, 28, -1))
    taken(B, 28)
    got = results(B, A)
    B.close()
    B = build(system, hook=(1, 27, -1))
    f, info = B.level_format(0), B.rowdict_info()
    assert not info['taken'] and info['reason'] == 'types', info
    assert f['half'] and not f['rowdict'], f
    assert same(got, results(B, A))
    B.close()


# ---------------------------------------------------------------------------
# perturbed values
# ---------------------------------------------------------------------------
def test_perturbed_with_mirror_still_taken(lib_built):
    """One interior block and its mirror scaled by 1 + 2^-40: two more row
    types (tests/test_rowdict_cases.py), still exact."""
    system = rc.perturbed(6, True)
    A = system[0]
    B = build(system)
    taken(B, 30)
    got = results(B, A)
    B.close()
    Bh = build(system, hook=None)
    assert Bh.level_format(0)['half']
    assert same(got, results(Bh, A))
    Bh.close()


def test_perturbed_without_mirror_matches_sell(lib_built):
    """The same edit on one side only: A_IJ != A_JI, the half layout is
    refused; the dictionary needs no symmetry and equals SELL-64 bitwise."""
    system = rc.perturbed(6, False)
    A = system[0]
    B = build(system)
    taken(B, 29)
    got = results(B, A, pcg=False)
    B.close()
    Bs = build(system, hook=None)
    fs = Bs.level_format(0)
    assert fs['sell'] and not fs['half'], fs
    assert same(got, results(Bs, A, pcg=False))
    Bs.close()


# ---------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('name,reason', [('permuted2d-32', 'types'), ('ragged96', 'types'), ('hub32-m500', 'length')])
def test_refused_inputs_unchanged(lib_built, name, reason):
    system = rc.REFUSED[name]()
    A = system[0]
    B = build(system)
    f, info = B.level_format(0), B.rowdict_info()
    assert not f['rowdict'] and not info['taken'] and info['reason'] == reason, (f, info)
    got = results(B, A, pcg=False)
    B.close()
    B0 = build(system, hook=None)
    assert B0.level_format(0) == f
    assert same(got, results(B0, A, pcg=False))
    B0.close()


def test_hash_collisions_refused_or_exact(lib_built):
    """Two bits of hash: 28 row types share at most 4 keys.  The verification
    pass must refuse the layout (or, were the keys to separate the types, the
    layout is exact): the bits are the half layout's either way."""
    system = rc.grid(3, 6)
    A = system[0]
    B = build(system, hook=(1, -1, 2))
    f, info = B.level_format(0), B.rowdict_info()
    if info['taken']:
        assert f['rowdict']
    else:
        assert info['reason'] == 'verification' and f['half'] and not f['rowdict'], (f, info)
    got = results(B, A)
    B.close()
    Bh = build(system, hook=None)
    assert same(got, results(Bh, A))
    Bh.close()


# ---------------------------------------------------------------------------
# other paths
# ---------------------------------------------------------------------------
def test_poison_graph_and_user_stream(lib_built):
    """MAMG_POISON=1 (every double array starts as NaN bytes: the padding of
    the type table is written), graph replay against the eager op list, and a
    user-created stream."""
    import torch
    set_opt('MAMG_POISON', '1')
    system = rc.grid(3, 10)
    A = system[0]
    B = build(system)
    taken(B, 28)
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
    set_opt('MAMG_POISON', '0')
    Bh = build(system, hook=None)
    assert np.array_equal(Bh * r, ref)
    Bh.close()


def test_fp32_cycle_storage(lib_built):
    """Ac copies the layout and narrows the block table: bit 1 of the level's
    storage, the half layout's bits under the same storage, and the rounding
    is really there (>= 1e-8 from the fp64 apply)."""
    system = rc.grid(3, 10)
    A = system[0]
    r = mo.seeded_rhs(A.shape[0], 1234)
    B = build(system)
    taken(B, 28)
    z64 = B * r
    b64 = B.apply_bytes
    B.set_cycle_storage('f32')
    assert B.level_storage(0)['A'] and B.level_format(0)['rowdict']
    assert B.apply_bytes < b64
    z32 = B * r
    # the Krylov operator stays fp64: the device PCG still converges to 1e-8
    M = _mamg()
    solver = M.ConjGrad(A, precond=B, tolerance=1e-8, maxiter=200)
    x = solver * r
    assert rel(A @ x, r) < 1e-6
    B.close()
    Bh = build(system, hook=None)
    Bh.set_cycle_storage('f32')
    assert Bh.level_format(0)['half'] and Bh.level_storage(0)['A']
    assert np.array_equal(z32, Bh * r)
    Bh.close()
    assert rel(z32, z64) >= 1e-8


def test_host_setup_equals_gpu_setup(lib_built):
    system = rc.grid(3, 6)
    A = system[0]
    Bg = build(system, setup='gpu')
    Bh = build(system, setup='host')
    taken(Bg, 28)
    taken(Bh, 28)
    for l in range(Bg.num_levels):
        assert Bg.level_format(l) == Bh.level_format(l)
    assert Bg.rowdict_info() == Bh.rowdict_info()
    assert same(results(Bg, A), results(Bh, A))
    Bg.close()
    Bh.close()


def test_rank_local_a_keeps_half(lib_built):
    """Rank-local A's with ghost columns are out of the dictionary's scope."""
    M = _mamg()
    set_opt('MAMG_SELL_MIN_ROWS', '1')
    M._lib.set_rowdict(1, -1, -1)
    s = M.problems.bidomain(3, 8, 1e6)
    hs = [M.DistMetricAMG(s, s.W, idofs=s.idofs, rank=p, nranks=2, comm_id=None, rep_nodes=100, num_functions=2)
          for p in range(2)]
    try:
        for h in hs:
            f = h.level_format(0)
            assert f['half'] and not f['rowdict'], f
    finally:
        for h in hs:
            h.close()


def test_default_threshold_keeps_half(lib_built):
    system = rc.grid(3, 16)
    B = build(system, hook=None)
    f, info = B.level_format(0), B.rowdict_info()
    assert f['half'] and not f['rowdict'], f
    assert not info['taken'] and info['reason'] == 'threshold', info
    B.close()
