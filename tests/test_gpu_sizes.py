"""GPU parity at node counts on the kernels' size boundaries (tests/size_cases.py).

Every other -m gpu test runs (n + 1)^d node rows with an even n: an odd count
that is 1, 9, 17, 25, 33 or 49 mod 64.  The inputs here are principal
submatrices of the grid systems with m = 1 .. 4097 node rows, chosen around
the places where the kernels take their index decisions: fewer rows than the
8 XCDs, than a wavefront's share of a SELL slice (32) or than a slice (64);
m = 0, 1, 63 mod 64; multiples of the 128 rows a workgroup of
msell_kernel<LPR = 2> covers and of 256; even m (the second field of [u1; u2]
then starts 16-byte aligned); scalar levels of 4096 / 4097 rows (one-workgroup
point GS against colour-by-colour launches).  All hierarchies use
coarse_dof = 4, so even the tiny sizes keep a level 0 with K and a restriction.

  a  apply and device PCG against the oracle
  b  SpMV against the per-row rounding bound
  c  layout variants stay bitwise equal
  d  GPU setup = host setup bit for bit
  e  multicolour node-block SGS and the node-patch Schwarz
  f  fp32 cycle storage against its restatement
  g  scalar (CSR layout) hierarchies, point GS / SGS on both sides of 4096 rows
  h  row partition on virtual ranks

Modes (each id asserts through level_format that the branch was taken):
default = lane-group BSR2 kernels; sell = MAMG_SELL_MIN_ROWS=1 (half-symmetric
A_0, SELL P / R, two-lane SELL K with 16-bit columns and sorted slices);
sell-full = sell with MAMG_HALF=0 (sell2_kernel for A_0); msell =
MAMG_MSELL_MIN_ROWS=1 (multi-lane SELL on the coarse levels).

Tolerances are the project's own: APPLY_TOL = 1e-10, PCG histories at rtol
1e-6, 1e-12 against one GPU, 1e-10 against the fp32 restatement.  The
reference's sensitivity to summation order on these inputs is at most 1.2e-13
(tests/test_size_cases.py).
"""
import functools

import numpy as np
import pytest

import irregular
import mamg_oracle as mo
import pointgs_ref as pr
import size_cases as sc
from conftest import set_opt
from cycle_storage_ref import ALL, StorageRef
from test_gpu import APPLY_TOL, rel
from test_gpu_cycle_storage import bits
from test_gpu_irregular import to_c
from test_gpu_setup import hierarchies_equal

pytestmark = pytest.mark.gpu

ERR_UNSUPPORTED = -4
PATCHES = 6
CD = sc.COARSE_DOF

ORDERED = sc.nodal_cases(('slice', 'stencil3d', 'big32', 'big64', 'tiny'))     # the run order: SLICE first, TINY last
MID = sc.nodal_cases(('slice', 'stencil3d'))
VARIANT = [c for c in MID if c[1] in sc.VARIANT_SIZES]
SMOOTHER = [c for c in MID if c[1] in sc.SMOOTHER_SIZES]
ids = lambda cases: [sc.case_id(c) for c in cases]       # noqa: E731


def _mamg():
    import metric_amg_examples_amd as M
    return M


def set_mode(mode):
    if mode in ('sell', 'sell-full'):
        set_opt('MAMG_SELL_MIN_ROWS', '1')
    if mode == 'sell-full':
        set_opt('MAMG_HALF', '0')
    if mode == 'msell':
        set_opt('MAMG_MSELL_MIN_ROWS', '1')


def check_mode(B, mode, jacobi=True):
    """The layout branch the mode names was really taken.  jacobi: the cycle
    has the fused K post operator (Jacobi family), so its layout is checked too."""
    if B.num_levels == 1:
        return                      # m = 1, 2: one dense level, no level-0 operator
    f = B.level_format(0)
    if mode == 'sell':
        assert f['half'] and f['sym'] and not f['sell'], f
        if jacobi:
            assert f['post_k'] and f['post_sell'] and f['k_col16'], f
    elif mode == 'sell-full':
        assert f['sell'] and f['sym'] and not f['half'], f
        if jacobi:
            assert f['post_k'] and f['post_sell'], f
    else:
        assert not f['sell'] and not f['half'] and not f['post_sell'], f
        if mode == 'msell':
            assert B.num_levels >= 3 and B.level_format(1)['sell'], B.level_format(1)


def build(family, m, mode, setup, **kw):
    """MetricAMG of a nodal case; kw in the oracle's spelling."""
    M = _mamg()
    set_mode(mode)
    A, nv, idofs = sc.nodal(family, m)
    B = M.MetricAMG(A, [nv, nv], idofs=idofs, num_functions=2, coarse_dof=CD, setup=setup, **to_c(kw))
    assert B.layout == 'bsr2' and B.setup_path == setup, (B.layout, B.setup_path)
    return B


def rhs(family, m, seed=1234):
    return mo.seeded_rhs(2 * m, seed)


def device_apply(B, r):
    import torch
    z = B.matvec(torch.as_tensor(r).cuda())
    torch.cuda.synchronize()
    return z.cpu().numpy()


def device_pcg(B, A, b):
    solver = _mamg().ConjGrad(A, precond=B, tolerance=1e-8, maxiter=500, device=True)
    x = solver * b
    return np.asarray(solver.residuals), (x.cpu().numpy() if hasattr(x, 'cpu') else np.asarray(x))


def assert_history(res, ref):
    """Same length, every entry within rtol 1e-6 -- except that an entry below
    1e-12 residuals[0] is the rounding noise of a direct solve (the one-level
    and 6-dof hierarchies) and is compared only as being below that bound on
    both sides.  At most the last entry of a history may be such noise, so the
    exemption cannot hide a diverging solve."""
    res, ref = np.asarray(res), np.asarray(ref)
    assert len(res) == len(ref), (len(res), len(ref))
    floor = 1e-12 * ref[0]
    noise = (res < floor) | (ref < floor)
    assert not noise[:-1].any(), np.flatnonzero(noise)
    assert np.all(res[noise] < floor) and np.all(ref[noise] < floor), (res[-1], ref[-1], floor)
    assert np.allclose(res[~noise], ref[~noise], rtol=1e-6, atol=0), np.abs(res - ref) / ref


# ---------------------------------------------------------------------------
# the reference side, computed once per session and never modified
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def oracle_applies(family, m, cycle='V', smoother='JACOBI_RHO', kw=()):
    h = sc.oracle(family, m, cycle, smoother, **dict(kw))
    return {seed: h.apply(rhs(family, m, seed)) for seed in sc.SEEDS}


@functools.lru_cache(maxsize=None)
def oracle_pcg(family, m, cycle='V', smoother='JACOBI_RHO'):
    A = sc.nodal(family, m)[0]
    return mo.pcg(A, sc.oracle(family, m, cycle, smoother), rhs(family, m), 1e-8, 500)


# ---------------------------------------------------------------------------
# a. apply and device PCG against the oracle
# ---------------------------------------------------------------------------
PART_A = [(f, m, mode) for mode in ('default', 'sell') for f, m in ORDERED] + \
         [(f, m, mode) for mode in ('sell-full', 'msell') for f, m in MID]


@pytest.mark.parametrize('family,m,mode', PART_A, ids=['%s-%d-%s' % c for c in PART_A])
def test_apply_and_pcg_match_oracle(lib_built, family, m, mode):
    """Host and GPU setup; host-pointer and device-pointer applies for seeds
    1234 and 7 against the oracle to APPLY_TOL; device PCG (1e-8, 500) with the
    oracle's iteration count and residual history.  V + JACOBI_RHO everywhere,
    W and POLY on 63 / 64 / 65, 255 / 256 / 257 and 511 / 512 / 513.  m = 1, 2:
    one dense level, compared with np.linalg.solve as well."""
    A = sc.nodal(family, m)[0]
    combos = [('V', 'JACOBI_RHO')]
    if m in sc.WP_SIZES:
        combos += [('W', 'JACOBI_RHO'), ('V', 'POLY'), ('W', 'POLY')]
    worst = 0.0
    for cycle, smoother in combos:
        zo = oracle_applies(family, m, cycle, smoother)
        ref = oracle_pcg(family, m, cycle, smoother)
        for setup in ('host', 'gpu'):
            B = build(family, m, mode, setup, cycle_type=cycle, smoother=smoother)
            try:
                check_mode(B, mode)
                assert B.num_levels == len(sc.HIER[(family, m)])
                for seed, z_ref in zo.items():
                    r = rhs(family, m, seed)
                    z1, z2 = B * r, device_apply(B, r)
                    e1, e2 = rel(z1, z_ref), rel(z2, z_ref)
                    worst = max(worst, e1, e2)
                    assert e1 < APPLY_TOL and e2 < APPLY_TOL, (cycle, smoother, setup, seed, e1, e2)
                    if B.num_levels == 1:
                        assert rel(z1, np.linalg.solve(A.toarray(), r)) < 1e-12
                res, x = device_pcg(B, A, rhs(family, m))
                assert_history(res, ref.residuals)
                assert rel(x, ref.x) < 1e-6
            finally:
                B.close()
    print('part a', family, m, mode, 'worst apply err %.2e' % worst, 'pcg iters', ref.niters)


# ---------------------------------------------------------------------------
# b. SpMV against the rounding bound of each row
# ---------------------------------------------------------------------------
PART_B = [(f, m, mode) for mode in ('default', 'sell', 'sell-full') for f, m in ORDERED]


@pytest.mark.parametrize('family,m,mode', PART_B, ids=['%s-%d-%s' % c for c in PART_B])
def test_spmv_within_row_bound(lib_built, family, m, mode):
    """spmv_device against A x accumulated in long double, row by row:
    |y_i - ref_i| <= (len_i + 2) 2^-53 sum_j |a_ij x_j|, the bound of any
    summation order of len_i products."""
    import torch
    A = sc.nodal(family, m)[0]
    B = build(family, m, mode, 'host')
    try:
        check_mode(B, mode)
        x = np.random.default_rng(3).standard_normal(A.shape[0])
        y = torch.full((A.shape[0],), float('nan'), dtype=torch.float64, device='cuda')
        B.spmv_device(torch.as_tensor(x).cuda(), y)
        torch.cuda.synchronize()
        y = y.cpu().numpy()
    finally:
        B.close()
    prod = A.data.astype(np.longdouble) * x[A.indices].astype(np.longdouble)
    ref = np.add.reduceat(prod, A.indptr[:-1])
    mag = np.add.reduceat(np.abs(prod), A.indptr[:-1])
    ln = np.diff(A.indptr)
    assert ln.min() >= 1
    bound = (ln + 2) * np.longdouble(2.0) ** -53 * mag
    err = np.abs(y.astype(np.longdouble) - ref)
    assert np.isfinite(y).all()
    worst = int(np.argmax(err / bound))
    print('part b', family, m, mode, 'worst err / bound %.3f at row %d' % (float(err[worst] / bound[worst]), worst))
    assert np.all(err <= bound), (worst, float(err[worst]), float(bound[worst]))


# ---------------------------------------------------------------------------
# c. layout variants stay bitwise equal at the boundaries
# ---------------------------------------------------------------------------
def run_variant(family, m, mode, opt, values, check=None):
    """One handle per value of opt (GPU setup): host-pointer applies of both
    seeds and the device PCG history.  Returns them per value."""
    A = sc.nodal(family, m)[0]
    out = []
    for v in values:
        set_opt(opt, v)
        B = build(family, m, mode, 'gpu')
        try:
            if check:
                check(B.level_format(0), v)
            zs = [B * rhs(family, m, seed) for seed in sc.SEEDS]
            res, _ = device_pcg(B, A, rhs(family, m))
            out.append((zs, list(res)))
        finally:
            B.close()
    zo = oracle_applies(family, m)
    ref = oracle_pcg(family, m)
    for zs, res in out:
        for seed, z in zip(sc.SEEDS, zs):
            assert rel(z, zo[seed]) < APPLY_TOL
        assert_history(res, ref.residuals)
    return out


def assert_bitwise(a, b):
    for x, y in zip(a[0], b[0]):
        assert np.array_equal(x, y), float(np.abs(x - y).max())
    assert a[1] == b[1]


@pytest.mark.parametrize('family,m', VARIANT, ids=ids(VARIANT))
def test_half_symmetric_equals_full_sell(lib_built, family, m):
    """MAMG_HALF 1 / 0: hsell2_kernel sums every row in sell2_kernel's order."""
    def check(f, v):
        assert f['sym'] and f['half'] == (v == '1') and f['sell'] == (v == '0'), f
    a, b = run_variant(family, m, 'sell', 'MAMG_HALF', ('1', '0'), check)
    assert_bitwise(a, b)


@pytest.mark.parametrize('family,m', VARIANT, ids=ids(VARIANT))
def test_k_col16_bitwise(lib_built, family, m):
    """MAMG_K_COL16 1 / 0: the per-slice column base, last slice partial or full."""
    def check(f, v):
        assert f['post_sell'] and f['k_col16'] == (v == '1'), f
    a, b = run_variant(family, m, 'sell', 'MAMG_K_COL16', ('1', '0'), check)
    assert_bitwise(a, b)


@pytest.mark.parametrize('family,m', VARIANT, ids=ids(VARIANT))
def test_k_sort_bitwise(lib_built, family, m):
    """MAMG_K_SORT 1 / 0: the in-slice row sort on a last slice of 63, 64 and 1 rows."""
    def check(f, v):
        assert f['post_sell'], f
    a, b = run_variant(family, m, 'sell', 'MAMG_K_SORT', ('1', '0'), check)
    assert_bitwise(a, b)


@pytest.mark.parametrize('mode', ['default', 'sell'])
@pytest.mark.parametrize('family,m', VARIANT, ids=ids(VARIANT))
def test_post_operator_variants(lib_built, family, m, mode):
    """MAMG_POST_K 1 (K = P - W A P), 0 (merged [P | AP]) and 2 (K as two
    16-byte streams): each is the oracle's z to APPLY_TOL (run_variant); K and
    the merged window agree to 1e-12 (test_post_operator_k_equals_merged's
    bound), the two K layouts are bitwise equal (test_k_block_layouts_bitwise)."""
    def check(f, v):
        assert f['post_fused'] and f['post_k'] == (v != '0'), f
        if v != '0':                # the merged window has its own storage; K is SELL-stored in sell mode
            assert f['post_sell'] == (mode == 'sell'), f
    k1, k0, k2 = run_variant(family, m, mode, 'MAMG_POST_K', ('1', '0', '2'), check)
    for x, y in zip(k1[0], k0[0]):
        assert rel(x, y) < 1e-12
    assert_bitwise(k1, k2)


@pytest.mark.parametrize('mode', ['default', 'sell'])
@pytest.mark.parametrize('family,m', VARIANT, ids=ids(VARIANT))
def test_fuse_rbd_bitwise(lib_built, family, m, mode):
    """MAMG_FUSE_RBD 2 / 1 / 0: the restriction's epilogue writing the next
    level's first sweep is bitwise the separate launch."""
    a, b, c = run_variant(family, m, mode, 'MAMG_FUSE_RBD', ('2', '1', '0'))
    assert_bitwise(a, b)
    assert_bitwise(a, c)


# ---------------------------------------------------------------------------
# d. GPU setup = host setup, bit for bit
# ---------------------------------------------------------------------------
# sizes the GPU setup refuses (MAMG_ERR_UNSUPPORTED): none; every size from one
# node up is accepted and must then give the host setup's hierarchy
GPU_SETUP_REFUSES = set()


def host_and_gpu_equal(family, m, kw):
    M = _mamg()
    A, nv, idofs = sc.nodal(family, m)
    ckw = to_c(dict(kw, num_functions=2, coarse_dof=CD))
    Hh = M.HostHierarchy(A, idofs=idofs, **ckw)
    try:
        assert Hh.num_levels == len(sc.level_dofs(sc.oracle(family, m, **kw)))
        if (family, m) in GPU_SETUP_REFUSES:
            with pytest.raises(M._lib.MamgError) as ei:
                M.HostHierarchy(A, idofs=idofs, gpu=True, **ckw)
            assert ei.value.code == ERR_UNSUPPORTED and len(str(ei.value)) > 20, str(ei.value)
            B = M.MetricAMG(A, [nv, nv], idofs=idofs, setup='auto', **ckw)
            try:
                assert B.setup_path.startswith('host (') and len(B.setup_path) > 20, B.setup_path
            finally:
                B.close()
            return
        Hg = M.HostHierarchy(A, idofs=idofs, gpu=True, **ckw)
        try:
            hierarchies_equal(Hh, Hg)
        finally:
            Hg.close()
    finally:
        Hh.close()


@pytest.mark.parametrize('family,m', ORDERED, ids=ids(ORDERED))
def test_gpu_setup_bitwise_equals_host(lib_built, family, m):
    """Default parameters at every size: the staged SpGEMM pass over node row
    pairs on even and odd node counts, MIS-2 and the CSR -> BSR2 waves on
    partial and full last waves."""
    host_and_gpu_equal(family, m, {})


@pytest.mark.parametrize('kw', irregular.PARAM_SETS[1:], ids=irregular.param_id)
@pytest.mark.parametrize('family,m', SMOOTHER, ids=ids(SMOOTHER))
def test_gpu_setup_parameter_sets(lib_built, family, m, kw):
    """HEM, UA and strong_coupled = 0.25 on 63 / 64 / 65 and 255 / 256 / 257."""
    host_and_gpu_equal(family, m, kw)


KNOBS = [dict(MAMG_SPGEMM_PAIR='0'), dict(MAMG_SPGEMM_STAGE_GB='0'), dict(MAMG_CSR2BSR_FILL='0'),
         dict(MAMG_MIS_STAGED='0')]
BOUNDARY_256 = [c for c in MID if c[1] in (255, 256, 257)]


@pytest.mark.parametrize('knobs', KNOBS, ids=lambda k: ','.join('%s=%s' % kv for kv in k.items()))
@pytest.mark.parametrize('family,m', BOUNDARY_256, ids=ids(BOUNDARY_256))
def test_gpu_setup_variants(lib_built, family, m, knobs):
    """The SpGEMM row by row and unstaged, the staged CSR -> BSR2 merge and the
    lane-per-row MIS-2 maxima on 255 / 256 / 257 node rows: the host setup's
    hierarchy bit for bit, and (the CSR -> BSR2 fill shapes the handle's
    layouts, not the exported hierarchy) the default's applies bit for bit."""
    base = build(family, m, 'default', 'gpu')
    try:
        z0 = [base * rhs(family, m, seed) for seed in sc.SEEDS]
    finally:
        base.close()
    for k, v in knobs.items():
        set_opt(k, v)
    host_and_gpu_equal(family, m, {})
    B = build(family, m, 'default', 'gpu')
    try:
        for seed, z in zip(sc.SEEDS, z0):
            assert np.array_equal(B * rhs(family, m, seed), z)
    finally:
        B.close()


# ---------------------------------------------------------------------------
# e. other smoothers with their own launch geometry
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('mode', ['default', 'sell'])
@pytest.mark.parametrize('family,m', SMOOTHER, ids=ids(SMOOTHER))
def test_node_block_sgs(lib_built, family, m, mode):
    """Multicolour node-block SGS (smoother 11; the level-0 seed blocks take
    the level smoother) against the oracle, host and GPU setup."""
    zo = oracle_applies(family, m, 'V', 'SGS')
    worst = 0.0
    for setup in ('host', 'gpu'):
        set_mode(mode)
        A, nv, idofs = sc.nodal(family, m)
        B = _mamg().MetricAMG(A, [nv, nv], idofs=idofs, num_functions=2, coarse_dof=CD, setup=setup,
                              smoother=11, Schwarz_type=7)
        try:
            assert B.setup_path == setup and B.level_format(0)['gs']
            check_mode(B, mode, jacobi=False)
            for seed, z_ref in zo.items():
                r = rhs(family, m, seed)
                e1, e2 = rel(B * r, z_ref), rel(device_apply(B, r), z_ref)
                worst = max(worst, e1, e2)
                assert e1 < APPLY_TOL and e2 < APPLY_TOL, (setup, seed, e1, e2)
        finally:
            B.close()
    print('part e sgs', family, m, mode, 'worst %.2e' % worst)


@pytest.mark.parametrize('mode', ['default', 'sell'])
@pytest.mark.parametrize('family,m', SMOOTHER, ids=ids(SMOOTHER))
def test_node_patches(lib_built, family, m, mode):
    """Node-patch Schwarz with MAMG_PATCH_INV 1, 2 (scalar Gauss-Jordan, one
    and two patches per wave) and 3 (matrix-core block sweep): m patches, 0 / 1
    / 7 mod 8 and 0 / 1 / 3 mod 4.  Each against the oracle to 1e-10
    (test_patch_apply_matches_oracle's bound); 1 and 2 bitwise equal in the
    applies and the device PCG history, 2 and 3 to 1e-10 with the same
    iteration count and the history to 1e-6 (test_patch_inverse_kernels_bitwise,
    test_patch_inverse_matrix_cores)."""
    zo = oracle_applies(family, m, 'V', 'JACOBI_RHO', (('Schwarz_type', PATCHES),))
    A, nv, idofs = sc.nodal(family, m)
    zs, hist, worst = {}, {}, 0.0
    for inv in ('1', '2', '3'):
        set_opt('MAMG_PATCH_INV', inv)
        for setup in ('host', 'gpu'):
            set_mode(mode)
            B = _mamg().MetricAMG(A, [nv, nv], idofs=idofs, num_functions=2, coarse_dof=CD, setup=setup,
                                  Schwarz_type=PATCHES)
            try:
                assert B.setup_path == setup and B.level_format(0)['patches']
                check_mode(B, mode, jacobi=False)
                for seed, z_ref in zo.items():
                    z = device_apply(B, rhs(family, m, seed))
                    e = rel(z, z_ref)
                    worst = max(worst, e)
                    assert e < 1e-10, (inv, setup, seed, e)
                    zs[(inv, setup, seed)] = z
                hist[(inv, setup)] = list(device_pcg(B, A, rhs(family, m))[0])
            finally:
                B.close()
    for setup in ('host', 'gpu'):
        for seed in sc.SEEDS:
            assert np.array_equal(zs[('1', setup, seed)], zs[('2', setup, seed)])
            assert rel(zs[('3', setup, seed)], zs[('2', setup, seed)]) < 1e-10
        assert hist[('1', setup)] == hist[('2', setup)]
        assert len(hist[('3', setup)]) == len(hist[('2', setup)])
        assert all(abs(a - b) <= 1e-6 * abs(a) for a, b in zip(hist[('2', setup)], hist[('3', setup)]))
    print('part e patches', family, m, mode, 'worst %.2e' % worst)


# ---------------------------------------------------------------------------
# f. fp32 cycle storage
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('mode', ['default', 'sell'])
@pytest.mark.parametrize('family,m', SMOOTHER, ids=ids(SMOOTHER))
def test_fp32_cycle_storage(lib_built, family, m, mode):
    """cycle_storage='f32' against the fp64 cycle on rounded operators
    (tests/cycle_storage_ref.py) under the mask the handle reports: within 1e-10
    of it and more than 1e-10 from the unrounded cycle, as
    tests/test_gpu_cycle_storage.py checks its inputs."""
    set_mode(mode)
    A, nv, idofs = sc.nodal(family, m)
    B = _mamg().MetricAMG(A, [nv, nv], idofs=idofs, num_functions=2, coarse_dof=CD, setup='gpu',
                          cycle_storage='f32')
    try:
        check_mode(B, mode)
        n = B.num_levels
        assert bits(B, 0) == ALL, B.level_storage(0)
        assert bits(B, n - 1) == 0
        h = sc.oracle(family, m)
        kform = [bool(B.level_format(l)['post_fused']) for l in range(n)]
        ref = StorageRef(h, masks=[bits(B, l) for l in range(n)], kform=kform)
        ref64 = StorageRef(h, masks=0, kform=kform)
        for seed in sc.SEEDS:
            r = rhs(family, m, seed)
            z = B * r
            e, d = rel(z, ref.apply(r)), rel(z, ref64.apply(r))
            print('part f', family, m, mode, 'seed', seed, 'vs rounded %.2e, vs unrounded %.2e' % (e, d))
            assert e < APPLY_TOL, e
            assert d > APPLY_TOL, d
    finally:
        B.close()


# ---------------------------------------------------------------------------
# g. scalar (CSR layout) hierarchies
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('k', sc.SCALAR)
def test_scalar_jacobi_matches_oracle(lib_built, k):
    M = _mamg()
    A = sc.scalar(k)
    h = sc.oracle_scalar(k)
    zo = {seed: h.apply(mo.seeded_rhs(k, seed)) for seed in sc.SEEDS}
    for setup in ('host', 'gpu'):
        B = M.MetricAMG(A, None, num_functions=1, coarse_dof=CD, setup=setup)
        try:
            assert B.setup_path == setup and B.layout == 'csr' and B.num_levels == len(sc.HIER_SCALAR[k])
            for seed, z_ref in zo.items():
                r = mo.seeded_rhs(k, seed)
                e1, e2 = rel(B * r, z_ref), rel(device_apply(B, r), z_ref)
                print('part g jacobi', k, setup, 'seed', seed, '%.2e / %.2e' % (e1, e2))
                assert e1 < APPLY_TOL and e2 < APPLY_TOL
        finally:
            B.close()


@functools.lru_cache(maxsize=None)
def pointgs(k, smo):
    ref = pr.PointGS(sc.scalar(k), smo, num_functions=1, coarse_dof=CD)
    return ref, {seed: ref.apply(mo.seeded_rhs(k, seed)) for seed in sc.SEEDS}


def pointgs_handle(k, smo, setup='auto', **extra):
    return _mamg().MetricAMG(sc.scalar(k), None, setup=setup,
                             **dict(pr.to_c(dict(num_functions=1, coarse_dof=CD, smoother=smo)), **extra))


@pytest.mark.parametrize('smo', ['GS', 'SGS'])
@pytest.mark.parametrize('k', sc.SCALAR)
def test_point_gs_matches_restatement(lib_built, k, smo):
    """SMOOTHER_GS_POINT / SGS_POINT against tests/pointgs_ref.PointGS to
    1e-10, host and GPU setup, every lane-group width; level 0 in
    csr_gs_small_kernel (k <= 4096: one workgroup, x in LDS) or colour by colour."""
    ref, zs = pointgs(k, smo)
    worst = 0.0
    for setup in ('host', 'gpu'):
        for lanes in (2, 4, 8, 16, 32, 64):
            B = pointgs_handle(k, smo, setup, spmv_lanes=lanes)
            try:
                assert B.setup_path == setup and B.layout == 'csr' and B.num_levels == len(ref.levels)
                assert all(B.level_format(l)['gs'] for l in range(B.num_levels - 1))
                for seed in sc.SEEDS:
                    e = rel(B * mo.seeded_rhs(k, seed), zs[seed])
                    worst = max(worst, e)
                    assert e <= 1e-10, (setup, lanes, seed, e)
            finally:
                B.close()
    print('part g', smo, k, 'worst %.2e' % worst)


@pytest.mark.parametrize('k', sc.SCALAR)
def test_point_gs_side_of_the_small_level_boundary(lib_built, k):
    """Which side of the 4096-row boundary level 0 ran on, from
    time_apply(mode=1)'s class split: launched colour by colour, the sweep
    from zero starts with a zeroing launch of class C_L0_WB (2, 8 bytes per
    row); in one workgroup the kernel zeroes x in LDS and the class is empty."""
    import torch
    B = pointgs_handle(k, 'SGS')
    try:
        r = torch.as_tensor(mo.seeded_rhs(k, 1234)).cuda()
        z = torch.empty_like(r)
        ms, kms, cb = B.time_apply(r, z, 2, mode=1)
        torch.cuda.synchronize()
        assert cb[1] > 0 and cb[5] > 0
        assert (cb[2] > 0) == (k > sc.GS_SMALL_MAX_ROWS), (k, cb[2])
        if k > sc.GS_SMALL_MAX_ROWS:
            assert cb[2] == 8.0 * k
        assert rel(z.cpu().numpy(), pointgs(k, 'SGS')[1][1234]) <= 1e-10
    finally:
        B.close()


@pytest.mark.parametrize('k', [4096, 4097])
def test_point_gs_pcg_matches_restatement(lib_built, k):
    A = sc.scalar(k)
    b = mo.seeded_rhs(k)
    ref = pr.pcg(A, pointgs(k, 'SGS')[0], b, 1e-8, 500)
    B = pointgs_handle(k, 'SGS')
    try:
        res, x = device_pcg(B, A, b)
        print('part g pcg', k, len(res) - 1, 'restatement', ref.niters)
        assert len(res) == len(ref.residuals)
        assert np.allclose(res, ref.residuals, rtol=1e-6, atol=0)
        assert rel(x, ref.x) < 1e-6
    finally:
        B.close()


# ---------------------------------------------------------------------------
# h. row partition on virtual ranks of one GPU
# ---------------------------------------------------------------------------
PART_H = [(127, 2), (128, 2), (129, 2), (127, 3), (128, 3), (129, 3), (65, 8)]


@pytest.mark.parametrize('mode', ['default', 'sell'])
@pytest.mark.parametrize('m,P', PART_H)
def test_virtual_ranks_equal_one_gpu(lib_built, m, P, mode):
    """rep_nodes 1: every level above the coarsest is partitioned (m = 65 on 8
    ranks: 8 or 9 node rows per rank).  The gathered apply equals the one-GPU
    apply to 1e-12 (tests/test_gpu_dist_csr.py's bound) and the oracle's to
    APPLY_TOL."""
    import torch
    M = _mamg()
    A, nv, idofs = sc.nodal('slice', m)
    B1 = build('slice', m, mode, 'gpu')
    hs = []
    try:
        check_mode(B1, mode)
        for p in range(P):
            hs.append(M.DistMetricAMG(A, [nv, nv], idofs=idofs, rank=p, nranks=P, comm_id=None, rep_nodes=1,
                                      num_functions=2, coarse_dof=CD))
        assert [h.o0 for h in hs[1:]] == [h.o1 for h in hs[:-1]] and hs[0].o0 == 0 and hs[-1].o1 == m
        assert all(h.nloc >= 1 for h in hs)
        if mode == 'sell':
            assert all(f['sell'] or f['half'] for f in (h.level_format(0) for h in hs))
        for seed in sc.SEEDS:
            r = rhs('slice', m, seed)
            rs = [torch.as_tensor(h.local_slice(r)).cuda() for h in hs]
            zs = [torch.zeros_like(x) for x in rs]
            M.DistMetricAMG.virtual_apply(hs, rs, zs)
            torch.cuda.synchronize()
            z = np.zeros(2 * m)
            for h, zl in zip(hs, zs):
                zl = zl.cpu().numpy()
                z[h.o0:h.o1] = zl[:h.nloc]
                z[m + h.o0:m + h.o1] = zl[h.nloc:]
            e1, eo = rel(z, B1 * r), rel(z, oracle_applies('slice', m)[seed])
            print('part h', m, P, mode, 'seed', seed, 'vs one GPU %.2e, vs oracle %.2e' % (e1, eo))
            assert e1 < 1e-12 and eo < APPLY_TOL
    finally:
        for h in hs:
            h.close()
        B1.close()
