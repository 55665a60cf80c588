"""GPU parity on inputs that are not grids in grid order (tests/irregular.py).

Every other -m gpu test feeds the library a lexicographically ordered grid:
rows of at most 30 entries, row halves of equal length, neighbouring rows
reaching neighbouring columns.  The layout and setup code takes most of its
decisions from exactly those properties; the tests here drive the other side
of each decision and assert -- through level_format, setup_path or a count
taken from the oracle's hierarchy -- that the branch was really taken:

  a  apply and device PCG against the oracle (lane-group and SELL layouts,
     host and GPU setup, V / W, JACOBI_RHO / POLY)
  b  SpMV against the per-row rounding bound of a row of len_i products
  c  the half-symmetric ELL-64 decision against its stated padding rule
  d  32-bit K columns when a SELL slice spans more than 65535 coarse nodes
  e  GPU setup = host setup bit for bit, all SpGEMM / MIS / CSR->BSR variants,
     the 2048-slot SpGEMM tier included
  f  SpGEMM rows of more than 2048 distinct columns: loud, and 'auto' falls
     back to the host setup
  g  a row longer than the 16-bit SELL row length
  h  a node patch that is not SPD

Every case runs with the library's defaults (lane-group BSR2 kernels at
these sizes) and with MAMG_SELL_MIN_ROWS=1 (the benchmark's SELL-64,
half-symmetric and K layouts).

Tolerances: APPLY_TOL = 1e-10 throughout.  The sensitivity of every part-a
case to summation order, measured from the reference alone as the relative
difference between the numpy oracle's apply and the oracle's C cycle
(oracle/vcycle_ref.c) on the same hierarchy, is at most 6.1e-14
(permuted3d-16, POLY; 1.3e-15 and below for the 2-D cases), so no case
needs more than 1e-10 ("Inputs that are not grids").
"""
import dataclasses
import functools

import numpy as np
import pytest

import irregular
import mamg_oracle as mo
from conftest import set_opt
from test_gpu import APPLY_TOL, rel
from test_gpu_setup import hierarchies_equal

pytestmark = pytest.mark.gpu

MODES = ['default', 'sell']
PATCHES = 6
ERR_SETUP, ERR_UNSUPPORTED = -3, -4
SPGEMM_MAX_COLS = 2048          # csrc/gsetup.hip spgemm_gl: the last hash tier


def _mamg():
    import metric_amg_examples_amd as M
    return M


def to_c(kw):
    c = dict(kw)
    for key, names in (('AMG_type', {'SA': 2, 'UA': 1}), ('cycle_type', {'V': 1, 'W': 2}),
                       ('smoother', {'JACOBI_RHO': 3, 'POLY': 12}),
                       ('aggregation_type', {'VMB': 1, 'MIS': 2, 'HEM': 5})):
        if key in c:
            c[key] = names[c[key]]
    return c


def set_mode(mode):
    if mode == 'sell':
        set_opt('MAMG_SELL_MIN_ROWS', '1')


CASES, SMALL, LONG_ROW, RULE_CASES = irregular.CASES, irregular.SMALL, irregular.LONG_ROW, irregular.RULE_CASES


def case(name):
    if name == 'long-row':
        return LONG_ROW[0](), LONG_ROW[1]
    gen, kw = CASES[name]
    return gen(), kw


# ---------------------------------------------------------------------------
# the reference side, computed once per session and never modified
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def oracle_setup(name, smoother):
    (A, nv, idofs), kw = case(name)
    return mo.setup(A, mo.Params(num_functions=2, smoother=smoother, **kw), idofs=idofs)


def oracle(name, cycle='V', smoother='JACOBI_RHO'):
    """The oracle's hierarchy; the cycle type is read by the apply only, so
    the V and W hierarchies share their levels."""
    h = oracle_setup(name, smoother)
    return mo.Hierarchy(h.levels, dataclasses.replace(h.params, cycle_type=cycle))


@functools.lru_cache(maxsize=None)
def oracle_applies(name, cycle, smoother):
    (A, nv, idofs), _ = case(name)
    h = oracle(name, cycle, smoother)
    return {seed: h.apply(mo.seeded_rhs(A.shape[0], seed)) for seed in (1234, 7)}


@functools.lru_cache(maxsize=None)
def oracle_pcg(name, cycle, smoother):
    (A, nv, idofs), _ = case(name)
    return mo.pcg(A, oracle(name, cycle, smoother), mo.seeded_rhs(A.shape[0]), 1e-8, 500)


@functools.lru_cache(maxsize=None)
def spgemm_widest(name):
    return irregular.spgemm_rows(oracle_setup(name, 'JACOBI_RHO'))[0]


def build(name, mode, setup, **kw):
    """MetricAMG of a case (BSR2 layout) with the case's parameters and kw."""
    M = _mamg()
    (A, nv, idofs), okw = case(name)
    B = M.MetricAMG(A, [nv, nv], idofs=idofs, num_functions=2, setup=setup, **to_c(dict(okw, **kw)))
    assert B.layout == 'bsr2'
    return B


def check_mode(B, mode):
    f = B.level_format(0)
    if mode == 'sell':
        assert f['sell'] or f['half'], f
    else:
        assert not f['sell'] and not f['half'], f


def assert_unsupported_spgemm(fn):
    M = _mamg()
    with pytest.raises(M._lib.MamgError) as ei:
        fn()
    assert ei.value.code == ERR_UNSUPPORTED and 'more than 2048 distinct columns' in str(ei.value), str(ei.value)


# ---------------------------------------------------------------------------
# a. apply and PCG against the oracle
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('cycle,smoother', [('V', 'JACOBI_RHO'), ('W', 'JACOBI_RHO'), ('V', 'POLY'), ('W', 'POLY')])
@pytest.mark.parametrize('name', list(CASES))
def test_apply_and_pcg_match_oracle(lib_built, name, cycle, smoother, mode):
    """Host-pointer and device-pointer applies against the oracle's to
    APPLY_TOL for two right-hand sides, device PCG with the oracle's iteration
    count and residual history (rtol 1e-6), for the host and the GPU setup.
    Branches: lane-group BSR2 kernels on rows of 1 to 3008 blocks (default
    mode); SELL-64 A_0, P and R with scattered columns and slices whose rows
    differ in length, SELL K where its rows average at most 40 blocks (the
    renumbered grids; K of the ragged and hub inputs stays in lane groups)
    (sell mode).  Where the
    oracle's hierarchy has a product row of more than 2048 distinct columns
    (hub96-m3000-theta0.25: 2448) the GPU setup must refuse and 'auto' must
    fall back to the host setup (part f), which is then what is compared."""
    import torch
    M = _mamg()
    set_mode(mode)
    (A, nv, idofs), _ = case(name)
    zo = oracle_applies(name, cycle, smoother)
    ref = oracle_pcg(name, cycle, smoother)
    nlev = len(oracle_setup(name, smoother).levels)
    overflow = spgemm_widest(name) > SPGEMM_MAX_COLS
    for setup in ('host', 'gpu'):
        kw = dict(cycle_type=cycle, smoother=smoother)
        if setup == 'gpu' and overflow:
            assert_unsupported_spgemm(lambda: build(name, mode, 'gpu', **kw))
            B = build(name, mode, 'auto', **kw)
            assert B.setup_path.startswith('host (') and '2048 distinct columns' in B.setup_path
        else:
            B = build(name, mode, setup, **kw)
            assert B.setup_path == setup
        try:
            check_mode(B, mode)
            assert B.num_levels == nlev
            for seed, z_ref in zo.items():
                r = mo.seeded_rhs(A.shape[0], seed)
                e1 = rel(B * r, z_ref)
                zt = B.matvec(torch.as_tensor(r).cuda())
                torch.cuda.synchronize()
                e2 = rel(zt.cpu().numpy(), z_ref)
                print(name, cycle, smoother, mode, setup, 'seed', seed, 'apply err %.2e / %.2e' % (e1, e2))
                assert e1 < APPLY_TOL and e2 < APPLY_TOL, (e1, e2)
            solver = M.ConjGrad(A, precond=B, tolerance=1e-8, maxiter=500, device=True)
            solver * mo.seeded_rhs(A.shape[0])
            print(name, cycle, smoother, mode, setup, 'pcg iters', len(solver.residuals) - 1, 'oracle', ref.niters)
            assert len(solver.residuals) == len(ref.residuals)
            assert np.allclose(solver.residuals, ref.residuals, rtol=1e-6, atol=0)
        finally:
            B.close()


# ---------------------------------------------------------------------------
# b. SpMV against the rounding bound of each row
# ---------------------------------------------------------------------------
# each matrix once (the two hub96 cases share theirs); long-row has no SELL
# layout (part g asserts that error): default mode only
@pytest.mark.parametrize('name,mode', [(n, m) for n in CASES if not n.endswith('theta0.25') for m in MODES]
                         + [('long-row', 'default')])
def test_spmv_within_row_bound(lib_built, name, mode):
    """spmv_device against A x accumulated in long double, row by row:
    |y_i - ref_i| <= (len_i + 2) 2^-53 sum_j |a_ij x_j|, the bound of any
    summation order of len_i products (FMA or not).  Rows here hold 1 to 3008
    entries (66008 for long-row), so the bound is ~100 times tighter than a
    global 1e-14 on the short rows and honest on the hub's.  Lane-group BSR2
    kernels (default) and the SELL-64 / half-symmetric A_0 (sell)."""
    import torch
    M = _mamg()
    (A, nv, idofs), okw = case(name)
    set_mode(mode)
    B = M.MetricAMG(A, [nv, nv], idofs=idofs, num_functions=2, setup='host', **to_c(okw))
    try:
        check_mode(B, mode)
        x = np.random.default_rng(3).standard_normal(A.shape[0])
        y = torch.empty(A.shape[0], dtype=torch.float64, device='cuda')
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
    worst = int(np.argmax(err / bound))
    print(name, mode, 'longest row', int(ln.max()), 'worst err / bound %.3f at row %d (len %d)'
          % (float(err[worst] / bound[worst]), worst, int(ln[worst])))
    assert np.all(err <= bound), (worst, float(err[worst]), float(bound[worst]))


# ---------------------------------------------------------------------------
# c. the half-symmetric decision against its stated rule
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('setup', ['host', 'gpu'])
@pytest.mark.parametrize('name', list(RULE_CASES))
def test_half_decision_matches_rule(lib_built, name, setup):
    """Under MAMG_SELL_MIN_ROWS=1, level_format(0)['half'] equals the padding
    / length rule recomputed in numpy and ['sell'] is its complement (both
    reject branches of try_half and the accept branch on irregular inputs).
    Where half is accepted, MAMG_HALF=1 and MAMG_HALF=0 give bitwise equal
    applies and PCG histories."""
    M = _mamg()
    A, nv, idofs = RULE_CASES[name]()
    want, detail, sell_ok = irregular.half_rule(A, nv)
    assert sell_ok
    set_opt('MAMG_SELL_MIN_ROWS', '1')
    r = mo.seeded_rhs(A.shape[0])
    outs, its = [], []
    for half in ('1', '0') if want else ('1',):
        set_opt('MAMG_HALF', half)
        B = M.MetricAMG(A, [nv, nv], idofs=idofs, num_functions=2, setup=setup)
        try:
            f = B.level_format(0)
            print(name, setup, 'MAMG_HALF', half, 'rule', want, detail, f)
            assert f['sym']
            assert f['half'] == (want and half == '1'), (f, detail)
            assert f['sell'] == (not f['half']), f
            outs.append(B * r)
            solver = M.ConjGrad(A, precond=B, tolerance=1e-8, maxiter=500)
            solver * r
            its.append(list(solver.residuals))
        finally:
            B.close()
    if want:
        assert np.array_equal(outs[0], outs[1])
        assert its[0] == its[1]


# ---------------------------------------------------------------------------
# d. wide K columns
# ---------------------------------------------------------------------------
# permuted(2, n, 1e3, seed 1): level 1 has 65484 nodes at n = 826 and 65592 at
# n = 827, the smallest n above 65536 (host setup, CPU); at n = 827, 260 of the
# 10712 K slices then span more than 65535 coarse nodes
WIDE_N = 827


@pytest.mark.parametrize('n,wide', [(64, False), (WIDE_N, True)])
def test_k_columns_on_scattered_rows(lib_built, n, wide):
    """compress_sell_cols / sell_span_kernel on a renumbered grid, GPU setup,
    MAMG_SELL_MIN_ROWS=1.  n = 64: every slice's columns are scattered over
    all 405 coarse nodes but span less than 2^16, so k_col16 stays on and the
    per-slice base subtraction is exercised on unordered columns.  n = 827:
    65592 coarse nodes and slices spanning more than 65535 of them, so the
    detection must keep 32-bit columns (k_col16 false with MAMG_K_COL16 at its
    default); a wrong detection would truncate columns.  Either way the apply
    and the device PCG history are bitwise those of MAMG_K_COL16=0, <Br, r> > 0
    and <Br, q> = <r, Bq> to 1e-9."""
    import torch
    M = _mamg()
    A, nv, idofs = irregular.permuted(2, n, 1e3, 1)
    set_opt('MAMG_SELL_MIN_ROWS', '1')
    N = A.shape[0]
    r = torch.as_tensor(mo.seeded_rhs(N)).cuda()
    q = torch.as_tensor(mo.seeded_rhs(N, 7)).cuda()
    zs, its = [], []
    for c16 in (None, '0'):
        if c16 is not None:
            set_opt('MAMG_K_COL16', c16)
        B = M.MetricAMG(A, [nv, nv], idofs=idofs, num_functions=2, setup='gpu')
        try:
            f = B.level_format(0)
            print('n', n, 'MAMG_K_COL16', c16, f)
            assert f['post_sell'] and f['post_k']
            assert f['k_col16'] == (c16 is None and not wide), f
            Br, Bq = B.matvec(r), B.matvec(q)
            zs.append(Br)
            if c16 is None:
                a, b = torch.dot(Br, q).item(), torch.dot(r, Bq).item()
                assert abs(a - b) <= 1e-9 * (abs(a) + abs(b)), (a, b)
                assert torch.dot(Br, r).item() > 0
            cg = M.ConjGrad(A, precond=B, tolerance=1e-8, maxiter=500)
            cg * mo.seeded_rhs(N)
            its.append(list(cg.residuals))
            torch.cuda.synchronize()
        finally:
            B.close()
    assert torch.equal(zs[0], zs[1])
    assert its[0] == its[1] and len(its[0]) < 500
    if wide:
        irregular.permuted.cache_clear()        # 1.4 M rows: not kept for the session


# ---------------------------------------------------------------------------
# e. GPU setup = host setup, bit for bit
# ---------------------------------------------------------------------------
def host_and_gpu_equal(A, idofs, kw, hub=None):
    """hierarchies_equal(host setup, GPU setup).  hub: the hub's node, where
    the input has one; the rows it drives through the SpGEMM are then counted
    on the host hierarchy's P and R (bitwise the oracle's,
    tests/test_irregular_host.py), and where one exceeds the last hash tier
    the GPU setup must refuse with MAMG_ERR_UNSUPPORTED instead.  Returns that
    count."""
    import scipy.sparse as sp
    M = _mamg()
    ckw = to_c(dict(kw, num_functions=2))
    Hh = M.HostHierarchy(A, idofs=idofs, **ckw)
    try:
        assert Hh.num_levels >= 2
        width = 0
        if hub is not None:
            nv = A.shape[0] // 2
            lv = Hh.level(0, with_A=False)
            P, R = (sp.csr_matrix((m[2], m[1], m[0]), shape=m[3]) for m in (lv['P'], lv['R']))
            width = irregular.hub_product_width(A, P, R, [hub, nv + hub])
            print('hub rows of A P / R (A P): %d distinct columns' % width)
        if width > SPGEMM_MAX_COLS:
            assert_unsupported_spgemm(lambda: M.HostHierarchy(A, idofs=idofs, gpu=True, **ckw))
            return width
        Hg = M.HostHierarchy(A, idofs=idofs, gpu=True, **ckw)
        try:
            hierarchies_equal(Hh, Hg)
        finally:
            Hg.close()
    finally:
        Hh.close()
    return width


def hub_of(name):
    return irregular.hub_node(int(name[3:5])) if name.startswith('hub') else None


@pytest.mark.parametrize('kw', irregular.PARAM_SETS, ids=irregular.param_id)
@pytest.mark.parametrize('name', list(SMALL))
def test_gpu_setup_bitwise_equals_host(lib_built, name, kw):
    """MIS-2 / HEM hash tie-breaking, mis2's staged row maxima, the strength
    filter, the node-pair SpGEMM and the Galerkin products of csrc/gsetup.hip
    on graphs that are not grids: every level array equals the host setup's
    (which tests/test_irregular_host.py pins to the oracle).  Where a hub
    drives a product row past 2048 distinct columns the documented refusal is
    asserted instead (host_and_gpu_equal)."""
    A, nv, idofs = SMALL[name]()
    width = host_and_gpu_equal(A, idofs, kw, hub_of(name))
    # hub64-m500 with HEM: 2196 coarse dofs, and the hub aggregate's rows of
    # R (A P) reach 2144 of them -- the GPU setup refuses (asserted above)
    assert (width > SPGEMM_MAX_COLS) == (name == 'hub64-m500' and kw.get('aggregation_type') == 'HEM')


KNOBS = [dict(MAMG_SPGEMM_STAGE_GB='16', MAMG_SPGEMM_STAGE_STRIDE='16', MAMG_SPGEMM_PAIR='1'),
         dict(MAMG_SPGEMM_STAGE_GB='16', MAMG_SPGEMM_STAGE_STRIDE='128', MAMG_SPGEMM_PAIR='1'),
         dict(MAMG_SPGEMM_STAGE_GB='16', MAMG_SPGEMM_STAGE_STRIDE='128', MAMG_SPGEMM_PAIR='0'),
         dict(MAMG_SPGEMM_STAGE_GB='0', MAMG_SPGEMM_STAGE_STRIDE='128', MAMG_SPGEMM_PAIR='1'),
         dict(MAMG_MIS_STAGED='0')]


def knob_id(k):
    return ','.join('%s=%s' % (a.replace('MAMG_', '').replace('SPGEMM_', ''), b) for a, b in k.items())


@pytest.mark.parametrize('knobs', KNOBS, ids=knob_id)
@pytest.mark.parametrize('kw', [dict(), dict(aggregation_type='HEM')], ids=irregular.param_id)
@pytest.mark.parametrize('name', ['permuted2d-64', 'permuted3d-8', 'hub64-m500', 'ragged64'])
def test_gpu_setup_variants_bitwise(lib_built, name, kw, knobs):
    """The SpGEMM staging strides, the row-by-row count pass, two-pass SpGEMM
    and the lane-per-row MIS-2 maxima (the settings of
    test_gpu_spgemm_staging_bitwise / test_csr2bsr_fill_variants_bitwise) on
    irregular graphs: each gives the host setup's hierarchy bit for bit (or,
    for hub64-m500 with HEM, the same refusal of a row past 2048 columns).  With
    stride 16 the hub's and the ragged rows take the long-row list; with
    renumbered nodes the pair kernel's two rows still share their columns."""
    for k, v in knobs.items():
        set_opt(k, v)
    A, nv, idofs = SMALL[name]()
    host_and_gpu_equal(A, idofs, kw, hub_of(name))


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('name', ['permuted2d-64', 'hub64-m500', 'ragged64', 'hub96-m3000'])
def test_csr2bsr_fill_variants_irregular(lib_built, name, mode):
    """MAMG_CSR2BSR_FILL=1 (slots in LDS, values scattered) against 0 (the
    staged merge) where a wave's 64 node rows do not fit the LDS stage (the
    hub's workgroup: 3008 + 64 x 7 entries per field against RS_CAP 2048 takes
    the global-memory merge) and where row lengths differ inside the wave:
    same level formats, bitwise equal applies."""
    M = _mamg()
    set_mode(mode)
    A, nv, idofs = (SMALL.get(name) or CASES[name][0])()
    if name.startswith('hub'):
        assert np.diff(A.indptr).max() > (2048 if name == 'hub96-m3000' else 500)
    outs, fmts = [], []
    for fill in ('1', '0'):
        set_opt('MAMG_CSR2BSR_FILL', fill)
        B = M.MetricAMG(A, [nv, nv], idofs=idofs, num_functions=2, setup='gpu')
        try:
            check_mode(B, mode)
            fmts.append([B.level_format(lv) for lv in range(B.num_levels)])
            outs.append([B * mo.seeded_rhs(A.shape[0], seed) for seed in (1234, 7)])
        finally:
            B.close()
    assert fmts[0] == fmts[1]
    for a, b in zip(outs[0], outs[1]):
        assert np.array_equal(a, b)


@pytest.mark.parametrize('name,n,kw', [('hub64-m500', 64, {}), ('hub64-m500', 64, dict(strong_coupled=0.25)),
                                       ('hub96-m3000', 96, {})])
def test_gpu_setup_2048_slot_tier(lib_built, name, n, kw):
    """The hub's row of A P holds more than 512 and at most 2048 distinct
    columns (counted on the oracle's P: 770 / 1060 / 1710), and no row of any
    product more than 2048: the 128- and 512-slot hash tables overflow, the
    2048-slot launch of spgemm_gl computes the row, and the hierarchy is the
    host setup's bit for bit."""
    A, nv, idofs = (SMALL.get(name) or CASES[name][0])()
    h = mo.setup(A, mo.Params(num_functions=2, **kw), idofs=idofs) if kw or name in SMALL \
        else oracle_setup(name, 'JACOBI_RHO')
    c = irregular.hub_node(n)
    widest, hub_row = irregular.spgemm_rows(h, rows=[c, nv + c])
    print(name, kw, 'hub row of A P:', hub_row, 'widest product row:', widest)
    assert 512 < hub_row <= SPGEMM_MAX_COLS and widest <= SPGEMM_MAX_COLS
    host_and_gpu_equal(A, idofs, kw)


# ---------------------------------------------------------------------------
# f. SpGEMM overflow is loud, the fallback is right
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('mode', MODES)
def test_spgemm_overflow_is_loud_and_auto_falls_back(lib_built, mode):
    """hub(96, m = 3000) at strong_coupled 0.25: the hub's row of A P reaches
    2444 distinct columns and a row of R (A P) 2448 (counted on the oracle's
    hierarchy, asserted), more than the last hash tier holds.  setup='gpu'
    and the GPU HostHierarchy return MAMG_ERR_UNSUPPORTED naming the limit;
    setup='auto' records the reason in setup_path, runs the host setup and
    its apply matches the oracle to APPLY_TOL."""
    M = _mamg()
    name = 'hub96-m3000-theta0.25'
    (A, nv, idofs), okw = case(name)
    c = irregular.hub_node(96)
    widest, hub_row = irregular.spgemm_rows(oracle_setup(name, 'JACOBI_RHO'), rows=[c, nv + c])
    print('hub row of A P:', hub_row, 'widest product row:', widest)
    assert hub_row > SPGEMM_MAX_COLS and widest > SPGEMM_MAX_COLS
    set_mode(mode)
    assert_unsupported_spgemm(lambda: build(name, mode, 'gpu'))
    assert_unsupported_spgemm(lambda: M.HostHierarchy(A, idofs=idofs, gpu=True, num_functions=2, **to_c(okw)))
    B = build(name, mode, 'auto')
    try:
        assert B.setup_path.startswith('host (') and 'more than 2048 distinct columns' in B.setup_path
        check_mode(B, mode)
        for seed, z_ref in oracle_applies(name, 'V', 'JACOBI_RHO').items():
            assert rel(B * mo.seeded_rhs(A.shape[0], seed), z_ref) < APPLY_TOL
    finally:
        B.close()


# ---------------------------------------------------------------------------
# g. the 16-bit row length
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('mode', MODES)
def test_row_longer_than_16_bit_length(lib_built, mode):
    """A node row of 66008 blocks (hub with 66000 neighbours, nv = 74529),
    host setup.  Default mode: the lane-group BSR2 layout (64-bit row
    pointers) must match the oracle.  MAMG_SELL_MIN_ROWS=1: the mean row
    length (8.8 blocks) passes nb <= 40 nr, so the SELL path is entered and
    must return MAMG_ERR_UNSUPPORTED "SELL: row longer than 65534 blocks".

    Read in csrc/device.hip before this ran on a GPU: finalize_bsr calls
    try_half first; half_meta_kernel tests nu / nl > 255 before it packs
    meta[I] and skips the row, and try_half returns on wm[2] straight after
    copying the four flags back, before half_gwidth_kernel or half_fill_kernel
    read any meta.  finalize_bsr then runs sell_meta_kernel, which tests
    e - a >= 0xffff before packing len | plen << 16, leaves the row out of the
    slice width, and finalize_bsr returns on the flag before the scan of soff,
    the allocation of col / val and sell_fill_kernel.  The host packing
    (convert.cpp to_sell) has the same test before its fill loop.  The CSR ->
    BSR2 conversion ahead of both takes the global-memory merge for the hub's
    workgroup (stage_rows: the wave's ranges exceed RS_CAP, uniform branch)."""
    import torch
    M = _mamg()
    (A, nv, idofs), okw = case('long-row')
    assert np.diff(A[:nv, :nv].tocsr().indptr).max() > 65535
    set_mode(mode)
    if mode == 'sell':
        _, detail, sell_ok = irregular.half_rule(A, nv)
        assert sell_ok and detail['too_long']
        with pytest.raises(M._lib.MamgError) as ei:
            build('long-row', mode, 'host')
        assert ei.value.code == ERR_UNSUPPORTED and 'row longer than 65534 blocks' in str(ei.value), str(ei.value)
        return
    B = build('long-row', mode, 'host')
    try:
        check_mode(B, mode)
        for seed, z_ref in oracle_applies('long-row', 'V', 'JACOBI_RHO').items():
            r = mo.seeded_rhs(A.shape[0], seed)
            zt = B.matvec(torch.as_tensor(r).cuda())
            torch.cuda.synchronize()
            e1, e2 = rel(B * r, z_ref), rel(zt.cpu().numpy(), z_ref)
            print('long-row seed', seed, 'apply err %.2e / %.2e' % (e1, e2))
            assert e1 < APPLY_TOL and e2 < APPLY_TOL
    finally:
        B.close()


# ---------------------------------------------------------------------------
# h. a node patch that is not SPD
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('inv', ['2', '3'])
def test_indefinite_patch_is_an_error(lib_built, inv):
    """MAMG_PATCH_INV 2 (scalar Gauss-Jordan, two patches per wave) and 3
    (matrix-core block sweep, the default; its check is dp > 0 on the pivots
    inside each 4x4 block) both return MAMG_ERR_SETUP "a patch matrix is not
    SPD" instead of storing the inverse of an indefinite patch, with partly
    dead waves in the last workgroup, and the GPU setup reports what the host
    setup reports."""
    M = _mamg()
    A, nv, idofs = irregular.indefinite_patch_system()
    set_opt('MAMG_PATCH_INV', inv)
    msgs = []
    for setup in ('host', 'gpu'):
        with pytest.raises(M._lib.MamgError) as ei:
            M.MetricAMG(A, [nv, nv], idofs=idofs, num_functions=2, Schwarz_type=PATCHES, setup=setup)
        assert ei.value.code == ERR_SETUP, str(ei.value)
        assert 'node patches' in str(ei.value) and 'not SPD' in str(ei.value), str(ei.value)
        msgs.append(str(ei.value))
    assert msgs[0] == msgs[1]
    # the same system without the perturbation sets up with this kernel
    o = mo.bidomain_system(2, 16, 1e2)
    B = M.MetricAMG(o['A'], [nv, nv], idofs=idofs, num_functions=2, Schwarz_type=PATCHES)
    assert B.level_format(0)['patches']
    B.close()
