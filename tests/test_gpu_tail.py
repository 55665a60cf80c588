"""The coarse tail (device.hip tail_kernel: one workgroup runs the whole cycle
below tail_level as an op program) over every plan its planner can build.

Cases and their pinned sizes: tests/tail_cases.py (checked on the CPU by
tests/test_tail_cases.py, with the >= 1e-4 sensitivity of every right-hand
side to the tail's correction).  Three assertions throughout:

(a) the tail apply equals the oracle's ``h.apply(r)`` to 1e-10 relative (the
    project's contract; every system here has gamma < 1e8);
(b) it equals the same configuration with MAMG_TAIL_NODES=0 (the launch
    path) to 1e-13: each op computes its rows as its kernel does, up to FMA
    contraction;
(c) ``tail_info()`` shows the plan the case names, so a case that drifted off
    its branch fails instead of passing on another one.
"""
import functools

import numpy as np
import pytest

import mamg_oracle as mo
import tail_cases as tc
from conftest import set_opt
from cycle_storage_ref import ALL, BIT_A, BIT_KP, BIT_R, StorageRef
from tail_cases import JAC, POLY, SGS, W2S, frozen, rel

pytestmark = pytest.mark.gpu

TOL_ORACLE = 1e-10
TOL_LAUNCH = 1e-13


def _mamg():
    import metric_amg_examples_amd as M
    return M


def build(hn, kw, opts=None, setup='host', nodes=tc.ALL_NODES, A=None):
    """A handle of HIER[hn] under the oracle keys kw and the switches opts;
    nodes: MAMG_TAIL_NODES ('0': the launch path)."""
    M = _mamg()
    for k, v in (opts or {}).items():
        set_opt(k, v)
    set_opt('MAMG_TAIL_NODES', nodes)
    s = tc.system(hn)
    B = M.MetricAMG(s.scipy() if A is None else A, s.W, idofs=s.idofs, num_functions=2, setup=setup,
                    **tc.to_c(dict(tc.HIER[hn]['kw'], **kw)))
    assert B.layout == 'bsr2' and B.setup_path == setup
    for k in (opts or {}):
        set_opt(k, None)
    set_opt('MAMG_TAIL_NODES', None)
    return B


@functools.lru_cache(maxsize=None)
def _oracle_apply(hn, fkw):
    h = tc.oracle(hn, **dict(fkw))
    return tuple(h.apply(tc.rhs(hn, seed)) for seed in tc.SEEDS)


_LAUNCH = {}
LAYOUT_OPTS = ('MAMG_POST_K', 'MAMG_FUSE_RBD')     # the switches that also shape the launch path


def launch_apply(hn, kw, opts, setup):
    """The launch path's applies of the same configuration (computed once)."""
    lo = {k: v for k, v in (opts or {}).items() if k in LAYOUT_OPTS}
    key = (hn, frozen(kw), frozen(lo), setup)
    if key not in _LAUNCH:
        B = build(hn, kw, lo, setup, nodes='0')
        try:
            z = tuple(B * tc.rhs(hn, seed) for seed in tc.SEEDS)
            info = B.tail_info()
            assert info['tail_level'] == 0 and info['programs'] == [] and not info['refused'], info
        finally:
            B.close()
        _LAUNCH[key] = z
    return _LAUNCH[key]


def check(hn, kw, opts=None, setup='host', taken=True):
    """(a) and (b) for both right-hand sides; returns (tail_info, applies).
    tail_info() before the first apply says nothing is planned yet."""
    assert (hn, frozen(kw), 1) in tc.APPLIED_KEYS, 'list the case in tail_cases.APPLIED (sensitivity pin)'
    zo = _oracle_apply(hn, frozen(kw))
    zl = launch_apply(hn, kw, opts, setup)
    B = build(hn, kw, opts, setup)
    try:
        before = B.tail_info()
        assert before['tail_level'] == 1 and before['programs'] == [] and not before['refused'], before
        zt = tuple(B * tc.rhs(hn, seed) for seed in tc.SEEDS)
        info = B.tail_info()
    finally:
        B.close()
    for z, o, l, seed in zip(zt, zo, zl, tc.SEEDS):
        d_o, d_l, d_lo = rel(z, o), rel(z, l), rel(l, o)
        print('TAILDEV %s %s %s %s seed %d: tail-oracle %.2e tail-launch %.2e launch-oracle %.2e'
              % (hn, tc.key(kw), opts or '', setup, seed, d_o, d_l, d_lo))
        assert d_o < TOL_ORACLE, d_o
        assert d_l < TOL_LAUNCH, d_l
    assert info['tail_level'] == 1, info
    if taken:
        assert not info['refused'], info
        assert len(info['programs']) == (2 if kw.get('cycle_type') == 'W' else 1), info
    return info, zt


def assert_resident(info, hn, dense='lds'):
    """Every program holds the rows tail_cases.residency names, its overflow
    blocks, and runs ops from them; the dense inverse where ``dense`` says."""
    lv, rows, nov, region = tc.residency(hn)
    dofs = 2 * tc.HIER[hn]['levels'][-1][0]
    for p in info['programs']:
        assert p['res'] == 1 and p['replanned'] == 0, p
        assert p['resident_rows'] == rows and p['nov'] == nov, (p, rows, nov)
        assert p['ops_res'] > 0 and p['ops_global'] > 0, p       # A from registers; P, R, K from global arrays
        assert p['lds_bytes'] >= region, p
        assert p['gemv'] and set(p['gemv']) == {(dofs, dense)}, p


def assert_all_lds(info):
    for p in info['programs']:
        assert p['xl'] == 1 and p['vec_global'] == 0 and p['vec_lds'] > 0 and p['lds_bytes'] > 0, p


# ---------------------------------------------------------------------------
# smoother families inside the tail
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('setup', ['host', 'gpu'])
@pytest.mark.parametrize('kw', tc.FAMILY_VARIANTS, ids=tc.key)
@pytest.mark.parametrize('hn', tc.FAMILY_HIERS)
def test_families(lib_built, hn, kw, setup):
    """Jacobi family and POLY run by the tail: T_BD, T_BSR with EPI_BJAC and
    EPI_KPOST (K = P - W A P), POLY's step weights, the W cycle's second
    program, the coarse scaling -- from resident rows (tail_res: sa3d16 with
    long overflow rows, sa2d64c40 with two resident levels) with every vector
    in LDS."""
    info, _ = check(hn, kw, setup=setup)
    assert_resident(info, hn)
    assert_all_lds(info)
    for p in info['programs']:
        assert p['prog_lds'] == -1, p


@pytest.mark.parametrize('kw', [JAC, dict(JAC, **W2S), dict(POLY, coarse_scaling=1)], ids=tc.key)
@pytest.mark.parametrize('res', ['0', '1'])
def test_families_from_global_rows(lib_built, kw, res):
    """The same epilogues in tail_bsr (MAMG_TAIL_RES=0: no resident rows)."""
    info, _ = check('sa3d16', kw, {'MAMG_TAIL_RES': res})
    for p in info['programs']:
        assert p['res'] == int(res) and (p['ops_res'] > 0) == (res == '1'), p
        assert p['gemv'] and set(p['gemv']) == {(14, 'lds' if res == '1' else 'global')}, p


@pytest.mark.parametrize('kw', [dict(JAC, coarse_scaling=1), dict(POLY, **W2S)], ids=tc.key)
@pytest.mark.parametrize('hn', tc.FAMILY_HIERS)
@pytest.mark.parametrize('post_k', ['0', '2'])
def test_post_k(lib_built, post_k, hn, kw):
    """MAMG_POST_K=0 stores the merged [P | AP] window, which the tail cannot
    express: to_tail refuses, tail_info says so, the level runs as launches.
    MAMG_POST_K=2 only re-lays SELL-stored K, which the coarse levels do not
    have: the tail takes the level.  The result is right either way."""
    info, _ = check(hn, kw, {'MAMG_POST_K': post_k}, taken=post_k == '2')
    if post_k == '0':
        assert info['refused'] and info['programs'] == [], info
    else:
        assert_resident(info, hn)


@pytest.mark.parametrize('fuse', ['0', '1', '2'])
@pytest.mark.parametrize('setup', ['host', 'gpu'])
def test_fuse_rbd(lib_built, fuse, setup):
    """The restriction into the tail level must not also write the first
    sweep the tail's own T_BD redoes (starts_with_bd excludes tail_level)."""
    kw = dict(JAC, presmooth_iter=2, postsmooth_iter=2)
    info, _ = check('sa2d64c40', kw, {'MAMG_FUSE_RBD': fuse}, setup=setup)
    assert_resident(info, 'sa2d64c40')


# ---------------------------------------------------------------------------
# lane caps
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('res', ['0', '1'])
@pytest.mark.parametrize('kw', [dict(JAC, coarse_scaling=1), SGS], ids=tc.key)
def test_lane_caps(lib_built, kw, res):
    """MAMG_TAIL_VL 1, 2, 4, 8, 64: tail_bsr's reductions -- none, DPP quad
    permutations (2, 4), __shfl_xor of width VL (8 and the matrices' own 16 or
    more lanes).  With MAMG_TAIL_RES=0 every op runs there, with 1 the
    transfers and K do.  All agree with the launch path and with each other."""
    zs = {}
    for cap in (1, 2, 4, 8, 64):
        info, z = check('sa3d16', kw, {'MAMG_TAIL_VL': str(cap), 'MAMG_TAIL_RES': res})
        for p in info['programs']:
            assert p['res'] == int(res), p
            if cap <= 8:
                assert p['max_vl'] == cap, p
            else:
                assert p['max_vl'] >= 16, p
        zs[cap] = z
    for cap in (2, 4, 8, 64):
        for a, b in zip(zs[cap], zs[1]):
            assert rel(a, b) < TOL_LAUNCH


# ---------------------------------------------------------------------------
# vector placement, program placement
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('kw', [dict(JAC, cycle_type='W', coarse_scaling=1), SGS], ids=tc.key)
def test_vectors_global(lib_built, kw):
    """MAMG_TAIL_LDS=0: the global side of every TVec::ld / st (XL = false).
    Without LDS there is no region for resident rows either: the residency
    plan is discarded (replanned), or never made with MAMG_TAIL_RES=0."""
    for res in ('1', '0'):
        info, _ = check('sa3d16', kw, {'MAMG_TAIL_LDS': '0', 'MAMG_TAIL_RES': res})
        for p in info['programs']:
            assert p['vec_lds'] == 0 and p['vec_global'] > 0 and p['lds_bytes'] == 0 and p['xl'] == 0, p
            assert p['res'] == 0 and p['resident_rows'] == 0 and p['replanned'] == int(res), p
            assert set(p['gemv']) == {(14, 'global')}, p


def test_vectors_partly_in_lds(lib_built):
    """ua3d16 from level 1, W cycle with two sweeps and scaling: the vectors
    do not all fit beside the region (tail_cases pins it), so some operands
    are LDS offsets and some global pointers, and a gathered x is among the
    global ones (xl = 0); level 1 (1109 rows) runs from global arrays above
    resident levels 2 .. 4."""
    info, _ = check('ua3d16', dict(JAC, **W2S))
    assert_resident(info, 'ua3d16')
    for p in info['programs']:
        assert p['vec_lds'] > 0 and p['vec_global'] > 0 and p['xl'] == 0, p


@pytest.mark.parametrize('kw', [dict(JAC, cycle_type='W', coarse_scaling=1), SGS, POLY], ids=tc.key)
@pytest.mark.parametrize('res', ['0', '1'])
def test_program_in_lds(lib_built, kw, res):
    """MAMG_TAIL_PROG_LDS=1: the descriptors copied into LDS and rebuilt with
    readfirstlane.  The ops are the same, only the fetch of the descriptor
    differs: the results are bitwise those of MAMG_TAIL_PROG_LDS=0."""
    i0, z0 = check('sa3d16', kw, {'MAMG_TAIL_PROG_LDS': '0', 'MAMG_TAIL_RES': res})
    i1, z1 = check('sa3d16', kw, {'MAMG_TAIL_PROG_LDS': '1', 'MAMG_TAIL_RES': res})
    for p0, p1 in zip(i0['programs'], i1['programs']):
        assert p0['prog_lds'] == -1 and p1['prog_lds'] >= 0, (p0, p1)
        assert p1['prog_lds'] % 16 == 0 and p1['lds_bytes'] > p1['prog_lds'], p1
        assert p0['res'] == p1['res'] == int(res), (p0, p1)
        assert p0['ops'] == p1['ops'] and p0['nov'] == p1['nov'], (p0, p1)
    for a, b in zip(z0, z1):
        assert np.array_equal(a, b)


# ---------------------------------------------------------------------------
# residency plans and the dense solve
# ---------------------------------------------------------------------------
def test_non_resident_level_above_resident_ones(lib_built):
    """ua3d16, V cycle: rbase + 1109 > 512 skips level 1, levels 2 .. 4 fit
    (383 rows, 800 overflow blocks); the dense solve (40 dofs) joins the region."""
    info, _ = check('ua3d16', JAC)
    assert_resident(info, 'ua3d16')
    assert info['programs'][0]['resident_rows'] == 383 < tc.HIER['ua3d16']['levels'][1][0]


def test_deep_hierarchy_poly(lib_built):
    """ua3d12c40: levels 1 and 3 resident (475 + 35 rows; 125 does not fit
    behind 475 and is skipped while a deeper one still fits, the coarsest 9
    no longer do), POLY, W, scaling."""
    info, _ = check('ua3d12c40', dict(POLY, cycle_type='W', coarse_scaling=1))
    lv, rows, nov, _ = tc.residency('ua3d12c40')
    assert lv == [1, 3] and rows == 510
    assert_resident(info, 'ua3d12c40')


@pytest.mark.parametrize('scaling', [0, 1])
def test_no_smoothed_level_resident(lib_built, scaling):
    """sa3d24: 606 rows exceed the workgroup; only the coarsest level's A has
    rows in registers, and only the coarse scaling's q = A_c e reads them."""
    info, _ = check('sa3d24', dict(JAC, coarse_scaling=scaling) if scaling else JAC)
    p = info['programs'][0]
    assert p['res'] == 1 and p['resident_rows'] == 12 and p['nov'] == 0 and p['replanned'] == 0, p
    assert p['ops_res'] == scaling and p['ops_global'] == 3, p      # level 1's residual, R and K
    assert p['gemv'] == [(24, 'lds')], p
    assert_all_lds(info)


@pytest.mark.parametrize('kw', [JAC, SGS], ids=tc.key)
def test_region_does_not_fit(lib_built, kw):
    """sa3d20: 369 rows fit the threads, their 6256 overflow blocks do not fit
    the LDS: the residency plan is discarded and the plain program planned
    anew (its vectors all in LDS, its operators and dense inverse global)."""
    info, _ = check('sa3d20', kw)
    p = info['programs'][0]
    assert p['replanned'] == 1 and p['res'] == 0 and p['resident_rows'] == 0 and p['nov'] == 0, p
    assert p['ops_res'] == 0 and p['gemv'] == [(18, 'global')], p
    assert_all_lds(info)


@pytest.mark.parametrize('hn,dofs', [('ua3d16c200', 148), ('ua3d16c600', 578)])
def test_dense_solve_sizes(lib_built, hn, dofs):
    """T_GEMV past the LDS form (n <= 64: test_families, and global with
    MAMG_TAIL_RES=0: test_families_from_global_rows): one thread per row from
    global memory (64 < 148 <= 512) and one wave per row (578 > 512)."""
    info, _ = check(hn, JAC)
    p = info['programs'][0]
    assert p['gemv'] == [(dofs, 'global')], p
    assert p['res'] == 1 and p['resident_rows'] == tc.residency(hn)[1], p


# ---------------------------------------------------------------------------
# fp32 cycle storage above a tail
# ---------------------------------------------------------------------------
def _bits(B, l):
    s = B.level_storage(l)
    return (BIT_A if s['A'] else 0) | (BIT_KP if s['KP'] else 0) | (BIT_R if s['R'] else 0)


@pytest.mark.parametrize('apply_first', [True, False])
@pytest.mark.parametrize('kw', [JAC, dict(POLY, cycle_type='W', coarse_scaling=1)], ids=tc.key)
def test_f32_storage_above_a_tail(lib_built, kw, apply_first):
    """sa2d64c40 with the tail from level 2: set_cycle_storage('f32') narrows
    levels 0 and 1 only (the tail reads its operators as fp64), and the apply
    is the restatement with exactly those levels rounded -- with the tail
    program planned before the narrowing (apply_first) or after it."""
    hn = 'sa2d64c40'
    assert (hn, frozen(kw), 2) in tc.APPLIED_KEYS
    h = tc.oracle(hn, **kw)
    B = build(hn, kw, nodes='30')       # level 2 has 26 node rows, level 1 412
    try:
        assert B.tail_info()['tail_level'] == 2
        if apply_first:
            for seed in tc.SEEDS:
                r = tc.rhs(hn, seed)
                assert rel(B * r, h.apply(r)) < TOL_ORACLE
            assert len(B.tail_info()['programs']) >= 1
        B.set_cycle_storage('f32')
        n = B.num_levels
        assert n == 4
        assert _bits(B, 0) == ALL and _bits(B, 1) == ALL, [B.level_storage(l) for l in range(n)]
        assert _bits(B, 2) == 0 and _bits(B, 3) == 0, [B.level_storage(l) for l in range(n)]
        kform = [bool(B.level_format(l)['post_fused']) for l in range(n)]
        ref = StorageRef(h, masks=ALL, kform=kform, levels=[0, 1])
        whole = StorageRef(h, masks=ALL, kform=kform)
        for seed in tc.SEEDS:
            r = tc.rhs(hn, seed)
            z = B * r
            e, d64, dall = rel(z, ref.apply(r)), rel(z, h.apply(r)), rel(z, whole.apply(r))
            print('TAILDEV f32 %s seed %d: vs levels 0, 1 rounded %.2e, unrounded %.2e, every level rounded %.2e'
                  % (tc.key(kw), seed, e, d64, dall))
            assert e < TOL_ORACLE, e
            assert d64 > TOL_ORACLE and dall > TOL_ORACLE     # rounded above the tail, not inside it
        info = B.tail_info()
        assert len(info['programs']) == (2 if kw.get('cycle_type') == 'W' else 1), info
        for p in info['programs']:
            assert p['res'] == 1 and p['resident_rows'] == 29, p
    finally:
        B.close()


# ---------------------------------------------------------------------------
# graph replay and the device PCG with a Jacobi tail
# ---------------------------------------------------------------------------
def test_replay_and_pcg(lib_built):
    """sa2d32, Jacobi W cycle with scaling, tail from level 1: two programs
    (the second visit's (c, e) entry); graph replays are bitwise equal and
    equal the eager apply's contract; ConjGrad.solve_device matches mo.pcg."""
    import torch
    M = _mamg()
    hn, kw = 'sa2d32', dict(JAC, cycle_type='W', coarse_scaling=1)
    assert (hn, frozen(kw), 1) in tc.APPLIED_KEYS
    s = tc.system(hn)
    A = s.scipy()
    h = tc.oracle(hn, **kw)
    r = tc.rhs(hn, tc.SEEDS[0])
    zo = _oracle_apply(hn, frozen(kw))[0]
    B = build(hn, kw, A=A)       # the device PCG takes its level-0 operator from the handle built on this A
    try:
        rt = torch.as_tensor(r).cuda()
        z1 = B.matvec(rt)
        z2 = B.matvec(rt)
        torch.cuda.synchronize()
        assert torch.equal(z1, z2)
        ze = B * r
        assert rel(z1.cpu().numpy(), zo) < TOL_ORACLE and rel(ze, zo) < TOL_ORACLE
        assert rel(ze, z1.cpu().numpy()) < TOL_LAUNCH
        info = B.tail_info()
        assert info['tail_level'] == 1 and len(info['programs']) == 2, info
        assert_resident(info, hn)
        b = torch.as_tensor(r).cuda()
        x = torch.zeros_like(b)
        cg = M.ConjGrad(A, precond=B, tolerance=1e-8, maxiter=500)
        cg.solve_device(b, x)
        torch.cuda.synchronize()
        ref = mo.pcg(A, h, r, 1e-8, 500)
        assert len(cg.residuals) == len(ref.residuals)
        assert np.allclose(cg.residuals, ref.residuals, rtol=1e-6, atol=0)
        assert rel(x.cpu().numpy(), ref.x) < 1e-6
        assert len(B.tail_info()['programs']) == 2
    finally:
        B.close()
