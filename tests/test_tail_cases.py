"""The inputs of tests/test_gpu_tail.py do what those tests rely on, checked
with the CPU oracle alone (tests/tail_cases.py).  These are conditions on the
inputs, not measurements: a case that misses one is replaced, the margin
stays."""
import numpy as np
import pytest

import tail_cases as tc


@pytest.mark.parametrize('name', sorted(tc.HIER))
def test_level_sizes(lib_built, name):
    """Node rows, longest and mean node row of every level's A, and the dofs
    of the coarsest level: what the planner's decisions depend on."""
    hc = tc.HIER[name]
    facts = tc.level_facts(name)
    print(name, facts)
    assert facts == hc['levels']
    h = tc.oracle(name)
    assert h.levels[-1].Ainv is not None and h.levels[-1].Ainv.shape[0] == 2 * hc['levels'][-1][0]
    assert all(lev.Ainv is None for lev in h.levels[:-1])
    assert len(h.levels) >= 3                              # level 1 is smoothed: the tail may start there


def test_resident_overflow_case(lib_built):
    """sa3d16: level 1 fully resident with rows far past RES_RB, its region in
    the LDS; pick_lanes_bsr gives its A 16 lanes (lanes double while 2 * lanes <= mean: 16 <= 25.5 < 32),
    so MAMG_TAIL_VL 1/2/4/8/64 run 1/2/4/8/16 lanes; dense solve of 14 dofs."""
    lv, rows, nov, region = tc.residency('sa3d16')
    assert lv == [1, 2] and rows == 206 and nov == 2988
    assert tc.HIER['sa3d16']['levels'][1][1] > 3 * tc.RES_RB
    assert region + 14 * 14 * 8 + 16 < tc.TAIL_LDS_MAX
    mean = tc.HIER['sa3d16']['levels'][1][2]
    assert 16 <= mean < 32


def test_two_resident_levels_case(lib_built):
    """sa2d64c40: levels 1 and 2 (and the coarsest) resident together, short
    rows with a few overflow blocks."""
    lv, rows, nov, region = tc.residency('sa2d64c40')
    assert lv == [1, 2, 3] and rows == 412 + 26 + 3 and nov == 240
    assert max(m for _, m, _ in tc.HIER['sa2d64c40']['levels'][1:]) <= 17


def test_non_resident_above_resident_case(lib_built):
    """ua3d16 from level 1: 1109 rows cannot be resident, the levels below are;
    the work vectors of a W cycle with two sweeps and coarse scaling (b, x, t,
    t2, r on level 1; these and c, e, q on levels 2 and 3) exceed what the
    region and the dense inverse leave of the LDS, while any one fits."""
    lv, rows, nov, region = tc.residency('ua3d16')
    assert lv == [2, 3, 4] and rows == 289 + 74 + 20 and nov == 800
    n1, n2, n3, n4 = (2 * lv[0] for lv in tc.HIER['ua3d16']['levels'][1:])
    left = tc.TAIL_LDS_MAX - region - 8 * n4 * n4 - 16
    assert 8 * (5 * n1 + 8 * n2 + 8 * n3) > left       # not all of them: some operands stay global
    assert 8 * n1 < left                               # the largest alone does: some are in LDS


def test_no_resident_smoothed_level_case(lib_built):
    """sa3d24: level 1 has more rows than the workgroup has threads; only the
    coarsest level's A (12 rows, read by the coarse scaling alone) is resident."""
    lv, rows, nov, region = tc.residency('sa3d24')
    assert lv == [2] and rows == 12 and nov == 0
    assert tc.HIER['sa3d24']['levels'][1][0] > tc.TAIL_THREADS


def test_region_case(lib_built):
    """The smallest 3-D SA grid between n = 18 and 22 whose level 1 has at most
    512 rows and an LDS region (block inverses + overflow blocks at 34 B) past
    TAIL_LDS_MAX is n = 20: the residency plan is made, then discarded."""
    lv, rows, nov, region = tc.residency('sa3d20')
    assert lv == [1, 2] and rows == 369 and nov == 6256
    assert region > tc.TAIL_LDS_MAX
    # n = 18 (268 rows, 4240 overflow blocks with gamma = 1e4) stays below it
    assert tc.GD_BYTES + 34 * 4240 < tc.TAIL_LDS_MAX


def test_dense_cases():
    """The coarsest sizes of the three T_GEMV branches, each below a smoothed tail level."""
    dofs = {n: 2 * tc.HIER[n]['levels'][-1][0] for n in tc.HIER}
    assert dofs['sa3d16'] == 14 and dofs['sa3d24'] == 24 and dofs['ua3d16'] == 40       # <= 64: may join the LDS region
    assert 64 < dofs['ua3d16c200'] == 148 <= tc.TAIL_THREADS                              # thread per row, global
    assert dofs['ua3d16c600'] == 578 > tc.TAIL_THREADS                                    # wave per row
    assert len(tc.HIER['ua3d16c200']['levels']) == 4 and len(tc.HIER['ua3d16c600']['levels']) == 3


@pytest.mark.parametrize('hn,kw,tl', tc.APPLIED, ids=['%s-%s-%d' % (hn, tc.key(kw), tl) for hn, kw, tl in tc.APPLIED])
def test_rhs_is_sensitive_to_the_tail(lib_built, hn, kw, tl):
    """Dropping the correction from tail_level down moves the apply by at least
    1e-4 relative for every right-hand side the GPU tests use: a tail that
    returned zeros or stale LDS cannot meet their 1e-10."""
    h = tc.oracle(hn, **kw)
    cut = tc.NoTail(h, tl)
    for seed in tc.SEEDS:
        r = tc.rhs(hn, seed)
        d = tc.rel(cut.apply(r), h.apply(r))
        print(hn, kw, 'seed', seed, 'without the tail: %.3e' % d)
        assert np.isfinite(d) and d >= 1e-4
