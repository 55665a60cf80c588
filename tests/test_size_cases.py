"""The inputs of tests/test_gpu_sizes.py (tests/size_cases.py) are what those
tests rely on, checked without a GPU: the generators' invariants, the residue
classes the size lists stand for, the oracle's level sizes, host setup =
oracle bit for bit at every size, and the reference's own sensitivity to
summation order (numpy oracle against the C cycle, oracle/vcycle_ref.c), which
is what entitles every case to APPLY_TOL = 1e-10."""
import dataclasses

import numpy as np
import pytest

import irregular
import mamg_oracle as mo
import size_cases as sc
from test_host_setup import assert_equals_oracle, to_c

NODAL = sc.nodal_cases()
ALL_M = [m for _, m in NODAL]


def _bitwise_symmetric(A):
    T = A.T.tocsr()
    T.sort_indices()
    return (np.array_equal(A.indptr, T.indptr) and np.array_equal(A.indices, T.indices)
            and np.array_equal(A.data, T.data))


def _sorted_rows(A):
    rows = np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))
    return A.has_sorted_indices and bool(np.all(np.diff(A.indices)[np.diff(rows) == 0] > 0))


# ---------------------------------------------------------------------------
# generator invariants
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('family,m', NODAL, ids=[sc.case_id(c) for c in NODAL])
def test_truncated_invariants(family, m):
    """2m x 2m, A == A^T bitwise, sorted int64 CSR, equal off-diagonal field
    blocks, a positive diagonal, Cholesky for m <= 513, and the half-symmetric
    padding rule accepts it (so MAMG_SELL_MIN_ROWS=1 gives the half layout)."""
    A, nv, idofs = sc.nodal(family, m)
    assert nv == m and A.shape == (2 * m, 2 * m)
    assert A.indptr.dtype == np.int64 and _sorted_rows(A) and _bitwise_symmetric(A)
    B01, B10 = A[:m, m:].tocsr(), A[m:, :m].tocsr()
    assert np.array_equal(B01.indices, B10.indices) and np.array_equal(B01.data, B10.data)
    assert np.array_equal(idofs, np.arange(m, 2 * m)) and A.diagonal().min() > 0
    if m <= 513:
        np.linalg.cholesky(A.toarray())
    ok, detail, sell_ok = irregular.half_rule(A, m)
    assert ok and sell_ok, detail
    # the principal submatrix it claims to be
    dim, n, g, _ = sc.FAMILIES[family]
    F = mo.bidomain_system(dim, n, g)['A'].tocsr()
    nv0 = F.shape[0] // 2
    assert A[m - 1, 2 * m - 1] == F[m - 1, nv0 + m - 1] and A[0, 0] == F[0, 0]


@pytest.mark.parametrize('k', sc.SCALAR)
def test_truncated_rows_invariants(k):
    A = sc.scalar(k)
    assert A.shape == (k, k) and A.indptr.dtype == np.int64
    assert _sorted_rows(A) and _bitwise_symmetric(A) and A.diagonal().min() > 0
    F = mo.bidomain_system(*sc.SCALAR_GRID)['A'].tocsr()
    assert np.array_equal(A[k - 1].toarray(), F[k - 1, :k].toarray())
    if k <= 1025:
        np.linalg.cholesky(A.toarray())


def test_stencil3d_rows_reach_15_blocks():
    """The 3-D family is there for its long rows; its first 81 nodes are the Dirichlet plane."""
    import tail_cases
    longest = {m: int(tail_cases.row_blocks(sc.nodal('stencil3d', m)[0]).max()) for m in sc.STENCIL3D}
    print(longest)
    assert max(longest.values()) == 15 and min(longest.values()) > 7        # 7: the 2-D families' longest row
    assert min(sc.STENCIL3D) > 81 and bool(mo.bidomain_system(3, 8, 1e6)['bc'][:81].all())


# ---------------------------------------------------------------------------
# coverage: which boundary classes the lists hold
# ---------------------------------------------------------------------------
def test_size_lists_cover_the_boundary_classes():
    """Computed from the lists, so a later edit cannot quietly drop a class."""
    assert sc.TINY == [1, 2, 3, 7, 8, 9]
    assert {0, 1, 31, 32, 33, 63} <= {m % 64 for m in ALL_M}
    assert {0, 1, 255} <= {m % 256 for m in ALL_M}
    assert {0, 1, 127} <= {m % 128 for m in ALL_M}
    assert {m % 2 for m in ALL_M} == {0, 1}
    assert any(m < 8 for m in ALL_M) and any(8 <= m < 32 for m in ALL_M) and any(32 <= m < 64 for m in ALL_M)
    assert {4096, 4097} <= set(sc.SCALAR) and sc.GS_SMALL_MAX_ROWS == 4096
    assert {k % 2 for k in sc.SCALAR} == {0, 1}
    # the patch-inverse kernels' patches per wave: 0, 1, 7 mod 8 and 0, 1, 3 mod 4
    assert {0, 1, 7} <= {m % 8 for m in sc.SMOOTHER_SIZES} and {0, 1, 3} <= {m % 4 for m in sc.SMOOTHER_SIZES}
    # the subsets name sizes that exist
    have = set(ALL_M)
    assert sc.WP_SIZES <= have and sc.VARIANT_SIZES <= have and sc.SMOOTHER_SIZES <= have
    # every multiple of 64 has both neighbours
    for m in ALL_M:
        if m % 64 == 0 and m != 192:
            assert m - 1 in have and m + 1 in have, m
    assert 191 in have


# ---------------------------------------------------------------------------
# the oracle's level sizes
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('family,m', NODAL, ids=[sc.case_id(c) for c in NODAL])
def test_level_sizes(family, m):
    h = sc.oracle(family, m)
    dofs = sc.level_dofs(h)
    print(family, m, dofs)
    assert dofs == sc.HIER[(family, m)]
    assert (len(dofs) == 1) == (m <= 2)                    # only m = 1, 2 are one dense level
    assert h.levels[-1].Ainv is not None and all(lv.Ainv is None for lv in h.levels[:-1])
    r = mo.seeded_rhs(2 * m)
    z = h.apply(r)
    assert np.isfinite(z).all() and r @ z > 0


@pytest.mark.parametrize('k', sc.SCALAR)
def test_level_sizes_scalar(k):
    dofs = sc.level_dofs(sc.oracle_scalar(k))
    print('scalar', k, dofs)
    assert dofs == sc.HIER_SCALAR[k]
    assert (dofs[0] <= sc.GS_SMALL_MAX_ROWS) == (k <= 4096) and all(d <= sc.GS_SMALL_MAX_ROWS for d in dofs[1:])


# ---------------------------------------------------------------------------
# host setup = oracle, bit for bit
# ---------------------------------------------------------------------------
PARAM_CASES = [(f, m, kw) for f, m in NODAL for kw in irregular.PARAM_SETS
               if not kw or m in sc.SMOOTHER_SIZES]        # 63 / 64 / 65 and both families' 255 / 256 / 257


@pytest.mark.parametrize('family,m,kw', PARAM_CASES,
                         ids=['%s-%d-%s' % (f, m, irregular.param_id(kw)) for f, m, kw in PARAM_CASES])
def test_host_setup_bitwise_equals_oracle(lib_built, family, m, kw):
    import metric_amg_examples_amd as M
    A, nv, idofs = sc.nodal(family, m)
    H = M.HostHierarchy(A, idofs=idofs, **to_c(dict(kw, num_functions=2, coarse_dof=sc.COARSE_DOF)))
    try:
        assert_equals_oracle(H, sc.oracle(family, m, **kw))
    finally:
        H.close()


@pytest.mark.parametrize('k', sc.SCALAR)
def test_host_setup_bitwise_equals_oracle_scalar(lib_built, k):
    import metric_amg_examples_amd as M
    H = M.HostHierarchy(sc.scalar(k), idofs=None, num_functions=1, coarse_dof=sc.COARSE_DOF)
    try:
        assert_equals_oracle(H, sc.oracle_scalar(k))
    finally:
        H.close()


# ---------------------------------------------------------------------------
# the reference's own sensitivity to summation order
# ---------------------------------------------------------------------------
SENS_BOUND = 1e-13 * 10     # measured at most 1.2e-13; a factor 100 below APPLY_TOL


@pytest.mark.parametrize('family', list(sc.FAMILIES) + ['scalar'])
def test_reference_sensitivity_to_summation_order(lib_built, family):
    """Relative difference between the numpy oracle's apply and the C cycle on
    the same hierarchy, V / W x JACOBI_RHO / POLY x two seeds, maximum over the
    family's sizes: printed, and at most 1e-13 times a margin of 10, so that
    APPLY_TOL = 1e-10 keeps two orders of magnitude on every case."""
    import cref
    worst, where = 0.0, None
    sizes = sc.SCALAR if family == 'scalar' else sc.FAMILIES[family][3]
    for m in sizes:
        for smoother in ('JACOBI_RHO', 'POLY'):
            for cycle in ('V', 'W'):
                h = sc.oracle_scalar(m, cycle, smoother) if family == 'scalar' else sc.oracle(family, m, cycle, smoother)
                c = cref.from_oracle(h)
                for seed in sc.SEEDS:
                    r = mo.seeded_rhs(h.levels[0].A.shape[0], seed)
                    z = h.apply(r)
                    d = np.linalg.norm(z - c.apply(r)) / np.linalg.norm(z)
                    if d > worst:
                        worst, where = d, (m, cycle, smoother, seed)
    print('sensitivity', family, '%.2e' % worst, 'at', where)
    assert worst <= SENS_BOUND, (worst, where)
