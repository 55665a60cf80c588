"""Host setup = oracle, bit for bit, on graphs that are not grids in grid
order (tests/irregular.py): randomly renumbered 2-D / 3-D bidomain systems, a
hub node with 500 neighbours, ragged row lengths.  Drives MIS-2 and HEM hash
tie-breaking, the strength filter, SA smoothing and the Galerkin products of
csrc/setup.cpp on rows whose neighbours are scattered over the whole column
range and whose lengths differ by two orders of magnitude.  CPU only: a GPU
mismatch on these inputs is the device's when this file passes."""
import numpy as np
import pytest

import irregular
import mamg_oracle as mo
from test_host_setup import assert_equals_oracle, to_c

GENERATORS = irregular.SMALL      # 2-D n = 32 and 64, 3-D n = 8, hub m = 500, ragged


@pytest.mark.parametrize('name', list(GENERATORS))
def test_generator_is_bitwise_symmetric(name):
    """A == A^T bitwise, sorted field-major CSR, symmetric 2x2 node blocks and
    a positive diagonal: the half-symmetric layout can then only be refused by
    its length or padding rules."""
    A, nv, idofs = GENERATORS[name]()
    assert A.shape == (2 * nv, 2 * nv) and A.has_sorted_indices
    assert np.all(np.diff(A.indices)[np.diff(np.repeat(np.arange(2 * nv), np.diff(A.indptr))) == 0] > 0)
    T = A.T.tocsr()
    T.sort_indices()
    assert np.array_equal(A.indptr, T.indptr) and np.array_equal(A.indices, T.indices)
    assert np.array_equal(A.data, T.data)
    # node blocks: A[i, nv + j] == A[nv + i, j]  <=>  the two off-diagonal field blocks are equal
    B01, B10 = A[:nv, nv:].tocsr(), A[nv:, :nv].tocsr()
    assert np.array_equal(B01.indices, B10.indices) and np.array_equal(B01.data, B10.data)
    assert np.array_equal(idofs, np.arange(nv, 2 * nv))
    assert A.diagonal().min() > 0


def test_generators_break_the_grid_properties():
    """What the generators are for: long rows, unequal row halves, columns far
    from the row."""
    A, nv, _ = irregular.hub(32, 1e3, 500, 1.0, 4)
    assert np.diff(A.indptr).max() > 500
    A, nv, _ = irregular.ragged(64, 1e3, 7)
    ln = np.diff(A[:nv, :nv].tocsr().indptr)
    sl = ln[:nv // 64 * 64].reshape(-1, 64)
    assert ln.max() >= 2 * np.median(ln) and (sl.max(axis=1) - sl.min(axis=1)).min() >= 4
    A, nv, _ = irregular.permuted(2, 64, 1e4, 2)
    G = A[:nv, :nv].tocoo()
    assert np.abs(G.row - G.col).mean() > nv / 8


@pytest.mark.parametrize('kw', irregular.PARAM_SETS, ids=irregular.param_id)
@pytest.mark.parametrize('name', list(GENERATORS))
def test_host_setup_bitwise_equals_oracle(lib_built, name, kw):
    """M.HostHierarchy == mo.setup on every level (aggregates, P, R, smoother
    blocks, coarse operators, coarsest inverse), and the oracle's PCG with
    that hierarchy converges."""
    import metric_amg_examples_amd as M
    A, nv, idofs = GENERATORS[name]()
    kw = dict(kw, num_functions=2)
    H = M.HostHierarchy(A, idofs=idofs, **to_c(kw))
    h = mo.setup(A, mo.Params(**kw), idofs=idofs)
    assert len(h.levels) >= 2
    assert_equals_oracle(H, h)
    H.close()
    maxiter = 300
    ref = mo.pcg(A, h, mo.seeded_rhs(A.shape[0]), 1e-8, maxiter)
    print(name, kw, 'levels', [lv.A.shape[0] for lv in h.levels], 'iters', ref.niters)
    assert ref.niters < maxiter


# ---------------------------------------------------------------------------
# what tests/test_gpu_irregular.py expects of its inputs, checked without a GPU
# ---------------------------------------------------------------------------
def test_half_rule_cases_cover_both_outcomes():
    """The half-symmetric layout's padding / length rule (try_half,
    csrc/device.hip) evaluated in numpy: the unpermuted grids are accepted
    (controls), permuted2d-32 is an irregular input it accepts (the 4096-slot
    allowance covers its padding), the other renumbered grids and the ragged
    graphs are rejected by the padding rule, and so is hub32-m500, whose
    longest row parts (254 upper, 251 lower blocks) just fit the 8-bit part
    lengths; the larger hubs are rejected by the 255-block row part."""
    got = {k: irregular.half_rule(*g()[:2]) for k, g in irregular.RULE_CASES.items()}
    for k, (ok, d, sell_ok) in got.items():
        print(k, ok, d)
        assert sell_ok, k
    assert got['grid2d-64'][0] and got['grid3d-16'][0]
    assert got['permuted2d-32'][0]
    for k in ('permuted2d-64', 'permuted3d-8', 'permuted3d-16', 'permuted2d-256', 'ragged32', 'ragged64',
              'ragged96', 'hub32-m500'):
        assert not got[k][0] and not got[k][1]['too_long'], k          # the padding rule
    assert 250 < got['hub32-m500'][1]['max_upper'] <= 255
    for k in ('hub96-m3000', 'hub64-m500'):
        assert not got[k][0] and got[k][1]['too_long'], k              # the length rule


@pytest.mark.parametrize('name,n,kw,lo,hi', [('hub32-m500', 32, {}, 128, 512),
                                             ('hub64-m500', 64, {}, 512, 2048),
                                             ('hub64-m500', 64, dict(strong_coupled=0.25), 512, 2048),
                                             ('hub96-m3000', 96, {}, 512, 2048),
                                             ('hub96-m3000-theta0.25', 96, dict(strong_coupled=0.25), 2048, 1 << 30)])
def test_hub_rows_reach_the_spgemm_tiers(name, n, kw, lo, hi):
    """Distinct columns of the hub's row of A P on the oracle's hierarchy:
    which hash tier of the GPU setup's SpGEMM (128 / 512 / 2048 slots,
    csrc/gsetup.hip) each hub input drives, and which one overflows."""
    A, nv, idofs = (irregular.SMALL.get(name) or irregular.CASES[name][0])()
    h = mo.setup(A, mo.Params(num_functions=2, **kw), idofs=idofs)
    c = irregular.hub_node(n)
    widest, hub_row = irregular.spgemm_rows(h, rows=[c, nv + c])
    print(name, kw, 'hub row of A P', hub_row, 'widest product row', widest)
    assert lo < hub_row <= hi
    assert widest <= hi


def test_indefinite_patch_reaches_the_patch_inversion(lib_built):
    """irregular.indefinite_patch_system passes the host setup (no earlier
    'not SPD' from the smoother blocks or the coarsest inverse), and the
    oracle's patch inversion rejects it with a non-positive Gauss-Jordan
    pivot; 289 patches leave dead waves in the last workgroup."""
    import metric_amg_examples_amd as M
    A, nv, idofs = irregular.indefinite_patch_system()
    assert nv % 4 == 1 and nv % 8 == 1
    H = M.HostHierarchy(A, idofs=idofs, num_functions=2, Schwarz_type=6)
    assert H.num_levels >= 2
    H.close()
    with pytest.raises(np.linalg.LinAlgError, match='non-positive pivot'):
        mo.Patches(A, idofs)


def test_long_row_case_matches_oracle_on_the_host(lib_built):
    """The 66008-entry row (hub with 66000 weak edges, unsmoothed
    aggregation): host setup = oracle bit for bit."""
    import metric_amg_examples_amd as M
    A, nv, idofs = irregular.LONG_ROW[0]()
    kw = dict(irregular.LONG_ROW[1], num_functions=2)
    assert np.diff(A[:nv, :nv].tocsr().indptr).max() > 65535
    H = M.HostHierarchy(A, idofs=idofs, **to_c(kw))
    assert_equals_oracle(H, mo.setup(A, mo.Params(**kw), idofs=idofs))
    H.close()
