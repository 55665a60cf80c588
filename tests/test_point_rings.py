"""Seed-ring Schwarz on hierarchies of the CSR layout (Schwarz_type RINGS = 8 on
a scalar system, or a nodal one with point smoothers; DESIGN.md section
2.12.1): what the CPU restatement (tests/pointrings_ref.py) and the host side
decide, without a device.  The hierarchy is the Schwarz_levels 0 one bit for
bit, the effective parameters keep RINGS, every refusal keeps its message, the
.dat mapping has a multiplicative mode and the 3D-1D drivers take -schwarz.
The GPU parity is tests/test_gpu_point_rings.py."""
import functools
import os

import numpy as np
import pytest

import mamg_oracle as mo
import pointrings_ref as rr

HERE = os.path.dirname(os.path.abspath(__file__))


def _mamg():
    import metric_amg_examples_amd as M
    return M


@functools.lru_cache(maxsize=None)
def small():
    """emi_3d1d n = 8 (N = 737, 8 seeds) and its restatement, SGS below the rings"""
    s = _mamg().problems.emi_3d1d(8, 1e6, 0.0)
    A = s.scipy()
    return s, A, rr.PointRings(A, s.idofs, 'SGS', num_functions=1, Schwarz_maxlvl=2, Schwarz_mmsize=200)


# ---- the restatement's own properties --------------------------------------
def test_rest_colours_are_valid_on_the_filtered_graph():
    s, A, R = small()
    F, c, cov = R.F, R.rest_colour, R.cov
    assert len(R.rings.blocks) == 8 and R.rings.ncolours == 8 and len(R.rest_rows) == 9
    rows = np.repeat(np.arange(F.shape[0]), np.diff(F.indptr))
    assert not cov[rows].any() and not cov[F.indices].any()          # covered rows emptied, covered columns dropped
    assert (c[rows] != c[F.indices]).all()                            # no edge inside a colour
    listed = np.concatenate(R.rest_rows)
    assert np.array_equal(np.sort(listed), np.flatnonzero(~cov))      # every uncovered row once, no covered row
    # every entry of A between two uncovered rows is an edge of the filtered graph
    G = rr.pr.offdiag_pattern(A)
    gr = np.repeat(np.arange(G.shape[0]), np.diff(G.indptr))
    keep = ~cov[gr] & ~cov[G.indices]
    assert int(keep.sum()) == F.nnz


def test_rest_sweeps_leave_covered_dofs_alone():
    s, A, R = small()
    b = mo.seeded_rhs(s.N, 7)
    x0 = mo.seeded_rhs(s.N, 8)
    for fwd in (True, False):
        x = R.rest_sweep(x0.copy(), b, fwd)
        assert np.array_equal(x[R.cov], x0[R.cov])
        assert not np.array_equal(x[~R.cov], x0[~R.cov])


@pytest.mark.parametrize('cycle', ['V', 'W'])
@pytest.mark.parametrize('smoother', ['SGS', 'JACOBI_RHO'])
def test_operator_is_symmetric_without_scaling(cycle, smoother):
    s = _mamg().problems.emi_3d1d(8, 1e6, 0.0)
    A = s.scipy()
    R = rr.PointRings(A, s.idofs, smoother, num_functions=1, Schwarz_maxlvl=2, Schwarz_mmsize=200,
                      cycle_type=cycle, coarse_dof=20)
    assert len(R.levels) >= 3
    u, v = mo.seeded_rhs(s.N, 1), mo.seeded_rhs(s.N, 2)
    a, c = float(u @ R.apply(v)), float(v @ R.apply(u))
    # the bound of the GPU test (tests/test_gpu_point_rings.py): the exact local
    # solves at gamma = 1e6 lose more digits than a point sweep does
    assert abs(a - c) <= 1e-10 * abs(a)


def test_colour_order_is_a_sequential_block_order():
    """blocks of one colour do not interact, so the colour sweep equals the
    blocks taken one at a time in (colour, seed) order"""
    M = _mamg()
    s = M.problems.bidomain(2, 16, 1.0)
    A = s.scipy()
    seeds = np.arange(5, s.N, 37, dtype=np.int32)
    rings = mo.Rings(A, seeds, 2, 100)
    assert rings.ncolours < len(rings.blocks)                         # some colour holds several blocks
    b, x0 = mo.seeded_rhs(s.N, 3), mo.seeded_rhs(s.N, 4)
    order = np.argsort(rings.colour, kind='stable')
    for fwd in (True, False):
        x = rings.sweep(A, x0.copy(), b, fwd)
        y = x0.copy()
        for k in (order if fwd else order[::-1]):
            blk = rings.blocks[k]
            y[blk] += rings.Minv[k] @ (b[blk] - A[blk] @ y)
        assert np.linalg.norm(x - y) <= 1e-13 * np.linalg.norm(x)


# ---- the host setup ---------------------------------------------------------
def _level_equal(a, b):
    assert set(a) == set(b)
    for k in a:
        if isinstance(a[k], tuple):
            for u, v in zip(a[k][:3], b[k][:3]):
                assert np.array_equal(u, v), k
            assert a[k][3] == b[k][3]
        elif isinstance(a[k], np.ndarray):
            assert np.array_equal(a[k], b[k]), k
        else:
            assert a[k] == b[k], k


def test_hierarchy_builds_on_a_scalar_system(lib_built):
    M = _mamg()
    s, A, R = small()
    H = M.HostHierarchy(A, idofs=s.idofs, parameters=M.parameters.parameters_metric_3d1d_rings)
    assert H.num_levels == 2
    ep = H.effective_params
    assert ep['Schwarz_type'] == M.parameters.SCHWARZ_RINGS and ep['Schwarz_levels'] == 1


@pytest.mark.parametrize('kw', [
    dict(num_functions=1),                                                       # Jacobi-rho below the rings
    dict(num_functions=1, smoother=14, AMG_type=1, cycle_type=2, aggregation_type=5),
    dict(num_functions=1, smoother=13),
    dict(num_functions=1, smoother=12),
    dict(num_functions=2, node_block_smoother=0),
    dict(num_functions=2, smoother=14),
])
def test_hierarchy_is_the_schwarz_levels_0_one(lib_built, kw):
    M = _mamg()
    P = M.parameters
    s = M.problems.bidomain(2, 16, 1e2)
    A = s.scipy()
    seeds = np.arange(5, s.N, 37, dtype=np.int32)
    base = dict(Schwarz_maxlvl=2, Schwarz_mmsize=100, **kw)
    H = M.HostHierarchy(A, idofs=seeds, Schwarz_levels=1, Schwarz_type=P.SCHWARZ_RINGS, **base)
    Z = M.HostHierarchy(A, Schwarz_levels=0, **base)
    assert H.num_levels == Z.num_levels >= 2
    for l in range(H.num_levels):
        a, b = H.level(l), Z.level(l)
        assert 'WB' not in a
        _level_equal(a, b)
    ep = H.effective_params
    assert ep['Schwarz_type'] == P.SCHWARZ_RINGS and ep['Schwarz_levels'] == 1
    assert ep['smoother'] == kw.get('smoother', P.SMOOTHER_JACOBI_RHO)
    if kw.get('smoother') in (13, 14):               # for a point-GS smoother: the JACOBI_RHO hierarchy, as before
        J = M.HostHierarchy(A, Schwarz_levels=0, **dict(base, smoother=P.SMOOTHER_JACOBI_RHO, node_block_smoother=0))
        for l in range(H.num_levels):
            _level_equal(H.level(l), J.level(l))
        assert ep['node_block_smoother'] == 0


def test_rings_without_seeds_resolve_to_no_schwarz_level(lib_built):
    M = _mamg()
    s = M.problems.bidomain(2, 16, 1e2)
    H = M.HostHierarchy(s.scipy(), parameters=M.parameters.parameters_metric_3d1d_rings)
    assert H.effective_params['Schwarz_levels'] == 0 and H.num_levels >= 2


# ---- refusals that stay -----------------------------------------------------
def _refused(M, A, code=-4, **kw):
    with pytest.raises(M._lib.MamgError) as ei:
        M.HostHierarchy(A, **kw)
    assert ei.value.code == code and len(str(ei.value)) > 20
    return str(ei.value)


def test_refusals(lib_built):
    M = _mamg()
    P = M.parameters
    s, A, R = small()
    rings = dict(P.parameters_metric_3d1d_rings)
    # the reference's names with rings on a scalar system: refused, and the message names the way in
    for t in (P.SCHWARZ_SYMMETRIC, P.SCHWARZ_FORWARD, P.SCHWARZ_BACKWARD):
        msg = _refused(M, A, idofs=s.idofs, parameters=dict(rings, Schwarz_type=t))
        assert 'SCHWARZ_RINGS' in msg and 'SCHWARZ_ADDITIVE' in msg
    # point GS with seeds and any other Schwarz_type
    for t in (P.SCHWARZ_BLOCK_JACOBI, P.SCHWARZ_ADDITIVE, P.SCHWARZ_SEED_BLOCKS):
        msg = _refused(M, A, idofs=s.idofs, parameters=dict(rings, Schwarz_type=t, smoother=P.SMOOTHER_SGS_POINT,
                                                             Schwarz_maxlvl=2 if t == P.SCHWARZ_ADDITIVE else 1))
        assert 'Schwarz_levels 0' in msg and 'SCHWARZ_RINGS' in msg
    # the existing bounds
    msg = _refused(M, A, idofs=s.idofs, parameters=dict(rings, Schwarz_mmsize=257))
    assert 'Schwarz_mmsize' in msg
    many = np.arange(s.N, dtype=np.int32).repeat(200)[:120000]          # 120000 x 200^2 > 4e9
    msg = _refused(M, A, idofs=many, parameters=rings)
    assert 'sparse seed sets' in msg
    _refused(M, A, code=-1, idofs=np.array([s.N], np.int32), parameters=rings)         # seed out of range
    _refused(M, A, idofs=s.idofs, parameters=dict(rings, Schwarz_maxlvl=0))
    _refused(M, A, idofs=s.idofs, parameters=dict(rings, Schwarz_levels=2))
    # node-block GS / SGS stay node-block smoothers
    _refused(M, A, idofs=s.idofs, parameters=dict(rings, smoother=P.SMOOTHER_SGS))
    # more than two functions
    msg = _refused(M, mo.laplace1d(300), idofs=np.array([3], np.int32), parameters=dict(rings, num_functions=3))
    assert 'num_functions 1 or 2' in msg


def test_multi_gpu_refused(lib_built):
    """the N-GPU path has no CSR hierarchies: refused before a rank touches its GPU"""
    M = _mamg()
    s, A, R = small()
    for extra in (dict(), dict(smoother=M.parameters.SMOOTHER_SGS_POINT)):
        with pytest.raises(M._lib.MamgError) as ei:
            M.DistMetricAMG(A, None, idofs=s.idofs, parameters=dict(M.parameters.parameters_metric_3d1d_rings, **extra),
                            rank=0, nranks=2, comm_id=None)
        assert ei.value.code == -4 and 'multi-GPU' in str(ei.value)


# ---- Python: .dat mapping, preset, drivers ----------------------------------
def test_dat_mapping_in_both_modes():
    M = _mamg()
    P = M.parameters
    d = M.fileio.read_dat(os.path.join(HERE, 'golden', 'solver_3d1d.dat'))
    add, solver, notes = M.fileio.dat_to_parameters(d)
    assert M.fileio.dat_to_parameters(d, multiplicative=False) == (add, solver, notes)
    assert add['Schwarz_type'] == P.SCHWARZ_ADDITIVE and add['smoother'] == P.SMOOTHER_JACOBI_RHO
    assert add['relaxation'] == 4.0 / 3.0
    mul, solver2, notes2 = M.fileio.dat_to_parameters(d, multiplicative=True)
    assert solver2 == solver
    assert mul['Schwarz_type'] == P.SCHWARZ_RINGS and mul['Schwarz_levels'] == 1
    assert mul['Schwarz_maxlvl'] == 2 and mul['Schwarz_mmsize'] == 200             # the same blocks
    assert mul['smoother'] == P.SMOOTHER_GS_POINT and mul['relaxation'] == 1.0     # relaxation does not enter
    assert 'num_functions' not in mul
    assert {k: v for k, v in mul.items() if k not in ('Schwarz_type', 'smoother', 'relaxation')} == \
        {k: v for k, v in add.items() if k not in ('Schwarz_type', 'smoother', 'relaxation')}
    assert any("colour order instead of HAZmath's sequential seed and dof order" in n for n in notes2)
    assert any('SMOOTHER_GS_POINT' in n for n in notes2) and not any('relaxation 1.0 ->' in n for n in notes2)
    P.make_params(mul)
    sgs = M.fileio.dat_to_parameters(dict(d, AMG_smoother='SGS'), multiplicative=True)[0]
    assert sgs['smoother'] == P.SMOOTHER_SGS_POINT
    with pytest.raises(ValueError):
        M.fileio.dat_to_parameters(dict(d, Schwarz_type=1), multiplicative=True)    # forward-only: not built


def test_preset_and_driver_option():
    M = _mamg()
    P = M.parameters
    from metric_amg_examples_amd import drivers as D
    assert P.parameters_metric_3d1d_rings == dict(P.parameters_metric_3d1d, Schwarz_type=P.SCHWARZ_RINGS)
    assert P.parameters_metric_3d1d['Schwarz_type'] == P.SCHWARZ_ADDITIVE          # the default preset is unchanged
    for parser in (D.emi_3d1d_parser, D.run_solver_3d1d_parser, D.emi_3d1d_sweep_parser):
        assert parser().parse_known_args([])[0].schwarz == 'additive'              # no default changes
        assert parser().parse_known_args(['-schwarz', 'rings'])[0].schwarz == 'rings'
        with pytest.raises(SystemExit):
            parser().parse_known_args(['-schwarz', 'symmetric'])
    assert D._params_3d1d('additive') is P.parameters_metric_3d1d
    assert D._params_3d1d('rings') is P.parameters_metric_3d1d_rings
