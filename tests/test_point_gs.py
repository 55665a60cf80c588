"""Point-wise multicolour GS / SGS (SMOOTHER_GS_POINT = 13, SMOOTHER_SGS_POINT =
14): what the host side decides, without a device.  The hierarchy is the point
JACOBI_RHO one bit for bit, node_block_smoother resolves to 0, level-0 seeds
are refused, and the hazmath tags of the reference's bidomain drivers
(src/bidomain_2d.py:122-123, src/bidomain_3d.py:70-71) reach the point-wise
AMG factory.  The GPU parity is tests/test_gpu_point_gs.py."""
import numpy as np
import pytest


def _mamg():
    import metric_amg_examples_amd as M
    return M


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


@pytest.mark.parametrize('smoother', [13, 14])
@pytest.mark.parametrize('kw', [
    dict(num_functions=1),
    dict(num_functions=2),                                  # nodal aggregates, point sweeps
    dict(num_functions=1, AMG_type=1, cycle_type=2, aggregation_type=1, strong_coupled=0.1, coarse_scaling=1,
         relaxation=1.2, Schwarz_levels=0),                 # parameters_standard
])
def test_hierarchy_is_the_point_jacobi_rho_one(lib_built, smoother, kw):
    M = _mamg()
    s = M.problems.bidomain(2, 16, 1e2)
    A = s.scipy()
    H = M.HostHierarchy(A, smoother=smoother, **kw)
    J = M.HostHierarchy(A, smoother=M.parameters.SMOOTHER_JACOBI_RHO, node_block_smoother=0, **kw)
    assert H.num_levels == J.num_levels >= 2
    for l in range(H.num_levels):
        a, b = H.level(l), J.level(l)
        assert 'WB' not in a and (l == H.num_levels - 1 or 'winv' in a)
        _level_equal(a, b)
    ep = H.effective_params
    assert ep['node_block_smoother'] == 0 and ep['smoother'] == smoother
    assert ep['num_functions'] == kw['num_functions']


def test_enum_values(lib_built):
    P = _mamg().parameters
    assert (P.SMOOTHER_GS_POINT, P.SMOOTHER_SGS_POINT) == (13, 14)
    assert P.make_params(smoother=P.SMOOTHER_SGS_POINT).smoother == 14


@pytest.mark.parametrize('smoother', [13, 14])
def test_seeds_refused(lib_built, smoother):
    M = _mamg()
    s = M.problems.bidomain(2, 16, 1.0)
    with pytest.raises(M._lib.MamgError) as ei:
        M.HostHierarchy(s.scipy(), idofs=s.idofs, smoother=smoother, num_functions=2)
    assert ei.value.code == -4 and len(str(ei.value)) > 20
    assert 'Schwarz_levels 0' in str(ei.value)             # names the alternatives
    # without seeds the same dict runs (the level smoother everywhere)
    assert M.HostHierarchy(s.scipy(), smoother=smoother, num_functions=2).num_levels >= 2


def test_node_block_sgs_on_scalar_system_still_refused(lib_built):
    M = _mamg()
    from mamg_oracle import laplace1d
    with pytest.raises(M._lib.MamgError) as ei:
        M.HostHierarchy(laplace1d(30), smoother=11, num_functions=1)
    assert ei.value.code == -4


def test_multi_gpu_refused(lib_built):
    """the multi-GPU path keeps refusing: refused on the parameters, before the rank touches a GPU"""
    M = _mamg()
    s = M.problems.bidomain(2, 16, 1.0)
    for nf in (1, 2):
        with pytest.raises(M._lib.MamgError) as ei:
            M.DistMetricAMG(s.scipy(), None, smoother=14, num_functions=nf, rank=0, nranks=2, comm_id=None)
        assert ei.value.code == -4 and 'multi-GPU' in str(ei.value)


def test_pointwise_factory_mapping():
    M = _mamg()
    P = M.parameters
    from metric_amg_examples_amd.precond import amg_pointwise_parameters
    d, notes = amg_pointwise_parameters(P.parameters_standard)
    assert d['smoother'] == P.SMOOTHER_SGS_POINT and d['num_functions'] == 1 and d['Schwarz_levels'] == 0
    assert {k: v for k, v in d.items() if k not in ('smoother', 'num_functions')} == \
        {k: v for k, v in P.parameters_standard.items() if k != 'smoother'}
    assert len(notes) == 1 and "multicolour order instead of HAZmath's sequential dof order" in notes[0]
    assert P.parameters_standard['smoother'] == P.SMOOTHER_SGS       # the preset itself is untouched
    d, notes = amg_pointwise_parameters(dict(P.parameters_standard, smoother=P.SMOOTHER_GS))
    assert d['smoother'] == P.SMOOTHER_GS_POINT
    d, notes = amg_pointwise_parameters(P.parameters_standard_schwarz)
    assert d['smoother'] == P.SMOOTHER_SGS_POINT and d['Schwarz_levels'] == 0
    assert any('Schwarz_levels 1 -> 0' in n for n in notes) and len(notes) == 2
    d, notes = amg_pointwise_parameters(dict(P.parameters_standard, smoother=P.SMOOTHER_JACOBI))
    assert d['smoother'] == P.SMOOTHER_JACOBI and notes == []
    d, notes = amg_pointwise_parameters(None)                        # the factory's default dict
    assert d['smoother'] == P.SMOOTHER_SGS_POINT and d['aggregation_type'] == P.VMB


def test_driver_tags():
    from metric_amg_examples_amd import drivers as D
    P = _mamg().parameters
    for dim in (2, 3):
        for tag in ('hazmath', 'hazmath_HEM'):
            args, _ = D.bidomain_parser(dim).parse_known_args(['-precond', tag])
            assert args.precond == tag
        assert D.bidomain_parser(dim).parse_known_args([])[0].precond == 'metric_mono'   # default unchanged
    assert D.bidomain_parser(2).parse_known_args(['-precond', 'hazmath_Schwarz'])[0].precond == 'hazmath_Schwarz'
    with pytest.raises(SystemExit):
        D.bidomain_parser(3).parse_known_args(['-precond', 'hazmath_Schwarz'])
    # -profile reference: the dicts the reference passes
    assert D._profile_params('reference', 'hazmath') is P.parameters_standard
    assert D._profile_params('reference', 'hazmath_Schwarz') is P.parameters_standard_schwarz
    assert D._profile_params('reference', 'hazmath_HEM') is P.parameters_metric
    # the output file names carry the tag
    assert 'iters_precondhazmath_HEM_' in D._iters_path('r', 'hazmath_HEM', gamma=1.0)
