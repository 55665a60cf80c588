"""The nonlinear AMLI cycle (K-cycle, cycle_type 4) without a GPU: the CPU
restatement tests/kcycle_ref.py against the oracle, the properties the GPU
cases of tests/test_gpu_kcycle.py rely on, the .dat mapping and the parameter
checks of the library.

* With the visit set to V and to W the restatement is the oracle's cycle bit
  for bit, so only the visit differs.
* Every GPU case has Krylov levels, K(m) is far from W (a GPU that ran W
  would fail the 1e-10 parity), and the nonlinearity does not eat that
  contract: a 1e-13 relative perturbation of r moves the apply by < 1e-11
  (measured: at most 5.4e-13 over the cases).
"""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import kcycle_cases as kc
import kcycle_ref as kr
import mamg_oracle as mo
import pointgs_ref as pr
import pointrings_ref as rr


def _M():
    import metric_amg_examples_amd as M
    return M


@pytest.mark.parametrize('name', ['ua2d_sgs_m2', 'ua3d_sgs_scaling_m2', 'sa2d_poly_m2', 'scalar_jacobi_m2'])
@pytest.mark.parametrize('visit', ['V', 'W'])
def test_restatement_is_the_oracles_cycle(name, visit):
    ref = kc.restatement(name, visit)
    h = ref.h
    ho = mo.Hierarchy(h.levels, dataclasses.replace(h.params, cycle_type=visit))
    for seed in kc.SEEDS:
        r = kc.rhs(name, seed)
        assert np.array_equal(ref.cycle(0, r), ho.cycle(0, r))
    assert np.array_equal(ref.apply(r), ho.apply(r))


@pytest.mark.parametrize('visit', ['V', 'W'])
def test_csr_restatements_are_their_references(visit):
    """KPointGS / KPointRings against pointgs_ref / pointrings_ref, bitwise"""
    name = 'scalar_sgs_point_m2'
    A = kc.problem(*kc.CASES[name][:2])[0]
    r = kc.rhs(name, 7)
    pg = pr.PointGS(A, 'SGS', **dict(kc.CASES[name][2], cycle_type=visit))
    assert np.array_equal(kr.KPointGS(pg, 2, visit).apply(r), pg.apply(r))
    name = 'rings_3d1d_deep_m2'
    A, _, seeds = kc.problem(*kc.CASES[name][:2])
    r = kc.rhs(name, 7)
    ring = rr.PointRings(A, seeds, 'JACOBI_RHO', **dict(kc.RINGS_KW, **dict(kc.CASES[name][2], cycle_type=visit)))
    assert np.array_equal(kr.KPointRings(ring, 2, visit).apply(r), ring.apply(r))


@pytest.mark.parametrize('name', kc.APPLY_CASES)
def test_gpu_cases_have_krylov_levels_and_are_not_w(name):
    ref = kc.restatement(name)
    nlev = len(ref.levels)
    assert nlev >= kc.CASES[name][4], [lv.A.shape[0] for lv in ref.levels]
    refw = kc.restatement(name, 'W')
    for seed in kc.SEEDS:
        r = kc.rhs(name, seed)
        z = kc.reference(name)[seed]
        assert np.isfinite(z).all()
        d = kc.rel(z, refw.apply(r))
        if nlev == 2:
            assert d == 0.0            # no Krylov level: the visit is the dense solve, as in V and W
        else:
            assert d > 1e-4, d
        # the nonlinearity against the 1e-10 contract
        rp = r * (1.0 + 1e-13 * np.where(np.arange(r.size) % 2, 1.0, -1.0))
        moved = kc.rel(ref.apply(rp), z)
        print('%s seed %d: K - W %.2e, 1e-13 in -> %.2e out' % (name, seed, d, moved))
        assert moved < 1e-11, moved


@pytest.mark.parametrize('name', ['ua2d_sgs_m3', 'ua3d_sgs_scaling_m2', 'scalar_jacobi_m2'])
def test_homogeneous_and_zero(name):
    ref = kc.restatement(name)
    r = kc.rhs(name, 1234)
    z = kc.reference(name)[1234]
    assert kc.rel(ref.apply(2.0 * r), 2.0 * z) <= 1e-12
    assert kc.rel(ref.apply(-0.37 * r), -0.37 * z) <= 1e-12
    z0 = ref.apply(np.zeros_like(r))          # every direction dead: the guard, no 0 / 0
    assert np.isfinite(z0).all() and not z0.any()


def test_dat_mapping():
    M = _M()
    P = M.parameters
    assert P.NL_AMLI_CYCLE == 4
    base = dict(AMG_type='UA', AMG_cycle_type='NA', AMG_amli_degree=2)
    prm, _, _ = M.fileio.dat_to_parameters(base)
    assert prm['cycle_type'] == P.NL_AMLI_CYCLE and prm['amli_degree'] == 2
    prm, _, _ = M.fileio.dat_to_parameters(dict(base, AMG_nl_amli_krylov_type=5))
    assert prm['cycle_type'] == P.NL_AMLI_CYCLE
    with pytest.raises(ValueError, match='AMG_nl_amli_krylov_type'):
        M.fileio.dat_to_parameters(dict(base, AMG_nl_amli_krylov_type=6))
    for word in ('A', 'ADD'):
        with pytest.raises(ValueError, match='AMG_cycle_type'):
            M.fileio.dat_to_parameters(dict(base, AMG_cycle_type=word))
    # the krylov type is not looked at under V and W
    prm, _, _ = M.fileio.dat_to_parameters(dict(base, AMG_cycle_type='W', AMG_nl_amli_krylov_type=6))
    assert prm['cycle_type'] == P.W_CYCLE


def test_preset():
    P = _M().parameters
    k = P.parameters_metric_kcycle
    assert k['cycle_type'] == P.NL_AMLI_CYCLE and k['amli_degree'] == 2
    assert {a: b for a, b in k.items() if a not in ('cycle_type', 'amli_degree')} == \
        {a: b for a, b in P.parameters_metric.items() if a not in ('cycle_type', 'amli_degree')}
    mapped, _ = P.to_gpu_profile(k)
    assert mapped['cycle_type'] == P.NL_AMLI_CYCLE and mapped['amli_degree'] == 2
    assert P.make_params(mapped).cycle_type == 4


@pytest.mark.parametrize('degree', [0, 5, -1])
def test_degree_out_of_range_is_invalid(lib_built, degree):
    M = _M()
    with pytest.raises(M._lib.MamgError) as ei:
        M.HostHierarchy(mo.laplace1d(30), cycle_type=4, amli_degree=degree)
    assert ei.value.code == -1 and 'amli_degree' in str(ei.value)


def test_kcycle_parameters_build_and_other_cycles_keep_their_rules(lib_built):
    M = _M()
    for degree in (1, 2, 4):
        H = M.HostHierarchy(mo.laplace1d(300), cycle_type=4, amli_degree=degree)
        assert H.num_levels >= 2
        assert H.effective_params['cycle_type'] == 4 and H.effective_params['amli_degree'] == degree
        H.close()
    # V and W take any amli_degree, as before; linear AMLI (3) is still not built
    for cyc in (1, 2):
        M.HostHierarchy(mo.laplace1d(30), cycle_type=cyc, amli_degree=0).close()
    with pytest.raises(M._lib.MamgError) as ei:
        M.HostHierarchy(mo.laplace1d(30), cycle_type=3)
    assert ei.value.code == -4


def test_dist_setup_refuses_the_kcycle_before_the_gpu(lib_built):
    """mamg_setup_dist: MAMG_ERR_UNSUPPORTED with a message, with or without a device
    (the check runs before the rank touches its GPU)"""
    M = _M()
    P = M.parameters
    s = M.problems.bidomain(2, 16, 1e4)
    L = M._lib.lib()
    csr = M._lib.as_csr_struct(s.indptr, s.indices, s.data, s.N)
    prm = P.make_params(P.parameters_metric_mi355x, cycle_type=P.NL_AMLI_CYCLE, amli_degree=2)
    cid, out = (C.c_char * 128)(), C.c_void_p()
    rc = L.mamg_setup_dist(C.byref(csr), None, 0, C.byref(prm), 0, 2, cid, 0, C.byref(out))
    msg = L.mamg_last_error().decode()
    assert rc == -4 and 'single-GPU' in msg, (rc, msg)
    # a degree out of range is the parameter error first
    prm = P.make_params(P.parameters_metric_mi355x, cycle_type=P.NL_AMLI_CYCLE, amli_degree=7)
    rc = L.mamg_setup_dist(C.byref(csr), None, 0, C.byref(prm), 0, 2, cid, 0, C.byref(out))
    assert rc == -1, L.mamg_last_error().decode()
