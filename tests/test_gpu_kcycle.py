"""GPU parity of the nonlinear AMLI cycle (K-cycle, cycle_type 4: the visit
builders coarse_visit_ops_bsr / _csr, kdot_kernel, korth_kernel, kupd_kernel)
against the CPU restatement tests/kcycle_ref.py.

Tolerances are the project's: one apply to 1e-10 relative (the hierarchy, the
colourings and the smoothers are exact; the summation order of a row and of a
dot product differs, and tests/test_kcycle_ref.py shows that the nonlinearity
amplifies a 1e-13 perturbation to less than 1e-11), PCG iteration count equal
to the restatement's with residuals within 1e-6 (tests/test_gpu_gs.py).

The coarse tail does not express the K-cycle's ops: its planner refuses a tail
level with a Krylov level below it and those levels run the launch path
(asserted below); a tail level directly above the coarsest has no K op inside
and keeps its program (case sa2d_sgs_m2).
"""
import numpy as np
import pytest

import kcycle_cases as kc
import mamg_oracle as mo
import stream_cases as st

pytestmark = pytest.mark.gpu

rel = kc.rel


def _mamg():
    import metric_amg_examples_amd as M
    return M


@pytest.mark.parametrize('setup', ['host', 'gpu'])
@pytest.mark.parametrize('name', kc.APPLY_CASES)
def test_apply_matches_restatement(lib_built, name, setup):
    import torch
    B = kc.handle(name, setup)
    assert B.setup_path == setup, B.setup_path
    ref = kc.restatement(name)
    assert B.num_levels == len(ref.levels)
    ep = B.effective_params
    assert ep['cycle_type'] == 4 and ep['amli_degree'] == kc.CASES[name][3]
    assert B.layout == ('bsr2' if kc.CASES[name][0] == 'nodal' else 'csr')
    for seed in kc.SEEDS:
        r = kc.rhs(name, seed)
        zo = kc.reference(name)[seed]
        z = B * r
        zt = B.matvec(torch.as_tensor(r).cuda())
        torch.cuda.synchronize()
        e1, e2 = rel(z, zo), rel(zt.cpu().numpy(), zo)
        print('%s %s seed %d: rel err host vectors %.3e, device vectors %.3e' % (name, setup, seed, e1, e2))
        assert e1 < 1e-10 and e2 < 1e-10
    B.close()


def test_tail_program_of_a_krylov_level(lib_built):
    """SA + SGS, three levels: the tail level is the Krylov level itself, so the
    inner CG's preconditioner is a tail program per (rhs, result) pair"""
    name = 'sa2d_sgs_m2'
    B = kc.handle(name)
    z = B * kc.rhs(name, 1234)
    info = B.tail_info()
    print('tail', info)
    assert info['tail_level'] == 1 and not info['refused'] and len(info['programs']) == 2, info
    assert rel(z, kc.reference(name)[1234]) < 1e-10
    B.close()


@pytest.mark.parametrize('name', ['ua2d_sgs_m2', 'sa2d_m2'])
def test_pcg_matches_restatement(lib_built, name):
    M = _mamg()
    A = kc.problem(*kc.CASES[name][:2])[0]
    b = kc.rhs(name, 1234)
    B = kc.handle(name)
    solver = M.ConjGrad(A, precond=B, tolerance=1e-8, maxiter=500, device=True)
    x = solver * b
    ref = mo.pcg(A, kc.restatement(name), b, 1e-8, 500)
    print('%s: PCG iterations %d (restatement %d)' % (name, len(solver.residuals) - 1, ref.niters))
    assert len(solver.residuals) == len(ref.residuals)
    assert np.allclose(solver.residuals, ref.residuals, rtol=1e-6, atol=0)
    assert rel(x, ref.x) < 1e-6
    B.close()


@pytest.mark.parametrize('name', ['ua2d_sgs_m3', 'ua3d_sgs_scaling_m2', 'scalar_jacobi_m2'])
def test_deterministic_homogeneous_and_zero(lib_built, name):
    """two replays of the apply graph give the same bits; K(a r) = a K(r) to
    1e-12; K(0) is exactly 0 (every direction dead: alpha and beta 0, no 0 / 0)"""
    import torch
    B = kc.handle(name)
    r = torch.as_tensor(kc.rhs(name, 1234)).cuda()
    z = torch.empty_like(r)
    B.apply_device(r, z)
    z1 = z.clone()
    z.fill_(float('nan'))
    B.apply_device(r, z)
    torch.cuda.synchronize()
    assert torch.equal(z, z1)
    for a in (2.0, -0.37):
        za = B.matvec(a * r)
        torch.cuda.synchronize()
        e = rel(za.cpu().numpy(), a * z1.cpu().numpy())
        print('%s: homogeneity at %g: %.3e' % (name, a, e))
        assert e <= 1e-12
    z0 = B * np.zeros(r.numel())
    assert np.isfinite(z0).all() and not z0.any()
    zt = B.matvec(torch.zeros_like(r))
    torch.cuda.synchronize()
    assert not bool(zt.isnan().any()) and not bool(zt.any())
    B.close()


def test_apply_on_a_user_stream(lib_built):
    """one apply on a user stream behind pending work (tests/stream_cases.py)
    equals the default-stream result of the same handle and buffers bitwise"""
    import torch
    name = 'ua3d_sgs_scaling_m2'
    s1, _ = st.streams()
    B, T = kc.handle(name), kc.handle(name)
    r = kc.rhs(name, 7)
    src = torch.as_tensor(r).cuda()
    rb, zb = torch.full_like(src, float('nan')), torch.full_like(src, float('nan'))
    tr, tz = src.clone(), torch.empty_like(src)
    call_ms = st.host_ms(lambda: T.apply_device(tr, tz))
    st.behind_delay('kcycle apply', s1, call_ms, lambda: rb.copy_(src), lambda: B.apply_device(rb, zb, s1))
    zu = zb.clone()
    zb.fill_(float('nan'))
    B.apply_device(rb, zb)
    torch.cuda.synchronize()
    assert torch.equal(zu, zb)
    assert rel(zu.cpu().numpy(), kc.reference(name)[7]) < 1e-10
    B.close()
    T.close()


def test_refusals_and_launch_path(lib_built):
    """fp32 operator storage is refused (MAMG_ERR_UNSUPPORTED) and leaves the
    handle as it was; the coarse tail's planner refuses a program that would
    hold the K-cycle's ops"""
    M = _mamg()
    name = 'ua3d_jacobi_m2'
    B = kc.handle(name)
    r = kc.rhs(name, 1234)
    z = B * r
    with pytest.raises(M._lib.MamgError) as ei:
        B.set_cycle_storage('f32')
    assert ei.value.code == -4 and 'AMLI' in str(ei.value)
    assert not any(B.level_storage(l)['A'] for l in range(B.num_levels))
    B.set_cycle_storage('f64')
    assert np.array_equal(B * r, z)
    assert rel(z, kc.reference(name)[1234]) < 1e-10
    B.close()
    for name in ('ua3d_jacobi_m2', 'ua3d_sgs_scaling_m2', 'ua2d_sgs_m3'):
        B = kc.handle(name)
        B * kc.rhs(name, 7)
        info = B.tail_info()
        print(name, 'tail', info)
        # a handle with a tail level: its planner met the K-cycle's ops and refused
        assert info['programs'] == [] and info['refused'] == (info['tail_level'] > 0), info
        B.close()
