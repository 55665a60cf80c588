"""The K-cycle's inner CG inside the coarse tail (mamg_set_kcycle_tail: T_KDOT,
T_KORTH, T_KUPD of tail_kernel) on the GPU.

Every handle here has ``kcycle_tail`` on, and every test reads ``tail_info()``:
not refused, the expected tail level and number of programs, K ops in every
program -- a case that drifted off its branch fails instead of passing on the
launch path.

Bounds.  One apply against the restatement tests/kcycle_ref.py: 1e-10, the
project's contract.  Tail against launch path on one handle: 1e-11, the tail's
1e-13 against its launch path (tests/test_gpu_tail.py TOL_LAUNCH) times the 100
by which the nonlinearity may amplify a perturbation (tests/test_kcycle_ref.py).
Homogeneity 1e-12, PCG residual histories 1e-6, as tests/test_gpu_kcycle.py.

Systems (tests/kcycle_cases.py): bidomain 2-D n = 64 (4225 / 1102 / 295 / 78 / 21
nodes) and 3-D n = 16 (4913 / 1109 / 289 / 74 / 20).  The default tail level is
2: a Krylov level and the tail level, with the Krylov level 3 inside it;
MAMG_TAIL_NODES=2000 makes level 1 the tail level (two Krylov levels inside).

Measured on an MI355X (printed by the tests): see DESIGN.md section 2.13.
"""
import functools

import numpy as np
import pytest

import kcycle_cases as kc
import kcycle_ref as kcr
import mamg_oracle as mo
import stream_cases as st
from conftest import set_opt

pytestmark = pytest.mark.gpu

rel = kc.rel
TOL = 1e-10          # against the restatement
TOL_LAUNCH = 1e-11   # tail against launch path


def _mamg():
    import metric_amg_examples_amd as M
    return M


# name -> (case of kcycle_cases, extra parameters, MAMG_TAIL_NODES or None, tail level)
CASES = {
    'ua2d_sgs_m2': ('ua2d_sgs_m2', {}, None, 2),
    'ua2d_sgs_m3': ('ua2d_sgs_m3', {}, None, 2),
    'ua2d_sgs_m1': ('ua2d_sgs_m1', {}, None, 2),
    # J = 3: three earlier directions (the restatement is built here)
    'ua2d_sgs_m4': ('ua2d_sgs_m2', dict(amli_degree=4), None, 2),
    # coarse scaling: T_DOT2 / T_CSCALE next to the K ops
    'ua3d_sgs_scaling_m2': ('ua3d_sgs_scaling_m2', {}, None, 2),
    'ua2d_sgs_maxit2_m2': ('ua2d_sgs_maxit2_m2', {}, None, 2),
    # Jacobi has no tail by default; its EPI_KPOST op reads the e T_KUPD wrote
    'ua3d_jacobi_m2': ('ua3d_jacobi_m2', {}, 1024, 2),
    'ua3d_jacobi_nu2_m2': ('ua3d_jacobi_nu2_m2', {}, 1024, 2),
}


def degree(name):
    base, extra = CASES[name][:2]
    return extra.get('amli_degree', kc.CASES[base][3])


@functools.lru_cache(maxsize=None)
def restatement(name):
    base, extra = CASES[name][:2]
    if not extra:
        return kc.restatement(base)
    return kcr.KCycle(kc.restatement(base).h, extra['amli_degree'], 'K')


@functools.lru_cache(maxsize=None)
def reference(name):
    """{seed: apply of the restatement}, computed once and left unchanged"""
    base, extra = CASES[name][:2]
    if not extra:
        return kc.reference(base)
    out = {seed: restatement(name).apply(kc.rhs(base, seed)) for seed in kc.SEEDS}
    for v in out.values():
        v.setflags(write=False)
    return out


def build(name, setup='auto', opts=None, nodes='case', tail=True, **extra):
    """the case's handle under the switches opts, with the K ops in the tail"""
    base, kw, cn = CASES[name][:3]
    nodes = cn if nodes == 'case' else nodes
    opts = dict(opts or {})
    if nodes is not None:
        opts['MAMG_TAIL_NODES'] = nodes
    for k, v in opts.items():
        set_opt(k, v)
    B = kc.handle(base, setup, kcycle_tail=tail, **dict(kw, **extra))
    for k in opts:
        set_opt(k, None)
    assert B.layout == 'bsr2' and B.kcycle_tail == tail
    return B


def programs_of(name):
    """one tail program per (right-hand side, result) pair of the tail level's
    inner CG: (C.b -> p_0), and (r -> z) from step 1 on"""
    return 1 if degree(name) == 1 else 2


def check_plan(B, level, nprog):
    info = B.tail_info()
    print('tail', info)
    assert not info['refused'] and info['tail_level'] == level and len(info['programs']) == nprog, info
    for p in info['programs']:
        assert p['ops_k'] > 0, info
    return info


@pytest.mark.parametrize('setup', ['host', 'gpu'])
@pytest.mark.parametrize('name', list(CASES))
def test_apply_matches_restatement(lib_built, name, setup):
    import torch
    base = CASES[name][0]
    B = build(name, setup)
    assert B.setup_path == setup, B.setup_path
    assert B.num_levels == len(restatement(name).levels) == 5
    assert B.effective_params['amli_degree'] == degree(name)
    for seed in kc.SEEDS:
        r = kc.rhs(base, seed)
        zo = reference(name)[seed]
        z = B * r
        zt = B.matvec(torch.as_tensor(r).cuda())
        torch.cuda.synchronize()
        e1, e2 = rel(z, zo), rel(zt.cpu().numpy(), zo)
        print('%s %s seed %d: rel err host vectors %.3e, device vectors %.3e' % (name, setup, seed, e1, e2))
        assert e1 < TOL and e2 < TOL
    check_plan(B, CASES[name][3], programs_of(name))
    B.close()


def test_tail_level_one(lib_built):
    """MAMG_TAIL_NODES=2000: level 1 (1102 nodes) is Krylov and the tail level,
    the Krylov levels 2 and 3 lie strictly inside, and the 17 vectors of 17.6 KB
    of level 1 do not all fit the LDS: operands of both kinds in one program"""
    name = 'ua2d_sgs_m2'
    B = build(name, nodes=2000)
    for seed in kc.SEEDS:
        e = rel(B * kc.rhs(name, seed), reference(name)[seed])
        print('tail level 1, seed %d: %.3e' % (seed, e))
        assert e < TOL
    info = check_plan(B, 1, 2)
    for p in info['programs']:
        assert p['vec_lds'] > 0 and p['vec_global'] > 0, info
    B.close()


@pytest.mark.parametrize('opt,value', [('MAMG_TAIL_LDS', 0), ('MAMG_TAIL_RES', 0), ('MAMG_TAIL_PROG_LDS', 1),
                                       ('MAMG_TAIL_VL', 1), ('MAMG_TAIL_VL', 64)])
def test_planner_switches(lib_built, opt, value):
    name = 'ua2d_sgs_m3'
    B = build(name, opts={opt: value})
    e = rel(B * kc.rhs(name, 1234), reference(name)[1234])
    print('%s=%s: %.3e' % (opt, value, e))
    assert e < TOL
    info = check_plan(B, 2, 2)
    for p in info['programs']:
        if opt == 'MAMG_TAIL_LDS':
            assert p['lds_bytes'] == 0 and p['vec_lds'] == 0 and p['vec_global'] > 0 and not p['res'], info
        elif opt == 'MAMG_TAIL_RES':
            assert not p['res'] and p['ops_res'] == 0 and p['vec_lds'] > 0, info
        elif opt == 'MAMG_TAIL_PROG_LDS':
            assert p['prog_lds'] >= 0, info
        else:
            assert p['vec_lds'] > 0, info
    B.close()


@pytest.mark.parametrize('name', list(CASES))
def test_tail_against_launch_path_and_launch_counts(lib_built, name):
    """off, on, off on one handle: the two launch-path applies are bitwise
    equal, the tail's stays within 1e-11 of them, and the second off leaves no
    program and the refusal the launch path has always had.  apply_launches():
    fewer with the tail on, and the count the op builders imply."""
    base = CASES[name][0]
    B = build(name, tail=False)
    r = kc.rhs(base, 1234)
    n_off = B.apply_launches()
    z_off = B * r
    info = B.tail_info()
    assert info['programs'] == [] and info['refused'], info
    B.set_kcycle_tail(True)
    assert B.kcycle_tail
    n_on = B.apply_launches()
    z_on = B * r
    check_plan(B, CASES[name][3], programs_of(name))
    B.set_kcycle_tail(False)
    assert not B.kcycle_tail
    z_off2 = B * r
    info = B.tail_info()
    assert info['programs'] == [] and info['refused'], info
    assert np.array_equal(z_off, z_off2)
    assert B.apply_launches() == n_off
    e = rel(z_on, z_off)
    print('%s: tail against launch path %.3e, restatement %.3e; launches per apply %d off, %d on'
          % (name, e, rel(z_on, reference(name)[1234]), n_off, n_on))
    assert rel(z_on, reference(name)[1234]) < TOL
    assert n_on < n_off
    assert e < TOL_LAUNCH
    if name == 'ua2d_sgs_m2':
        assert n_on == expected_launches_ua2d_sgs_m2()
    B.close()


def expected_launches_ua2d_sgs_m2():
    """cycle_ops_bsr / coarse_visit_ops_bsr / kstep_ops, m = 2, SGS with
    nu1 = nu2 = 1, c_l non-empty colours on level l, the tail at level 2:
      a K visit's vector steps: step 0 KORTH + KUPD, step 1 KDOT + KORTH + KUPD = 5
      visit(2) = 2 x (tail program + w = A z) + 5                          =  9
      cycle(1) = zero + 2 c_1 sweeps + residual + restriction + visit(2)
                 + prolongation + 2 c_1 sweeps                             = 13 + 4 c_1
      visit(1) = 2 x (cycle(1) + w = A z) + 5                              = 33 + 8 c_1
      cycle(0) = zero + 2 c_0 + residual + restriction + visit(1)
                 + prolongation + 2 c_0 + the copy out to the caller's layout
                                                                           = 38 + 4 c_0 + 8 c_1"""
    lv = restatement('ua2d_sgs_m2').levels
    c = [len([rows for rows in lv[l].crows if len(rows)]) for l in (0, 1)]
    return 38 + 4 * c[0] + 8 * c[1]


@pytest.mark.parametrize('name', ['ua2d_sgs_m3', 'ua3d_sgs_scaling_m2', 'ua3d_jacobi_m2'])
def test_deterministic_homogeneous_and_zero(lib_built, name):
    """two replays of the apply graph give the same bits; K(a r) = a K(r) to
    1e-12; K(0) is exactly 0 (every direction dead: alpha and beta 0, no 0 / 0)"""
    import torch
    base = CASES[name][0]
    B = build(name)
    r = torch.as_tensor(kc.rhs(base, 1234)).cuda()
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
    check_plan(B, CASES[name][3], programs_of(name))
    B.close()


def test_pcg_matches_restatement(lib_built):
    M = _mamg()
    name = 'ua2d_sgs_m2'
    A = kc.problem(*kc.CASES[name][:2])[0]
    b = kc.rhs(name, 1234)
    B = build(name)
    solver = M.ConjGrad(A, precond=B, tolerance=1e-8, maxiter=500, device=True)
    x = solver * b
    ref = mo.pcg(A, restatement(name), b, 1e-8, 500)
    print('%s: PCG iterations %d (restatement %d)' % (name, len(solver.residuals) - 1, ref.niters))
    assert len(solver.residuals) == len(ref.residuals)
    assert np.allclose(solver.residuals, ref.residuals, rtol=1e-6, atol=0)
    assert rel(x, ref.x) < 1e-6
    check_plan(B, 2, 2)
    B.close()


def test_apply_on_a_user_stream(lib_built):
    """one apply on a user stream behind pending work (tests/stream_cases.py)
    equals the default-stream result of the same handle and buffers bitwise"""
    import torch
    name = 'ua3d_sgs_scaling_m2'
    s1, _ = st.streams()
    B, T = build(name), build(name)
    r = kc.rhs(name, 7)
    src = torch.as_tensor(r).cuda()
    rb, zb = torch.full_like(src, float('nan')), torch.full_like(src, float('nan'))
    tr, tz = src.clone(), torch.empty_like(src)
    call_ms = st.host_ms(lambda: T.apply_device(tr, tz))
    st.behind_delay('kcycle tail apply', s1, call_ms, lambda: rb.copy_(src), lambda: B.apply_device(rb, zb, s1))
    zu = zb.clone()
    zb.fill_(float('nan'))
    B.apply_device(rb, zb)
    torch.cuda.synchronize()
    assert torch.equal(zu, zb)
    assert rel(zu.cpu().numpy(), reference(name)[7]) < TOL
    check_plan(B, 2, 2)
    B.close()
    T.close()


def test_refusals(lib_built):
    M = _mamg()
    # not a K-cycle handle (V, W) and the CSR layout: -4, the reason named, the apply unchanged
    for base, extra, word in (('ua2d_sgs_m2', dict(cycle_type=1), 'AMLI'), ('ua2d_sgs_m2', dict(cycle_type=2), 'AMLI'),
                              ('scalar_jacobi_m2', {}, 'BSR2')):
        B = kc.handle(base, **extra)
        r = kc.rhs(base, 1234)
        z = B * r
        before = B.tail_info()
        with pytest.raises(M._lib.MamgError) as ei:
            B.set_kcycle_tail(True)
        assert ei.value.code == -4 and word in str(ei.value), str(ei.value)
        with pytest.raises(M._lib.MamgError) as ei:      # the constructor's keyword makes the same call
            kc.handle(base, kcycle_tail=True, **extra)
        assert ei.value.code == -4
        assert not B.kcycle_tail and B.tail_info() == before
        assert np.array_equal(B * r, z)
        B.close()
    # another value: -1, whatever the handle
    B = build('ua3d_jacobi_m2', nodes=None, tail=False)
    for bad in (2, -1, 7):
        with pytest.raises(M._lib.MamgError) as ei:
            B.set_kcycle_tail(bad)
        assert ei.value.code == -1
    # a K-cycle handle without a tail level (Jacobi, default switches): OK, no effect on the apply
    r = kc.rhs('ua3d_jacobi_m2', 7)
    z = B * r
    n = B.apply_launches()
    B.set_kcycle_tail(True)
    info = B.tail_info()
    assert info['tail_level'] == 0 and info['programs'] == [] and not info['refused'], info
    assert np.array_equal(B * r, z) and B.apply_launches() == n
    B.set_kcycle_tail(False)
    B.close()
    # fp32 operator storage stays refused with the tail on
    B = build('ua2d_sgs_m2')
    z = B * kc.rhs('ua2d_sgs_m2', 7)
    with pytest.raises(M._lib.MamgError) as ei:
        B.set_cycle_storage('f32')
    assert ei.value.code == -4 and 'AMLI' in str(ei.value)
    assert np.array_equal(B * kc.rhs('ua2d_sgs_m2', 7), z)
    check_plan(B, 2, 2)
    B.close()
