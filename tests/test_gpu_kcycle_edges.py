"""GPU parity where the K-cycle drops directions, and where the reductions run
past their grid caps (cases and reasons: tests/kcycle_edge_cases.py).

Indefinite systems.  A - sigma I makes every level's operator indefinite, so
kupd_kernel's alpha = 0, korth_kernel's beta_i = 0, their copies in
tail_kernel (tail_kdot, tail_korth, tail_kupd) and cscale_kernel's alpha = 1
decide on non-zero data.  tests/test_kcycle_edges_ref.py establishes, on the
CPU reference alone, that every (case, seed) here meets a kept step followed
by a dropped one, an all-dropped visit and (scaling cases) denominators of
both signs, each by a margin of at least 1e-3, that the reference amplifies a
1e-13 perturbation to at most 1e-11, and that a cycle without the guards is
more than 1e-3 away.  The bounds are therefore the project's own: one apply to
1e-10 against the restatement, the tail to 1e-11 against its launch path
(tests/test_gpu_kcycle_tail.py), homogeneity to 1e-12.

Past the caps.  bidomain(2, 384, 1e4): level 1 (79 132 dofs) is a Krylov level
above SCALE_BLOCKS * 256, so dot2_partial_kernel, cscale_kernel, kdot_kernel,
korth_kernel and kupd_kernel take a second grid-stride pass and their
consumers sum all 256 partial slots; level 0 (296 450) is above
DOT_BLOCKS * 256 for the device PCG's dots.  The stopping rule ||r|| <= tol ||b||
exists on the device only in the row-partitioned PCG (dpcg_dot_kernel,
dpcg_r0_kernel; ConjGrad(device=True) refuses stop_type and device=None takes
the host loop for it), which one virtual rank that owns every row runs at this
size; that PCG refuses the K-cycle, so it is the V handle's alone.

Measured on an MI355X (printed by the tests): see DESIGN.md section 2.13.1.
"""
import warnings

import numpy as np
import pytest

import kcycle_cases as kc
import kcycle_edge_cases as ke
import mamg_oracle as mo
import stream_cases as st
from conftest import set_opt

pytestmark = pytest.mark.gpu

rel = kc.rel
TOL = 1e-10          # one apply against the restatement (tests/test_gpu.py APPLY_TOL)
TOL_LAUNCH = 1e-11   # tail against launch path (tests/test_gpu_kcycle_tail.py)
TAIL_LEVEL = 2       # 4225 / 1102 / 295 / 78 / 21 nodes: the first level of at most 1024


def _mamg():
    import metric_amg_examples_amd as M
    return M


def _cuda(v):
    import torch
    return torch.as_tensor(np.ascontiguousarray(v)).cuda()


# ---------------------------------------------------------------- indefinite
def _check_handle(B, name, setup):
    kind, _, _, m, visit = ke.INDEFINITE[name]
    assert B.setup_path == setup, B.setup_path
    assert B.num_levels == len(ke.hierarchy(name).levels) == 5
    ep = B.effective_params
    if visit == 'K':
        assert ep['cycle_type'] == 4 and ep['amli_degree'] == m
    else:
        assert ep['cycle_type'] == 2
    assert ep['coarse_scaling'] == ke.INDEFINITE[name][2].get('coarse_scaling', 0)
    assert B.layout == ('bsr2' if kind == 'nodal' else 'csr')


def _applies(B, name, label):
    """host vectors and device vectors against the restatement, then replay
    and homogeneity on the first seed"""
    import torch
    for seed in ke.SEEDS:
        r = ke.rhs(name, seed)
        zo = ke.reference(name)[seed]
        z = B * r
        zt = B.matvec(_cuda(r))
        torch.cuda.synchronize()
        e1, e2 = rel(z, zo), rel(zt.cpu().numpy(), zo)
        print('%s seed %d: rel err host vectors %.3e, device vectors %.3e' % (label, seed, e1, e2))
        assert e1 < TOL and e2 < TOL
    r = _cuda(ke.rhs(name, ke.SEEDS[0]))
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
        print('%s: homogeneity at %g: %.3e' % (label, a, e))
        assert e <= 1e-12


@pytest.mark.parametrize('setup', ['host', 'gpu'])
@pytest.mark.parametrize('name', list(ke.INDEFINITE))
def test_indefinite_apply_matches_restatement(lib_built, name, setup):
    B = ke.handle(name, setup)
    _check_handle(B, name, setup)
    _applies(B, name, '%s %s' % (name, setup))
    if ke.INDEFINITE[name][4] == 'K' and B.layout == 'bsr2':
        assert B.tail_info()['programs'] == []      # the launch path: kdot_kernel, korth_kernel, kupd_kernel
    B.close()


def _tail_handle(name, setup='auto', tail=True):
    nodes = ke.TAIL_CASES[name]
    if nodes is not None:
        set_opt('MAMG_TAIL_NODES', nodes)
    try:
        B = ke.handle(name, setup, kcycle_tail=tail)
    finally:
        if nodes is not None:
            set_opt('MAMG_TAIL_NODES', None)
    assert B.layout == 'bsr2' and B.kcycle_tail == tail
    return B


def _check_plan(B):
    info = B.tail_info()
    print('tail', info)
    assert not info['refused'] and info['tail_level'] == TAIL_LEVEL and len(info['programs']) == 2, info
    for p in info['programs']:
        assert p['ops_k'] > 0, info


@pytest.mark.parametrize('setup', ['host', 'gpu'])
@pytest.mark.parametrize('name', list(ke.TAIL_CASES))
def test_indefinite_apply_in_the_tail(lib_built, name, setup):
    """the K ops of levels 2 and 3 inside tail_kernel, those of level 1 launched"""
    B = _tail_handle(name, setup)
    _check_handle(B, name, setup)
    _applies(B, name, '%s %s tail' % (name, setup))
    _check_plan(B)
    B.close()


@pytest.mark.parametrize('name', list(ke.TAIL_CASES))
def test_indefinite_tail_against_launch_path(lib_built, name):
    """one handle, tail on and then off: both drop the same directions"""
    B = _tail_handle(name)
    for seed in ke.SEEDS:
        r = ke.rhs(name, seed)
        B.set_kcycle_tail(True)
        z_on = B * r
        _check_plan(B)
        B.set_kcycle_tail(False)
        z_off = B * r
        assert B.tail_info()['programs'] == []
        e = rel(z_on, z_off)
        print('%s seed %d: tail against launch path %.3e, restatement %.3e'
              % (name, seed, e, rel(z_on, ke.reference(name)[seed])))
        assert rel(z_on, ke.reference(name)[seed]) < TOL and rel(z_off, ke.reference(name)[seed]) < TOL
        assert e < TOL_LAUNCH
    B.close()


@pytest.mark.parametrize('kind', ['nodal', 'scalar'])
def test_gpu_setup_accepts_what_the_oracle_accepts(lib_built, kind):
    """gsetup.hip's pivot rule is the oracle's (setup.cpp's:
    tests/test_kcycle_edges_ref.py): the first refused shift is refused"""
    M = _mamg()
    name = 'sgs_m3' if kind == 'nodal' else 'scalar_jacobi_m2'
    A, W, idofs = ke.shifted(kind, ke.SIGMA_REFUSED)
    with pytest.raises(np.linalg.LinAlgError, match='non-positive pivot'):
        mo.setup(A, ke.oracle_params(name), idofs=idofs)
    for setup in ('gpu', 'host'):
        with pytest.raises(M._lib.MamgError) as ei:
            M.MetricAMG(A, W, idofs=idofs, setup=setup, **ke.c_params(name))
        assert ei.value.code == -3 and 'not SPD' in str(ei.value), str(ei.value)       # MAMG_ERR_SETUP


# -------------------------------------------------------------- past the caps
@pytest.fixture(scope='module')
def big(lib_built):
    """name -> the case's handle: one per case and module, closed at the end"""
    made = {}

    def get(name):
        if name not in made:
            made[name] = ke.big_handle(name)
        return made[name]
    yield get
    for B in made.values():
        B.close()


def test_large_system_crosses_both_caps():
    """from the restatement's level sizes, so the system cannot drift under a cap unnoticed"""
    for name, (_, _, visit) in ke.BIG_CASES.items():
        n = [lv.A.shape[0] for lv in ke.big_restatement(name).levels]
        assert n[0] > ke.DOT_CAP, n
        if visit != 'V':        # level 1 is a Krylov level (W: scaled), its second pass ends in a partial block
            assert len(n) > 3 and ke.SCALE_CAP < n[1] < 2 * ke.SCALE_CAP and n[1] % 256 != 0, n


@pytest.mark.parametrize('name', ['k_sgs_scaling_m2', 'k_jacobi_m4', 'w_jacobi_scaling'])
def test_large_apply_matches_restatement(big, name):
    """K: kdot / korth / kupd (and, with scaling, dot2_partial / cscale) on 256
    blocks of level 1; W: mamg_oracle's own cycle, dot2_partial / cscale alone"""
    B = big(name)
    ref = ke.big_restatement(name)
    assert B.num_levels == len(ref.levels) and B.layout == 'bsr2'
    ep = B.effective_params
    _, m, visit = ke.BIG_CASES[name]
    assert ep['cycle_type'] == (4 if visit == 'K' else 2) and (visit != 'K' or ep['amli_degree'] == m)
    assert ep['coarse_scaling'] == ke.BIG_CASES[name][0].get('coarse_scaling', 0)
    for seed in ke.SEEDS:
        z = B * ke.big_rhs(seed)
        e = rel(z, ke.big_reference(name, seed))
        print('%s seed %d: rel err %.3e' % (name, seed, e))
        assert e < TOL


@pytest.mark.parametrize('name', ['k_jacobi_m4', 'v_default'])
def test_large_device_pcg_matches_restatement(big, name):
    """ConjGrad(device=True): dot_partial_kernel's 1024 blocks in a second pass
    over level 0, their consumers over all 1024 partials"""
    M = _mamg()
    A = ke.big_problem()[0]
    b = ke.big_rhs(1234)
    solver = M.ConjGrad(A, precond=big(name), tolerance=1e-8, maxiter=500, device=True)
    x = solver * b
    ref = mo.pcg(A, ke.big_restatement(name), b, 1e-8, 500)
    print('%s: PCG iterations %d (restatement %d), x rel err %.3e'
          % (name, len(solver.residuals) - 1, ref.niters, rel(x, ref.x)))
    assert len(solver.residuals) == len(ref.residuals)
    assert np.allclose(solver.residuals, ref.residuals, rtol=1e-6, atol=0)
    assert rel(x, ref.x) < 1e-6


class _OracleB:
    """the oracle's apply behind the `B * r` the host ConjGrad calls"""

    def __init__(self, apply):
        self.apply = apply

    def __mul__(self, r):
        return self.apply(r)


@pytest.mark.parametrize('stop', [None, 1])
def test_large_rank_pcg_both_stopping_rules(lib_built, stop):
    """one virtual rank that owns every row: dpcg_dot_kernel at 1024 blocks
    under both rules, and under stop type 1 dpcg_r0_kernel's two further
    partial regions (||r||^2, ||b||^2), each read at nb = 1024.  Reference: the
    cbc.block rule is mamg_oracle.pcg; stop type 1 is the host loop around the
    oracle's apply, as tests/pcg_edges_ref.py"""
    import torch
    M = _mamg()
    A, W, idofs = ke.big_problem()
    b = ke.big_rhs(1234)
    tol = 1e-6 if stop else 1e-8
    h = M.DistMetricAMG(A, W, idofs=idofs, rank=0, nranks=1, comm_id=None, **ke.big_c_params('v_default'))
    assert h.local_size == b.size > ke.DOT_CAP
    cg = M.DistConjGrad.for_handles([h], device=True, tolerance=tol, maxiter=500, stop_type=stop)
    xs = cg.solve([_cuda(h.local_slice(b))])
    torch.cuda.synchronize()
    x = xs[0].cpu().numpy()
    h.close()
    oracle = ke.big_restatement('v_default')
    if stop:
        host = M.ConjGrad(A, precond=_OracleB(oracle.apply), tolerance=tol, maxiter=500, device=False, stop_type=1)
        with warnings.catch_warnings():
            warnings.simplefilter('error')
            xo = host * b
        res, norms = host.residuals, host.residual_norms
    else:
        ref = mo.pcg(A, oracle, b, tol, 500)
        xo, res, norms = ref.x, ref.residuals, None
    print('stop %s: PCG iterations %d (reference %d), x rel err %.3e' % (stop, len(cg.residuals) - 1, len(res) - 1,
                                                                        rel(x, xo)))
    assert not cg.breakdown and len(cg.residuals) == len(res)
    assert np.allclose(cg.residuals, res, rtol=1e-6, atol=0)
    if stop:
        assert len(cg.residual_norms) == len(norms)
        assert np.allclose(cg.residual_norms, norms, rtol=1e-6, atol=0)
    assert rel(x, xo) < 1e-6


def test_large_apply_on_a_user_stream(big):
    """one apply of the scaled K case on a user stream behind pending work
    (tests/stream_cases.py): bitwise the default-stream result of the same
    handle and buffers"""
    import torch
    name = 'k_sgs_scaling_m2'
    s1, _ = st.streams()
    B, T = big(name), ke.big_handle(name)
    src = _cuda(ke.big_rhs(7))
    rb, zb = torch.full_like(src, float('nan')), torch.full_like(src, float('nan'))
    tr, tz = src.clone(), torch.empty_like(src)
    call_ms = st.host_ms(lambda: T.apply_device(tr, tz))
    st.behind_delay('large kcycle apply', s1, call_ms, lambda: rb.copy_(src), lambda: B.apply_device(rb, zb, s1))
    zu = zb.clone()
    zb.fill_(float('nan'))
    B.apply_device(rb, zb)
    torch.cuda.synchronize()
    assert torch.equal(zu, zb)
    assert rel(zu.cpu().numpy(), ke.big_reference(name, 7)) < TOL
    T.close()
