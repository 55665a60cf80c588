"""The cases of the nonlinear AMLI (K-cycle) tests, shared by
tests/test_kcycle_ref.py (CPU) and tests/test_gpu_kcycle.py (GPU): the
restatement (tests/kcycle_ref.py) of each case and its applies to the two
seeded vectors are computed once per process.  A helper, not a test.

Sizes: the smallest that give Krylov levels (levels 1 .. coarsest - 1) above
and inside the coarse tail.
"""
import functools

import numpy as np

import kcycle_ref as kc
import mamg_oracle as mo
import pointgs_ref as pr
import pointrings_ref as rr

NL_AMLI = 4
SEEDS = (1234, 7)
UA = dict(AMG_type='UA', aggregation_type='HEM')
SMO = {'JACOBI': 1, 'L1DIAG': 2, 'JACOBI_RHO': 3, 'GS': 10, 'SGS': 11, 'POLY': 12}

# name -> (kind, system, oracle keywords, amli_degree, least number of levels)
#   'nodal':  bidomain (dim, n, gamma), num_functions 2, BSR2 layout (mamg_oracle.Hierarchy)
#   'point':  the same system as a scalar one, CSR layout, point-wise SGS (pointgs_ref.PointGS)
#   'scalar': the same, Jacobi default (mamg_oracle.Hierarchy)
#   'rings':  3D-1D, the seed rings on level 0 (pointrings_ref.PointRings)
CASES = {
    'ua2d_sgs_m2': ('nodal', (2, 64, 1e4), dict(UA, smoother='SGS'), 2, 4),
    'ua2d_sgs_m3': ('nodal', (2, 64, 1e4), dict(UA, smoother='SGS'), 3, 4),
    # the components of parameters_metric_kcycle
    'ua3d_sgs_scaling_m2': ('nodal', (3, 16, 1e6), dict(UA, smoother='SGS', coarse_scaling=1), 2, 4),
    # Jacobi: the K-post fused path (e is read by the prolongation's epilogue)
    'ua3d_jacobi_m2': ('nodal', (3, 16, 1e6), dict(UA), 2, 4),
    # default SA profile: 3 levels, the only Krylov level is level 1 (rhs from the fused restriction)
    'sa2d_m2': ('nodal', (2, 64, 1e3), dict(), 2, 3),
    'sa2d_poly_m2': ('nodal', (2, 64, 1e3), dict(smoother='POLY'), 2, 3),
    # SA + SGS: level 1 is the Krylov level and the coarse tail's level (its cycle has no K op inside: one
    # tail program per (right-hand side, result) pair of the inner CG)
    'sa2d_sgs_m2': ('nodal', (2, 64, 1e3), dict(smoother='SGS'), 2, 3),
    'ua2d_sgs_m1': ('nodal', (2, 64, 1e4), dict(UA, smoother='SGS'), 1, 4),
    'ua3d_jacobi_nu2_m2': ('nodal', (3, 16, 1e6), dict(UA, presmooth_iter=2, postsmooth_iter=2), 2, 4),
    'ua2d_sgs_maxit2_m2': ('nodal', (2, 64, 1e4), dict(UA, smoother='SGS', maxit=2), 2, 4),
    'scalar_sgs_point_m2': ('point', (2, 64, 1e4), dict(UA, num_functions=1), 2, 4),
    'scalar_jacobi_m2': ('scalar', (2, 64, 1e4), dict(UA, num_functions=1), 2, 4),
    # parameters_metric_3d1d_rings as it is at the smallest size of tests/test_gpu_point_rings.py: two
    # levels, so the visit is the dense solve (cycle_ops_csr_rings' call of the visit builder) ...
    'rings_3d1d_m2': ('rings', (8, 1e6, 0.0), dict(coarse_dof=300), 2, 2),
    # ... and with coarse_dof lowered until level 1 is a Krylov level
    'rings_3d1d_deep_m2': ('rings', (8, 1e6, 0.0), dict(coarse_dof=20), 2, 3),
}
# the oracle's names of parameters_metric_3d1d_rings' values (SMOOTHER_JACOBI_RHO below the rings)
RINGS_KW = dict(AMG_type='SA', aggregation_type='MIS', max_levels=30, Schwarz_maxlvl=2, Schwarz_mmsize=200,
                num_functions=1)
APPLY_CASES = tuple(CASES)


def _mamg():
    import metric_amg_examples_amd as M
    return M


@functools.lru_cache(maxsize=None)
def problem(kind, sys_):
    """(A, W, idofs) of a case's system"""
    M = _mamg()
    if kind == 'rings':
        s = M.problems.emi_3d1d(*sys_)
        return s.scipy(), None, np.asarray(s.idofs, np.int32)
    s = M.problems.bidomain(*sys_)
    if kind == 'nodal':
        return s.scipy(), s.W, np.asarray(s.idofs, np.int32)
    return s.scipy(), None, None


@functools.lru_cache(maxsize=None)
def restatement(name, visit='K'):
    """the case's CPU restatement with the given coarse visit"""
    kind, sys_, kw, m, _ = CASES[name]
    A, W, idofs = problem(kind, sys_)
    if kind == 'nodal':
        return kc.KCycle(mo.setup(A, mo.Params(num_functions=2, **kw), idofs=idofs), m, visit)
    if kind == 'scalar':
        return kc.KCycle(mo.setup(A, mo.Params(**kw)), m, visit)
    if kind == 'point':
        return kc.KPointGS(pr.PointGS(A, 'SGS', **kw), m, visit)
    return kc.KPointRings(rr.PointRings(A, idofs, 'JACOBI_RHO', **dict(RINGS_KW, **kw)), m, visit)


def rhs(name, seed):
    kind, sys_ = CASES[name][:2]
    return mo.seeded_rhs(problem(kind, sys_)[0].shape[0], seed)


@functools.lru_cache(maxsize=None)
def reference(name):
    """{seed: K-cycle apply of the restatement}, computed once and left unchanged"""
    ref = restatement(name)
    out = {seed: ref.apply(rhs(name, seed)) for seed in SEEDS}
    for v in out.values():
        v.setflags(write=False)
    return out


def c_params(name):
    """the library's parameter dict of a case"""
    kind, sys_, kw, m, _ = CASES[name]
    k = dict(cycle_type=NL_AMLI, amli_degree=m)
    if kind == 'rings':
        return dict(_mamg().parameters.parameters_metric_3d1d_rings, **dict(kw, **k))
    c = dict(kw)
    smo = c.pop('smoother', None)
    c = dict(pr.to_c(c), **k)
    if kind == 'point':
        c['smoother'] = pr.SMOOTHER['SGS']
    elif smo is not None:
        c['smoother'] = SMO[smo]
        if smo in ('GS', 'SGS'):
            c['Schwarz_type'] = 7        # the level-0 seed blocks take the level smoother (SCHWARZ_SEED_BLOCKS)
    if kind == 'nodal':
        c['num_functions'] = 2
    return c


def handle(name, setup='auto', **extra):
    """the case on the GPU"""
    kind, sys_ = CASES[name][:2]
    A, W, idofs = problem(kind, sys_)
    M = _mamg()
    return M.MetricAMG(A, W, idofs=idofs, setup=setup, **dict(c_params(name), **extra))


def rel(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)
