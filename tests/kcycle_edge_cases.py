"""The cases of tests/test_kcycle_edges_ref.py (CPU) and
tests/test_gpu_kcycle_edges.py (GPU): the K-cycle's dropped directions on
indefinite systems, and the reductions past their grid caps.  A helper, not a
test.

Indefinite systems.  A - sigma I with A = bidomain(2, 64, 1e4) (field-major,
the W and idofs of the unshifted system).  A's diagonal is at least 1 and its
lowest eigenvalues are 0.0059, 0.0117, 0.0237, 0.0291, ...: a sigma in
[0.03, 0.05] makes the operator of every level indefinite while every diagonal
entry, every smoother block and every pivot of the coarsest Gauss-Jordan
stays positive (sigma = 0.07 is the first value the setup refuses).  There the
inner CG meets d_j = <p_j, A_c p_j> <= 0 and the coarse scaling meets
<A_c e, e> <= 0, which no SPD system reaches.

Large system.  bidomain(2, 384, 1e4) with UA / HEM: 296 450 dofs on level 0
(above DOT_BLOCKS * 256 = 262 144, the PCG dots' grid cap) and 79 132 on level 1
(above SCALE_BLOCKS * 256 = 65 536, the cap of the coarse scaling's and the
K-cycle's reductions: a second grid-stride pass over 13 596 entries that ends
in a partial block).

Everything here is built once per process and left unchanged.
"""
import contextlib
import dataclasses
import functools

import numpy as np
import scipy.sparse as sp

import kcycle_cases as kc
import kcycle_ref as kr
import mamg_oracle as mo

SEEDS = kc.SEEDS
UA = kc.UA
SYSTEM = (2, 64, 1e4)
SIGMA_REFUSED = 0.07
SCALE_CAP = 256 * 256        # SCALE_BLOCKS blocks of 256 threads (csrc/device_int.h)
DOT_CAP = 1024 * 256         # DOT_BLOCKS blocks of 256 threads

# name -> (kind, sigma, oracle keywords, amli_degree, visit); kinds as tests/kcycle_cases.py
INDEFINITE = {
    'sgs_m3': ('nodal', 0.05, dict(UA, smoother='SGS'), 3, 'K'),
    'sgs_scaling_m2': ('nodal', 0.05, dict(UA, smoother='SGS', coarse_scaling=1), 2, 'K'),
    # Jacobi: the K-post fused path, and three earlier directions (kdot_kernel<3>, korth_kernel<3>)
    'jacobi_m4': ('nodal', 0.03, dict(UA), 4, 'K'),
    # the CSR layout's visit builder (coarse_visit_ops_csr)
    'scalar_jacobi_m2': ('scalar', 0.05, dict(UA, num_functions=1), 2, 'K'),
    # no K op: cscale_kernel's alpha = 1 on the BSR2 layout
    'w_sgs_scaling': ('nodal', 0.05, dict(UA, smoother='SGS', coarse_scaling=1, cycle_type='W'), 2, 'W'),
}
K_CASES = tuple(n for n, c in INDEFINITE.items() if c[4] == 'K')
# the K cases the coarse tail expresses (the BSR2 layout; Jacobi has a tail level under MAMG_TAIL_NODES only)
# -- not the scalar case: the tail refuses the CSR layout (tests/test_gpu_kcycle_tail.py::test_refusals)
TAIL_CASES = {'sgs_m3': None, 'sgs_scaling_m2': None, 'jacobi_m4': 1024}


def _mamg():
    import metric_amg_examples_amd as M
    return M


# ------------------------------------------------------------------ systems
@functools.lru_cache(maxsize=None)
def shifted(kind, sigma):
    """(A - sigma I, W, idofs): kind 'nodal' or 'scalar' as kcycle_cases.problem"""
    A, W, idofs = kc.problem(kind, SYSTEM)
    S = sp.csr_matrix(A - sigma * sp.identity(A.shape[0], format='csr'))
    S.sort_indices()
    return S, W, idofs


def oracle_params(name):
    kind, _, kw, _, _ = INDEFINITE[name]
    return mo.Params(**(dict(kw, num_functions=2) if kind == 'nodal' else kw))


@functools.lru_cache(maxsize=None)
def hierarchy(name):
    kind, sigma = INDEFINITE[name][:2]
    A, _, idofs = shifted(kind, sigma)
    return mo.setup(A, oracle_params(name), idofs=idofs)


def restatement(name, trace=None, guards=True):
    """the case's restatement (one hierarchy per case; the restatement itself
    is a thin object, so a traced or an unguarded one is built per call)"""
    _, _, _, m, visit = INDEFINITE[name]
    return kr.KCycle(hierarchy(name), m, visit, trace=trace, guards=guards)


def rhs(name, seed):
    return mo.seeded_rhs(shifted(*INDEFINITE[name][:2])[0].shape[0], seed)


@functools.lru_cache(maxsize=None)
def reference(name):
    """{seed: apply of the restatement}; the W case is mamg_oracle's own cycle"""
    ref = hierarchy(name) if INDEFINITE[name][4] == 'W' else restatement(name)
    out = {seed: ref.apply(rhs(name, seed)) for seed in SEEDS}
    for v in out.values():
        v.setflags(write=False)
    return out


def c_params(name):
    """the library's parameter dict of a case"""
    kind, _, kw, m, visit = INDEFINITE[name]
    c = dict(kw)
    smo = c.pop('smoother', None)
    c.pop('cycle_type', None)
    c = kc.pr.to_c(c)
    c.update(dict(cycle_type=kc.NL_AMLI, amli_degree=m) if visit == 'K' else dict(cycle_type=2))
    if smo is not None:
        c['smoother'] = kc.SMO[smo]
        c['Schwarz_type'] = 7        # the level-0 seed blocks take the level smoother (SCHWARZ_SEED_BLOCKS)
    if kind == 'nodal':
        c['num_functions'] = 2
    return c


def handle(name, setup='auto', **extra):
    """the case on the GPU"""
    A, W, idofs = shifted(*INDEFINITE[name][:2])
    return _mamg().MetricAMG(A, W, idofs=idofs, setup=setup, **dict(c_params(name), **extra))


# ------------------------------------------------------------------ census
def visits(trace):
    """a KCycle trace as [(level, [(d, ||p|| ||q||), ...])], one entry per K visit
    (a level's visits do not nest, so its steps appear in order)"""
    out, cur = [], {}
    for level, step, d, pq in trace:
        if step == 0:
            cur[level] = []
            out.append((level, cur[level]))
        cur[level].append((d, pq))
    return out


@contextlib.contextmanager
def scaling_recorded(log):
    """mamg_oracle.coarse_scale wrapped for the length of the block: every
    call appends (<A_c e, e>, ||e|| ||A_c e||) to log; the oracle is not edited
    and its result is returned as it is"""
    inner = mo.coarse_scale

    def recording(Ac, bc, e):
        q = Ac @ e
        log.append((float(np.dot(e, q)), float(np.linalg.norm(e) * np.linalg.norm(q))))
        return inner(Ac, bc, e)
    mo.coarse_scale = recording
    try:
        yield log
    finally:
        mo.coarse_scale = inner


@functools.lru_cache(maxsize=None)
def census(name, seed):
    """what one apply of the case met, and how decisively:
    visits        [(level, [(d, ||p|| ||q||), ...])]
    scalings      [(den, ||e|| ||A_c e||)]
    margin        the smallest |d| / (||p|| ||q||) and |den| / (||e|| ||A_c e||) over the non-zero ones
    zeros         number of steps / scalings with ||p|| ||q|| = 0 or ||e|| ||A_c e|| = 0
    moved         relative change of the apply under a relative 1e-13 perturbation of r
    unguarded     {guards kept: relative distance of the apply without the others}, inf where that apply
                  is not finite: () is the cycle that always divides, and one entry per pair of kept guards
                  shows what the third guard alone decides"""
    r = rhs(name, seed)
    trace, scal = [], []
    with scaling_recorded(scal):
        ref = hierarchy(name) if INDEFINITE[name][4] == 'W' else restatement(name, trace)
        z = ref.apply(r)
    assert np.array_equal(z, reference(name)[seed])
    vs = visits(trace)
    cos = [abs(d) / pq for _, steps in vs for d, pq in steps if pq > 0] + [abs(d) / eq for d, eq in scal if eq > 0]
    zeros = sum(1 for _, steps in vs for d, pq in steps if pq == 0) + sum(1 for d, eq in scal if eq == 0)
    plain = hierarchy(name) if INDEFINITE[name][4] == 'W' else restatement(name)
    rp = r * (1.0 + 1e-13 * np.where(np.arange(r.size) % 2, 1.0, -1.0))
    ung = {}
    for kept in ((), ('beta', 'scale'), ('alpha', 'scale'), ('alpha', 'beta')):
        zu = restatement(name, guards=kept).apply(r)
        ung[kept] = kc.rel(zu, z) if np.isfinite(zu).all() else float('inf')
    return dict(visits=vs, scalings=scal, margin=min(cos), zeros=zeros, moved=kc.rel(plain.apply(rp), z),
                unguarded=ung)


# ------------------------------------------------------------ the large system
BIG = (2, 384, 1e4)
# name -> (oracle keywords, amli_degree or None, visit)
BIG_CASES = {
    'k_sgs_scaling_m2': (dict(UA, smoother='SGS', coarse_scaling=1), 2, 'K'),
    'k_jacobi_m4': (dict(UA), 4, 'K'),
    'w_jacobi_scaling': (dict(UA, coarse_scaling=1, cycle_type='W'), None, 'W'),
    'v_default': (dict(), None, 'V'),
}


def big_problem():
    return kc.problem('nodal', BIG)


@functools.lru_cache(maxsize=None)
def _big_levels(key):
    """one oracle setup per (aggregation, smoother): the cycle type and the
    coarse scaling do not enter the hierarchy"""
    A, _, idofs = big_problem()
    return mo.setup(A, mo.Params(num_functions=2, **dict(key)), idofs=idofs)


def big_hierarchy(name):
    kw = BIG_CASES[name][0]
    base = _big_levels(tuple(sorted((k, v) for k, v in kw.items() if k not in ('coarse_scaling', 'cycle_type'))))
    return mo.Hierarchy(base.levels, dataclasses.replace(
        base.params, coarse_scaling=kw.get('coarse_scaling', 0), cycle_type=kw.get('cycle_type', 'V')))


@functools.lru_cache(maxsize=None)
def big_restatement(name):
    """what the GPU handle of the case is compared with: the K restatement, or
    mamg_oracle's own cycle for V and W"""
    _, m, visit = BIG_CASES[name]
    h = big_hierarchy(name)
    return kr.KCycle(h, m, 'K') if visit == 'K' else h


def big_rhs(seed):
    return mo.seeded_rhs(big_problem()[0].shape[0], seed)


@functools.lru_cache(maxsize=None)
def big_reference(name, seed):
    z = big_restatement(name).apply(big_rhs(seed))
    z.setflags(write=False)
    return z


def big_c_params(name):
    kw, m, visit = BIG_CASES[name]
    c = dict(kw)
    smo = c.pop('smoother', None)
    c.pop('cycle_type', None)
    c = dict(kc.pr.to_c(c), num_functions=2)
    if visit == 'K':
        c.update(cycle_type=kc.NL_AMLI, amli_degree=m)
    elif visit == 'W':
        c['cycle_type'] = 2
    if smo is not None:
        c['smoother'] = kc.SMO[smo]
        c['Schwarz_type'] = 7
    return c


def big_handle(name, **extra):
    A, W, idofs = big_problem()
    return _mamg().MetricAMG(A, W, idofs=idofs, **dict(big_c_params(name), **extra))
