"""The cases of tests/test_gpu_tail.py: one table, shared with the CPU checks
of tests/test_tail_cases.py.

The coarse tail (device.hip tail_kernel) runs the cycle below ``tail_level``
as one op program; which branches a handle takes is decided by its planner
(to_tail, tail_res_plan, tail_lds_plan, tail_ops) from the sizes of the
hierarchy.  Every case names the plan it is meant to reach; the sizes that put
it there are pinned here (``HIER``) and checked against the oracle on the CPU,
so a change in coarsening cannot quietly move a case off its branch.  The GPU
tests read the plan a handle really took from ``MetricAMG.tail_info()``.

All systems are the bidomain model problem with ``num_functions=2``; a node
row of a level's A holds one 2x2 block per neighbouring node.
"""
import dataclasses
import functools

import numpy as np
import scipy.sparse as sp

import mamg_oracle as mo

# the planner's constants (device.hip)
TAIL_THREADS = 512                     # one resident row per thread
RES_RB = 12                            # blocks of a resident row held in registers
TAIL_LDS_MAX = 160 * 1024 - 1024       # dynamic LDS of the tail's workgroup
GD_BYTES = 32 * TAIL_THREADS           # the resident region's block inverses

UA = dict(AMG_type='UA', aggregation_type='HEM')

# name -> system (dim, n, gamma), the keys that shape the hierarchy, and per
# level (node rows, max blocks per node row, mean blocks per node row rounded
# to one decimal); the last level is the coarsest (dense solve of 2 x rows dofs)
HIER = {
    'sa3d16': dict(dim=3, n=16, g=1e6, kw={},
                   levels=[(4913, 15, 12.1), (199, 44, 25.5), (7, 7, 7.0)]),
    'sa2d64': dict(dim=2, n=64, g=1e4, kw={},
                   levels=[(4225, 7, 6.7), (412, 15, 10.5), (26, 17, 10.1)]),
    'sa2d64c40': dict(dim=2, n=64, g=1e4, kw=dict(coarse_dof=40),
                      levels=[(4225, 7, 6.7), (412, 15, 10.5), (26, 17, 10.1), (3, 3, 3.0)]),
    'sa2d32': dict(dim=2, n=32, g=1e3, kw={},
                   levels=[(1089, 7, 6.4), (106, 15, 9.8), (7, 7, 5.9)]),
    'ua3d16': dict(dim=3, n=16, g=1e6, kw=UA,
                   levels=[(4913, 15, 12.1), (1109, 21, 13.2), (289, 22, 12.5), (74, 18, 10.7), (20, 11, 8.0)]),
    'ua3d12c40': dict(dim=3, n=12, g=1e6, kw=dict(UA, coarse_dof=40),
                      levels=[(2197, 15, 11.3), (475, 20, 12.4), (125, 19, 11.5), (35, 14, 8.7), (9, 8, 6.3)]),
    'sa3d24': dict(dim=3, n=24, g=1e6, kw={},
                   levels=[(15625, 15, 13.0), (606, 49, 30.1), (12, 12, 10.7)]),
    # the resident region does not fit the LDS (test_tail_cases.test_region_case)
    'sa3d20': dict(dim=3, n=20, g=1e6, kw={},
                   levels=[(9261, 15, 12.6), (360, 47, 27.8), (9, 9, 8.3)]),
    # the dense solve's other two branches: 64 < 148 dofs <= 512 < 578 dofs
    'ua3d16c200': dict(dim=3, n=16, g=1e6, kw=dict(UA, coarse_dof=200),
                       levels=[(4913, 15, 12.1), (1109, 21, 13.2), (289, 22, 12.5), (74, 18, 10.7)]),
    'ua3d16c600': dict(dim=3, n=16, g=1e6, kw=dict(UA, coarse_dof=600),
                       levels=[(4913, 15, 12.1), (1109, 21, 13.2), (289, 22, 12.5)]),
}

ALL_NODES = '100000000'     # MAMG_TAIL_NODES: the tail from level 1


@functools.lru_cache(maxsize=None)
def system(name):
    import metric_amg_examples_amd as M
    hc = HIER[name]
    return M.problems.bidomain(hc['dim'], hc['n'], hc['g'])


@functools.lru_cache(maxsize=None)
def _levels(name, smoother, poly_degree):
    s = system(name)
    return mo.setup(s.scipy(), mo.Params(num_functions=2, smoother=smoother, poly_degree=poly_degree,
                                         **HIER[name]['kw']), idofs=s.idofs)


APPLY_ONLY = ('cycle_type', 'presmooth_iter', 'postsmooth_iter', 'coarse_scaling', 'maxit')


def oracle(name, **kw):
    """The oracle's hierarchy of HIER[name] under kw (mo.Params keys).  The
    keys in APPLY_ONLY are read by the apply alone, so one setup per smoother
    serves every variant (a computed reference, shared and never modified)."""
    kw = dict(kw)
    h = _levels(name, kw.pop('smoother', 'JACOBI_RHO'), kw.pop('poly_degree', 2))
    assert set(kw) <= set(APPLY_ONLY), kw
    return mo.Hierarchy(h.levels, dataclasses.replace(h.params, **kw))


def row_blocks(A):
    """Blocks per node row of a field-major 2-function operator (diagonal included)."""
    nv = A.shape[0] // 2
    r = np.repeat(np.arange(A.shape[0]), np.diff(A.indptr)) % nv
    G = sp.csr_matrix((np.ones(len(r)), (r, A.indices % nv)), shape=(nv, nv))
    G.sum_duplicates()
    return np.diff(G.indptr)


def level_facts(name):
    """(node rows, max blocks, mean blocks to one decimal) per level, from the oracle."""
    out = []
    for lev in oracle(name).levels:
        L = row_blocks(lev.A)
        out.append((len(L), int(L.max()), round(float(L.mean()), 1)))
    return out


def overflow_blocks(name, l):
    """Blocks of level l's rows past RES_RB, each row in whole fours (tail_res_plan)."""
    L = row_blocks(oracle(name).levels[l].A)
    return int(sum((max(0, int(x) - RES_RB) + 3) // 4 * 4 for x in L))


def residency(name, tail_level=1):
    """The plan tail_res_plan makes from the level sizes: levels from
    tail_level down take one thread per row while they fit the workgroup (a
    level that does not fit is skipped, a deeper one may still fit; the
    coarsest level's A is there for the coarse scaling).  Returns (resident
    levels, resident rows, overflow blocks, LDS region bytes without the dense
    inverse)."""
    rows, lv, nov = 0, [], 0
    for l in range(tail_level, len(HIER[name]['levels'])):
        n = HIER[name]['levels'][l][0]
        if rows + n > TAIL_THREADS:
            continue
        lv.append(l)
        rows += n
        nov += overflow_blocks(name, l)
    return lv, rows, nov, GD_BYTES + 34 * nov


class NoTail(mo.Hierarchy):
    """The oracle's cycle with the correction from ``tail_level`` down dropped."""

    def __init__(self, h, tail_level):
        super().__init__(h.levels, h.params)
        self.tail_level = tail_level

    def cycle(self, l, b):
        if l == self.tail_level:
            return np.zeros_like(b)
        return super().cycle(l, b)


SEEDS = (1234, 7)


def rhs(name, seed):
    """The right-hand sides of every tail test (CPU pin and GPU run alike):
    seeded_rhs alone loses 0.3 .. 0.98 of the apply without the tail
    (test_tail_cases.test_rhs_is_sensitive_to_the_tail), so no smooth
    component is added."""
    return mo.seeded_rhs(system(name).N, seed)


def rel(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


SMO = {'JACOBI': 1, 'L1DIAG': 2, 'JACOBI_RHO': 3, 'SGS': 11, 'GS': 10, 'POLY': 12}


def to_c(kw):
    """mo.Params keys -> MetricAMG keywords."""
    c = dict(kw)
    if 'smoother' in c:
        if c['smoother'] in ('SGS', 'GS'):
            c['Schwarz_type'] = 7      # the level-0 seed blocks take the level smoother
        c['smoother'] = SMO[c['smoother']]
    if 'cycle_type' in c:
        c['cycle_type'] = {'V': 1, 'W': 2}[c['cycle_type']]
    if 'AMG_type' in c:
        c['AMG_type'] = {'SA': 2, 'UA': 1}[c['AMG_type']]
    if 'aggregation_type' in c:
        c['aggregation_type'] = {'MIS': 2, 'HEM': 5}[c['aggregation_type']]
    return c


# ---------------------------------------------------------------------------
# the smoother variants run inside the tail (test_gpu_tail.test_families)
# ---------------------------------------------------------------------------
W2S = dict(cycle_type='W', presmooth_iter=2, postsmooth_iter=2, coarse_scaling=1)
FAMILY_VARIANTS = [
    dict(smoother='JACOBI_RHO'),
    dict(smoother='JACOBI_RHO', presmooth_iter=2, postsmooth_iter=2),
    dict(smoother='JACOBI_RHO', cycle_type='W', coarse_scaling=1),
    dict(smoother='L1DIAG', coarse_scaling=1),
    dict(smoother='JACOBI', **W2S),
    dict(smoother='POLY', poly_degree=2),
    dict(smoother='POLY', poly_degree=2, **W2S),
]
FAMILY_HIERS = ['sa3d16', 'sa2d64c40']

# every (hierarchy, oracle keys, tail level) a GPU test applies: the
# sensitivity pin of test_tail_cases covers each with both right-hand sides,
# and test_gpu_tail refuses to apply a combination that is not listed
JAC = dict(smoother='JACOBI_RHO')
SGS = dict(smoother='SGS')
POLY = dict(smoother='POLY', poly_degree=2)
APPLIED = [(hn, v, 1) for hn in FAMILY_HIERS for v in FAMILY_VARIANTS] + [
    ('sa3d16', SGS, 1),
    ('sa3d16', dict(JAC, **W2S), 1),
    ('sa3d16', dict(JAC, coarse_scaling=1), 1),
    ('sa3d16', dict(POLY, coarse_scaling=1), 1),
    ('sa2d64c40', dict(JAC, coarse_scaling=1), 1),
    ('sa2d64c40', JAC, 2),
    ('sa2d64c40', dict(POLY, cycle_type='W', coarse_scaling=1), 2),
    ('sa2d32', dict(JAC, cycle_type='W', coarse_scaling=1), 1),
    ('ua3d16', dict(JAC, **W2S), 1),
    ('ua3d16', JAC, 1),
    ('ua3d12c40', dict(POLY, cycle_type='W', coarse_scaling=1), 1),
    ('sa3d24', JAC, 1),
    ('sa3d24', dict(JAC, coarse_scaling=1), 1),
    ('sa3d20', JAC, 1),
    ('sa3d20', SGS, 1),
    ('ua3d16c200', JAC, 1),
    ('ua3d16c600', JAC, 1),
]


def key(kw):
    return '-'.join('%s' % v for v in kw.values())


def frozen(d):
    return tuple(sorted((d or {}).items()))


APPLIED_KEYS = {(hn, frozen(kw), tl) for hn, kw, tl in APPLIED}
