"""Inputs whose node count is not (n + 1)^d.

Every other parity test feeds the library a square or cubic grid with an even
n, so the level-0 node count is always odd and, for the n in use, 1, 9, 17,
25, 33 or 49 mod 64.  The hand-written kernels take their index decisions --
`slot >= nr` guards, dead-lane mirroring, slice offsets, rows per workgroup,
patches per wave -- from exactly that count.  The generators here cut a grid
system down to any node count while staying SPD, field-major [u1; u2] and
bitwise symmetric:

  truncated(dim, n, gamma, m)        the principal submatrix of
                                     bidomain_system(dim, n, gamma) on nodes
                                     [0, m) of both fields: A[q][:, q],
                                     q = [0..m) U nv + [0..m)
  truncated_rows(dim, n, gamma, k)   A[:k, :k], for the scalar (CSR layout)
                                     tests: odd and even row counts

A principal submatrix of an SPD matrix is SPD, mirrors stay bitwise equal and
the rows keep the grid's band structure, so the half-symmetric padding rule
accepts the nodal cases (irregular.half_rule).  numpy / scipy / the oracle
only.
"""
import dataclasses
import functools

import numpy as np
import scipy.sparse as sp

import mamg_oracle as mo


def _finish(A):
    A = sp.csr_matrix(A)
    A.sum_duplicates()
    A.sort_indices()
    A.indptr = A.indptr.astype(np.int64)
    A.indices = A.indices.astype(np.int64)
    return A


@functools.lru_cache(maxsize=None)
def _grid(dim, n, gamma):
    o = mo.bidomain_system(dim, n, gamma)
    return o['A'].tocsr(), o['nv']


@functools.lru_cache(maxsize=None)
def truncated(dim, n, gamma, m):
    """(A, m, idofs): nodes [0, m) of both fields of bidomain_system(dim, n, gamma)."""
    A, nv = _grid(dim, n, gamma)
    if not 1 <= m <= nv:
        raise ValueError('truncated: m=%d outside [1, %d]' % (m, nv))
    q = np.concatenate([np.arange(m), nv + np.arange(m)])
    return _finish(A[q][:, q]), m, np.arange(m, 2 * m, dtype=np.int32)


@functools.lru_cache(maxsize=None)
def truncated_rows(dim, n, gamma, k):
    """The leading k x k block of bidomain_system(dim, n, gamma)'s matrix."""
    A, nv = _grid(dim, n, gamma)
    if not 1 <= k <= A.shape[0]:
        raise ValueError('truncated_rows: k=%d outside [1, %d]' % (k, A.shape[0]))
    return _finish(A[:k][:, :k])


# ---------------------------------------------------------------------------
# the sizes, each standing for a boundary
# ---------------------------------------------------------------------------
# every hierarchy is built with coarse_dof = 4, so that even the tiny sizes
# keep a level 0 with a K operator and a restriction
COARSE_DOF = 4

# from 2-D n = 16 (289 nodes)
TINY = [
    1,      # 2 dofs: one dense level, no level-0 kernel at all
    2,      # 4 dofs = coarse_dof: still one dense level
    3,      # the smallest two-level hierarchy; fewer node rows than the 8 XCDs (row_block_of)
    7,      # one row short of the XCD count
    8,      # exactly one row per XCD
    9,      # one more; three levels; still far below a wavefront's 32 rows at two lanes per row
]
SLICE = [
    31, 32, 33,         # a wavefront's share of a SELL slice at two lanes per row
    63, 64, 65,         # one SELL-64 slice: one row short, no partial slice, one row into the second
    127, 128, 129,      # the 128 rows a workgroup of msell_kernel<LPR = 2> covers; 256 / VL rows at VL = 2
    191, 192,           # three slices, a multiple of 64 that is no multiple of 128
    255, 256, 257,      # a whole workgroup of one lane per row; four slices
]
# from 3-D n = 8, gamma = 1e6 (729 nodes): rows reach 15 blocks; the first 81
# nodes are the Dirichlet plane, so no smaller m
STENCIL3D = [255, 256, 257, 511, 512, 513]
# from 2-D n = 32 (1089 nodes) and 2-D n = 64 (4225 nodes)
BIG32 = [1023, 1024, 1025]
BIG64 = [2047, 2048, 2049, 4095, 4096, 4097]
# scalar rows of 2-D n = 64, gamma = 1e4: 4096 / 4097 is the boundary between
# csr_gs_small_kernel (one workgroup, x in LDS) and the colour-by-colour launches
SCALAR = [1023, 1024, 1025, 4095, 4096, 4097]
GS_SMALL_MAX_ROWS = 4096        # csrc/device.hip GS_SMALL_MAX

# family -> (dim, n, gamma, sizes)
FAMILIES = {
    'tiny': (2, 16, 1e3, TINY),
    'slice': (2, 16, 1e3, SLICE),
    'stencil3d': (3, 8, 1e6, STENCIL3D),
    'big32': (2, 32, 1e3, BIG32),
    'big64': (2, 64, 1e4, BIG64),
}
SCALAR_GRID = (2, 64, 1e4)

# the sizes that also run W / POLY, the layout variants, the other smoothers
WP_SIZES = {63, 64, 65, 255, 256, 257, 511, 512, 513}
VARIANT_SIZES = {63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513}
SMOOTHER_SIZES = {63, 64, 65, 255, 256, 257}


def nodal_cases(families=tuple(FAMILIES)):
    """[(family, m)] in the order the GPU file runs them."""
    return [(f, m) for f in families for m in FAMILIES[f][3]]


def case_id(c):
    return '%s-%d' % c


def nodal(family, m):
    dim, n, g, sizes = FAMILIES[family]
    return truncated(dim, n, g, m)


def scalar(k):
    return truncated_rows(*SCALAR_GRID, k)


# dofs per level of the oracle's hierarchy (default parameters, coarse_dof = 4);
# pinned so that a change in coarsening shows up in tests/test_size_cases.py
# and not as the silent loss of a multi-level case
HIER = {
    ('tiny', 1): [2], ('tiny', 2): [4],                     # one dense level
    ('tiny', 3): [6, 2], ('tiny', 7): [14, 4], ('tiny', 8): [16, 4],
    ('tiny', 9): [18, 6, 2],
    ('slice', 31): [62, 10, 4], ('slice', 32): [64, 10, 4], ('slice', 33): [66, 10, 4],
    ('slice', 63): [126, 16, 4], ('slice', 64): [128, 18, 4], ('slice', 65): [130, 16, 4],
    ('slice', 127): [254, 26, 2], ('slice', 128): [256, 26, 2], ('slice', 129): [258, 26, 2],
    ('slice', 191): [382, 38, 4], ('slice', 192): [384, 38, 4],
    ('slice', 255): [510, 46, 4], ('slice', 256): [512, 46, 4], ('slice', 257): [514, 48, 6, 2],
    ('stencil3d', 255): [510, 26, 2], ('stencil3d', 256): [512, 26, 2], ('stencil3d', 257): [514, 26, 2],
    ('stencil3d', 511): [1022, 52, 4], ('stencil3d', 512): [1024, 52, 4], ('stencil3d', 513): [1026, 52, 4],
    ('big32', 1023): [2046, 200, 14, 2], ('big32', 1024): [2048, 200, 14, 2], ('big32', 1025): [2050, 200, 14, 2],
    ('big64', 2047): [4094, 416, 30, 2], ('big64', 2048): [4096, 416, 30, 2], ('big64', 2049): [4098, 416, 30, 2],
    ('big64', 4095): [8190, 802, 54, 4], ('big64', 4096): [8192, 802, 54, 4], ('big64', 4097): [8194, 802, 54, 4],
}
HIER_SCALAR = {
    1023: [1023, 107, 8, 1], 1024: [1024, 107, 8, 1], 1025: [1025, 107, 8, 1],
    4095: [4095, 401, 27, 2], 4096: [4096, 401, 27, 2], 4097: [4097, 401, 27, 2],
}


# ---------------------------------------------------------------------------
# the reference side, computed once per session and never modified
# ---------------------------------------------------------------------------
def _frozen(kw):
    return tuple(sorted(kw.items()))


@functools.lru_cache(maxsize=None)
def _nodal_setup(family, m, smoother, kw):
    A, nv, idofs = nodal(family, m)
    return mo.setup(A, mo.Params(num_functions=2, coarse_dof=COARSE_DOF, smoother=smoother, **dict(kw)), idofs=idofs)


def oracle(family, m, cycle='V', smoother='JACOBI_RHO', **kw):
    """The oracle's hierarchy of a nodal case; the cycle type is read by the
    apply only, so the V and W hierarchies share their levels."""
    h = _nodal_setup(family, m, smoother, _frozen(kw))
    return mo.Hierarchy(h.levels, dataclasses.replace(h.params, cycle_type=cycle))


@functools.lru_cache(maxsize=None)
def _scalar_setup(k, smoother):
    return mo.setup(scalar(k), mo.Params(num_functions=1, coarse_dof=COARSE_DOF, smoother=smoother))


def oracle_scalar(k, cycle='V', smoother='JACOBI_RHO'):
    h = _scalar_setup(k, smoother)
    return mo.Hierarchy(h.levels, dataclasses.replace(h.params, cycle_type=cycle))


def level_dofs(h):
    return [lv.A.shape[0] for lv in h.levels]


SEEDS = (1234, 7)
