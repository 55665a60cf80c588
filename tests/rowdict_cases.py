"""Inputs and numpy counts for the row-pattern dictionary of a level-0 A
(DESIGN.md section 3), shared by tests/test_rowdict_cases.py (CPU) and
tests/test_gpu_rowdict.py.

A node row of the field-major 2-function matrix A is the sequence of its 2x2
blocks (J, [[A[I, J], A[I, J + nv]], [A[I + nv, J], A[I + nv, J + nv]]]) over
the union of the four sub-patterns, in column order.  Its type is the sequence
of (J - I, the four doubles bitwise); the dictionary layout is taken when the
types are few and every row is short.
"""
import functools

import numpy as np
import scipy.sparse as sp

import irregular
import mamg_oracle as mo

GAMMA = 1e6
# the builder's defaults (csrc/opts.h)
MAX_TYPES, MAX_LEN = 256, 32


def node_rows(A, nv):
    """(type id per node row, number of types, longest row in blocks)."""
    A = sp.csr_matrix(A)
    parts = [A[:nv, :nv], A[:nv, nv:], A[nv:, :nv], A[nv:, nv:]]
    pat = sp.csr_matrix((nv, nv))
    for p in parts:
        q = p.copy().tocsr()
        q.data = np.ones_like(q.data)
        pat = pat + q
    pat = pat.tocsr()
    pat.sort_indices()
    rows = np.repeat(np.arange(nv), np.diff(pat.indptr))
    cols = pat.indices
    vals = np.stack([np.asarray(p[rows, cols]).ravel() for p in parts], axis=1)
    bits = np.ascontiguousarray(vals).view(np.int64)
    delta = (cols - rows).astype(np.int64)
    types = {}
    code = np.empty(nv, np.int64)
    for i in range(nv):
        a, b = pat.indptr[i], pat.indptr[i + 1]
        key = (delta[a:b].tobytes(), bits[a:b].tobytes())
        code[i] = types.setdefault(key, len(types))
    return code, len(types), int(np.diff(pat.indptr).max())


@functools.lru_cache(maxsize=None)
def grid(dim, n):
    return irregular.grid(dim, n, GAMMA)


def interior_pair(n):
    """An interior node of the 3-D n-cell mesh and its +x neighbour."""
    m = n + 1
    i = (n // 2) * m * m + (n // 2) * m + n // 2
    return i, i + 1


@functools.lru_cache(maxsize=None)
def perturbed(n, mirror):
    """3-D grid with the block (I, J) of one interior edge scaled by
    1 + 2^-40, and its mirror (J, I) too if `mirror` (A stays bitwise
    symmetric) -- without it the half-symmetric layout is refused."""
    A, nv, idofs = grid(3, n)
    A = A.tocsr().copy()
    i, j = interior_pair(n)
    s = 1.0 + 2.0 ** -40
    hit = 0
    for (r, c) in ([(i, j), (j, i)] if mirror else [(i, j)]):
        for fr in (0, 1):
            for fc in (0, 1):
                R, Cc = r + fr * nv, c + fc * nv
                for k in range(A.indptr[R], A.indptr[R + 1]):
                    if A.indices[k] == Cc:
                        A.data[k] *= s
                        hit += A.data[k] != 0.0
    assert hit >= 2, hit
    return A, nv, idofs


# refused inputs, as tests/test_gpu_cycle_storage.py builds them
REFUSED = {
    'permuted2d-32': lambda: irregular.permuted(2, 32, GAMMA),
    'ragged96': lambda: irregular.ragged(96, GAMMA),
    # one row of 500 neighbours: longer than the builder's 32 blocks
    'hub32-m500': lambda: irregular.hub(32, GAMMA, 500, 1.0, 4),
}
