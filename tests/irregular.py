"""Deterministic inputs that are not grids in grid order.

Every -m gpu parity test used to feed the library a lexicographically ordered
tensor-grid matrix: rows of at most 30 entries, upper and lower row halves of
equal length, neighbouring rows reaching neighbouring columns.  The generators
here break each of those properties while staying SPD, field-major [u1; u2]
and bitwise symmetric (so the half-symmetric layout is decided by its padding
rule, never by the mirror check):

  permuted(dim, n, gamma, seed)   the bidomain system under one random node
                                  renumbering (both fields alike)
  hub(n, gamma, m, w, seed)       2-D bidomain + one interior node joined to m
                                  others (one very long row)
  ragged(n, gamma, seed)          2-D bidomain + a geometric number of
                                  long-range edges per node (row lengths vary
                                  inside every 64-row slice)

Each returns (A, nv, idofs): A scipy CSR with sorted indices, nv nodes,
idofs = the second field's dofs.  numpy / scipy / the oracle only.
"""
import functools

import numpy as np
import scipy.sparse as sp

import mamg_oracle as mo


def _finish(A, nv):
    A = sp.csr_matrix(A)
    A.sum_duplicates()
    A.sort_indices()
    A.indptr = A.indptr.astype(np.int64)
    A.indices = A.indices.astype(np.int64)
    return A, nv, np.arange(nv, 2 * nv, dtype=np.int32)


def _free_nodes(o):
    """Nodes that carry no Dirichlet condition."""
    nv = o['nv']
    return np.flatnonzero(~o['bc'][:nv])


def _with_edges(A, nv, ei, ej, w):
    """A + blockdiag(L, L), L = the graph Laplacian of the (distinct,
    unordered, loop-free) edges (ei, ej) with weight w: -w off the diagonal,
    w * degree on it.  L is assembled without duplicate entries, so every
    entry of the sum is one floating-point addition and mirrors stay bitwise
    equal; L is positive semidefinite, so A stays SPD."""
    deg = np.bincount(np.concatenate([ei, ej]), minlength=nv)
    d = np.flatnonzero(deg)
    rows = np.concatenate([ei, ej, d])
    cols = np.concatenate([ej, ei, d])
    vals = np.concatenate([np.full(2 * len(ei), -w), w * deg[d].astype(np.float64)])
    L = sp.csr_matrix((vals, (rows, cols)), shape=(nv, nv))
    return A + sp.block_diag([L, L], format='csr')


@functools.lru_cache(maxsize=None)
def permuted(dim, n, gamma=1e3, seed=0):
    """bidomain_system(dim, n, gamma) with nodes renumbered by one random
    permutation p: A[q][:, q], q = [p, p + nv]."""
    o = mo.bidomain_system(dim, n, gamma)
    nv = o['nv']
    p = np.random.default_rng(seed).permutation(nv)
    q = np.concatenate([p, p + nv])
    return _finish(o['A'].tocsr()[q][:, q], nv)


def hub_node(n):
    """The interior node the hub generator joins to the others."""
    return (n // 2) * (n + 1) + n // 2


@functools.lru_cache(maxsize=None)
def hub(n, gamma=1e3, m=500, w=1.0, seed=0):
    """2-D bidomain, node hub_node(n) joined to m random non-Dirichlet nodes
    by Laplacian edges of weight w in both diagonal field blocks."""
    o = mo.bidomain_system(2, n, gamma)
    nv = o['nv']
    c = hub_node(n)
    free = _free_nodes(o)
    free = free[free != c]
    if m > len(free):
        raise ValueError('hub: m=%d exceeds the %d free nodes' % (m, len(free)))
    nb = np.sort(np.random.default_rng(seed).choice(free, size=m, replace=False))
    return _finish(_with_edges(o['A'], nv, np.full(m, c, np.int64), nb, w), nv)


@functools.lru_cache(maxsize=None)
def ragged(n, gamma=1e3, seed=0, w=1e-3):
    """2-D bidomain, every non-Dirichlet node with k_i extra edges of weight w
    to random non-Dirichlet nodes; k_i geometric (mean 2), capped at 64."""
    o = mo.bidomain_system(2, n, gamma)
    nv = o['nv']
    rng = np.random.default_rng(seed)
    free = _free_nodes(o)
    k = np.minimum(rng.geometric(0.5, size=len(free)), 64)
    ei = np.repeat(free, k)
    ej = free[rng.integers(0, len(free), size=len(ei))]
    keep = ei != ej
    lo, hi = np.minimum(ei, ej)[keep], np.maximum(ei, ej)[keep]
    e = np.unique(lo * nv + hi)
    return _finish(_with_edges(o['A'], nv, e // nv, e % nv, w), nv)


# ---------------------------------------------------------------------------
# named cases shared by tests/test_irregular_host.py and tests/test_gpu_irregular.py
# ---------------------------------------------------------------------------
# name -> (generator, oracle parameters)
CASES = {
    'permuted2d-64': (lambda: permuted(2, 64, 1e4, 2), {}),
    'permuted3d-16': (lambda: permuted(3, 16, 1e6, 3), {}),
    'permuted2d-256': (lambda: permuted(2, 256, 1e3, 4), {}),
    'ragged96': (lambda: ragged(96, 1e3, 5), {}),
    # strong_coupled 0: the hub and its 3000 neighbours are one aggregate, the
    # graph collapses within two levels (18818 / 1710 / 2 dofs) and A_1 is
    # nearly dense; 0.25: 18818 / 2448 / 210 / 2
    'hub96-m3000': (lambda: hub(96, 1e3, 3000, 1.0, 4), {}),
    'hub96-m3000-theta0.25': (lambda: hub(96, 1e3, 3000, 1.0, 4), dict(strong_coupled=0.25)),
}
# part g: 66000 neighbours (> 65535) on nv = 273^2 = 74529 nodes.  The hub
# edges are weak (1e-6 against couplings of ~1, strong_coupled 0.25) and the
# prolongator is unsmoothed, so the hub row stays one long row of A_0 instead
# of making every coarse operator dense: setup and oracle stay at ~1 s.
LONG_ROW = (lambda: hub(272, 1e3, 66000, 1e-6, 9), dict(strong_coupled=0.25, AMG_type='UA'))
# smaller inputs for the layout rule and the setup parity
SMALL = {
    'permuted2d-32': lambda: permuted(2, 32, 1e3, 1),
    'permuted2d-64': CASES['permuted2d-64'][0],
    'permuted3d-8': lambda: permuted(3, 8, 1e6, 3),
    'hub32-m500': lambda: hub(32, 1e3, 500, 1.0, 4),
    'hub64-m500': lambda: hub(64, 1e3, 500, 1.0, 5),
    'ragged32': lambda: ragged(32, 1e3, 6),
    'ragged64': lambda: ragged(64, 1e3, 7),
}


def grid(dim, n, gamma):
    o = mo.bidomain_system(dim, n, gamma)
    return o['A'], o['nv'], o['idofs']


RULE_CASES = dict({k: v[0] for k, v in CASES.items() if not k.endswith('theta0.25')},
                  **{k: v for k, v in SMALL.items() if k != 'permuted2d-64'},
                  **{'grid2d-64': lambda: grid(2, 64, 1e3), 'grid3d-16': lambda: grid(3, 16, 1e6)})


# the parameter sets of the setup parity tests, in the oracle's spelling
PARAM_SETS = [
    dict(),
    dict(aggregation_type='HEM'),
    dict(AMG_type='UA'),
    dict(strong_coupled=0.25),
]


def param_id(kw):
    return '-'.join('%s=%s' % (k, v) for k, v in kw.items()) or 'MIS'


# ---------------------------------------------------------------------------
# what the library's data-dependent branches should decide, from numpy alone
# ---------------------------------------------------------------------------
def _pattern(M):
    M = M.tocsr().copy()
    M.data[:] = 1.0
    return M


def spgemm_rows(h, rows=None):
    """Distinct columns per row of the products the GPU setup's hash SpGEMM
    forms on every level of the oracle's hierarchy h -- A T (smoothed
    aggregation only), A P and R (A P) -- counted on the patterns, as the hash
    tables see them (a column whose sum cancels still takes a slot).  Returns
    (largest count over all rows, largest count over level 0's `rows` of A P)."""
    big, at_rows = 0, 0
    for l, lv in enumerate(h.levels):
        if lv.P is None:
            break
        A1, P1, R1 = _pattern(lv.A), _pattern(lv.P), _pattern(lv.R)
        AP = (A1 @ P1).tocsr()
        counts = [np.diff(AP.indptr).max(), np.diff((R1 @ AP).tocsr().indptr).max()]
        if h.params.AMG_type == 'SA':
            counts.append(np.diff((A1 @ _pattern(mo.tentative_nodal(lv.agg, lv.nagg, 2))).tocsr().indptr).max())
        big = max(big, int(max(counts)))
        if l == 0 and rows is not None:
            at_rows = int(np.diff(AP.indptr)[np.asarray(rows)].max())
    return big, at_rows


def hub_product_width(A, P, R, rows):
    """The same count for the rows a hub drives, without forming the
    products: the distinct columns of rows `rows` of A P, and of every row of
    R (A P) that holds one of them (the coarse rows i with P[r, i] != 0)."""
    A1, P1, R = _pattern(A), _pattern(P), R.tocsr()
    widest = 0
    for r in rows:
        widest = max(widest, (A1[[r]] @ P1).nnz)
        for i in P1.indices[P1.indptr[r]:P1.indptr[r + 1]]:
            fine = R.indices[R.indptr[i]:R.indptr[i + 1]]
            widest = max(widest, len(np.unique((A1[fine] @ P1).indices)))
    return widest


def half_rule(A, nv):
    """try_half's decision (csrc/device.hip) recomputed from A's node-block
    pattern: accepted when no row part exceeds 255 blocks, su < 2^31,
    su <= 1.3 nup + 4096 and sl <= 1.3 nlo + 4096, with su / sl = 64 ns times
    the longest upper (diagonal included) / lower row part, nlo / nup the
    lower / other blocks (no ghost columns on one GPU).  Returns (accepted,
    details, SELL precondition nb <= 40 nr)."""
    P = _pattern(A)
    G = (P[:nv, :nv] + P[:nv, nv:] + P[nv:, :nv] + P[nv:, nv:]).tocsr()
    G.sort_indices()
    rows = np.repeat(np.arange(nv), np.diff(G.indptr))
    nl = np.bincount(rows[G.indices < rows], minlength=nv)
    nu = np.diff(G.indptr) - nl
    ns = (nv + 63) // 64
    su, sl = 64 * ns * int(nu.max()), 64 * ns * int(nl.max())
    nlo = int(nl.sum())
    nup = int(G.nnz) - nlo
    too_long = bool(nu.max() > 255 or nl.max() > 255)
    ok = (not too_long) and su < 2 ** 31 and su <= 1.3 * nup + 4096 and sl <= 1.3 * nlo + 4096
    return ok, dict(max_upper=int(nu.max()), max_lower=int(nl.max()), su=su, sl=sl, nup=nup, nlo=nlo,
                    too_long=too_long), G.nnz <= 40 * nv


def indefinite_patch_system():
    """bidomain 2-D n = 16 (289 nodes = 289 patches: 1 mod 4 and 1 mod 8, so
    the last workgroup of every patch-inverse kernel has dead waves) with the
    coupling of two neighbouring interior nodes set to +3 sqrt(a_ii a_jj) in
    both fields.  Every 2x2 node block stays SPD (the node-block smoother and
    the SA prolongator accept it) and the negative direction e_i - e_j is not
    in the range of P (the coarsest matrix stays SPD), so the host setup
    completes; the patches holding both nodes are indefinite."""
    o = mo.bidomain_system(2, 16, 1e2)
    A, nv = o['A'].tolil(), o['nv']
    i = 8 * 17 + 8
    j = i + 1
    for f in (0, 1):
        c = 3.0 * np.sqrt(A[f * nv + i, f * nv + i] * A[f * nv + j, f * nv + j])
        A[f * nv + i, f * nv + j] = c
        A[f * nv + j, f * nv + i] = c
    A = A.tocsr()
    A.sort_indices()
    return A, nv, o['idofs']
