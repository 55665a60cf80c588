"""numpy restatement of the GPU setup's VMB aggregation (gsetup.hip, the
vmb_* kernels) on a strength pattern.

Phase 1 of the sequential loop (oracle aggregate_vmb) picks the
lexicographically first maximal independent set of the squared strong graph.
Two local rules reach it, over states UNDECIDED, ROOT and OUT (isolated
nodes start OUT):
  ROOT  when every node of smaller index within two strong hops is OUT,
  OUT   when a ROOT lies within two strong hops.
The schedule fixes rounds and work as functions of the graph alone:
  round 1 evaluates every non-isolated node;
  in a round, the active nodes test the ROOT rule against the state at the
  start of the round, then every undecided node within two hops of a new
  root goes OUT;
  the next round's active list is the undecided nodes within two hops of a
  node that went OUT in this round (the two-hop neighbourhood of a new root
  holds no undecided node any more).
Every round asserts that no undecided node outside the next list satisfies
the ROOT rule: the list misses nothing.
"""
import numpy as np
import scipy.sparse as sp

OUT, UND, ROOT = 0, 1, 2


class VmbResult:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def _pattern(M):
    M = sp.csr_matrix(M)
    M.sort_indices()
    return M


def vmb_schedule(S, Wabs=None, max_rounds=None):
    """S: symmetric strong pattern (CSR, no diagonal).  Wabs: the weights
    of phase 2 (|a_ij| or s_IJ); None stops after phase 1 (agg1).
    Returns roots (bool), agg, nagg, rounds, evaluations, nonisolated, joiners;
    with max_rounds, rounds is capped and `finished` says whether phase 1 ended."""
    S = _pattern(S)
    n = S.shape[0]
    Sb = sp.csr_matrix((np.ones(S.nnz, dtype=np.int64), S.indices, S.indptr), shape=(n, n))
    S2 = _pattern(Sb @ Sb + Sb)                    # within two hops (the diagonal entries are harmless below)
    r2 = np.repeat(np.arange(n), np.diff(S2.indptr))
    low = r2 > S2.indices
    L = sp.csr_matrix((np.ones(int(low.sum()), dtype=np.int64), (r2[low], S2.indices[low])), shape=(n, n))
    nonisol = np.diff(S.indptr) > 0
    state = np.where(nonisol, UND, OUT)
    active = np.flatnonzero(nonisol)
    rounds = evaluations = 0
    finished = True
    while (state == UND).any():
        if max_rounds is not None and rounds >= max_rounds:
            finished = False
            break
        rounds += 1
        evaluations += len(active)
        assert len(active) and (state[active] == UND).all()
        blockers = L[active] @ (state != OUT).astype(np.int64)
        new_roots = active[blockers == 0]
        assert len(new_roots), 'no progress'
        state[new_roots] = ROOT
        near = np.unique(S2[new_roots].indices)
        went_out = near[state[near] == UND]
        state[went_out] = OUT
        near = np.unique(S2[went_out].indices) if len(went_out) else np.zeros(0, dtype=np.int64)
        active = near[state[near] == UND]
        rest = np.setdiff1d(np.flatnonzero(state == UND), active)
        if len(rest):      # a root missed outside the list would show here
            assert (L[rest] @ (state != OUT).astype(np.int64) > 0).all()
    roots = state == ROOT
    res = VmbResult(roots=roots, rounds=rounds, evaluations=evaluations, nonisolated=int(nonisol.sum()),
                    finished=finished, agg=None, nagg=int(roots.sum()), joiners=None)
    if not finished:
        return res
    # numbering: exclusive scan of the root flags in index order; a root's
    # strong neighbours take its id (roots are three hops apart: one at most)
    rid = np.cumsum(roots) - 1
    agg = np.where(roots, rid, -1).astype(np.int64)
    rows = np.repeat(np.arange(n), np.diff(S.indptr))
    e = roots[S.indices] & ~roots[rows]
    assert len(np.unique(rows[e])) == int(e.sum())
    agg[rows[e]] = rid[S.indices[e]]
    agg1 = agg.copy()
    need = np.flatnonzero(nonisol & (agg1 < 0))
    res.joiners = len(need)
    if Wabs is not None and len(need):
        W = _pattern(sp.csr_matrix(Wabs).multiply(Sb))
        for i in need:
            best_w, best_a = -1.0, -1
            for j, w in zip(W.indices[W.indptr[i]:W.indptr[i + 1]], W.data[W.indptr[i]:W.indptr[i + 1]]):
                a = agg1[j]
                if w == 0.0 or a < 0:
                    continue
                if w > best_w or (w == best_w and a < best_a):
                    best_w, best_a = w, a
            assert best_a >= 0, 'VMB aggregation left a non-isolated node unassigned'
            agg[i] = best_a
    res.agg = agg
    return res


def level_graph(A, nf, theta, measure=1):
    """(S, Wabs) of one level as the setups build them: the node graph for
    nf = 2, |A| for nf = 1 (oracle node_strength / strength)."""
    import mamg_oracle as mo
    A = sp.csr_matrix(A)
    if nf == 1:
        return mo.strength(A, theta, measure), abs(A).tocsr()
    return mo.node_strength(A, nf, theta, measure)
