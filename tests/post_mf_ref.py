"""The matrix-free level-0 prolongation restated on the
oracle, shared by tests/test_post_mf_identity.py (CPU) and
tests/test_gpu_post_mf.py.

Setup step 4 builds P = T - w D_B^-1 (A T) with T the tentative prolongator
(one 1 per aggregated node and field, a zero row for an isolated node), D_B
the node-block diagonal of A and w = sa_omega / rho_B.  So

    P e = (I - w D_B^-1 A)(T e),

and a cycle can prolongate through the aggregates and A without a stored P.
``matrix_free(h)`` is the oracle's hierarchy with level 0's P replaced by that
map (R, the Galerkin operators and everything else unchanged).  A helper, not
a test.
"""
import copy

import mamg_oracle as mo


class MatrixFreeP:
    """e -> T e - w D_B^-1 (A (T e)) for one oracle level; A: the matrix the
    product reads (the level's own, or a rounded copy: fp32 cycle storage);
    D_B always comes from the level's fp64 A, as in the library."""

    def __init__(self, lev, A=None):
        n = lev.A.shape[0]
        self.T = mo.tentative_nodal(lev.agg, lev.nagg, 2)
        self.A = lev.A if A is None else A
        self.Dinv = mo.block_inverse_csr(lev.A, *mo.node_blocks(n, 2))
        self.w = lev.w_sa
        self.shape = lev.P.shape
        assert self.T.shape == self.shape and self.w > 0.0

    def __matmul__(self, e):
        y = self.T @ e
        return y - self.w * (self.Dinv @ (self.A @ y))


def matrix_free(h, A=None):
    """h with level 0's P replaced by its matrix-free form"""
    levels = list(h.levels)
    levels[0] = copy.copy(levels[0])
    levels[0].P = MatrixFreeP(h.levels[0], A)
    return mo.Hierarchy(levels, h.params)
