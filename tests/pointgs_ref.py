"""CPU restatement of the point-wise multicolour GS / SGS preconditioner
(SMOOTHER_GS_POINT / SMOOTHER_SGS_POINT).  A helper of
tests/test_point_gs.py and tests/test_gpu_point_gs.py, not a test.

* hierarchy: ``mamg_oracle.setup`` with ``smoother='JACOBI_RHO'`` and
  ``node_block_smoother=0`` (the point smoother's hierarchy; its winv is not
  used);
* colours: ``mamg_oracle.jp_colouring`` on each level's off-diagonal pattern
  (stored entries, explicit zeros included), level l hashed with l;
* sweep: colours ascending (forward) or descending (backward), every row of
  a colour at once: x_i += (b_i - sum_j a_ij x_j) / a_ii;
* cycle: x = 0, nu1 x (forward [+ backward if SGS]), r = b - A x, restrict,
  recurse (W: second visit on the updated residual), ``mamg_oracle.coarse_scale``,
  x += P e, nu2 x ([forward if SGS] + backward);
* ``mamg_oracle.pcg`` for the Krylov loop.
"""
import numpy as np
import scipy.sparse as sp

import mamg_oracle as mo

SMOOTHER = {'GS': 13, 'SGS': 14}


def offdiag_pattern(A: sp.csr_matrix) -> sp.csr_matrix:
    """stored off-diagonal entries of A as a 0/1 pattern (explicit zeros stay)"""
    A = sp.csr_matrix(A)
    rows = np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))
    keep = rows != A.indices
    G = sp.csr_matrix((np.ones(int(keep.sum())), (rows[keep], A.indices[keep])), shape=A.shape)
    G.sort_indices()
    return G


class PointGS:
    """B r of the point-wise multicolour GS ('GS') / SGS ('SGS') cycle."""

    def __init__(self, A, smoother='SGS', **kw):
        assert smoother in SMOOTHER
        self.sgs = smoother == 'SGS'
        p = mo.Params(**dict(kw, smoother='JACOBI_RHO', node_block_smoother=0))
        self.h = mo.setup(A, p)
        self.p = self.h.params
        self.levels = self.h.levels
        self.crows, self.dinv = [], []
        for l, lev in enumerate(self.levels):
            if lev.Ainv is not None:
                self.crows.append(None)
                self.dinv.append(None)
                continue
            c = mo.jp_colouring(offdiag_pattern(lev.A), l)
            self.crows.append([np.flatnonzero(c == k) for k in range(int(c.max()) + 1)])
            self.dinv.append(1.0 / lev.A.diagonal())

    def ncolours(self):
        return [len(c) for c in self.crows if c is not None]

    def sweep(self, l, x, b, forward):
        A, cr, dinv = self.levels[l].A, self.crows[l], self.dinv[l]
        for k in (range(len(cr)) if forward else range(len(cr) - 1, -1, -1)):
            I = cr[k]
            x[I] = x[I] + dinv[I] * (b[I] - A[I] @ x)
        return x

    def cycle(self, l, b):
        p, lev = self.p, self.levels[l]
        if lev.Ainv is not None:
            return lev.Ainv @ b
        x = np.zeros_like(b)
        for _ in range(p.presmooth_iter):
            x = self.sweep(l, x, b, True)
            if self.sgs:
                x = self.sweep(l, x, b, False)
        r = b - lev.A @ x
        bc = lev.R @ r
        C = self.levels[l + 1]
        e = self.cycle(l + 1, bc)
        if p.cycle_type == 'W' and C.Ainv is None:
            e = e + self.cycle(l + 1, bc - C.A @ e)
        if p.coarse_scaling:
            e = mo.coarse_scale(C.A, bc, e)
        x = x + lev.P @ e
        for _ in range(p.postsmooth_iter):
            if self.sgs:
                x = self.sweep(l, x, b, True)
            x = self.sweep(l, x, b, False)
        return x

    def apply(self, r):
        z = self.cycle(0, r)
        A0 = self.levels[0].A
        for _ in range(self.p.maxit - 1):
            z = z + self.cycle(0, r - A0 @ z)
        return z

    __call__ = apply


# parameters_standard (src/amg_parameters.py:47-65) in the oracle's names, as
# precond.amg_pointwise_parameters maps it: UA + VMB + W + SGS + scaling,
# theta 0.1, point-wise (relaxation 1.2 does not enter the sweeps)
STANDARD = dict(AMG_type='UA', cycle_type='W', aggregation_type='VMB', strong_coupled=0.1, coarse_scaling=1,
                relaxation=1.2, coarse_dof=100, Schwarz_levels=0, num_functions=1)


def to_c(kw):
    """oracle keyword names -> the library's dict values"""
    c = dict(kw)
    if 'smoother' in c:
        c['smoother'] = SMOOTHER[c['smoother']]
    if 'cycle_type' in c:
        c['cycle_type'] = {'V': 1, 'W': 2}[c['cycle_type']]
    if 'AMG_type' in c:
        c['AMG_type'] = {'SA': 2, 'UA': 1}[c['AMG_type']]
    if 'aggregation_type' in c:
        c['aggregation_type'] = {'MIS': 2, 'HEM': 5, 'VMB': 1}[c['aggregation_type']]
    return c


def pcg(A, B, b, tol=1e-8, maxiter=500):
    return mo.pcg(A, B, b, tol, maxiter)
