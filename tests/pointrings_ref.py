"""CPU restatement of the seed-ring Schwarz on hierarchies of the CSR layout
(Schwarz_type RINGS on a scalar system, or a nodal one with point smoothers;
DESIGN.md section 2.12.1).  A helper of tests/test_point_rings.py and
tests/test_gpu_point_rings.py, not a test.

* hierarchy: ``mamg_oracle.setup`` with ``Schwarz_levels=0`` and the given
  level smoother; for 'GS' / 'SGS' the point JACOBI_RHO one of
  ``pointgs_ref.PointGS`` (level 0 is not coloured as a whole);
* blocks, inverses, ring colours: ``mamg_oracle.Rings`` (``seed_ring_blocks``
  in seed order, Gauss-Jordan, greedy first-fit conflict colours);
* the rest: the rows in no block, coloured by ``mamg_oracle.jp_colouring`` at
  level 0 (keys by original row index) on A_0's off-diagonal pattern with
  every covered row emptied and every covered column dropped; covered rows
  take no update and are in no colour list;
* level-0 step: ring sweep with colours ascending, rest GS forward, rest GS
  backward, ring sweep with colours descending (palindromic), nu1 times from
  x = 0 before and nu2 times after the coarse correction, whatever the level
  smoother is;
* levels >= 1: the level smoother's own cycle (``Hierarchy.cycle`` for the
  Jacobi family and POLY, ``PointGS.cycle`` for GS / SGS); W cycle,
  ``mamg_oracle.coarse_scale`` and ``maxit`` as everywhere;
* ``mamg_oracle.pcg`` for the Krylov loop.
"""
import numpy as np
import scipy.sparse as sp

import mamg_oracle as mo
import pointgs_ref as pr

SCHWARZ_RINGS = 8
SMOOTHER = dict(pr.SMOOTHER, JACOBI=1, L1DIAG=2, JACOBI_RHO=3, POLY=12)


class _CoarsePointGS(pr.PointGS):
    """PointGS whose level 0 is left uncoloured (the rings own it)."""

    def __init__(self, A, smoother, **kw):
        self.sgs = smoother == 'SGS'
        p = mo.Params(**dict(kw, smoother='JACOBI_RHO', node_block_smoother=0, Schwarz_levels=0))
        self.h = mo.setup(A, p)
        self.p = self.h.params
        self.levels = self.h.levels
        self.crows, self.dinv = [], []
        for l, lev in enumerate(self.levels):
            if lev.Ainv is not None or l == 0:
                self.crows.append(None)
                self.dinv.append(None)
                continue
            c = mo.jp_colouring(pr.offdiag_pattern(lev.A), l)        # RuntimeError: more than 64 colours
            self.crows.append([np.flatnonzero(c == k) for k in range(int(c.max()) + 1)])
            self.dinv.append(1.0 / lev.A.diagonal())


def rest_pattern(A: sp.csr_matrix, cov: np.ndarray) -> sp.csr_matrix:
    """A's stored off-diagonal pattern restricted to uncovered x uncovered"""
    G = pr.offdiag_pattern(A)
    D = sp.diags((~cov).astype(float))
    F = sp.csr_matrix(D @ G @ D)
    F.eliminate_zeros()
    F.sort_indices()
    return F


class PointRings:
    """B r of the cycle with the level-0 seed rings + rest point GS."""

    def __init__(self, A, seeds, smoother='JACOBI_RHO', **kw):
        A = sp.csr_matrix(A)
        A.sort_indices()
        kw = dict(kw)
        kw.pop('Schwarz_levels', None)
        kw.pop('Schwarz_type', None)
        self.maxlvl = kw.get('Schwarz_maxlvl', 1)
        self.mmsize = kw.get('Schwarz_mmsize', 100)
        if smoother in pr.SMOOTHER:
            self.coarse = _CoarsePointGS(A, smoother, **kw)
            self.h = self.coarse.h
            self.coarse_cycle = self.coarse.cycle
        else:
            self.h = mo.setup(A, mo.Params(**dict(kw, smoother=smoother, Schwarz_levels=0)))
            self.coarse_cycle = self.h.cycle
        self.p = self.h.params
        self.levels = self.h.levels
        assert self.levels[0].Ainv is None, 'the rings need a level below level 0'
        A0 = self.levels[0].A
        self.rings = mo.Rings(A0, seeds, self.maxlvl, self.mmsize)
        self.cov = self.rings.cov
        self.F = rest_pattern(A0, self.cov)
        if (self.F != self.F.T).nnz:
            raise RuntimeError('rest pattern of level 0 not symmetric')
        c = mo.jp_colouring(self.F, 0)                               # RuntimeError: more than 64 colours
        self.rest_colour = c
        unc = np.flatnonzero(~self.cov)
        nc = int(c[unc].max()) + 1 if unc.size else 0
        self.rest_rows = [unc[c[unc] == k] for k in range(nc)]
        d = A0.diagonal()
        if unc.size and not (d[unc] > 0).all():
            raise ValueError('a diagonal entry of an uncovered row is missing or not positive')
        self.dinv = np.zeros(A0.shape[0])
        self.dinv[unc] = 1.0 / d[unc]

    def rest_sweep(self, x, b, forward):
        A, cr = self.levels[0].A, self.rest_rows
        for k in (range(len(cr)) if forward else range(len(cr) - 1, -1, -1)):
            I = cr[k]
            x[I] = x[I] + self.dinv[I] * (b[I] - A[I] @ x)
        return x

    def step(self, x, b, sequential=False):
        A = self.levels[0].A
        sw = self.rings.sweep_seed_order if sequential else self.rings.sweep
        x = sw(A, x, b, True)
        x = self.rest_sweep(x, b, True)
        x = self.rest_sweep(x, b, False)
        return sw(A, x, b, False)

    def cycle0(self, b):
        p, lev = self.p, self.levels[0]
        x = np.zeros_like(b)
        for _ in range(p.presmooth_iter):
            x = self.step(x, b)
        bc = lev.R @ (b - lev.A @ x)
        C = self.levels[1]
        e = self.coarse_cycle(1, bc)
        if p.cycle_type == 'W' and C.Ainv is None:
            e = e + self.coarse_cycle(1, bc - C.A @ e)
        if p.coarse_scaling:
            e = mo.coarse_scale(C.A, bc, e)
        x = x + lev.P @ e
        for _ in range(p.postsmooth_iter):
            x = self.step(x, b)
        return x

    def apply(self, r):
        z = self.cycle0(r)
        A0 = self.levels[0].A
        for _ in range(self.p.maxit - 1):
            z = z + self.cycle0(r - A0 @ z)
        return z

    __call__ = apply


def to_c(kw):
    """oracle keyword names -> the library's dict values (Schwarz_type RINGS)"""
    c = dict(kw)
    smo = c.pop('smoother', None)
    c = pr.to_c(c)
    if smo is not None:
        c['smoother'] = SMOOTHER[smo]
    return dict(c, Schwarz_levels=1, Schwarz_type=SCHWARZ_RINGS)


def pcg(A, B, b, tol=1e-8, maxiter=500):
    return mo.pcg(A, B, b, tol, maxiter)
