"""CPU restatement of the nonlinear AMLI cycle (K-cycle, MAMG_NL_AMLI_CYCLE).

``KCycle(h, degree)`` wraps an ``mamg_oracle.Hierarchy``: its ``cycle`` is
``Hierarchy.cycle`` line for line (the smoothing branches are the oracle's own
methods, called as it calls them) with the coarse visit replaced: on a level
that is not the coarsest, ``degree`` steps of flexible (generalised) CG on
A_c e = b_c, preconditioned by the cycle of that level,

    e = 0, r = b_c
    for j = 0 .. m-1:
        z = M(r);  w = A_c z
        beta_i = d_i > 0 ? <z, q_i> / d_i : 0        for i < j
        p_j = z - sum_i beta_i p_i ;  q_j = w - sum_i beta_i q_i
        d_j = <p_j, q_j>
        alpha = d_j > 0 ? <p_j, r> / d_j : 0
        e += alpha p_j ;  r -= alpha q_j

with a fixed step count (no residual-based exit) and a dropped direction where
d_j is not positive.  ``visit`` = 'V' or 'W' runs the oracle's own visits
through the same restatement (tests/test_kcycle_ref.py: bitwise the oracle's
cycle, so only the visit differs).  ``trace`` records every step's d_j and
``guards=False`` removes the dropped-direction rule (tests/kcycle_edge_cases.py).

``KPointGS`` / ``KPointRings`` do the same on the CSR-layout restatements
(tests/pointgs_ref.py, tests/pointrings_ref.py).  A helper, not a test.
"""
import numpy as np

import mamg_oracle as mo


class KCycle:
    def __init__(self, h, degree=2, visit='K', trace=None, guards=True):
        """trace: a list that every step of a K visit appends
        (level, step, d, ||p|| ||q||) to (None: nothing is recorded; the
        arithmetic is the same either way).  guards=False: the cycle a library
        without the dropped-direction rule would run -- alpha, the beta's and
        the coarse scaling always divide (tests/test_kcycle_edges_ref.py)."""
        assert visit in ('K', 'V', 'W') and degree >= 1
        self.h = h
        self.levels = h.levels
        self.params = h.params
        self.degree = degree
        self.visit_type = visit
        self.trace = trace
        self.guards = guards

    def guarded(self, guard):
        return self.guards is True or (bool(self.guards) and guard in self.guards)

    def ratio(self, num, den, dead, guard):
        """num / den where den is positive, else ``dead``; without the guard
        the quotient whatever den is (0 / 0 = NaN, as the hardware gives)"""
        if self.guarded(guard):
            return num / den if den > 0 else dead
        with np.errstate(all='ignore'):
            return float(np.float64(num) / np.float64(den))

    # ------------------------------------------------------------ the visit
    def visit(self, c, bc):
        """e ~ A_c^-1 b_c on level c"""
        C = self.levels[c]
        if C.Ainv is not None or self.visit_type == 'V':
            return self.cycle(c, bc)
        if self.visit_type == 'W':
            e = self.cycle(c, bc)
            return e + self.cycle(c, bc - C.A @ e)
        e = np.zeros_like(bc)
        r = bc
        ps, qs, ds = [], [], []
        for j in range(self.degree):
            z = self.cycle(c, r)
            w = C.A @ z
            betas = [self.ratio(float(np.dot(z, qs[i])), ds[i], 0.0, 'beta') for i in range(j)]
            p, q = z, w
            for i in range(j):
                p = p - betas[i] * ps[i]
                q = q - betas[i] * qs[i]
            d = float(np.dot(p, q))
            alpha = self.ratio(float(np.dot(p, r)), d, 0.0, 'alpha')
            if self.trace is not None:
                self.trace.append((c, j, d, float(np.linalg.norm(p) * np.linalg.norm(q))))
            e = e + alpha * p
            if j < self.degree - 1:
                r = r - alpha * q
            ps.append(p)
            qs.append(q)
            ds.append(d)
        return e

    # ------------------------------------------- Hierarchy.cycle, restated
    def pre(self, l, b):
        """the pre-smoothing of Hierarchy.cycle from x = 0"""
        p = self.params
        lev = self.levels[l]
        A = lev.A
        if lev.rings is not None:
            x = np.zeros_like(b)
            for _ in range(p.presmooth_iter):
                x = mo.Hierarchy.rings_step(lev, x, b)
        elif lev.patches is not None:
            x = np.zeros_like(b)
            for _ in range(p.presmooth_iter):
                x = lev.patches.sweep(A, x, b, True)
                x = lev.patches.sweep(A, x, b, False)
        elif lev.colour is not None:
            x = np.zeros_like(b)
            for _ in range(p.presmooth_iter):
                x = lev.gs_sweep(x, b, True)
                if p.smoother == 'SGS':
                    x = lev.gs_sweep(x, b, False)
        else:
            pre = [None] * p.presmooth_iter
            if lev.polyW is not None:
                pre = lev.polyW * p.presmooth_iter
            x = lev.smooth_apply(b, pre[0])
            for S in pre[1:]:
                x = x + lev.smooth_apply(b - A @ x, S)
        return x

    def post(self, l, x, b):
        """the post-smoothing of Hierarchy.cycle"""
        p = self.params
        lev = self.levels[l]
        A = lev.A
        post = [None]
        if lev.polyW is not None:
            post = lev.polyW[::-1]
        for _ in range(p.postsmooth_iter):
            if lev.rings is not None:
                x = mo.Hierarchy.rings_step(lev, x, b)
            elif lev.patches is not None:
                x = lev.patches.sweep(A, x, b, True)
                x = lev.patches.sweep(A, x, b, False)
            elif lev.colour is not None:
                if p.smoother == 'SGS':
                    x = lev.gs_sweep(x, b, True)
                x = lev.gs_sweep(x, b, False)
            else:
                for S in post:
                    x = x + lev.smooth_apply(b - A @ x, S)
        return x

    def cycle(self, l, b):
        p = self.params
        lev = self.levels[l]
        if lev.Ainv is not None:
            return lev.Ainv @ b
        x = self.pre(l, b)
        r = b - lev.A @ x
        bc = lev.R @ r
        C = self.levels[l + 1]
        e = self.visit(l + 1, bc)
        if p.coarse_scaling and self.guarded('scale'):
            e = mo.coarse_scale(C.A, bc, e)
        elif p.coarse_scaling:
            e = self.ratio(float(np.dot(bc, e)), float(np.dot(e, C.A @ e)), 1.0, 'scale') * e
        x = x + lev.P @ e
        return self.post(l, x, b)

    def apply(self, r):
        """z = B r: ``maxit`` cycles, x0 = 0 (Hierarchy.apply)"""
        z = self.cycle(0, r)
        A0 = self.levels[0].A
        for _ in range(self.params.maxit - 1):
            z = z + self.cycle(0, r - A0 @ z)
        return z

    def __call__(self, r):
        return self.apply(r)


class KPointGS(KCycle):
    """The same on ``pointgs_ref.PointGS`` (point-wise multicolour GS / SGS on
    every level): its sweeps, called as ``PointGS.cycle`` calls them."""

    def __init__(self, pg, degree=2, visit='K'):
        KCycle.__init__(self, pg.h, degree, visit)
        self.pg = pg

    def pre(self, l, b):
        x = np.zeros_like(b)
        for _ in range(self.params.presmooth_iter):
            x = self.pg.sweep(l, x, b, True)
            if self.pg.sgs:
                x = self.pg.sweep(l, x, b, False)
        return x

    def post(self, l, x, b):
        for _ in range(self.params.postsmooth_iter):
            if self.pg.sgs:
                x = self.pg.sweep(l, x, b, True)
            x = self.pg.sweep(l, x, b, False)
        return x


class KPointRings(KCycle):
    """The same on ``pointrings_ref.PointRings``: its level-0 step, and below
    level 0 the level smoother's cycle (``Hierarchy.cycle``'s branches, or
    ``PointGS``'s sweeps for GS / SGS)."""

    def __init__(self, rr, degree=2, visit='K'):
        KCycle.__init__(self, rr.h, degree, visit)
        self.rr = rr
        self.kpg = KPointGS(rr.coarse, degree, visit) if hasattr(rr, 'coarse') else None

    def pre(self, l, b):
        if l > 0:
            return self.kpg.pre(l, b) if self.kpg else KCycle.pre(self, l, b)
        x = np.zeros_like(b)
        for _ in range(self.params.presmooth_iter):
            x = self.rr.step(x, b)
        return x

    def post(self, l, x, b):
        if l > 0:
            return self.kpg.post(l, x, b) if self.kpg else KCycle.post(self, l, x, b)
        for _ in range(self.params.postsmooth_iter):
            x = self.rr.step(x, b)
        return x
