"""The BSR2 Jacobi / POLY cycle restated in numpy with selectable fp32 storage.

One apply of a handle narrowed by ``mamg_set_cycle_storage`` is the fp64 cycle
on operators rounded to fp32: values are converted on
load, every product, sum, vector and dot stays fp64.  ``StorageRef`` restates
that cycle from the oracle's hierarchy (``mo.setup``: per level A, the block
smoother WB, P, R, the POLY step smoothers, the coarsest inverse):

  x1 = S_1 b                                first sweep from x = 0
  x  = x + S_k (b - A x), k = 2 .. nu1 m    the other pre-smoothing steps
  r1 = b - A x,  b_c = R r1
  e  = cycle(b_c) [+ cycle(b_c - A_c e)]    W: the second visit
  e  = alpha e                              coarse scaling (mo.coarse_scale)
  x  = x + T_1 r1 + K e                     K form: K = P - T_1 (A P), formed in fp64
  x  = x + P e,  x = x + T_1 (b - A x)      plain P (post_fusion 0)
  x  = x + T_k (b - A x), k = 2 .. nu2 m    T_k: POLY steps m .. 1 on the post side

``masks[l]`` holds the three bits of ``mamg_level_storage``: bit 0 rounds the
A_l the cycle reads (the residuals, the smoothing steps, and -- for l >= 1 --
the W cycle's second-visit residual and the coarse scaling's q = A_l e of the
level above), bit 1 rounds K_l (after it is formed from the fp64 A, P and T_1)
or the plain P_l, bit 2 rounds R_l.  Rounding is ``astype(float32)`` and back.
The smoother blocks, the step smoothers, the coarsest inverse and all vectors
stay fp64.  ``kform[l]`` says whether level l's post side goes through K (the
level reports post fusion) or through plain P.
"""
import numpy as np
import scipy.sparse as sp

import mamg_oracle as mo

BIT_A, BIT_KP, BIT_R = 1, 2, 4
ALL = BIT_A | BIT_KP | BIT_R


def round32(M):
    """M with every stored value rounded to fp32 (nearest even) and widened again."""
    M = sp.csr_matrix(M, copy=True)
    M.data = M.data.astype(np.float32).astype(np.float64)
    return M


class StorageRef:
    """h: the oracle's Hierarchy (Jacobi family or POLY, node-block smoothers).
    masks: one int per level (missing levels and the coarsest: 0), or one int
    for every level.  kform: one bool per level, or one bool for every level.
    levels: the levels to narrow (None: every level masks names); the others
    keep their fp64 operators whatever masks says -- a handle with a coarse
    tail narrows the launch path's levels only."""

    def __init__(self, h, masks=0, kform=True, levels=None):
        self.params = h.params
        self.levels = h.levels
        n = len(h.levels)
        masks = [masks] * n if np.isscalar(masks) else list(masks) + [0] * (n - len(masks))
        kform = [kform] * n if isinstance(kform, (bool, np.bool_)) else list(kform) + [False] * (n - len(kform))
        if levels is not None:
            masks = [m if l in levels else 0 for l, m in enumerate(masks)]
        self.masks, self.kform = masks, kform
        self.A, self.R, self.P, self.K = [], [], [], []
        for l, lev in enumerate(h.levels):
            m = masks[l]
            if lev.Ainv is not None:
                self.A.append(lev.A)
                self.R.append(None)
                self.P.append(None)
                self.K.append(None)
                continue
            assert lev.colour is None and lev.patches is None and lev.rings is None, 'Jacobi family / POLY only'
            self.A.append(round32(lev.A) if m & BIT_A else lev.A)
            self.R.append(round32(lev.R) if m & BIT_R else lev.R)
            if kform[l] and h.params.postsmooth_iter >= 1:
                T1 = self._post(lev)[0]
                K = sp.csr_matrix(lev.P - self._mat(lev, T1) @ (lev.A @ lev.P))   # fp64, from the unrounded A
                self.K.append(round32(K) if m & BIT_KP else K)
                self.P.append(None)
            else:
                self.K.append(None)
                self.P.append(round32(lev.P) if m & BIT_KP else lev.P)

    @staticmethod
    def _mat(lev, S):
        if S is None:
            S = lev.WB if lev.WB is not None else lev.winv
        return S if sp.issparse(S) else sp.diags(S)

    def _pre(self, lev):
        steps = [None] if lev.polyW is None else list(lev.polyW)
        return steps * self.params.presmooth_iter

    def _post(self, lev):
        steps = [None] if lev.polyW is None else list(lev.polyW[::-1])   # POLY: steps m .. 1
        return steps * self.params.postsmooth_iter

    def cycle(self, l, b):
        p = self.params
        lev = self.levels[l]
        if lev.Ainv is not None:
            return lev.Ainv @ b
        A = self.A[l]
        pre, post = self._pre(lev), self._post(lev)
        x = lev.smooth_apply(b, pre[0])
        for S in pre[1:]:
            x = x + lev.smooth_apply(b - A @ x, S)
        r = b - A @ x
        bc = self.R[l] @ r
        C = self.levels[l + 1]
        e = self.cycle(l + 1, bc)
        if p.cycle_type == 'W' and C.Ainv is None:
            e = e + self.cycle(l + 1, bc - self.A[l + 1] @ e)
        if p.coarse_scaling:
            e = mo.coarse_scale(self.A[l + 1], bc, e)
        if self.K[l] is not None:
            x = x + lev.smooth_apply(r, post[0]) + self.K[l] @ e
            rest = post[1:]
        else:
            x = x + self.P[l] @ e
            rest = post
        for S in rest:
            x = x + lev.smooth_apply(b - A @ x, S)
        return x

    def apply(self, r):
        z = self.cycle(0, r)
        for _ in range(self.params.maxit - 1):
            z = z + self.cycle(0, r - self.A[0] @ z)
        return z

    def __call__(self, r):
        return self.apply(r)
