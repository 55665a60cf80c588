"""CPU restatement of the row-partitioned cycle of scalar (CSR) hierarchies --
TEST INFRASTRUCTURE ONLY.

The scalar counterpart of oracle/dist_ref.py: numpy on
the product's rank-local plans (``DistPlan`` of a num_functions 1 hierarchy),
halos through the Comm objects of dist_ref (``ThreadComm`` here).  A node is a
dof, vectors are [owned | ghost] doubles, the level-0 input and output are the
plain slices r[o0:o1], z[o0:o1].

Per distributed level (POLY: the step weights w_k; nu1 / nu2 repeat them):
  winv:  X = w_1 winv b ; [halo(X) ; X += w_k winv (b - A X)] ...
  WB:    halo(b) ; X = w_1 WB b ; [halo(X) ; r = b - A X ; halo(r) ; X += w_k WB r] ...
  halo(X) ; r = b - A X ; part = Rp r ;
  [next distributed: ghost partials to their owners, added in rank order |
   next replicated: all-reduce] ; xc = cycle(l+1, bc) ;
  [W-cycle: halo(xc) ; xc += cycle(l+1, bc - A_c xc)] ;
  [scaling: halo(xc) ; all-reduce(<bc, xc>, <A_c xc, xc>) ; xc *= alpha] ;
  halo(xc) ; X += P xc ; post steps as the pre steps, weights reversed.
Replicated levels run the same cycle on global arrays without exchange.
"""
import numpy as np
import scipy.sparse as sp


def csr(M):
    ptr, col, val, nr, nc = M
    return sp.csr_matrix((val, col, ptr), shape=(nr, nc))


class DistCycleCsr:
    def __init__(self, plan_levels, Ainv, comm, poly=None, wcycle=False, scaling=False, nu1=1, nu2=1):
        self.L = plan_levels
        self.Ainv = Ainv
        self.comm = comm
        self.ws = list(poly) if poly else [1.0]
        self.wcycle, self.scaling, self.nu1, self.nu2 = wcycle, scaling, nu1, nu2
        self.M = [{k: csr(lv[k]) for k in ('A', 'P', 'R', 'WB') if k in lv} for lv in plan_levels]

    def halo(self, lv, x):
        me, n = self.comm.rank, self.comm.n
        so, si, go = lv['send_off'], lv['send_idx'], lv['ghost_off']
        sends = {q: x[si[so[q]:so[q + 1]]] for q in range(n) if q != me and so[q + 1] > so[q]}
        shapes = {q: (go[q + 1] - go[q],) for q in range(n) if q != me and go[q + 1] > go[q]}
        for q, a in self.comm.sendrecv(sends, shapes).items():
            x[lv['nloc'] + go[q]: lv['nloc'] + go[q + 1]] = a

    def reverse_add(self, lv, part):
        me, n = self.comm.rank, self.comm.n
        so, si, go = lv['send_off'], lv['send_idx'], lv['ghost_off']
        nloc = lv['nloc']
        sends = {q: part[nloc + go[q]: nloc + go[q + 1]] for q in range(n) if q != me and go[q + 1] > go[q]}
        shapes = {q: (so[q + 1] - so[q],) for q in range(n) if q != me and so[q + 1] > so[q]}
        got = self.comm.sendrecv(sends, shapes)
        out = part[:nloc].copy()
        for q in sorted(got):
            np.add.at(out, si[so[q]:so[q + 1]], got[q])
        return out

    def ghosted(self, lv, x):
        if lv['replicated']:
            return x
        xg = np.zeros(lv['nloc'] + len(lv['ghosts']))
        xg[:lv['nloc']] = x
        self.halo(lv, xg)
        return xg

    def W(self, l, lv, r):
        """the level smoother applied to the owned rows of r"""
        if 'WB' in lv:
            return self.M[l]['WB'] @ self.ghosted(lv, r)
        return lv['winv'] * r

    def smooth(self, l, lv, b, X, ws):
        for w in ws:
            X = X + w * self.W(l, lv, b - self.M[l]['A'] @ self.ghosted(lv, X))
        return X

    def cycle(self, l, b):
        lv = self.L[l]
        if lv['coarsest']:
            return self.Ainv @ b
        C = self.L[l + 1]
        pre = self.ws * self.nu1
        post = self.ws[::-1] * self.nu2
        X = pre[0] * self.W(l, lv, b)
        X = self.smooth(l, lv, b, X, pre[1:])
        r = b - self.M[l]['A'] @ self.ghosted(lv, X)
        xc = self.coarse(l, r)
        X = X + self.M[l]['P'] @ self.ghosted(C, xc)
        return self.smooth(l, lv, b, X, post)

    def coarse(self, l, r):
        lv = self.L[l]
        C = self.L[l + 1]
        part = self.M[l]['R'] @ r
        if lv['replicated']:
            bc = part
        elif C['replicated']:
            bc = self.comm.allreduce_sum(part)
        else:
            bc = self.reverse_add(C, part)
        Ac = self.M[l + 1]['A']
        xc = self.cycle(l + 1, bc)
        if self.wcycle and not C['coarsest']:
            xc = xc + self.cycle(l + 1, bc - Ac @ self.ghosted(C, xc))
        if self.scaling:
            q = Ac @ self.ghosted(C, xc)
            sums = np.array([np.sum(bc * xc), np.sum(q * xc)])
            if not C['replicated']:
                sums = self.comm.allreduce_sum(sums)
            num, den = float(sums[0]), float(sums[1])
            xc = (num / den if den > 0 else 1.0) * xc
        return xc

    def apply_local(self, r_local):
        return self.cycle(0, np.asarray(r_local, dtype=np.float64))


# ---------------------------------------------------------------------------
# The systems the scalar multi-GPU tests share (tests/test_dist_csr.py on the
# CPU, tests/test_gpu_dist_csr.py on the GPU): name -> (A, idofs, C-ABI
# parameters, oracle Params keywords, expected level sizes)
# ---------------------------------------------------------------------------
_UA_HEM = (dict(AMG_type=1, aggregation_type=5), dict(AMG_type='UA', aggregation_type='HEM'))
_WSC = (dict(cycle_type=2, coarse_scaling=1, presmooth_iter=2, postsmooth_iter=2),
        dict(cycle_type='W', coarse_scaling=1, presmooth_iter=2, postsmooth_iter=2))
_3D1D = (dict(Schwarz_type=5, Schwarz_maxlvl=2, Schwarz_mmsize=200, coarse_dof=100, max_levels=30),) * 2


def _case_table():
    return {
        'bidomain2d': ('b2', False, ({}, {}), [2178, 102, 10]),
        # the same with the second field's dofs as seeds: non-overlapping seed blocks (WB) on level 0
        'bidomain2d_seeds': ('b2', True, ({}, {}), [2178, 102, 10]),
        'bidomain3d_ua_hem': ('b3', False, _UA_HEM, [9826, 2280, 591, 151, 41]),
        'bidomain3d_ua_hem_w': ('b3', False, tuple(dict(a, **b) for a, b in zip(_UA_HEM, _WSC)),
                                [9826, 2280, 591, 151, 41]),
        'bidomain3d_poly3': ('b3', False, (dict(smoother=12, poly_degree=3), dict(smoother='POLY', poly_degree=3)),
                             [9826, 200, 8]),
        'permuted2d': ('perm', False, ({}, {}), [2178, 106, 10]),
        '3d1d': ('3d1d', True, _3D1D, [4936, 215, 6]),
    }


CASE_NAMES = list(_case_table())
_cache = {}


def _matrix(key):
    if key not in _cache:
        import metric_amg_examples_amd as M
        if key == 'perm':
            import irregular
            A, _, idofs = irregular.permuted(2, 32)
        elif key == '3d1d':
            s = M.problems.emi_3d1d(16, 1e4, 1.0)
            A, idofs = s.scipy(), s.idofs
        else:
            s = M.problems.bidomain(2, 32, 1e4) if key == 'b2' else M.problems.bidomain(3, 16, 1e4)
            A, idofs = s.scipy(), s.idofs
        A = sp.csr_matrix(A)
        A.sort_indices()
        _cache[key] = (A, np.ascontiguousarray(idofs, dtype=np.int32))
    return _cache[key]


def case(name):
    """(A, idofs or None, C-ABI parameter keywords incl. num_functions 1, levels)"""
    key, seeds, (ckw, _), levels = _case_table()[name]
    A, idofs = _matrix(key)
    return A, (idofs if seeds else None), dict(ckw, num_functions=1), levels


def oracle_apply(name):
    """(r, z): the seeded right-hand side and mamg_oracle's one-rank apply to
    it, computed once per case and shared (do not modify)"""
    k = ('oracle', name)
    if k not in _cache:
        import mamg_oracle as mo
        key, seeds, (_, okw), _ = _case_table()[name]
        A, idofs = _matrix(key)
        h = mo.setup(A, mo.Params(num_functions=1, **okw), idofs=idofs if seeds else None)
        r = mo.seeded_rhs(A.shape[0])
        z = h.apply(r)
        r.setflags(write=False)
        z.setflags(write=False)
        _cache[k] = (r, z)
    return _cache[k]


def poly_of(name):
    import mamg_oracle as mo
    okw = _case_table()[name][2][1]
    return mo.poly_weights(mo.Params(num_functions=1, **okw)) if okw.get('smoother') == 'POLY' else None


def cycle_kw(name):
    okw = _case_table()[name][2][1]
    return dict(wcycle=okw.get('cycle_type') == 'W', scaling=bool(okw.get('coarse_scaling', 0)),
                nu1=okw.get('presmooth_iter', 1), nu2=okw.get('postsmooth_iter', 1))
