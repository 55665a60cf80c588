"""CPU restatement of the row-partitioned V-cycle -- TEST INFRASTRUCTURE ONLY.

Runs the distributed algorithm of DESIGN.md section 6 / csrc/dist.cpp on the product's
rank-local plans (``metric_amg_examples_amd.DistPlan``) with numpy, exchanging
halos through a Comm object: ``GlooComm`` (torch.distributed, one process per
rank) or ``ThreadComm`` (ranks as threads of one process, queue exchange).
Tests compare the gathered result with the single-rank oracle
(mamg_oracle.Hierarchy.apply): the partition must not change the cycle beyond
summation order.

Per distributed level (POLY: the step weights w_k; nu1 / nu2 repeat them):
  X = W b [; halo(X) ; X += w_k W (b - A X)] ; halo(X) ; r = b - A X ;
  part = Rp r ; [next distributed: reverse-add ghost partials to owners |
                 next replicated: all-reduce] ; xc = cycle(l+1, bc) ;
  [W-cycle: halo(xc) ; xc += cycle(l+1, bc - A_c xc)] ;
  [scaling: halo(xc) ; all-reduce(<bc, xc>, <A_c xc, xc>) ; xc *= alpha] ;
  [next distributed: halo(xc)] ; X += P xc ; halo(X) ; z = X + W (b - A X)
Multicolour GS / SGS (gs=...): X = 0 ; sweeps with a halo after every colour ;
  r = b - A X ; (coarse correction as above) ; X += P xc ; halo(X) ; sweeps.
Replicated levels run the same cycle on global arrays without exchange.
"""
from __future__ import annotations

import queue
import threading

import numpy as np


def bsr_mv(M, x2):
    """M = (ptr, col, val[nb,2,2], nr, nc); x2 (nc, 2) -> (nr, 2)."""
    ptr, col, val, nr, _ = M
    y = np.zeros((nr, 2))
    if len(col):
        rows = np.repeat(np.arange(nr), np.diff(ptr))
        np.add.at(y, rows, np.einsum('kfg,kg->kf', val, x2[col]))
    return y


def bd_mv(W, b2):
    return np.einsum('ifg,ig->if', W, b2)


class ThreadComm:
    """In-process exchange between rank threads (queues per ordered pair)."""

    def __init__(self, nranks):
        self.n = nranks
        self.q = {(a, b): queue.Queue() for a in range(nranks) for b in range(nranks)}
        self.bar = threading.Barrier(nranks)
        self.red = [None] * nranks

    def view(self, rank):
        return _ThreadView(self, rank)


class _ThreadView:
    def __init__(self, c, rank):
        self.c, self.rank, self.n = c, rank, c.n

    def sendrecv(self, sends, recv_shapes):
        """sends: {q: array}, recv_shapes: {q: shape} -> {q: array}"""
        for q, a in sends.items():
            self.c.q[(self.rank, q)].put(np.array(a, copy=True))
        return {q: self.c.q[(q, self.rank)].get(timeout=60).reshape(s)
                for q, s in recv_shapes.items()}

    def allreduce_sum(self, a):
        self.c.red[self.rank] = np.array(a, copy=True)
        self.c.bar.wait()
        out = self.c.red[0].copy()
        for r in range(1, self.n):           # fixed rank order
            out = out + self.c.red[r]
        self.c.bar.wait()
        return out


class GlooComm:
    """torch.distributed (gloo) exchange; one process per rank."""

    def __init__(self):
        import torch.distributed as dist
        self.d = dist
        self.rank, self.n = dist.get_rank(), dist.get_world_size()

    def sendrecv(self, sends, recv_shapes):
        import torch
        reqs, bufs = [], {}
        for q, s in recv_shapes.items():
            bufs[q] = torch.zeros(int(np.prod(s)), dtype=torch.float64)
            reqs.append(self.d.irecv(bufs[q], src=q))
        for q, a in sends.items():
            reqs.append(self.d.isend(torch.as_tensor(np.ascontiguousarray(a).ravel()), dst=q))
        for r in reqs:
            r.wait()
        return {q: bufs[q].numpy().reshape(recv_shapes[q]) for q in recv_shapes}

    def allreduce_sum(self, a):
        import torch
        parts = [torch.zeros(a.size, dtype=torch.float64) for _ in range(self.n)]
        self.d.all_gather(parts, torch.as_tensor(np.ascontiguousarray(a).ravel()))
        out = parts[0].numpy().reshape(a.shape).copy()
        for r in range(1, self.n):
            out = out + parts[r].numpy().reshape(a.shape)
        return out


class DistCycle:
    """poly: the POLY step weights (mamg_oracle.poly_weights): pre-smoothing
    takes x = w_1 W b then x += w_k W (b - A x) for k = 2..m (a halo before
    each), post-smoothing the steps m..1; None = one Jacobi step each.
    nu1 / nu2 repeat the pre / post steps (presmooth_iter, postsmooth_iter);
    wcycle: a second coarse visit on the updated coarse residual
    (src/amg_parameters.py:69); scaling: the coarse correction e scaled by
    <b_c, e> / <A_c e, e> with the two sums all-reduced over the ranks
    (src/amg_parameters.py:78; mamg_oracle.coarse_scale)."""

    def __init__(self, plan_levels, Ainv_nodemajor, comm, poly=None, wcycle=False, scaling=False, nu1=1, nu2=1,
                 gs=None, sgs=True):
        self.L = plan_levels
        self.Ainv = Ainv_nodemajor
        self.comm = comm
        self.ws = list(poly) if poly else [1.0]
        self.wcycle, self.scaling, self.nu1, self.nu2 = wcycle, scaling, nu1, nu2
        # multicolour GS (mamg_oracle Level.gs_sweep): per level the global
        # colour of every node and its (2, 2) block inverse; sgs: forward then
        # backward sweeps
        self.gs, self.sgs = gs, sgs

    # forward halo: fill ghost rows of x2 (nloc+ng, 2)
    def halo(self, lv, x2):
        me, n = self.comm.rank, self.comm.n
        so, si, go = lv['send_off'], lv['send_idx'], lv['ghost_off']
        sends = {q: x2[si[so[q]:so[q + 1]]] for q in range(n) if q != me and so[q + 1] > so[q]}
        shapes = {q: (go[q + 1] - go[q], 2) for q in range(n) if q != me and go[q + 1] > go[q]}
        got = self.comm.sendrecv(sends, shapes)
        for q, a in got.items():
            x2[lv['nloc'] + go[q]: lv['nloc'] + go[q + 1]] = a

    # reverse: ghost partials -> owners, added in rank order
    def reverse_add(self, lv, part):
        me, n = self.comm.rank, self.comm.n
        so, si, go = lv['send_off'], lv['send_idx'], lv['ghost_off']
        nloc = lv['nloc']
        sends = {q: part[nloc + go[q]: nloc + go[q + 1]] for q in range(n)
                 if q != me and go[q + 1] > go[q]}
        shapes = {q: (so[q + 1] - so[q], 2) for q in range(n) if q != me and so[q + 1] > so[q]}
        got = self.comm.sendrecv(sends, shapes)
        out = part[:nloc].copy()
        for q in sorted(got):
            np.add.at(out, si[so[q]:so[q + 1]], got[q])
        return out

    def ghosted(self, lv, x):
        """x (owned rows) -> [owned | ghost] with the ghosts filled (distributed
        level) or x itself (replicated level)."""
        if lv['replicated']:
            return x
        xg = np.zeros((lv['nloc'] + len(lv['ghosts']), 2))
        xg[:lv['nloc']] = x
        self.halo(lv, xg)
        return xg

    def smooth(self, lv, b2, X, ws):
        """steps x += w W (b - A x) for w in ws (X owned rows)."""
        for w in ws:
            X = X + w * bd_mv(lv['W'], b2 - bsr_mv(lv['A'], self.ghosted(lv, X)))
        return X

    def gs_sweep(self, l, lv, X, b2, fwd):
        """one multicolour GS sweep on the owned nodes of X ([owned | ghost]
        on a distributed level), the ghosts refreshed after every colour (the
        product refreshes only that colour's: the others did not change)."""
        colour, Dn = self.gs[l]
        o0, nloc = lv['o0'], lv['nloc']
        cl, D = colour[o0:o0 + nloc], Dn[o0:o0 + nloc]
        nc = int(colour.max()) + 1
        for c in (range(nc) if fwd else range(nc - 1, -1, -1)):
            I = np.flatnonzero(cl == c)
            if len(I):
                res = b2[I] - bsr_mv(lv['A'], X)[I]
                X[I] = X[I] + np.stack([D[I, 0, 0] * res[:, 0] + D[I, 0, 1] * res[:, 1],
                                        D[I, 1, 0] * res[:, 0] + D[I, 1, 1] * res[:, 1]], axis=1)
            if not lv['replicated']:
                self.halo(lv, X)
        return X

    def cycle(self, l, b2):
        lv = self.L[l]
        if lv['coarsest']:
            return (self.Ainv @ b2.ravel()).reshape(-1, 2)
        if self.gs is not None and self.gs[l] is not None:
            return self.cycle_gs(l, b2)
        C = self.L[l + 1]
        pre = self.ws * self.nu1
        post = self.ws[::-1] * self.nu2
        X = pre[0] * bd_mv(lv['W'], b2)
        X = self.smooth(lv, b2, X, pre[1:])
        r = b2 - bsr_mv(lv['A'], self.ghosted(lv, X))
        xc = self.coarse(l, r)
        X = X + bsr_mv(lv['P'], self.ghosted(C, xc))
        return self.smooth(lv, b2, X, post)

    def cycle_gs(self, l, b2):
        lv = self.L[l]
        C = self.L[l + 1]
        full = lv['nloc'] + (0 if lv['replicated'] else len(lv['ghosts']))
        X = np.zeros((full, 2))
        for _ in range(self.nu1):
            X = self.gs_sweep(l, lv, X, b2, True)
            if self.sgs:
                X = self.gs_sweep(l, lv, X, b2, False)
        r = b2 - bsr_mv(lv['A'], X)
        xc = self.coarse(l, r)
        X[:lv['nloc']] = X[:lv['nloc']] + bsr_mv(lv['P'], self.ghosted(C, xc))
        if not lv['replicated']:
            self.halo(lv, X)
        for _ in range(self.nu2):
            if self.sgs:
                X = self.gs_sweep(l, lv, X, b2, True)
            X = self.gs_sweep(l, lv, X, b2, False)
        return X[:lv['nloc']]

    def coarse(self, l, r):
        """coarse-grid correction from the owned residual rows r: restriction,
        reverse-add / all-reduce, coarse cycle (W: twice), scaling."""
        lv = self.L[l]
        C = self.L[l + 1]
        part = bsr_mv(lv['R'], r)
        if lv['replicated']:
            bc = part
        elif C['replicated']:
            bc = self.comm.allreduce_sum(part)
        else:
            bc = self.reverse_add(C, part)
        xc = self.cycle(l + 1, bc)
        if self.wcycle and not C['coarsest']:
            cc = bc - bsr_mv(C['A'], self.ghosted(C, xc))
            xc = xc + self.cycle(l + 1, cc)
        if self.scaling:
            q = bsr_mv(C['A'], self.ghosted(C, xc))
            sums = np.array([[np.sum(bc * xc), np.sum(q * xc)]])
            if not C['replicated']:
                sums = self.comm.allreduce_sum(sums)
            num, den = float(sums[0, 0]), float(sums[0, 1])
            xc = (num / den if den > 0 else 1.0) * xc
        return xc

    def apply_local(self, r_local_fieldmajor):
        """r_local: [u1 owned ; u2 owned] (length 2*nloc) -> z_local, same layout."""
        nloc = self.L[0]['nloc']
        b2 = np.stack([r_local_fieldmajor[:nloc], r_local_fieldmajor[nloc:]], axis=1)
        z2 = self.cycle(0, b2)
        return np.concatenate([z2[:, 0], z2[:, 1]])


def nodemajor_Ainv(Ainv):
    n = Ainv.shape[0]
    nv = n // 2
    pos = np.array([2 * (i % nv) + i // nv for i in range(n)])
    out = np.empty_like(Ainv)
    out[np.ix_(pos, pos)] = Ainv
    return out


def local_slice(v, nv, o0, o1):
    return np.concatenate([v[o0:o1], v[nv + o0: nv + o1]])


# --------------------------------------------------------------------------
# Node-patch Schwarz on P ranks (dist_layout.hip dist_patches
# / dist_apply.hip dcycle_patch): rank p owns the nodes [own[p], own[p+1]) (contiguous, as
# the level-0 z-slabs); its local copy of x covers the owned nodes and every
# node within 3 hops; it computes the patches centred within 1 hop of its
# nodes (each patch that writes an owned node) from its local x, writes the
# patch's dofs locally, and after each colour receives from the owners the
# nodes that colour's patches wrote inside its 3-hop region.  The owner of a
# written node computes the same patch from the same values, so the sweep is
# the sequential multiplicative sweep (mamg_oracle.Patches.sweep) exactly.
# --------------------------------------------------------------------------
def _hops(Gd, seeds_mask, k):
    """boolean mask of the nodes within k hops of the seeds (Gd: closed node graph)."""
    m = seeds_mask.copy()
    for _ in range(k):
        m = m | (Gd.T @ m.astype(np.int64) > 0)
    return m


class PartitionedPatchSweep:
    """P ranks of a node-patch sweep on one process (numpy), with the halo
    lists of the product: ghost region = 3 hops, centres = 1 hop, per colour
    the written nodes (a node is written by the colours of the patches
    centred in its closed neighbourhood)."""

    def __init__(self, A, patches, own):
        import scipy.sparse as sp
        from mamg_oracle import node_pattern
        self.A = A.tocsr()
        self.pt = patches
        self.own = list(own)
        nv = patches.nv
        G = node_pattern(self.A, 2)
        Gd = (G + sp.identity(nv, dtype=np.int8, format='csr')).tocsr()
        Gd.data[:] = 1
        self.Gd = Gd
        self.P = len(own) - 1
        # colours writing each node: the colours of the centres in its closed ring
        self.writers = [set(patches.colour[Gd.indices[Gd.indptr[J]:Gd.indptr[J + 1]]].tolist()) for J in range(nv)]
        self.region, self.centres, self.owner = [], [], np.zeros(nv, np.int64)
        for p in range(self.P):
            mine = np.zeros(nv, bool)
            mine[own[p]:own[p + 1]] = True
            self.owner[own[p]:own[p + 1]] = p
            self.region.append(_hops(Gd, mine, 3))
            self.centres.append(np.flatnonzero(_hops(Gd, mine, 1)))

    def sweep(self, x, b, forward=True):
        """the partitioned sweep from the global x (copied to every rank);
        returns the gathered owned values"""
        nv = self.pt.nv
        xs = [x.copy() for _ in range(self.P)]          # rank p's valid entries: region[p]
        cols = range(self.pt.ncolours) if forward else range(self.pt.ncolours - 1, -1, -1)
        for c in cols:
            written = []
            for p in range(self.P):
                I = self.centres[p][self.pt.colour[self.centres[p]] == c]
                xp = xs[p]
                D = self.pt.dofs[I]
                ok = D >= 0
                dd = D[ok]
                # a patch reads x within 2 hops of its centre: inside rank p's region
                rows = self.A[dd]
                assert np.all(self.region[p][rows.indices % nv]), 'patch reads outside the 3-hop region'
                res = np.zeros(D.shape)
                res[ok] = b[dd] - rows @ xp
                delta = np.einsum('kij,kj->ki', self.pt.Minv[I], res)
                xp[dd] = xp[dd] + delta[ok]
                written.append(set((dd % nv).tolist()))
            # colour c's halo: every rank takes the owner's value of each node
            # in its 3-hop region that colour c writes
            upd = np.array(sorted(set().union(*written)), np.int64)
            for p in range(self.P):
                if not len(upd):
                    break
                mine = upd[self.region[p][upd]]
                for J in mine:
                    q = self.owner[J]
                    if q != p:
                        assert c in self.writers[J]
                        for f in (0, 1):
                            xs[p][f * nv + J] = xs[q][f * nv + J]
        out = np.empty_like(x)
        for p in range(self.P):
            for f in (0, 1):
                out[f * nv + self.own[p]:f * nv + self.own[p + 1]] = xs[p][f * nv + self.own[p]:f * nv + self.own[p + 1]]
        return out


# --------------------------------------------------------------------------
# Seed-ring Schwarz on P ranks (dist_layout.hip dist_rings /
# dist_apply.hip dcycle_rings): rank p owns the nodes [own[p], own[p+1]); its local copy of x
# covers the owned nodes and every node within 2 maxlvl + 1 hops; it computes
# every block with a member node it owns (all members lie within 2 maxlvl
# hops of that node, their rows read within 2 maxlvl + 1) from its local x,
# writes the block's dofs locally, and after each colour receives from the
# owners the nodes that colour's blocks wrote inside its region.  The owner of
# a written node computes every block that writes it from the same values,
# so the sweep is mamg_oracle.Rings.sweep exactly.
# --------------------------------------------------------------------------
class PartitionedRingSweep:
    """P ranks of a seed-ring sweep on one process (numpy), with the halo
    lists of the product (region = 2 maxlvl + 1 hops, per colour the nodes
    its blocks write)."""

    def __init__(self, A, rings, own, maxlvl):
        import scipy.sparse as sp
        from mamg_oracle import node_pattern
        self.A = A.tocsr()
        self.rg = rings
        self.own = list(own)
        n = self.A.shape[0]
        nv = n // 2
        self.nv = nv
        G = node_pattern(self.A, 2)
        Gd = (G + sp.identity(nv, dtype=np.int8, format='csr')).tocsr()
        Gd.data[:] = 1
        self.P = len(own) - 1
        self.owner = np.zeros(nv, np.int64)
        self.region, self.blocks = [], []
        bnodes = [np.unique(np.asarray(b) % nv) for b in rings.blocks]
        for p in range(self.P):
            mine = np.zeros(nv, bool)
            mine[own[p]:own[p + 1]] = True
            self.owner[own[p]:own[p + 1]] = p
            self.region.append(_hops(Gd, mine, 2 * maxlvl + 1))
            self.blocks.append([k for k, bn in enumerate(bnodes) if np.any(mine[bn])])

    def sweep(self, x, b, forward=True):
        """the partitioned sweep from the global x (copied to every rank);
        returns the gathered owned values"""
        nv, rg = self.nv, self.rg
        xs = [x.copy() for _ in range(self.P)]
        cols = range(rg.ncolours) if forward else range(rg.ncolours - 1, -1, -1)
        for c in cols:
            written = set()
            for p in range(self.P):
                ks = [k for k in self.blocks[p] if rg.colour[k] == c]
                if not ks:
                    continue
                xp = xs[p]
                rows = np.concatenate([rg.blocks[k] for k in ks])
                assert np.all(self.region[p][self.A[rows].indices % nv]), 'a block reads outside the region'
                res = b[rows] - self.A[rows] @ xp
                off = 0
                for k in ks:
                    m = len(rg.blocks[k])
                    xp[rg.blocks[k]] += rg.Minv[k] @ res[off:off + m]
                    off += m
                written |= set((rows % nv).tolist())
            upd = np.array(sorted(written), np.int64)
            for p in range(self.P):
                if not len(upd):
                    break
                for J in upd[self.region[p][upd]]:
                    q = self.owner[J]
                    if q != p:
                        for f in (0, 1):
                            xs[p][f * nv + J] = xs[q][f * nv + J]
        out = np.empty_like(x)
        for p in range(self.P):
            for f in (0, 1):
                out[f * nv + self.own[p]:f * nv + self.own[p + 1]] = xs[p][f * nv + self.own[p]:f * nv + self.own[p + 1]]
        return out
