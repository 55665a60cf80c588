"""fp32 storage of the operators the cycle streams (mamg_set_cycle_storage).

The contract: a narrowed handle's apply is the fp64
cycle on operators rounded to fp32, up to summation order.  So the reference
is the numpy restatement (cycle_storage_ref.py, pinned against the oracle by
tests/test_cycle_storage.py) under the mask the handle itself reports, and
the bound is the suite's APPLY_TOL = 1e-10, the one every fp64 parity test
uses -- no tolerance of its own.  That the narrowed apply is more than 1e-10
away from the unrounded restatement shows the rounding happened.

Inputs are the smallest that reach each kernel: 3-D n = 8 (729 nodes: not a
multiple of the 64-row slices or the 256-thread workgroups), 2-D n = 32 (three
levels: the W cycle's second visit), and the renumbered / ragged matrices of
tests/irregular.py (SELL slices with rows of unequal length, a rejected
half-symmetric layout, a lane-group K).  Every input runs with the defaults
(lane-group BSR2 kernels on every level) and with MAMG_SELL_MIN_ROWS=1 (the
benchmark's half-symmetric A_0, SELL K with 16-bit columns, SELL coarse
operators).
"""
import dataclasses
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import irregular
import mamg_oracle as mo
from conftest import set_opt
from cycle_storage_ref import ALL, BIT_A, BIT_KP, BIT_R, StorageRef
from test_gpu import APPLY_TOL, rel

pytestmark = pytest.mark.gpu

ERR_UNSUPPORTED = -4
MODES = ['default', 'sell']
GAMMA = 1e6

INPUTS = {
    'grid3d-8': lambda: irregular.grid(3, 8, GAMMA),
    'grid2d-32': lambda: irregular.grid(2, 32, GAMMA),
    'permuted2d-64': lambda: irregular.permuted(2, 64, GAMMA),
    'ragged96': lambda: irregular.ragged(96, GAMMA),
    'permuted2d-32': lambda: irregular.permuted(2, 32, GAMMA),
    'grid3d-16': lambda: irregular.grid(3, 16, GAMMA),
}


def _mamg():
    import metric_amg_examples_amd as M
    return M


def to_c(kw):
    c = dict(kw)
    for key, names in (('cycle_type', {'V': 1, 'W': 2}), ('smoother', {'JACOBI_RHO': 3, 'POLY': 12, 'SGS': 11})):
        if key in c:
            c[key] = names[c[key]]
    return c


@functools.lru_cache(maxsize=None)
def system(name):
    return INPUTS[name]()


@functools.lru_cache(maxsize=None)
def oracle_levels(name, smoother):
    A, nv, idofs = system(name)
    return mo.setup(A, mo.Params(num_functions=2, smoother=smoother), idofs=idofs)


def oracle(name, **kw):
    """The oracle's hierarchy under kw; every key but the smoother is read by the apply only."""
    kw = dict(kw)
    kw.pop('post_fusion', None)
    h = oracle_levels(name, kw.pop('smoother', 'JACOBI_RHO'))
    return mo.Hierarchy(h.levels, dataclasses.replace(h.params, **kw))


def build(name, mode, setup='gpu', narrow=True, **kw):
    M = _mamg()
    if mode == 'sell':
        set_opt('MAMG_SELL_MIN_ROWS', '1')
    A, nv, idofs = system(name)
    B = M.MetricAMG(A, [nv, nv], idofs=idofs, num_functions=2, setup=setup, **to_c(kw))
    assert B.layout == 'bsr2' and B.setup_path == setup
    if narrow:
        B.set_cycle_storage('f32')
    return B


def bits(B, l):
    s = B.level_storage(l)
    return (BIT_A if s['A'] else 0) | (BIT_KP if s['KP'] else 0) | (BIT_R if s['R'] else 0)


def restatement(B, name, **kw):
    """The numpy cycle under the storage mask and the post forms the handle reports."""
    n = B.num_levels
    return StorageRef(oracle(name, **kw), masks=[bits(B, l) for l in range(n)],
                      kform=[bool(B.level_format(l)['post_fused']) for l in range(n)])


def check_parity(B, name, expect0=ALL, **kw):
    """Two seeded right-hand sides: within APPLY_TOL of the restatement under
    the reported mask, more than APPLY_TOL from the unrounded restatement."""
    A = system(name)[0]
    assert bits(B, 0) == expect0, B.level_storage(0)
    assert bits(B, B.num_levels - 1) == 0          # the coarsest level holds no streamed operator
    ref = restatement(B, name, **kw)
    ref64 = StorageRef(oracle(name, **kw), masks=0, kform=ref.kform)
    for seed in (1234, 7):
        r = mo.seeded_rhs(A.shape[0], seed)
        z = B * r
        e, d = rel(z, ref.apply(r)), rel(z, ref64.apply(r))
        print(name, kw, 'seed', seed, 'vs rounded restatement %.2e, vs unrounded %.2e' % (e, d))
        assert e < APPLY_TOL, e
        assert d > APPLY_TOL, d


# ---------------------------------------------------------------------------
# parity
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('name', ['grid3d-8', 'grid2d-32', 'permuted2d-64', 'ragged96', 'permuted2d-32'])
def test_parity_inputs(lib_built, name, mode):
    B = build(name, mode)
    try:
        f = B.level_format(0)
        if mode == 'sell':
            assert f['sell'] or f['half'], f
            if name.startswith('grid'):     # the benchmark's layouts, really taken
                assert f['half'] and f['post_sell'] and f['k_col16'], f
            if name == 'permuted2d-64':     # scattered mirrors: the half-symmetric layout is rejected
                assert not f['half'] and f['sell'], f
            if name == 'ragged96':          # K rows too long for SELL: lane groups
                assert not f['post_sell'], f
        else:
            assert not f['sell'] and not f['half'] and not f['post_sell'], f
        check_parity(B, name)
    finally:
        B.close()


@pytest.mark.parametrize('name', ['grid3d-8', 'grid2d-32'])
@pytest.mark.parametrize('opt', ['MAMG_HALF', 'MAMG_K_COL16', 'MAMG_HALF_BANDS', 'MAMG_POST_K'])
def test_parity_sell_switches(lib_built, opt, name):
    """Full symmetric SELL instead of the half-symmetric layout, 32-bit K
    columns, the half-symmetric kernel without its band schedule, and every
    SELL K as two 16-byte streams per slot (MAMG_POST_K=2: 8-byte streams in
    fp32)."""
    set_opt(opt, '2' if opt == 'MAMG_POST_K' else '0')
    B = build(name, 'sell')
    try:
        f = B.level_format(0)
        if opt == 'MAMG_POST_K':
            assert f['post_k'] and f['post_sell'], f
        if opt == 'MAMG_HALF':
            assert not f['half'] and f['sell'] and f['sym'], f
        if opt == 'MAMG_K_COL16':
            assert f['post_sell'] and not f['k_col16'], f
        if opt == 'MAMG_HALF_BANDS':
            assert f['half'] and not f['bands'], f
        check_parity(B, name)
    finally:
        B.close()


VARIANTS = [dict(), dict(cycle_type='W'), dict(smoother='POLY', poly_degree=2),
            dict(presmooth_iter=2, postsmooth_iter=2), dict(coarse_scaling=1), dict(post_fusion=0),
            dict(cycle_type='W', smoother='POLY', poly_degree=2, presmooth_iter=2, postsmooth_iter=2,
                 coarse_scaling=1)]


def vid(kw):
    return '-'.join('%s=%s' % kv for kv in kw.items()) or 'defaults'


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('setup', ['host', 'gpu'])
@pytest.mark.parametrize('kw', VARIANTS, ids=vid)
def test_parity_parameters(lib_built, kw, setup, mode):
    B = build('grid3d-8', mode, setup, **kw)
    try:
        if kw.get('post_fusion') == 0:
            assert not B.level_format(0)['post_fused']
        check_parity(B, 'grid3d-8', **kw)
    finally:
        B.close()


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('kw', [v for v in VARIANTS if v.get('cycle_type') == 'W'], ids=vid)
def test_parity_w_cycle_three_levels(lib_built, kw, mode):
    """2-D n = 32 has three levels, so the W cycle's second visit and the
    coarse scaling read a narrowed A_1."""
    B = build('grid2d-32', mode, **kw)
    try:
        assert B.num_levels >= 3 and bits(B, 1) & BIT_A
        check_parity(B, 'grid2d-32', **kw)
    finally:
        B.close()


@pytest.mark.parametrize('mode', MODES)
def test_merged_post_operator_stays_fp64(lib_built, mode):
    """MAMG_POST_K=0 stores [P | AP]: that operator keeps fp64, A and R narrow."""
    set_opt('MAMG_POST_K', '0')
    B = build('grid3d-8', mode)
    try:
        f = B.level_format(0)
        assert f['post_fused'] and not f['post_k'], f
        check_parity(B, 'grid3d-8', expect0=BIT_A | BIT_R)
    finally:
        B.close()


# ---------------------------------------------------------------------------
# bitwise properties
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('mode', MODES)
def test_host_and_gpu_setup_bitwise_and_repeatable(lib_built, mode):
    import torch
    M = _mamg()
    A = system('grid3d-8')[0]
    r = torch.as_tensor(mo.seeded_rhs(A.shape[0])).cuda()
    zs = []
    for setup in ('host', 'gpu'):
        B = build('grid3d-8', mode, setup)
        try:
            z1 = B.matvec(r).clone()
            z2 = B.matvec(r).clone()
            B._Aop = A
            M.ConjGrad(A, precond=B, tolerance=1e-8, maxiter=500, device=True) * mo.seeded_rhs(A.shape[0], 7)
            z3 = B.matvec(r).clone()
            torch.cuda.synchronize()
            assert torch.equal(z1, z2) and torch.equal(z1, z3)
            zs.append(z1)
        finally:
            B.close()
    assert torch.equal(zs[0], zs[1])


@pytest.mark.parametrize('mode', MODES)
def test_narrowing_drops_cached_graphs(lib_built, mode):
    """Apply (a graph is cached for these pointers), narrow, apply into the
    same pointers: the result changes, and is bitwise that of a handle
    narrowed before its first apply."""
    import torch
    A = system('grid3d-8')[0]
    r = torch.as_tensor(mo.seeded_rhs(A.shape[0])).cuda()
    z = torch.empty_like(r)
    B = build('grid3d-8', mode, narrow=False)
    F = build('grid3d-8', mode)
    try:
        B.apply_device(r, z)
        torch.cuda.synchronize()
        z64 = z.clone()
        B.set_cycle_storage('f32')
        B.apply_device(r, z)
        torch.cuda.synchronize()
        assert not torch.equal(z, z64)
        assert torch.equal(z, F.matvec(r))
    finally:
        B.close()
        F.close()


@pytest.mark.parametrize('mode', MODES)
def test_krylov_operator_stays_fp64(lib_built, mode):
    import torch
    A = system('grid3d-8')[0]
    x = torch.as_tensor(mo.seeded_rhs(A.shape[0], 7)).cuda()
    B = build('grid3d-8', mode, narrow=False)
    try:
        y0 = B.spmv_device(x, torch.empty_like(x)).clone()
        B.set_cycle_storage('f32')
        y1 = B.spmv_device(x, torch.empty_like(x))
        torch.cuda.synchronize()
        assert torch.equal(y0, y1)
        assert rel(y1.cpu().numpy(), A @ x.cpu().numpy()) < 1e-13
    finally:
        B.close()


# ---------------------------------------------------------------------------
# device PCG
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('name,iters', [('grid3d-16', 38), ('grid2d-32', None)])
def test_device_pcg(lib_built, name, iters, mode):
    M = _mamg()
    A = system(name)[0]
    b = mo.seeded_rhs(A.shape[0])
    out = {}
    for narrow in (False, True):
        B = build(name, mode, narrow=narrow)
        try:
            B._Aop = A
            cg = M.ConjGrad(A, precond=B, tolerance=1e-8, maxiter=500, device=True)
            x = cg * b
            out[narrow] = (np.asarray(x), np.array(cg.residuals))
            if narrow:
                ref = mo.pcg(A, restatement(B, name), b, 1e-8, 500)
        finally:
            B.close()
    (x64, r64), (x32, r32) = out[False], out[True]
    dx = rel(x32, x64)
    print(name, mode, 'iters fp64 %d f32 %d restatement %d, solution diff %.2e'
          % (len(r64) - 1, len(r32) - 1, ref.niters, dx))
    assert len(r32) == len(ref.residuals)
    assert np.allclose(r32, ref.residuals, rtol=1e-6, atol=0)
    assert len(r32) == len(r64)
    if iters is not None:
        assert len(r32) - 1 == iters
    assert dx < 1e-9, dx


# ---------------------------------------------------------------------------
# bytes
# ---------------------------------------------------------------------------
def node_blocks(M):
    """(blocks, strictly lower blocks) of the 2x2 node-block pattern of a field-major matrix."""
    M = sp.csr_matrix(M)
    nr, nc = M.shape[0] // 2, M.shape[1] // 2
    C = M.tocoo()
    G = sp.csr_matrix((np.ones(C.nnz), (C.row % nr, C.col % nc)), shape=(nr, nc))
    G.sum_duplicates()
    G = G.tocoo()
    return G.nnz, int(np.sum(G.col < G.row))


def pattern(M):
    M = sp.csr_matrix(M, copy=True)
    M.data[:] = 1.0
    return M


def op_bytes(fmt, nb, nlo, nr, nc, epi, vb):
    """include/mamg.h: one launch of a BSR2 operator storing vb bytes per value."""
    idx = 4.0 * nr + 8.0 * (nr // 64 + 2) if fmt.get('sell') else 8.0 * (nr + 1)
    if fmt.get('half'):
        b = (3 * vb + 4.0) * (nb - nlo) + 4.0 * nlo + 4.0 * nr + 16.0 * nc + 16.0 * nr
    else:
        per = 3 * vb + 4.0 if fmt.get('sym') else 4 * vb + 2.0 if fmt.get('col16') else 4 * vb + 4.0
        b = per * nb + idx + (4.0 * (nr // 64 + 1) if fmt.get('col16') else 0.0) + 16.0 * nc + 16.0 * nr
    return b + {'resid': 16.0 * nr, 'kpost': 64.0 * nr, 'y': 0.0}[epi]


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('name', ['grid3d-8', 'grid2d-32'])
def test_bytes(lib_built, name, mode):
    """The level-0 residual (class 0) and K (class 1) report the documented
    per-format formula at 4 bytes per value; the apply's total drops by 4
    bytes per stored value of every narrowed operator (V cycle, nu = 1: each
    of A_l, K_l, R_l is read once per apply)."""
    import torch
    A = system(name)[0]
    h = oracle(name)
    r = torch.as_tensor(mo.seeded_rhs(A.shape[0])).cuda()
    z = torch.empty_like(r)
    B = build(name, mode, narrow=False)
    try:
        before = B.apply_bytes
        cb64 = B.time_apply(r, z, 0)[2]
        B.set_cycle_storage('f32')
        after = B.apply_bytes
        cb32 = B.time_apply(r, z, 0)[2]
        saved = 0.0
        for l, lev in enumerate(h.levels[:-1]):
            f = B.level_format(l)
            assert bits(B, l) == ALL
            nbA, nloA = node_blocks(lev.A)
            nbK, _ = node_blocks(pattern(lev.A) @ pattern(lev.P))
            nbR, _ = node_blocks(lev.R)
            nr, nc = lev.A.shape[0] // 2, lev.P.shape[1] // 2
            fA = dict(half=f['half'], sym=f['sym'], sell=f['sell'])
            fK = dict(sell=f['post_sell'], col16=f['k_col16'])
            if l == 0:
                for vb, cb in ((8.0, cb64), (4.0, cb32)):
                    assert cb[0] == op_bytes(fA, nbA, nloA, nr, nr, 'resid', vb), (vb, cb[0])
                    assert cb[1] == op_bytes(fK, nbK, 0, nr, nc, 'kpost', vb), (vb, cb[1])
            saved += 4.0 * ((3 * (nbA - nloA) if f['half'] else 3 * nbA if f['sym'] else 4 * nbA) + 4 * nbK + 4 * nbR)
        print(name, mode, 'apply bytes %.0f -> %.0f (saved %.0f)' % (before, after, saved))
        assert after == before - saved and after < before
    finally:
        B.close()


# ---------------------------------------------------------------------------
# refusals: MAMG_ERR_UNSUPPORTED, the reason named, the apply bitwise unchanged
# ---------------------------------------------------------------------------
def refused(B, r, storage, word):
    import torch
    M = _mamg()
    z0 = B.matvec(r).clone()
    with pytest.raises(M._lib.MamgError) as ei:
        B.set_cycle_storage(storage)
    assert ei.value.code == ERR_UNSUPPORTED and word in str(ei.value), str(ei.value)
    z1 = B.matvec(r)
    torch.cuda.synchronize()
    assert torch.equal(z0, z1)


def test_refusals(lib_built):
    import torch
    M = _mamg()
    A, nv, idofs = system('grid3d-8')
    r = torch.as_tensor(mo.seeded_rhs(A.shape[0])).cuda()
    s = M.problems.bidomain(3, 8, GAMMA)
    A16, nv16, idofs16 = irregular.grid(2, 16, GAMMA)
    big = sp.csr_matrix(A16 * 1e40)
    cases = [
        (lambda: M.MetricAMG(A, [nv, nv], idofs=idofs, num_functions=1), r, 'CSR'),
        (lambda: M.MetricAMG(s.scipy(), s.W, idofs=s.idofs, num_functions=2, smoother=11, Schwarz_type=7), r, 'SGS'),
        (lambda: M.metricAMG(s.scipy(), s.W, idofs=s.idofs, parameters=M.parameters.parameters_metric_schwarz),
         r, 'SCHWARZ_PATCHES'),
        (lambda: M.MetricAMG(big, [nv16, nv16], idofs=idofs16, num_functions=2),
         torch.as_tensor(mo.seeded_rhs(big.shape[0])).cuda(), 'not representable'),
    ]
    for make, rr, word in cases:
        B = make()
        try:
            for l in range(B.num_levels):
                assert bits(B, l) == 0
            refused(B, rr, 'f32', word)
            for l in range(B.num_levels):
                assert bits(B, l) == 0
            B.set_cycle_storage('f64')          # un-narrowed: MAMG_OK
        finally:
            B.close()


def test_one_way(lib_built):
    """F32 twice is a no-op; F64 after F32 is refused, the handle unchanged."""
    import torch
    A = system('grid3d-8')[0]
    r = torch.as_tensor(mo.seeded_rhs(A.shape[0])).cuda()
    B = build('grid3d-8', 'default')
    try:
        z0 = B.matvec(r).clone()
        nbytes = B.apply_bytes
        B.set_cycle_storage('f32')
        assert B.apply_bytes == nbytes and bits(B, 0) == ALL
        assert torch.equal(B.matvec(r), z0)
        refused(B, r, 'f64', 'one way')
        assert bits(B, 0) == ALL
    finally:
        B.close()


def test_keyword(lib_built):
    """cycle_storage='f32' on the constructor and the factories is the call after setup."""
    import torch
    M = _mamg()
    A, nv, idofs = system('grid3d-8')
    r = torch.as_tensor(mo.seeded_rhs(A.shape[0])).cuda()
    prm = dict(parameters=M.parameters.parameters_metric_mi355x, num_functions=2, setup='gpu')
    B = M.MetricAMG(A, [nv, nv], idofs=idofs, **prm)
    B.set_cycle_storage('f32')
    K = M.metricAMG(A, [nv, nv], idofs=idofs, cycle_storage='f32', **prm)
    F = M.precond.get_hazmath_metric_precond_mono(A, [nv, nv], interface_dofs=idofs, cycle_storage='f32', **prm)
    try:
        assert bits(B, 0) == ALL and bits(K, 0) == ALL and bits(F, 0) == ALL
        z = B.matvec(r)
        assert torch.equal(K.matvec(r), z) and torch.equal(F.matvec(r), z)
    finally:
        for H in (B, K, F):
            H.close()
