"""GPU parity of the seed-ring Schwarz on the CSR layout (Schwarz_type RINGS on
a scalar system, or a nodal one with point smoothers: ring_csr_kernel, one
workgroup per block of a ring colour, and point-wise GS over the rows in no
block) against the CPU restatement tests/pointrings_ref.py, for the host
setup and the GPU setup.

Cases:
  0  emi_3d1d(8, 1e6, 0.0), SGS_POINT, mmsize 200: N = 737, 8 blocks in 8 ring
     colours, 9 rest colours; level 0 fits the one-workgroup rest kernel
  1  emi_3d1d(16, 1e4, 1.0), SA + MIS + V, Jacobi-rho, mmsize 100, coarse_dof
     300: N = 4936, 23 blocks capped at 100 dofs in 17 ring colours, member rows
     of 93 entries; launched rest sweeps, a Jacobi coarse level
  2  emi_3d1d(16, 1e4, 5.0), the same profile, mmsize 200: 23 ring colours,
     member rows of 404 entries, 10 rest colours; the whole level-0 graph needs
     more than 64 colours, so this passes only with the rest-only colouring
  3  bidomain 2-D n = 32 as a scalar system, seeds arange(5, N, 37), maxlvl 1,
     UA + HEM + W, SGS_POINT: N = 2178, 59 blocks in 1 colour, 4 levels
  4  the same system, SA + MIS + V, GS_POINT, maxlvl 2: 4 ring colours of up to
     21 blocks; forward before and backward after on the coarse levels
  5  emi(2, 32, 1e6), num_functions 2, UA + HEM + W, SGS_POINT + scaling,
     interface seeds, maxlvl 2: N = 1122, 33 blocks in 6 colours; nodal
     aggregation with point sweeps
and the refusal of case 2's system with UA + HEM + W (theta 0.1) and SGS_POINT:
level 1 has rows of 411 entries and needs more than 64 colours.

Tolerances as for every smoother (tests/test_gpu_gs.py, test_gpu_point_gs.py;
gamma <= 1e6 here): one apply to 1e-10 relative -- blocks, inverses, colours and
hierarchy are exact, only the summation order of a row, of a local solve, and
the multiplication by 1 / a_ii differ -- PCG iteration counts equal to the
restatement's with residual histories within 1e-6, <u, B v> = <v, B u> to 1e-10
without scaling.
"""
import functools
import os

import numpy as np
import pytest

import mamg_oracle as mo
import pointrings_ref as rr
from conftest import set_opt

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def _mamg():
    import metric_amg_examples_amd as M
    return M


def rel(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


SAV = dict(AMG_type='SA', aggregation_type='MIS', cycle_type='V', coarse_dof=300, max_levels=30, Schwarz_maxlvl=2,
           num_functions=1)
UAW = dict(AMG_type='UA', aggregation_type='HEM', cycle_type='W')
# (system, smoother below the rings, oracle keywords)
CASES = [
    (('3d1d', 8, 1e6, 0.0), 'SGS', dict(num_functions=1, Schwarz_maxlvl=2, Schwarz_mmsize=200)),
    (('3d1d', 16, 1e4, 1.0), 'JACOBI_RHO', dict(SAV, Schwarz_mmsize=100)),
    (('3d1d', 16, 1e4, 5.0), 'JACOBI_RHO', dict(SAV, Schwarz_mmsize=200)),
    (('bidomain', 32), 'SGS', dict(UAW, num_functions=1, Schwarz_maxlvl=1)),
    (('bidomain', 32), 'GS', dict(AMG_type='SA', aggregation_type='MIS', cycle_type='V', num_functions=1,
                                  Schwarz_maxlvl=2)),
    (('emi', 32, 1e6), 'SGS', dict(UAW, num_functions=2, coarse_scaling=1, Schwarz_maxlvl=2)),
]
# (blocks, ring colours, rest colours, levels) of each case, as the restatement builds them
SHAPE = [(8, 8, 9, 2), (23, 17, 11, 2), (23, 23, 10, 2), (59, 1, 10, 4), (59, 4, 9, 3), (33, 6, 5, 3)]
REFUSED = (('3d1d', 16, 1e4, 5.0), 'SGS', dict(UAW, strong_coupled=0.1, num_functions=1, Schwarz_maxlvl=2,
                                               Schwarz_mmsize=200))


@functools.lru_cache(maxsize=None)
def problem(sys_):
    M = _mamg()
    if sys_[0] == '3d1d':
        s = M.problems.emi_3d1d(sys_[1], sys_[2], sys_[3])
        return s.scipy(), np.asarray(s.idofs, np.int32)
    if sys_[0] == 'emi':
        s = M.problems.emi(2, sys_[1], sys_[2])
        return s.scipy(), np.asarray(s.idofs, np.int32)
    s = M.problems.bidomain(2, sys_[1], 1.0)
    return s.scipy(), np.arange(5, s.N, 37, dtype=np.int32)


@functools.lru_cache(maxsize=None)
def reference(k):
    """the restatement of CASES[k] and its applies to the two seeded vectors (computed once)"""
    sys_, smo, kw = CASES[k]
    A, seeds = problem(sys_)
    ref = rr.PointRings(A, seeds, smo, **kw)
    return ref, {seed: ref.apply(mo.seeded_rhs(A.shape[0], seed)) for seed in (1234, 7)}


def handle(k, setup='auto', **extra):
    sys_, smo, kw = CASES[k]
    A, seeds = problem(sys_)
    return _mamg().MetricAMG(A, None, idofs=seeds, setup=setup, **dict(rr.to_c(dict(kw, smoother=smo)), **extra))


@pytest.mark.parametrize('k', range(len(CASES)))
def test_restatement_shapes(k):
    """the cases exercise what the table above says (CPU only; shared with the GPU tests below)"""
    ref, _ = reference(k)
    nb, nrc, nrest, nlev = SHAPE[k]
    assert (len(ref.rings.blocks), ref.rings.ncolours, len(ref.rest_rows), len(ref.levels)) == SHAPE[k]
    A = ref.levels[0].A
    rowlen = np.diff(A.indptr)
    if k == 1:
        assert max(len(b) for b in ref.rings.blocks) == 100 and rowlen[ref.cov].max() == 93
    if k == 2:
        assert rowlen[ref.cov].max() == 404 and rowlen[~ref.cov].max() <= 15
        with pytest.raises(RuntimeError):                      # the whole graph: more than 64 colours
            mo.jp_colouring(rr.pr.offdiag_pattern(A), 0)
    if k == 3:
        assert len(ref.rings.cblocks[0]) == 59


@pytest.mark.parametrize('setup', ['host', 'gpu'])
@pytest.mark.parametrize('k', range(len(CASES)))
def test_apply_matches_restatement(lib_built, k, setup):
    import torch
    sys_, smo, kw = CASES[k]
    A, seeds = problem(sys_)
    B = handle(k, setup)
    assert B.setup_path == setup, B.setup_path
    ref, zs = reference(k)
    assert B.num_levels == len(ref.levels)
    assert B.layout == 'csr'
    ep = B.effective_params
    assert ep['Schwarz_type'] == rr.SCHWARZ_RINGS and ep['Schwarz_levels'] == 1
    f0 = B.level_format(0)
    assert f0['rings'] and f0['gs']
    for l in range(1, B.num_levels - 1):
        fl = B.level_format(l)
        assert not fl['rings'] and fl['gs'] == (smo in ('GS', 'SGS'))
    for seed in (1234, 7):
        r = mo.seeded_rhs(A.shape[0], seed)
        z = B * r
        zt = B.matvec(torch.as_tensor(r).cuda())
        torch.cuda.synchronize()
        e1, e2 = rel(z, zs[seed]), rel(zt.cpu().numpy(), zs[seed])
        print('case %d %s seed %d: rel err host vectors %.3e, device vectors %.3e' % (k, setup, seed, e1, e2))
        assert e1 <= 1e-10 and e2 <= 1e-10


@pytest.mark.parametrize('k', range(len(CASES)))
def test_pcg_matches_restatement(lib_built, k):
    M = _mamg()
    sys_, smo, kw = CASES[k]
    A, seeds = problem(sys_)
    b = mo.seeded_rhs(A.shape[0])
    solver = M.ConjGrad(A, precond=handle(k), tolerance=1e-8, maxiter=500)
    x = solver * b
    ref = rr.pcg(A, reference(k)[0], b, 1e-8, 500)
    print('case %d PCG: %d iterations, restatement %d' % (k, len(solver.residuals) - 1, ref.niters))
    assert len(solver.residuals) == len(ref.residuals)
    assert np.allclose(solver.residuals, ref.residuals, rtol=1e-6, atol=0)
    x = x.cpu().numpy() if hasattr(x, 'cpu') else np.asarray(x)
    assert rel(x, ref.x) < 1e-6


@pytest.mark.parametrize('k', [1, 3, 5])
def test_setups_bitwise_equal(lib_built, k):
    A, seeds = problem(CASES[k][0])
    Bg, Bh = handle(k, 'gpu'), handle(k, 'host')
    assert Bg.setup_path == 'gpu' and Bh.setup_path == 'host'
    r = mo.seeded_rhs(A.shape[0], 7)
    assert np.array_equal(Bg * r, Bh * r)


@pytest.mark.parametrize('k', [0, 2, 4])
def test_repeat_and_graph_equal_eager(lib_built, k):
    """two graph replays give identical bits, and so does the eager op list of mamg_time_apply"""
    import torch
    A, seeds = problem(CASES[k][0])
    B = handle(k)
    r = torch.as_tensor(mo.seeded_rhs(A.shape[0], 1234)).cuda()
    z1, z2 = B.matvec(r), B.matvec(r)
    ze = torch.empty_like(r)
    B.time_apply(r, ze, 1, mode=1)
    torch.cuda.synchronize()
    assert torch.equal(z1, z2) and torch.equal(z1, ze)
    assert rel(z1.cpu().numpy(), reference(k)[1][1234]) <= 1e-10


@pytest.mark.parametrize('k', [0, 2])
def test_poison(lib_built, k):
    """nothing reads a double that nothing wrote: with every double array
    starting as NaN bytes the result keeps its bits"""
    A, seeds = problem(CASES[k][0])
    r = mo.seeded_rhs(A.shape[0], 7)
    z = handle(k) * r
    set_opt('MAMG_POISON', '1')
    zp = handle(k) * r
    assert np.isfinite(zp).all() and np.array_equal(z, zp)


@pytest.mark.parametrize('k', [0, 1])
def test_two_cycles_per_apply(lib_built, k):
    """maxit 2: the second cycle runs on r - A z into the level-0 work vectors"""
    sys_, smo, kw = CASES[k]
    A, seeds = problem(sys_)
    B = handle(k, maxit=2)
    r = mo.seeded_rhs(A.shape[0], 1234)
    zo = rr.PointRings(A, seeds, smo, **dict(kw, maxit=2)).apply(r)
    e = rel(B * r, zo)
    print('case %d maxit 2: rel err %.3e' % (k, e))
    assert e <= 1e-10


@pytest.mark.parametrize('k', [1, 3, 4])
def test_symmetric_without_scaling(lib_built, k):
    """V and W cycles, Jacobi-rho, SGS and GS (forward before, backward after)
    below the palindromic level-0 step: a symmetric operator"""
    import torch
    sys_, smo, kw = CASES[k]
    assert not kw.get('coarse_scaling')
    A, seeds = problem(sys_)
    B = handle(k)
    u = torch.as_tensor(mo.seeded_rhs(A.shape[0], 1)).cuda()
    v = torch.as_tensor(mo.seeded_rhs(A.shape[0], 2)).cuda()
    Bu, Bv = B.matvec(u), B.matvec(v)
    torch.cuda.synchronize()
    a, c = float(torch.dot(u, Bv)), float(torch.dot(v, Bu))
    print('case %d: <u, B v> = %.17g, <v, B u> = %.17g' % (k, a, c))
    assert abs(a - c) <= 1e-10 * abs(a)


@pytest.mark.parametrize('k', [0, 2])
def test_time_apply_classes(lib_built, k):
    """mamg_time_apply: the ring colour steps and the rest's sweeps are class
    C_L0_SMOOTH (1), the level below C_COARSE (5) or, where level 1 is the
    coarsest, C_DENSE (6); bytes by the documented formula are positive"""
    import torch
    A, seeds = problem(CASES[k][0])
    B = handle(k)
    r = torch.as_tensor(mo.seeded_rhs(A.shape[0], 1234)).cuda()
    z = torch.empty_like(r)
    ms, kms, cb = B.time_apply(r, z, 2, mode=1)
    assert ms > 0 and kms[1] > 0 and cb[1] > 0
    assert (kms[5] > 0 and cb[5] > 0) or (kms[6] > 0 and cb[6] > 0)
    assert all(c >= 0 for c in cb) and B.apply_bytes > 0
    assert abs(sum(cb) - B.apply_bytes) <= 1e-9 * B.apply_bytes
    # the level-0 step dominates: 2 (nu1 + nu2) ring sweeps read every inverse
    ref = reference(k)[0]
    inv_bytes = 8.0 * sum(len(b) ** 2 for b in ref.rings.blocks)
    assert cb[1] >= 4 * inv_bytes
    assert rel(z.cpu().numpy(), reference(k)[1][1234]) <= 1e-10


@pytest.mark.parametrize('setup', ['host', 'gpu'])
def test_coarse_level_colour_cap_is_refused(lib_built, setup):
    """point GS below the rings on a coarse level that needs more than 64
    colours: MAMG_ERR_UNSUPPORTED naming level 1; the same hierarchy with
    Jacobi-rho below the rings runs"""
    M = _mamg()
    sys_, smo, kw = REFUSED
    A, seeds = problem(sys_)
    with pytest.raises(M._lib.MamgError) as ei:
        M.MetricAMG(A, None, idofs=seeds, setup=setup, **rr.to_c(dict(kw, smoother=smo)))
    assert ei.value.code == -4 and 'level 1' in str(ei.value) and '64 colours' in str(ei.value)
    B = M.MetricAMG(A, None, idofs=seeds, setup=setup, **rr.to_c(dict(kw, smoother='JACOBI_RHO')))
    assert B.num_levels >= 3 and B.level_format(0)['rings']


def test_driver_falls_back_to_jacobi_rho_below_the_rings(lib_built, capsys):
    """the 3D-1D drivers' -schwarz rings on that system: the refused point GS
    becomes Jacobi-rho on the coarse levels under the same rings, stated once"""
    M = _mamg()
    from metric_amg_examples_amd import drivers as D
    sys_, smo, kw = REFUSED
    A, seeds = problem(sys_)
    prm = rr.to_c(dict(kw, smoother=smo))
    D._rings_fallback_printed = False
    B = D._metric_amg_3d1d(A, None, seeds, prm)
    B2 = D._metric_amg_3d1d(A, None, seeds, prm)
    out = capsys.readouterr().out
    assert out.count('parameter substitution') == 1 and 'SMOOTHER_JACOBI_RHO' in out and 'level 1' in out
    for h in (B, B2):
        ep = h.effective_params
        assert ep['smoother'] == M.parameters.SMOOTHER_JACOBI_RHO and ep['Schwarz_type'] == rr.SCHWARZ_RINGS
        assert h.level_format(0)['rings'] and not h.level_format(1)['gs']
    ref = rr.PointRings(A, seeds, 'JACOBI_RHO', **kw)
    r = mo.seeded_rhs(A.shape[0], 7)
    assert rel(B * r, ref.apply(r)) <= 1e-10
    # another refusal is not swallowed
    with pytest.raises(M._lib.MamgError):
        D._metric_amg_3d1d(A, None, seeds, dict(prm, Schwarz_mmsize=257))


def _with_entry(A, i, j, v):
    import scipy.sparse as sp
    C = A.tocoo()
    B = sp.csr_matrix((np.r_[C.data, v], (np.r_[C.row, i], np.r_[C.col, j])), shape=A.shape)
    B.sort_indices()
    return B


@pytest.mark.parametrize('setup', ['host', 'gpu'])
def test_level_0_refusals(lib_built, setup):
    """On the rest: a stored explicit zero at (i, j) without (j, i) between two
    uncovered rows is MAMG_ERR_UNSUPPORTED naming level 0, a negated diagonal
    entry of an uncovered row MAMG_ERR_SETUP."""
    M = _mamg()
    k = 4
    sys_, smo, kw = CASES[k]
    A, seeds = problem(sys_)
    unc = np.flatnonzero(~reference(k)[0].cov)
    i, j = int(unc[3]), int(unc[-3])
    assert A[i, j] == 0 and A[j, i] == 0
    Z = _with_entry(A, i, j, 0.0)
    D = A.copy().tolil()
    D[i, i] = -D[i, i]
    D = D.tocsr()
    for X, code, word in ((Z, -4, 'level 0'), (D, -3, 'diagonal')):
        with pytest.raises(M._lib.MamgError) as ei:
            M.MetricAMG(X, None, idofs=seeds, setup=setup, **rr.to_c(dict(kw, smoother=smo)))
        assert ei.value.code == code and word in str(ei.value), str(ei.value)


def _relres_count(A, B, b, tol, maxit):
    """PCG stopped on ||r|| / ||b|| (HAZmath linear_stop_type 1), iteration count"""
    x = np.zeros_like(b)
    r = b.copy()
    z = B.apply(r)
    d = z.copy()
    rz = r @ z
    bn = np.linalg.norm(b)
    it = 0
    while np.linalg.norm(r) > tol * bn and it < maxit:
        q = A @ d
        al = rz / (d @ q)
        x += al * d
        r -= al * q
        z = B.apply(r)
        rz2 = r @ z
        d = z + (rz2 / rz) * d
        rz = rz2
        it += 1
    return it


def test_run_solver_3d1d_with_rings(lib_built, tmp_path, capsys):
    """emi_3d1d -dump 1 -> run_solver_3d1d -schwarz rings: the file's symmetric
    multiplicative Schwarz and GS as the seed rings and GS_POINT; the
    restatement's iteration count with the file's parameters and stopping rule"""
    M = _mamg()
    from metric_amg_examples_amd import drivers as D
    s = M.problems.emi_3d1d(8, 1e4, 1.0)
    A = s.scipy()
    b = M.problems.seeded_rhs(s.N)
    mdir, odir = tmp_path / 'mat', tmp_path / 'out'
    M.fileio.dump_system(A, b, s.W, str(mdir))
    dat = os.path.join(HERE, 'golden', 'solver_3d1d.dat')
    niters = D.run_solver_3d1d(['-infile', dat, '-indir', str(mdir), '-outdir', str(odir), '-schwarz', 'rings'])
    out = capsys.readouterr().out
    assert "colour order instead of HAZmath's sequential seed and dof order" in out
    x = M.fileio.read_solution(str(odir / 'solution.txt'))
    assert np.linalg.norm(b - A @ x) <= 1e-6 * np.linalg.norm(b) * (1 + 1e-9)
    ref = rr.PointRings(A, s.idofs, 'GS', AMG_type='SA', cycle_type='V', aggregation_type='VMB', coarse_dof=300,
                        max_levels=30, Schwarz_maxlvl=2, Schwarz_mmsize=200, num_functions=1)
    want = _relres_count(A, ref, b, 1e-6, 1000)
    print('run_solver_3d1d -schwarz rings: %d iterations, restatement %d' % (niters, want))
    assert niters == want
