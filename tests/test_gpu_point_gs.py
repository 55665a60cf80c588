"""GPU parity of the point-wise multicolour GS / SGS on the CSR layout
(SMOOTHER_GS_POINT / SMOOTHER_SGS_POINT: csr_gs_kernel, one launch per colour,
and csr_gs_small_kernel, a small level's whole smoothing call in one
workgroup) against the CPU restatement tests/pointgs_ref.py.

Sizes: N = 1458 (3-D n = 8) and 2178 (2-D n = 32) run every level in the
one-workgroup kernel (at most 4096 rows); N = 8450 (2-D n = 64) and 9826
(3-D n = 16) launch level 0 colour by colour and fuse the rest.

Tolerances as tests/test_gpu_gs.py: one apply to 1e-10 relative (colouring,
permutation and hierarchy are exact; only the summation order of a row and the
multiplication by 1 / a_ii instead of the division differ), PCG iteration
count equal to the restatement's, residuals and x within 1e-6.
"""
import functools

import numpy as np
import pytest

import mamg_oracle as mo
import pointgs_ref as pr
from conftest import set_opt

pytestmark = pytest.mark.gpu


def _mamg():
    import metric_amg_examples_amd as M
    return M


def rel(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


# (dim, n, gamma, smoother, oracle keywords); the bidomain as a scalar system
# unless num_functions says otherwise
CASES = [
    (2, 32, 1.0, 'SGS', dict(num_functions=1)),
    (2, 64, 1e6, 'SGS', dict(pr.STANDARD)),                                  # parameters_standard itself
    (3, 8, 1e6, 'GS', dict(num_functions=1)),
    (3, 16, 1e4, 'SGS', dict(num_functions=1, coarse_scaling=1, cycle_type='W')),
    (3, 16, 1e2, 'GS', dict(num_functions=1, presmooth_iter=2, postsmooth_iter=2)),
    (3, 16, 1e4, 'SGS', dict(num_functions=2)),                             # nodal aggregates, point sweeps
]


@functools.lru_cache(maxsize=None)
def problem(dim, n, g):
    s = _mamg().problems.bidomain(dim, n, g)
    return s, s.scipy()


@functools.lru_cache(maxsize=None)
def reference(k):
    """the restatement of CASES[k] and its applies to the two seeded vectors (computed once)"""
    dim, n, g, smo, kw = CASES[k]
    s, A = problem(dim, n, g)
    ref = pr.PointGS(A, smo, **kw)
    return ref, {seed: ref.apply(mo.seeded_rhs(s.N, seed)) for seed in (1234, 7)}


def handle(k, setup='auto', **extra):
    dim, n, g, smo, kw = CASES[k]
    s, A = problem(dim, n, g)
    return _mamg().MetricAMG(A, None, setup=setup, **dict(pr.to_c(dict(kw, smoother=smo)), **extra))


@pytest.mark.parametrize('setup', ['host', 'gpu'])
@pytest.mark.parametrize('k', range(len(CASES)))
def test_apply_matches_restatement(lib_built, k, setup):
    import torch
    dim, n, g, smo, kw = CASES[k]
    s, A = problem(dim, n, g)
    B = handle(k, setup)
    assert B.setup_path == setup, B.setup_path
    ref, zs = reference(k)
    assert B.num_levels == len(ref.levels)
    assert B.layout == 'csr' and B.effective_params['node_block_smoother'] == 0
    assert all(B.level_format(l)['gs'] for l in range(B.num_levels - 1))
    for seed in (1234, 7):
        r = mo.seeded_rhs(s.N, seed)
        z = B * r
        zt = B.matvec(torch.as_tensor(r).cuda())
        torch.cuda.synchronize()
        e1, e2 = rel(z, zs[seed]), rel(zt.cpu().numpy(), zs[seed])
        print('case %d %s seed %d: rel err host vectors %.3e, device vectors %.3e' % (k, setup, seed, e1, e2))
        assert e1 <= 1e-10 and e2 <= 1e-10


@pytest.mark.parametrize('k', [0, 3])
def test_two_cycles_per_apply(lib_built, k):
    """maxit 2: the second cycle runs on r - A z into the level-0 work vectors"""
    dim, n, g, smo, kw = CASES[k]
    s, A = problem(dim, n, g)
    B = handle(k, maxit=2)
    r = mo.seeded_rhs(s.N, 1234)
    zo = pr.PointGS(A, smo, **dict(kw, maxit=2)).apply(r)
    e = rel(B * r, zo)
    print('case %d maxit 2: rel err %.3e' % (k, e))
    assert e <= 1e-10


def test_time_apply_classes(lib_built):
    """mamg_time_apply: the launched level-0 colour steps are class C_L0_SMOOTH (1), the one-launch
    smoothing calls of the coarse levels C_COARSE (5); bytes by the documented formula are positive"""
    import torch
    k = 3
    dim, n, g, smo, kw = CASES[k]
    s, A = problem(dim, n, g)
    B = handle(k)
    r = torch.as_tensor(mo.seeded_rhs(s.N, 1234)).cuda()
    z = torch.empty_like(r)
    ms, kms, cb = B.time_apply(r, z, 2, mode=1)
    assert ms > 0 and kms[1] > 0 and kms[5] > 0 and cb[1] > 0 and cb[5] > 0
    assert abs(sum(cb) - B.apply_bytes) <= 1e-9 * B.apply_bytes
    assert rel(z.cpu().numpy(), reference(k)[1][1234]) <= 1e-10


@pytest.mark.parametrize('lanes', [2, 64])
@pytest.mark.parametrize('k', [0, 3])
def test_lanes(lib_built, k, lanes):
    """the narrow and the full-wave lane groups in both kernels"""
    dim, n, g, smo, kw = CASES[k]
    s, A = problem(dim, n, g)
    B = handle(k, spmv_lanes=lanes)
    ref, zs = reference(k)
    e = rel(B * mo.seeded_rhs(s.N, 1234), zs[1234])
    print('case %d lanes %d: rel err %.3e' % (k, lanes, e))
    assert e <= 1e-10


@pytest.mark.parametrize('k', [1, 3, 5])
def test_setups_bitwise_equal(lib_built, k):
    dim, n, g, smo, kw = CASES[k]
    s, A = problem(dim, n, g)
    Bg, Bh = handle(k, 'gpu'), handle(k, 'host')
    assert Bg.setup_path == 'gpu' and Bh.setup_path == 'host'
    assert Bg.layout == 'csr' and Bh.layout == 'csr'
    r = mo.seeded_rhs(s.N, 7)
    assert np.array_equal(Bg * r, Bh * r)


@pytest.mark.parametrize('dim,n,g', [(2, 64, 1e6), (3, 16, 1e4)])
def test_pcg_matches_restatement(lib_built, dim, n, g):
    """ConjGrad with the parameters_standard values (the hazmath preset)"""
    M = _mamg()
    s, A = problem(dim, n, g)
    b = mo.seeded_rhs(s.N)
    B = M.MetricAMG(A, None, **pr.to_c(dict(pr.STANDARD, smoother='SGS')))
    solver = M.ConjGrad(A, precond=B, tolerance=1e-8, maxiter=500)
    x = solver * b
    ref = pr.pcg(A, pr.PointGS(A, 'SGS', **pr.STANDARD), b, 1e-8, 500)
    print('PCG (%d, %d, %g): %d iterations, restatement %d' % (dim, n, g, len(solver.residuals) - 1, ref.niters))
    assert len(solver.residuals) == len(ref.residuals)
    assert np.allclose(solver.residuals, ref.residuals, rtol=1e-6, atol=0)
    x = x.cpu().numpy() if hasattr(x, 'cpu') else np.asarray(x)
    assert rel(x, ref.x) < 1e-6


@pytest.mark.parametrize('smo', ['SGS', 'GS'])
def test_symmetric_and_deterministic(lib_built, smo):
    """Without scaling the V-cycle is a symmetric linear operator (GS: forward
    before, backward after); two graph replays give identical bits."""
    import torch
    M = _mamg()
    s, A = problem(3, 16, 1e4)
    B = M.MetricAMG(A, None, num_functions=1, smoother=pr.SMOOTHER[smo])
    r1 = torch.as_tensor(mo.seeded_rhs(s.N, 1)).cuda()
    r2 = torch.as_tensor(mo.seeded_rhs(s.N, 2)).cuda()
    z1, z2 = B.matvec(r1), B.matvec(r2)
    z1b = B.matvec(r1)
    torch.cuda.synchronize()
    a = float(torch.dot(r2, z1))
    c = float(torch.dot(r1, z2))
    print('%s: <r2, B r1> = %.17g, <r1, B r2> = %.17g' % (smo, a, c))
    assert abs(a - c) <= 1e-12 * abs(a)
    assert torch.equal(z1, z1b)


@pytest.mark.parametrize('k', [0, 3])
def test_poison(lib_built, k):
    """nothing reads an x (or any double) that nothing wrote: with every
    double array starting as NaN bytes the result keeps its bits"""
    dim, n, g, smo, kw = CASES[k]
    s, A = problem(dim, n, g)
    r = mo.seeded_rhs(s.N, 7)
    z = handle(k) * r
    set_opt('MAMG_POISON', '1')
    zp = handle(k) * r
    assert np.isfinite(zp).all() and np.array_equal(z, zp)


def _with_entry(A, i, j, v):
    import scipy.sparse as sp
    C = A.tocoo()
    B = sp.csr_matrix((np.r_[C.data, v], (np.r_[C.row, i], np.r_[C.col, j])), shape=A.shape)
    B.sort_indices()
    return B


@pytest.mark.parametrize('setup', ['host', 'gpu'])
def test_refusals(lib_built, setup):
    """A stored explicit zero at (i, j) without (j, i): the colouring needs an
    undirected graph, MAMG_ERR_UNSUPPORTED.  A negated diagonal entry:
    MAMG_ERR_SETUP.  (Both setups accept both matrices with SMOOTHER_JACOBI_RHO,
    asserted here: the codes are the point-wise GS layout's own.)"""
    M = _mamg()
    s, A = problem(2, 32, 1.0)
    i, j = 3, 900
    assert A[i, j] == 0 and A[j, i] == 0
    Z = _with_entry(A, i, j, 0.0)
    assert Z.nnz == A.nnz + 1
    D = A.copy().tolil()
    D[5, 5] = -D[5, 5]
    D = D.tocsr()
    for X in (Z, D):
        assert M.MetricAMG(X, None, num_functions=1, node_block_smoother=0, setup=setup,
                           smoother=M.parameters.SMOOTHER_JACOBI_RHO).num_levels >= 2
    for X, code in ((Z, -4), (D, -3)):
        with pytest.raises(M._lib.MamgError) as ei:
            M.MetricAMG(X, None, num_functions=1, smoother=M.parameters.SMOOTHER_SGS_POINT, setup=setup)
        assert ei.value.code == code and len(str(ei.value)) > 20


def _cpu_count(tag, dim, n, gamma):
    """PCG iterations of the driver's solve on the CPU: the restatement for
    hazmath / hazmath_Schwarz (parameters_standard, the Schwarz level dropped),
    mamg_oracle.setup with the nodal parameters_metric values for hazmath_HEM"""
    M = _mamg()
    s, A = problem(dim, n, gamma)
    b = M.problems.bidomain_mms_rhs(dim, n, gamma, 2, 3)
    if tag == 'hazmath_HEM':
        B = mo.setup(A, mo.Params(AMG_type='UA', cycle_type='W', aggregation_type='HEM', smoother='SGS',
                                  relaxation=1.2, coarse_dof=100, coarse_scaling=1, strong_coupled=0.1,
                                  Schwarz_levels=0, num_functions=2))
    else:
        B = pr.PointGS(A, 'SGS', **pr.STANDARD)
    return mo.pcg(A, B, b, 1e-8, 500).niters


@pytest.mark.parametrize('tag,dim', [('hazmath', 2), ('hazmath_Schwarz', 2), ('hazmath_HEM', 2),
                                     ('hazmath', 3), ('hazmath_HEM', 3)])
def test_driver_tags_match_cpu_counts(lib_built, tmp_path, capsys, tag, dim):
    from metric_amg_examples_amd import drivers as D
    rows = D.bidomain(['-nrefs', '2', '-gamma', '1', '-precond', tag, '-results', str(tmp_path)], dim)
    out = capsys.readouterr().out
    sizes = [2 ** i for i in range(5 if dim == 2 else 3, (5 if dim == 2 else 3) + 2)]
    assert len(rows) == 2
    for row, n in zip(rows, sizes):
        want = _cpu_count(tag, dim, n, 1.0)
        print('%s %d-D n=%d: %d iterations, CPU %d' % (tag, dim, n, row[1], want))
        assert row[1] == want
    assert (tmp_path / ('bidomain_%dd' % dim) /
            ('iters_precond%s_kappa12_kappa23_gamma1.0_pdegree1.txt' % tag)).exists()
    if tag == 'hazmath_Schwarz':               # the dropped Schwarz level is stated, once
        assert out.count('Schwarz_levels 1 -> 0') == 1


def test_hazmath_schwarz_handle_records_the_dropped_level(lib_built):
    M = _mamg()
    s, A = problem(2, 32, 1.0)
    B = M.precond.get_hazmath_amg_precond(A, s.W, parameters=M.parameters.parameters_standard_schwarz,
                                          pointwise=True)
    assert any('Schwarz_levels 1 -> 0' in n for n in B.substitutions)
    assert any("multicolour order instead of HAZmath's sequential dof order" in n for n in B.substitutions)
    ep = B.effective_params
    assert ep['smoother'] == M.parameters.SMOOTHER_SGS_POINT and ep['num_functions'] == 1
    assert ep['Schwarz_levels'] == 0 and B.layout == 'csr'
