"""The inputs of tests/test_gpu_pcg_edges.py do what those tests rely on --
checked with the CPU reference alone (tests/pcg_edges_ref.py).  These are
conditions on the inputs, not measurements: an input that misses one is
replaced, the margin stays."""
import numpy as np
import pytest

import pcg_edges_ref as pe

RZ_NEG = [n for n, c in pe.CASES.items() if c['outcome'] == 'rz_neg']
NOT_POS = [n for n, c in pe.CASES.items() if c['outcome'] == 'not_pos']
HEALTHY = [n for n, c in pe.CASES.items() if c['outcome'] == 'converged']


def test_checker():
    v = pe.checker(2, 2)
    assert v.tolist() == [1, -1, 1, -1, 1, -1, 1, -1, 1] + [-1, 1, -1, 1, -1, 1, -1, 1, -1]
    assert pe.checker(3, 16).shape == (2 * 17 ** 3,) and abs(pe.checker(3, 16).sum()) == 0.0


@pytest.mark.parametrize('case', RZ_NEG)
def test_breaks_in_the_stated_iteration(lib_built, case):
    """<r,Br> turns negative in iteration k, by a margin many orders above
    round-off, and the restore moves x by far more than the 1e-6 the GPU
    tests allow: they cannot pass without it"""
    c = pe.CASES[case]
    outcome, k, x, res, al, be = pe.reference(case)
    assert outcome == 'rz_neg' and k == c['k']
    assert len(res) == k + 1 and len(al) == len(be) == k
    rz_prev, rz_neg, step, unrestored = pe.margins(case)
    print('%s: <r,Br> %.4g -> %.4g in iteration %d, ||alpha d|| / ||x_k + alpha d|| = %.3g'
          % (case, rz_prev, rz_neg, k, step / unrestored))
    assert rz_prev > 0 and rz_neg < 0 and abs(rz_neg) >= 1e-2 * rz_prev
    assert step >= 1e-2 * unrestored
    if k == 0:                       # x = x0 up to the round-off of (x0 + alpha d) - alpha d
        assert np.linalg.norm(x - pe.vectors(case)[1]) <= 1e-12 * step


@pytest.mark.parametrize('case', NOT_POS)
def test_not_positive_at_the_start(lib_built, case):
    outcome, k, x, res, al, be = pe.reference(case)
    assert outcome == 'not_pos' and k == 0 and np.array_equal(x, pe.vectors(case)[1])
    rz0, rr0 = pe.margins(case)
    print('%s: <r0,Br0> = %.4g, ||r0||^2 = %.4g' % (case, rz0, rr0))
    assert rz0 <= -1e-2 * rr0


@pytest.mark.parametrize('case', HEALTHY)
def test_healthy_counts(lib_built, case):
    c = pe.CASES[case]
    outcome, k, x, res, al, be = pe.reference(case)
    assert outcome == 'converged' and 0 < k < pe.MAXITER
    if c['k'] is not None:
        assert k == c['k']
    if c['stop'] == 1:
        norms = pe.reference_norms(case)
        bn = np.linalg.norm(pe.vectors(case)[0]) or 1.0
        assert len(norms) == k + 1 and norms[-1] <= c['tol'] * bn < norms[-2]
    else:
        thr = c['tol'] * res[0] if c['relativeconv'] else c['tol']
        assert res[-1] <= thr < res[-2]


@pytest.mark.parametrize('a,b,bound', [('h3', 'h3_x7', 2e-10), ('h2', 'h2_x7', 7e-10)])
def test_both_starts_reach_the_same_solution(lib_built, a, b, bound):
    """tabulated: 1.8e-10 (3-D) and 6.9e-10 (2-D)"""
    xa, xb = pe.reference(a)[2], pe.reference(b)[2]
    assert np.linalg.norm(xa - xb) / np.linalg.norm(xa) <= bound


@pytest.mark.parametrize('a,b', [('h3', 'h3_x7'), ('h2', 'h2_x7'), ('neg0', 'neg0_x7'), ('neg1', 'neg1_x7')])
def test_x0_enters_the_first_residual(lib_built, a, b):
    """a start-up r = b - A 0 in place of b - A x7 cannot pass the 1e-6
    contract: the first residual alone differs by >= 1e-2 relative"""
    r0, r7 = pe.reference(a)[3][0], pe.reference(b)[3][0]
    assert abs(r7 / r0 - 1.0) >= 1e-2


def test_stop_type_1_breaks_in_the_same_iteration(lib_built):
    """neg2 under stop type 1: the rule does not enter the recurrences"""
    assert pe.reference('neg2_s1')[1] == pe.reference('neg2')[1]
    assert np.array_equal(pe.reference('neg2_s1')[3], pe.reference('neg2')[3])
    assert len(pe.reference_norms('neg2_s1')) == 3
