"""The identity behind the matrix-free level-0 prolongation (DESIGN.md section
4.9), without a GPU: the oracle's cycle with level 0's stored P replaced by
e -> T e - w D_B^-1 (A (T e)) (tests/post_mf_ref.py) against the oracle's
cycle, on the grids of tests/test_gpu_post_mf.py.

The two differ by rounding only: the stored P sums A's entries per aggregate
before it multiplies e, the matrix-free form multiplies first, and on the
small mass-dominated grids T e - w D_B^-1 A T e cancels.  Measured: at most
2.4e-13 (3-D n = 6), 7.4e-14 (n = 10), 4.2e-14 (2-D n = 32), 4.3e-15 (2-D
n = 128).  The bound is a
tenth of the suite's APPLY_TOL, so that a GPU handle on the matrix-free path
keeps its 1e-10 against the stored-P oracle.
"""
import dataclasses
import functools

import numpy as np
import pytest

import mamg_oracle as mo
import post_mf_ref as pm
import rowdict_cases as rc
from test_gpu import APPLY_TOL, rel

GRIDS = {'grid3d-6': (3, 6), 'grid3d-10': (3, 10), 'grid2d-32': (2, 32), 'grid2d-128': (2, 128)}
FAMILIES = {
    'default': dict(),
    'poly': dict(smoother='POLY'),
    'sweeps2-maxit2': dict(presmooth_iter=2, postsmooth_iter=2, maxit=2),
    'wcycle': dict(cycle_type='W'),
}


@functools.lru_cache(maxsize=None)
def oracle(name, smoother):
    A, nv, idofs = rc.grid(*GRIDS[name])
    return mo.setup(A, mo.Params(num_functions=2, smoother=smoother), idofs=idofs)


@pytest.mark.parametrize('family', list(FAMILIES))
@pytest.mark.parametrize('name', list(GRIDS))
def test_matrix_free_prolongation_is_the_stored_one(name, family):
    kw = dict(FAMILIES[family])
    h = oracle(name, kw.pop('smoother', 'JACOBI_RHO'))
    h = mo.Hierarchy(h.levels, dataclasses.replace(h.params, **kw))
    lev = h.levels[0]
    assert lev.agg is not None and len(lev.agg) == lev.A.shape[0] // 2 and lev.w_sa > 0.0
    hm = pm.matrix_free(h)
    # P itself, column by column of a random e
    e = mo.seeded_rhs(lev.P.shape[1], 5)
    assert rel(hm.levels[0].P @ e, lev.P @ e) < APPLY_TOL / 10
    for seed in (1234, 7):
        r = mo.seeded_rhs(lev.A.shape[0], seed)
        d = rel(hm.apply(r), h.apply(r))
        print('%s %s seed %d: matrix-free vs stored P %.2e' % (name, family, seed, d))
        assert d < APPLY_TOL / 10, d


def test_isolated_nodes_prolongate_zero():
    """An isolated node (agg = -1: the Dirichlet nodes of these grids) has a
    zero row of T; P's row is then -w D_B^-1 (A T) there, not zero."""
    h = oracle('grid3d-6', 'JACOBI_RHO')
    lev = h.levels[0]
    assert int(np.sum(lev.agg < 0)) == 98
    P = pm.MatrixFreeP(lev)
    e = mo.seeded_rhs(lev.P.shape[1], 3)
    y = P.T @ e
    nv = len(lev.agg)
    assert np.all(y[:nv][lev.agg < 0] == 0.0) and np.all(y[nv:][lev.agg < 0] == 0.0)
    assert np.array_equal(y[:nv][lev.agg >= 0], e[lev.agg[lev.agg >= 0]])
