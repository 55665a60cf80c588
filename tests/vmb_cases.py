"""The systems of the VMB tests (tests/test_vmb_ref.py on the CPU,
tests/test_gpu_vmb.py on the GPU): name -> (A, idofs, parameter overrides).
Built once per process."""
import functools

import numpy as np
import scipy.sparse as sp

import mamg_oracle as mo

VMB = 1     # aggregation_type (include/mamg.h MAMG_VMB)
UA = 1      # AMG_type


def _scalar_chain_plus(n):
    """An SPD scalar system of n rows that is no grid in grid order: the 1-D
    Laplacian plus a weaker coupling i ~ i + 7 (every row keeps strong
    neighbours on both sides, so lists and blocks end mid-wavefront)."""
    i = np.arange(n - 7)
    E = sp.csr_matrix((np.full(n - 7, -0.5), (i, i + 7)), shape=(n, n))
    A = (mo.laplace1d(n) + 0.5 * sp.identity(n) - E - E.T).tocsr()
    A = A + sp.diags(np.asarray(abs(E + E.T).sum(axis=1)).ravel())
    A = sp.csr_matrix(A)
    A.sort_indices()
    return A


@functools.lru_cache(maxsize=None)
def system(name):
    """(A, idofs, kw): kw are HostHierarchy / make_params overrides."""
    import metric_amg_examples_amd as M
    if name == '3d16_nodal_ua':
        s = M.problems.bidomain(3, 16, 1e6)
        return s.scipy(), s.idofs, dict(num_functions=2, aggregation_type=VMB, AMG_type=UA, strong_coupled=0.1)
    if name == '2d64_nodal_sa':
        s = M.problems.bidomain(2, 64, 1e4)
        return s.scipy(), s.idofs, dict(num_functions=2, aggregation_type=VMB)
    if name == '3d16_scalar_ua':          # the hazmath preset's shape
        s = M.problems.bidomain(3, 16, 1.0)
        return s.scipy(), None, dict(num_functions=1, aggregation_type=VMB, AMG_type=UA, strong_coupled=0.1)
    if name == '2d32_strength_diag':
        s = M.problems.bidomain(2, 32, 1e3)
        return s.scipy(), s.idofs, dict(num_functions=2, aggregation_type=VMB, strength_measure=0)
    if name == 'emi_3d1d':                # the 3D-1D .dat file's values (tests/golden/solver_3d1d.dat)
        s = M.problems.emi_3d1d(8, 1e6, 1.0)
        return s.scipy(), s.idofs, dict(aggregation_type=VMB, coarse_dof=300, max_levels=30, Schwarz_mmsize=200,
                                        Schwarz_type=5, Schwarz_maxlvl=2)
    if name == 'laplace1d_3000':          # one chain in index order: about 1000 rounds
        return mo.laplace1d(3000), None, dict(num_functions=1, aggregation_type=VMB, coarse_dof=40, max_levels=2)
    if name == 'permuted_2d24':           # random order: few rounds
        import irregular
        A, nv, idofs = irregular.permuted(2, 24)
        return A, idofs, dict(num_functions=2, aggregation_type=VMB)
    if name.startswith('rows_'):          # list and block boundaries
        n = int(name[5:])
        return _scalar_chain_plus(n), None, dict(num_functions=1, aggregation_type=VMB, coarse_dof=10, max_levels=3)
    raise KeyError(name)


def unassignable():
    """laplace1d(30) with a stored 0.0 at (29, 28), its mirror (28, 29) kept:
    the chain's roots are 0, 3, ..., 27, node 29 is left to phase 2, and its
    only strong entry weighs nothing."""
    A = mo.laplace1d(30).tocsr().astype(np.float64)
    A.sort_indices()
    k = A.indptr[29] + int(np.flatnonzero(A.indices[A.indptr[29]:A.indptr[30]] == 28)[0])
    A.data[k] = 0.0
    return A


NAMES = ['3d16_nodal_ua', '2d64_nodal_sa', '3d16_scalar_ua', '2d32_strength_diag', 'emi_3d1d', 'laplace1d_3000',
         'permuted_2d24'] + ['rows_%d' % n for n in (63, 64, 65, 255, 256, 257)]


def level_systems(H):
    """Per aggregated level of a hierarchy H: (l, A_l as scipy CSR, agg)."""
    out = []
    A0 = H._A
    for l in range(H.num_levels):
        lv = H.level(l, with_A=(l > 0))
        if 'agg' not in lv:
            break
        if l == 0:
            n = lv['n']
            A = sp.csr_matrix((A0[2], A0[1], A0[0]), shape=(n, n))
        else:
            ip, ix, dv, shp = lv['A']
            A = sp.csr_matrix((dv, ix, ip), shape=shp)
        out.append((l, A, lv['agg']))
    return out
