"""fp32 cycle storage on rank handles: what needs no device.

The GPU tests (test_gpu_dist_cycle_storage.py) lean on two facts checked
here on the CPU: rounding is element-wise, so rounding a rank's rows of an
operator is taking the rank's rows of the rounded operator (K included: it is
formed in fp64 first), and the rounded restatement is far enough from the
fp64 oracle apply (more than 1e-8) for a rank that silently stayed fp64 to be
seen."""
import numpy as np
import pytest
import scipy.sparse as sp

import mamg_oracle as mo
from cycle_storage_ref import ALL, StorageRef, round32


def _M():
    import metric_amg_examples_amd as M
    return M


def test_entries_declared():
    M = _M()
    for name in ('mamg_dist_set_cycle_storage', 'mamg_dist_level_storage', 'mamg_dist_num_levels',
                 'mamg_dist_level_format'):
        assert name in M._lib.SIGNATURES
    for name in ('set_cycle_storage', 'level_storage', 'level_format', 'num_levels'):
        assert hasattr(M.DistMetricAMG, name)


def test_bad_storage_value_before_the_library():
    M = _M()
    h = object.__new__(M.DistMetricAMG)          # no handle, no library: the value is checked first
    for bad in ('f16', 2, True, None):
        with pytest.raises(ValueError, match="'f64' or 'f32'"):
            h.set_cycle_storage(bad)
    h._h = None


def test_rows_of_rounded_are_rounded_rows_and_rounding_shows():
    M = _M()
    s = M.problems.bidomain(2, 32, 1e6)
    h = mo.setup(s.scipy(), mo.Params(num_functions=2), idofs=s.idofs)
    ref = StorageRef(h, masks=ALL, kform=True)
    for G, name in ((ref.A[0], 'A'), (ref.K[0], 'K'), (ref.R[0], 'R')):
        full = {'A': h.levels[0].A, 'R': h.levels[0].R}.get(name)
        if full is None:
            full = StorageRef(h, masks=0, kform=True).K[0]
        n = full.shape[0]
        for P in (3, 8):
            for q in range(P):
                rows = slice(n * q // P, n * (q + 1) // P)
                a, b = round32(sp.csr_matrix(full)[rows]), sp.csr_matrix(G)[rows]
                assert (a != b).nnz == 0, (name, P, q)
    r = mo.seeded_rhs(s.N)
    z32, z64 = ref.apply(r), h.apply(r)
    d = np.linalg.norm(z32 - z64) / np.linalg.norm(z64)
    print('2-D n = 32: rounded restatement vs fp64 oracle apply %.2e' % d)
    assert d > 1e-8
