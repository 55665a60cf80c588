"""The inputs of tests/test_gpu_rowdict.py, pinned on the CPU with the oracle's
generator: how many distinct node rows (sequence of (column - row, 2x2 block
bitwise)) each holds and how long its longest row is.  The row-pattern
dictionary of a level-0 A is taken or refused on these
counts, so a generator change fails here and not silently on the GPU."""
import numpy as np
import pytest

import rowdict_cases as rc


@pytest.mark.parametrize('dim,n,nv,types,maxlen', [(3, 6, 343, 28, 15), (3, 10, 1331, 28, 15),
                                                   (2, 32, 1089, 10, 7)])
def test_grid_row_types(dim, n, nv, types, maxlen):
    A, nv_, _ = rc.grid(dim, n)
    code, nt, ml = rc.node_rows(A, nv_)
    assert (nv_, nt, ml) == (nv, types, maxlen)
    assert nt <= rc.MAX_TYPES and ml <= rc.MAX_LEN
    # types are numbered by first occurrence: row 0 holds type 0
    assert code[0] == 0 and code.max() == nt - 1


def test_type_count_does_not_depend_on_n():
    A, nv, _ = rc.grid(3, 16)
    assert rc.node_rows(A, nv)[1:] == (28, 15)


@pytest.mark.parametrize('mirror,types', [(True, 30), (False, 29)])
def test_perturbed_row_types(mirror, types):
    """One interior block scaled by 1 + 2^-40 (and its mirror): the two (one)
    rows that hold it become types of their own."""
    A, nv, _ = rc.perturbed(6, mirror)
    assert rc.node_rows(A, nv)[1:] == (types, 15)
    B = rc.grid(3, 6)[0]
    assert (A != B).nnz == (8 if mirror else 4)
    assert ((A != A.T).nnz == 0) == mirror


@pytest.mark.parametrize('name,nv,types,maxlen', [('permuted2d-32', 1089, 1024, 7), ('ragged96', 9409, 9204, 27),
                                                  ('hub32-m500', 1089, 510, 505)])
def test_refused_inputs_exceed_the_caps(name, nv, types, maxlen):
    A, nv_, _ = rc.REFUSED[name]()
    _, nt, ml = rc.node_rows(A, nv_)
    assert (nv_, nt, ml) == (nv, types, maxlen)
    assert nt > rc.MAX_TYPES or ml > rc.MAX_LEN
