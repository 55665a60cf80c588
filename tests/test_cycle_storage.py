"""fp32 cycle storage without a GPU: the numpy restatement (cycle_storage_ref.py)
pinned against the oracle, the PCG iteration counts under full rounding, and
the parts of the C ABI that need no device.

Bounds: the all-zero-mask restatement is the oracle's cycle with the post side
regrouped (K e + T r1 instead of T (b - A (x1 + P e))); both are fp64 sums of
the same terms, so 1e-12 relative separates a restatement error from rounding
(the oracle's own sensitivity to summation order is at most 6.1e-14 on these
hierarchies, tests/test_gpu_irregular.py).  The iteration counts 38 / 26 / 39
are the fp64 oracle's, asserted first, then required of the rounded cycle.
"""
import ctypes as C
import dataclasses
import functools

import numpy as np
import pytest

import mamg_oracle as mo
from cycle_storage_ref import ALL, StorageRef

ERR_ARG = -1


def rel(a, b):
    return np.linalg.norm(a - b) / np.linalg.norm(b)


@functools.lru_cache(maxsize=None)
def system(dim, n, gamma):
    return mo.bidomain_system(dim, n, gamma)


@functools.lru_cache(maxsize=None)
def hierarchy(dim, n, gamma, smoother):
    o = system(dim, n, gamma)
    kw = dict(poly_degree=2) if smoother == 'POLY' else {}
    return mo.setup(o['A'], mo.Params(num_functions=2, smoother=smoother, **kw), idofs=o['idofs'])


def with_params(h, **kw):
    """The same levels under other apply-time parameters (the setup reads none of them)."""
    return mo.Hierarchy(h.levels, dataclasses.replace(h.params, **kw))


@pytest.mark.parametrize('kform', [True, False])
@pytest.mark.parametrize('extra', [dict(), dict(presmooth_iter=2, postsmooth_iter=2), dict(coarse_scaling=1)],
                         ids=['nu1', 'nu2', 'scaling'])
@pytest.mark.parametrize('cycle', ['V', 'W'])
@pytest.mark.parametrize('smoother', ['JACOBI_RHO', 'POLY'])
@pytest.mark.parametrize('dim,n', [(3, 8), (2, 32)])
def test_zero_mask_restatement_is_the_oracle(dim, n, smoother, cycle, extra, kform):
    h = with_params(hierarchy(dim, n, 1e6, smoother), cycle_type=cycle, **extra)
    ref = StorageRef(h, masks=0, kform=kform)
    for seed in (1234, 7):
        r = mo.seeded_rhs(h.levels[0].A.shape[0], seed)
        e = rel(ref.apply(r), h.apply(r))
        print(dim, n, smoother, cycle, extra, kform, seed, 'restatement vs oracle %.2e' % e)
        assert e < 1e-12, e


def test_rounding_changes_the_apply():
    """The all-ones mask is not a no-op: the rounded cycle differs from the
    fp64 one by far more than the GPU tests' 1e-10, and by no more than
    a few fp32 ulps amplified by the cycle (1e-4 is three orders above the
    8.4e-7 measured for this input)."""
    h = hierarchy(3, 8, 1e6, 'JACOBI_RHO')
    r = mo.seeded_rhs(h.levels[0].A.shape[0])
    d = rel(StorageRef(h, masks=ALL).apply(r), h.apply(r))
    print('rounded vs fp64 apply %.2e' % d)
    assert 1e-10 < d < 1e-4, d


@pytest.mark.parametrize('dim,n,gamma,iters', [(3, 16, 1e6, 38), (3, 16, 1.0, 26), (2, 64, 1e6, 39)])
def test_rounded_cycle_keeps_the_iteration_count(dim, n, gamma, iters):
    o = system(dim, n, gamma)
    h = hierarchy(dim, n, gamma, 'JACOBI_RHO')
    b = mo.seeded_rhs(o['A'].shape[0])
    r64 = mo.pcg(o['A'], h, b, 1e-8, 500)
    r32 = mo.pcg(o['A'], StorageRef(h, masks=ALL), b, 1e-8, 500)   # the fp64 A as the Krylov operator
    dx = rel(r32.x, r64.x)
    print(dim, n, gamma, 'iters fp64 %d rounded %d, solution diff %.2e' % (r64.niters, r32.niters, dx))
    assert r64.niters == iters
    assert r32.niters == iters
    assert dx < 1e-9, dx


def _lib():
    import metric_amg_examples_amd as M
    return M, M._lib.lib()


def test_abi_symbols_and_version(lib_built):
    M, L = _lib()
    assert L.mamg_abi_version() == 4
    for name in ('mamg_set_cycle_storage', 'mamg_level_storage'):
        assert name in M._lib.SIGNATURES and hasattr(L, name)


def test_refusals_without_a_gpu(lib_built):
    """A NULL handle and a storage value other than 0 / 1 are MAMG_ERR_ARG
    before the handle is read: the second call passes 64 zero bytes as the
    handle, which nothing may dereference."""
    M, L = _lib()
    assert L.mamg_set_cycle_storage(None, 1) == ERR_ARG
    assert L.mamg_set_cycle_storage(None, 0) == ERR_ARG
    fake = C.create_string_buffer(64)
    for bad in (2, -1, 7):
        assert L.mamg_set_cycle_storage(C.cast(fake, C.c_void_p), bad) == ERR_ARG
        assert b'MAMG_STORE' in L.mamg_last_error()
    assert L.mamg_level_storage(None, 0) == ERR_ARG


def test_python_keyword_validation():
    M, _ = _lib()
    from metric_amg_examples_amd import amg
    assert amg._storage_code('f32') == 1 and amg._storage_code('f64') == 0
    for bad in ('fp32', 2, None, True):
        with pytest.raises(ValueError):
            amg._storage_code(bad)
    o = system(2, 32, 1e6)
    with pytest.raises(ValueError, match='single-GPU'):
        M.DistMetricAMG(o['A'], [o['nv'], o['nv']], num_functions=2, cycle_storage='f32')
