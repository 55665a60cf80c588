"""Argument checks of the device-resident distributed PCG that need no GPU:
the C entries refuse before anything touches the device, and
DistConjGrad.for_handles(device=True) validates its arguments itself."""
import ctypes as C

import numpy as np
import pytest


def _buffers(maxiter):
    import metric_amg_examples_amd as M
    res, rn = np.zeros(maxiter + 1), np.zeros(maxiter + 1)
    al, be = np.zeros(max(maxiter, 1)), np.zeros(max(maxiter, 1))
    ptr = M._lib.ptr
    return (res, rn, al, be), (ptr(res, C.c_double), ptr(rn, C.c_double), ptr(al, C.c_double), ptr(be, C.c_double))


def test_null_handle_is_an_argument_error(lib_built):
    import metric_amg_examples_amd as M
    L = M._lib.lib()
    keep, ptrs = _buffers(5)
    it = C.c_int(-7)
    rc = L.mamg_dist_pcg_device(None, None, None, 1e-8, 5, 0, 0, *ptrs, C.byref(it), None)
    assert rc == M._lib.ERR_ARG
    assert L.mamg_last_error().decode() != ''
    assert it.value == -7 and all(not a.any() for a in keep)
    c = (C.c_int64 * 5)()
    assert L.mamg_dist_pcg_launches(None, 0, c) == M._lib.ERR_ARG
    assert L.mamg_dist_virtual_pcg(None, 0, None, None, 1e-8, 5, 0, 0, 0, *ptrs, C.byref(it), None) == M._lib.ERR_ARG
    hs = (C.c_void_p * 2)(None, None)
    bx = (C.c_void_p * 2)(None, None)
    rc = L.mamg_dist_virtual_pcg(hs, 2, bx, bx, 1e-8, 5, 0, 0, 0, *ptrs, C.byref(it), None)
    assert rc == M._lib.ERR_ARG and 'null handle' in L.mamg_last_error().decode()


def test_for_handles_device_validates(lib_built):
    import metric_amg_examples_amd as M
    with pytest.raises(ValueError):
        M.DistConjGrad.for_handles([], device=True)
    with pytest.raises(ValueError):
        M.DistConjGrad.for_handles([object()], device=True, stop_type=2)
    with pytest.raises(ValueError):
        M.DistConjGrad.for_handles(object(), device=True, stop_type='hazmath')
    # the default stays the host loop, which takes no x0
    cg = M.DistConjGrad(lambda xs, ys: None, lambda rs, zs: None)
    with pytest.raises(ValueError):
        cg.solve([], xs=[])
