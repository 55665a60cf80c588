"""The K-cycle's inner CG inside the coarse tail (mamg_set_kcycle_tail,
mamg_kcycle_tail, mamg_apply_launches) without a GPU: the symbols and their
prototypes, the argument checks that come before the handle is read, the
Python keyword and the drivers' -kcycle_tail.
"""
import ctypes as C
import os
import re

import pytest

ERR_ARG = -1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib():
    import metric_amg_examples_amd as M
    return M, M._lib.lib()


def test_symbols_prototypes_and_version(lib_built):
    M, L = _lib()
    assert L.mamg_abi_version() == 4                     # no struct changed
    VP = C.c_void_p
    want = {'mamg_set_kcycle_tail': (C.c_int, [VP, C.c_int]),
            'mamg_kcycle_tail': (C.c_int, [VP]),
            'mamg_apply_launches': (C.c_int, [VP, C.POINTER(C.c_int64)])}
    for name, sig in want.items():
        assert M._lib.SIGNATURES[name] == sig and hasattr(L, name)
    text = re.sub(r'\s+', ' ', open(os.path.join(ROOT, 'include', 'mamg.h')).read())
    for proto in ('int mamg_set_kcycle_tail(mamg_handle* h, int on);',
                  'int mamg_kcycle_tail(const mamg_handle* h);',
                  'int mamg_apply_launches(const mamg_handle* h, int64_t* launches);'):
        assert proto in text, proto


def test_argument_checks_without_a_gpu(lib_built):
    """A NULL handle and a value of on other than 0 / 1 are MAMG_ERR_ARG before
    the handle is read: the second loop passes 64 zero bytes as the handle,
    which nothing may dereference."""
    M, L = _lib()
    for on in (0, 1):
        assert L.mamg_set_kcycle_tail(None, on) == ERR_ARG
    assert L.mamg_kcycle_tail(None) == ERR_ARG
    n = C.c_int64(-7)
    assert L.mamg_apply_launches(None, C.byref(n)) == ERR_ARG and n.value == -7
    fake = C.create_string_buffer(64)
    for bad in (2, -1, 7):
        assert L.mamg_set_kcycle_tail(C.cast(fake, C.c_void_p), bad) == ERR_ARG
        assert b'0 or 1' in L.mamg_last_error()
    assert L.mamg_apply_launches(C.cast(fake, C.c_void_p), None) == ERR_ARG


def test_python_keyword_validation(lib_built):
    """a bad kcycle_tail is refused before the matrix is looked at (A = None
    would raise a TypeError, not a ValueError, one line later)"""
    M, _ = _lib()
    from metric_amg_examples_amd import amg
    assert amg._kcycle_tail_flag(True) is True and amg._kcycle_tail_flag(0) is False
    for bad in ('on', 2, None, 1.0, -1):
        with pytest.raises(ValueError, match='kcycle_tail'):
            amg._kcycle_tail_flag(bad)
        with pytest.raises(ValueError, match='kcycle_tail'):
            M.MetricAMG(None, kcycle_tail=bad)


def test_drivers_option(lib_built, tmp_path):
    from metric_amg_examples_amd import drivers as D
    for dim in (2, 3):
        ap = D.bidomain_parser(dim)
        assert ap.parse_known_args([])[0].kcycle_tail == 0                       # default unchanged
        assert ap.parse_known_args(['-kcycle_tail', '1'])[0].kcycle_tail == 1
        with pytest.raises(SystemExit):
            ap.parse_known_args(['-kcycle_tail', '2'])
    assert D._ktail_kw(0, 'diag') == {} and D._ktail_kw(0, 'metric_mono') == {}
    assert D._ktail_kw(1, 'metric_mono') == dict(kcycle_tail=True)
    assert D._ktail_kw(1, 'hazmath_HEM') == dict(kcycle_tail=True)
    for tag in ('diag', 'metric_hazmath'):
        with pytest.raises(ValueError, match='-kcycle_tail 1 needs an AMG preconditioner built by a factory'):
            D._ktail_kw(1, tag)
    # through the drivers: refused before anything is built
    for drv, dim in ((D.bidomain, 2), (D.emi, 2)):
        with pytest.raises(ValueError, match='-kcycle_tail'):
            drv(['-precond', 'diag', '-kcycle_tail', '1', '-results', str(tmp_path)], dim)
