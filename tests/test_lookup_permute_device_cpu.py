"""The device lookup permutation's C ABI without a device: include/bzh2.h declares bzh_permute_expression_pair_batch,
bzh_pk_lookup_select and bzh_pk_lookup_selected, libbzh2.so exports them, and each refuses a NULL handle with BZH_E_ARG
before touching anything.  The kernels themselves are tests/test_gpu_lookup_permute.py (-m gpu)."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("bzh_permute_expression_pair_batch", "bzh_pk_lookup_select", "bzh_pk_lookup_selected")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    import bzh2
    if not os.path.exists(bzh2.lib_path()):
        g.build()
    return bzh2.load()


def test_header_declares_and_library_exports_the_new_functions(lib):
    import bzh2
    hdr = open(os.path.join(ROOT, "include", "bzh2.h")).read()
    declared = set(re.findall(r"\b(bzh_[a-z0-9_]+)\s*\(", hdr))
    for name in NEW:
        assert name in declared, name
        assert name in bzh2.EXPORTS, name
        assert hasattr(lib, name), name
    assert re.search(r"BZH_LOOKUP_HOST\s*=\s*0\b", hdr) and re.search(r"BZH_LOOKUP_DEVICE\s*=\s*1\b", hdr)


def test_batch_permute_refuses_a_null_ctx(lib):
    import bzh2
    vp = ctypes.c_void_p
    lib.bzh_permute_expression_pair_batch.argtypes = [vp, ctypes.c_int, vp, vp, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_int,
                                                      ctypes.c_int, vp, vp, ctypes.POINTER(ctypes.c_int32)]
    lib.bzh_permute_expression_pair_batch.restype = ctypes.c_int
    a = np.zeros((1, 8, 4), dtype=np.uint64)
    oa, ot = np.zeros_like(a), np.zeros_like(a)
    st = (ctypes.c_int32 * 1)(7)
    rc = lib.bzh_permute_expression_pair_batch(None, bzh2.FIELD_FP, a.ctypes.data, a.ctypes.data, 8, 8, 1, bzh2.FORM_CANONICAL, bzh2.MEM_HOST,
                                               oa.ctypes.data, ot.ctypes.data, st)
    assert rc == bzh2.E_ARG
    assert st[0] == 7 and not oa.any() and not ot.any()      # nothing was written


def test_lookup_select_refuses_a_null_key(lib):
    import bzh2
    lib.bzh_pk_lookup_select.argtypes = [ctypes.c_void_p, ctypes.c_int]
    lib.bzh_pk_lookup_select.restype = ctypes.c_int
    lib.bzh_pk_lookup_selected.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int)]
    lib.bzh_pk_lookup_selected.restype = ctypes.c_int
    assert lib.bzh_pk_lookup_select(None, 0) == bzh2.E_ARG
    assert lib.bzh_pk_lookup_select(None, 1) == bzh2.E_ARG
    w = ctypes.c_int(5)
    assert lib.bzh_pk_lookup_selected(None, ctypes.byref(w)) == bzh2.E_ARG
    assert w.value == 5
