"""bzh_batch_sqrt, bzh_affine_decompress and the verifier's point selection without a device: the header declares them,
libbzh2.so exports them, bad arguments are refused before anything is written, and the host path (ctx == NULL, BZH_MEM_HOST)
returns, element for element, the values Python integers give (tests/helpers/sqrt_cases.py: the root pasta_curves 0.4.1
returns).  The kernels are tests/test_gpu_sqrt_decompress.py (-m gpu)."""
import ctypes
import os
import re

import numpy as np
import pytest

from helpers import sqrt_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("bzh_batch_sqrt", "bzh_affine_decompress", "bzh_pk_verify_select", "bzh_pk_verify_selected")
VP, U8P = ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint8)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    import bzh2
    if not os.path.exists(bzh2.lib_path()):
        g.build()
    L = bzh2.load()
    L.bzh_batch_sqrt.argtypes = [VP, ctypes.c_int, VP, ctypes.c_size_t, ctypes.c_int, ctypes.c_int, U8P]
    L.bzh_affine_decompress.argtypes = [VP, ctypes.c_int, VP, ctypes.c_size_t, ctypes.c_int, ctypes.c_int, VP, U8P]
    return L


def test_header_declares_and_library_exports_the_new_functions(lib):
    import bzh2
    hdr = open(os.path.join(ROOT, "include", "bzh2.h")).read()
    declared = set(re.findall(r"\b(bzh_[a-z0-9_]+)\s*\(", hdr))
    for name in NEW:
        assert name in declared, name
        assert name in bzh2.EXPORTS, name
        assert hasattr(lib, name), name
    assert re.search(r"BZH_VERIFY_POINTS_HOST\s*=\s*0\b", hdr) and re.search(r"BZH_VERIFY_POINTS_DEVICE\s*=\s*1\b", hdr)
    for name, v in (("BZH_POINT_OK", 0), ("BZH_POINT_IDENTITY", 1), ("BZH_POINT_INVALID", 2)):
        assert re.search(r"%s\s*=\s*%d\b" % (name, v), hdr), name
    from bzh2 import native as N
    assert (N.VERIFY_POINTS_HOST, N.VERIFY_POINTS_DEVICE) == (0, 1)
    assert (bzh2.POINT_OK, bzh2.POINT_IDENTITY, bzh2.POINT_INVALID) == (0, 1, 2)


def test_verify_select_refuses_a_null_key(lib):
    import bzh2
    lib.bzh_pk_verify_select.argtypes = [VP, ctypes.c_int]
    lib.bzh_pk_verify_selected.argtypes = [VP, ctypes.POINTER(ctypes.c_int)]
    assert lib.bzh_pk_verify_select(None, 0) == bzh2.E_ARG
    assert lib.bzh_pk_verify_select(None, 1) == bzh2.E_ARG
    w = ctypes.c_int(5)
    assert lib.bzh_pk_verify_selected(None, ctypes.byref(w)) == bzh2.E_ARG
    assert w.value == 5


def test_bad_arguments_are_refused_and_nothing_is_written(lib):
    import bzh2
    a = np.full((3, 4), 4, dtype=np.uint64)
    st = np.full(3, 7, dtype=np.uint8)
    stp = st.ctypes.data_as(U8P)
    keep = a.copy()
    H, D, CAN = bzh2.MEM_HOST, bzh2.MEM_DEVICE, bzh2.FORM_CANONICAL
    assert lib.bzh_batch_sqrt(None, 0, VP(a.ctypes.data), 3, CAN, D, stp) == bzh2.E_ARG        # no ctx, device memory
    assert lib.bzh_batch_sqrt(None, 4, VP(a.ctypes.data), 3, CAN, H, stp) == bzh2.E_ARG        # field
    assert lib.bzh_batch_sqrt(None, -1, VP(a.ctypes.data), 3, CAN, H, stp) == bzh2.E_ARG
    assert lib.bzh_batch_sqrt(None, 0, VP(a.ctypes.data), 3, 2, H, stp) == bzh2.E_ARG          # form
    assert lib.bzh_batch_sqrt(None, 0, VP(a.ctypes.data), 3, CAN, 2, stp) == bzh2.E_ARG        # mem
    assert lib.bzh_batch_sqrt(None, 0, None, 3, CAN, H, stp) == bzh2.E_ARG                     # NULL buffer, n > 0
    assert lib.bzh_batch_sqrt(None, 0, None, 0, CAN, H, None) == bzh2.OK                       # n = 0
    raw = np.zeros(3 * 32, dtype=np.uint8)
    raw[0] = 9
    xy = np.full((3, 8), 5, dtype=np.uint64)
    args = (VP(raw.ctypes.data), 3)
    assert lib.bzh_affine_decompress(None, 0, *args, CAN, D, VP(xy.ctypes.data), stp) == bzh2.E_ARG
    assert lib.bzh_affine_decompress(None, 3, *args, CAN, H, VP(xy.ctypes.data), stp) == bzh2.E_ARG
    assert lib.bzh_affine_decompress(None, 0, *args, 2, H, VP(xy.ctypes.data), stp) == bzh2.E_ARG
    assert lib.bzh_affine_decompress(None, 0, *args, CAN, 2, VP(xy.ctypes.data), stp) == bzh2.E_ARG
    assert lib.bzh_affine_decompress(None, 0, None, 3, CAN, H, VP(xy.ctypes.data), stp) == bzh2.E_ARG
    assert lib.bzh_affine_decompress(None, 0, *args, CAN, H, None, stp) == bzh2.E_ARG
    assert lib.bzh_affine_decompress(None, 0, None, 0, CAN, H, None, None) == bzh2.OK
    assert (a == keep).all() and (st == 7).all() and (xy == 5).all()


@pytest.mark.parametrize("form", [0, 1])
@pytest.mark.parametrize("fid", [0, 1, 2, 3])
def test_host_batch_sqrt_returns_the_pasta_root(lib, fid, form):
    import bzh2
    p = K.FIELDS[fid].p
    cases = K.sqrt_cases(fid)
    a = np.frombuffer(K.limbs_bytes(K.to_form(u, p, form) for u, _ in cases), dtype=np.uint64).reshape(-1, 4)
    got, st = bzh2.batch_sqrt(fid, a, form)
    want_st = [0 if r is None else 1 for _, r in cases]
    want = [K.to_form(u if r is None else r, p, form) for u, r in cases]      # a non-square is left as it was
    assert st.tolist() == want_st
    assert got.tobytes() == K.limbs_bytes(want)
    # status == NULL: BZH_E_RANGE as soon as one element is not a square, and the squares' roots are still written
    b = a.copy()
    assert lib.bzh_batch_sqrt(None, fid, VP(b.ctypes.data), b.shape[0], form, bzh2.MEM_HOST, None) == bzh2.E_RANGE
    assert b.tobytes() == K.limbs_bytes(want)
    sq = np.ascontiguousarray(a[np.array(want_st, dtype=bool)])
    assert lib.bzh_batch_sqrt(None, fid, VP(sq.ctypes.data), sq.shape[0], form, bzh2.MEM_HOST, None) == bzh2.OK


@pytest.mark.parametrize("form", [0, 1])
@pytest.mark.parametrize("cid", [0, 1, 2])
def test_host_affine_decompress_matches_from_bytes(lib, cid, form):
    import bzh2
    p = K.curve_of(cid).base.p
    strings, pts, mixed, want = K.decompress_cases(cid)
    # round trip: bzh_affine_compress of the points gives the strings, which decompress to the same points
    xy = np.frombuffer(K.limbs_bytes(K.to_form(c, p, form) for pt in pts for c in pt), dtype=np.uint64).reshape(-1, 8)
    assert bzh2.affine_compress(cid, xy, form) == strings
    back, st = bzh2.affine_decompress(cid, strings, form)
    assert (st == bzh2.POINT_OK).all() and back.tobytes() == xy.tobytes()
    assert bzh2.affine_decompress(cid, strings, form, check=True)[0].tobytes() == xy.tobytes()
    got, st = bzh2.affine_decompress(cid, mixed, form)
    assert st.tolist() == [w[0] for w in want]
    assert {0, 1, 2} == set(st.tolist())
    want_xy = K.limbs_bytes(K.to_form(c, p, form) for w in want for c in w[1:])
    assert got.tobytes() == want_xy
    # status == NULL: BZH_E_RANGE, and the valid outputs are still correct
    raw = np.frombuffer(b"".join(mixed), dtype=np.uint8).copy()
    out = np.full((len(mixed), 8), 3, dtype=np.uint64)
    rc = lib.bzh_affine_decompress(None, cid, VP(raw.ctypes.data), len(mixed), form, bzh2.MEM_HOST, VP(out.ctypes.data), None)
    assert rc == bzh2.E_RANGE and out.tobytes() == want_xy
