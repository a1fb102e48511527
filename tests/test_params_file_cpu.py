"""The byte format of halo2_proofs 0.2.0's Params::write / Params::read (csrc/params_file.hpp) through the two host-only entry
points, bzh_params_file_info and bzh_params_encode: no ctx, no device.  The expected bytes are built here from oracle/pasta.py's
compression in the order the format states -- k as a u32 little-endian, g, g_lagrange, w, u -- with g_lagrange from its
definition, g_lagrange[i] = sum_j intt(e_i)_j g[j], in the oracle's curve arithmetic."""
import ctypes
import struct

import numpy as np
import pytest

import coracle as C
import pasta as O

E_ARG = -1


def _lib():
    from bzh2 import params as Pm
    return Pm._bind()


def _info(data: bytes, length=None):
    k, n = ctypes.c_uint(77), ctypes.c_size_t(77)
    rc = _lib().bzh_params_file_info(data, len(data) if length is None else length, ctypes.byref(k), ctypes.byref(n))
    return rc, k.value, n.value


def _file_len(k):
    return 4 + 32 * (2 * (1 << k) + 2)


def _blank(k, length=None):
    return struct.pack("<I", k) + bytes((_file_len(k) if length is None else length) - 4)


@pytest.mark.parametrize("k", [0, 1, 4])
def test_file_info_accepts_exactly_the_right_length(k):
    assert _info(_blank(k)) == (0, k, 1 << k)
    for off in (-1, 1):
        rc, kk, nn = _info(_blank(k, _file_len(k) + off))
        assert rc == E_ARG and (kk, nn) == (77, 77), off      # refused, outputs untouched


def test_file_info_refusals():
    assert _info(_blank(1), 3)[0] == E_ARG                                # shorter than the header
    assert _info(b"\x01\x00\x00")[0] == E_ARG
    assert _info(struct.pack("<I", 25) + bytes(64))[0] == E_ARG          # a k the library's Params do not take
    assert _info(struct.pack("<I", 0xFFFFFFFF) + bytes(64))[0] == E_ARG
    assert _info(_blank(4, _file_len(5)))[0] == E_ARG                    # a length that is another k's
    assert _info(_blank(5, _file_len(4)))[0] == E_ARG
    assert _lib().bzh_params_file_info(None, 100, None, None) == E_ARG
    assert _lib().bzh_params_file_info(_blank(4), _file_len(4), None, None) == 0   # the outputs are optional


def _srs(k):
    """(g, g_lagrange, w, u) of Params::new(k): arrays of canonical limbs; g_lagrange from the oracle"""
    from bzh2 import params as Pm
    cv, F = O.VESTA, O.FP
    n = 1 << k
    g_arr, w, u = Pm.generators(k)
    g = [C.array_to_point(g_arr[i]) for i in range(n)]
    gl = []
    for i in range(n):
        e = [0] * n
        e[i] = 1
        acc = None
        for c, pt in zip(O.intt(e, F.omega(k), F), g):
            acc = cv.add(acc, cv.mul(c, pt))
        gl.append(acc)
    return g, gl, w, u


def _model_bytes(k, g, gl, w, u):
    cv = O.VESTA
    return struct.pack("<I", k) + b"".join(cv.compress(p) for p in g) + b"".join(cv.compress(p) for p in gl) + cv.compress(w) + cv.compress(u)


@pytest.fixture(scope="module")
def srs():
    return {k: _srs(k) for k in (1, 2, 3)}


@pytest.mark.parametrize("k", [1, 2, 3])
def test_encode_equals_the_model(srs, k):
    from bzh2 import params as Pm
    g, gl, w, u = srs[k]
    want = _model_bytes(k, g, gl, w, u)
    assert len(want) == _file_len(k)
    got = Pm.encode(k, C.points_to_array(g), C.points_to_array(gl), C.points_to_array([w])[0], C.points_to_array([u])[0])
    assert got == want
    assert Pm.file_info(got) == (k, 1 << k)
    # the four sections are told apart: no two of them hold the same strings
    n = 1 << k
    assert got[4:4 + 32 * n] != got[4 + 32 * n:4 + 64 * n] and got[-64:-32] != got[-32:]


def test_encode_buffer_handling(srs):
    k = 2
    g, gl, w, u = srs[k]
    arrs = [C.points_to_array(g), C.points_to_array(gl), C.points_to_array([w])[0], C.points_to_array([u])[0]]
    ptrs = [ctypes.c_void_p(a.ctypes.data) for a in arrs]
    L = _lib()
    size = ctypes.c_size_t(0)
    assert L.bzh_params_encode(k, None, None, None, None, None, 0, ctypes.byref(size)) == 0      # the size query reads no point
    assert size.value == _file_len(k)
    for cap in (0, 4, _file_len(k) - 1):
        out = np.full(_file_len(k) + 8, 0xA5, dtype=np.uint8)
        size = ctypes.c_size_t(0)
        assert L.bzh_params_encode(k, *ptrs, ctypes.c_void_p(out.ctypes.data), cap, ctypes.byref(size)) == E_ARG
        assert size.value == _file_len(k), cap
        assert (out == 0xA5).all(), cap                                                         # no byte written
    out = np.full(_file_len(k) + 8, 0xA5, dtype=np.uint8)
    assert L.bzh_params_encode(k, *ptrs, ctypes.c_void_p(out.ctypes.data), _file_len(k), ctypes.byref(size)) == 0
    assert out[:_file_len(k)].tobytes() == _model_bytes(k, g, gl, w, u) and (out[_file_len(k):] == 0xA5).all()
    assert L.bzh_params_encode(25, *ptrs, None, 0, ctypes.byref(size)) == E_ARG
    assert L.bzh_params_encode(k, *ptrs, None, 0, None) == E_ARG
    assert L.bzh_params_encode(k, ptrs[0], None, ptrs[2], ptrs[3], ctypes.c_void_p(out.ctypes.data), out.size, ctypes.byref(size)) == E_ARG
