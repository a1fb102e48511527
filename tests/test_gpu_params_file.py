"""Params files in halo2_proofs 0.2.0's byte format on the GPU box: bzh_params_write / bzh_params_read (csrc/params.hip) and the
verdict kernel k_pf_verdict (csrc/params_file.hip) behind Params.to_bytes / Params.from_bytes.

k = 1, 4, 7 as tests/test_gpu_params.py, and k = 8, where the 2 n + 2 = 514 strings span three 256-lane workgroups of the verdict
kernel.  The files under test are made by Params(ctx, k, cache_dir="").to_bytes() once per k and corrupted string by string; what
every check level must say about each corruption follows from the definition of the level (include/bzh2.h), not from a run."""
import ctypes
import random
import struct

import numpy as np
import pytest

import coracle as C
import pasta as O

pytestmark = pytest.mark.gpu

KS = [1, 4, 7, 8]
LEVELS = ["points", "lagrange", "full"]
DECODE, LAGRANGE, GENERATORS = 1, 2, 4
SEC_G, SEC_GL, SEC_W, SEC_U = 0, 1, 2, 3


class _Srs:
    """Params::new(k) on the session's ctx, its points and its file, made once per k"""

    def __init__(self, ctx, k):
        from bzh2 import params as Pm
        self.k, self.n = k, 1 << k
        self.params = Pm.Params(ctx, k, cache_dir="")
        self.g, self.gl, self.w, self.u, _ = self.params.points()
        self.data = self.params.to_bytes()


@pytest.fixture(scope="module")
def srs(gpu_ctx):
    made = {}

    def get(k):
        if k not in made:
            made[k] = _Srs(gpu_ctx, k)
        return made[k]

    yield get
    for s in made.values():
        s.params.close()


def _strings(data):
    """the 2 n + 2 strings of a file, in file order"""
    return [data[o:o + 32] for o in range(4, len(data), 32)]


def _join(k, strings):
    return struct.pack("<I", k) + b"".join(strings)


def _lane(n, section, index=0):
    return {SEC_G: 0, SEC_GL: n, SEC_W: 2 * n, SEC_U: 2 * n + 1}[section] + index


def _refused(ctx, data, level):
    """the ParamsFileError of a read that must be refused"""
    from bzh2 import params as Pm
    with pytest.raises(Pm.ParamsFileError) as ei:
        Pm.Params.from_bytes(ctx, data, check=level).close()
    return ei.value


def _accepted(ctx, data, level):
    from bzh2 import params as Pm
    Pm.Params.from_bytes(ctx, data, check=level).close()


def _affine(ctx, bases, scalars):
    import bzh2
    return bzh2.jacobian_to_affine(bzh2.CURVE_VESTA, ctx.msm(bases, scalars))


@pytest.mark.parametrize("k", KS)
def test_round_trip(gpu_ctx, oracle_c, srs, k):
    from bzh2 import params as Pm
    s = srs(k)
    n = s.n
    cv = O.VESTA
    model = struct.pack("<I", k) + b"".join(cv.compress(C.array_to_point(r)) for r in s.g) + b"".join(cv.compress(C.array_to_point(r)) for r in s.gl) \
        + cv.compress(s.w) + cv.compress(s.u)
    assert s.data == model
    assert Pm.file_info(s.data) == (k, n)
    p = Pm.Params.from_bytes(gpu_ctx, s.data, check="full")
    try:
        g, gl, w, u, from_cache = p.points()
        assert (g == s.g).all() and (gl == s.gl).all() and (w, u) == (s.w, s.u) and not from_cache
        assert p.to_bytes() == s.data
        L = Pm._bind()
        L.bzh_bases_len.restype = ctypes.c_size_t
        L.bzh_bases_len.argtypes = [ctypes.c_void_p]
        assert (p.k, p.n, L.bzh_bases_len(p.bases.handle), L.bzh_bases_len(p.bases_lagrange.handle)) == (k, n, n + 2, n + 3)
        rng = np.random.default_rng(100 + k)
        for mine, theirs, count in ((p.bases, s.params.bases, n + 2), (p.bases_lagrange, s.params.bases_lagrange, n + 3)):
            sc = np.frombuffer(rng.bytes(count * 32), dtype=np.uint64).reshape(count, 4).copy()
            sc[:, 3] &= (1 << 61) - 1
            a, b = _affine(gpu_ctx, mine, sc), _affine(gpu_ctx, theirs, sc)
            assert a.any() and (a == b).all()
    finally:
        p.close()


@pytest.mark.parametrize("k", KS)
def test_unmodified_file_passes_every_level(gpu_ctx, srs, k):
    for level in LEVELS:
        _accepted(gpu_ctx, srs(k).data, level)


@pytest.mark.parametrize("k", KS)
def test_lagrange_catches_a_wrong_g_lagrange(gpu_ctx, srs, k):
    s = srs(k)
    n = s.n
    good = _strings(s.data)
    for j in sorted({0, n // 2, n - 1}):
        at = _lane(n, SEC_GL, j)
        negated = list(good)
        negated[at] = good[at][:31] + bytes([good[at][31] ^ 0x80])     # -P: the same x, an x-only comparison would miss it
        replaced = list(good)
        replaced[at] = good[_lane(n, SEC_G, 0)]
        swapped = list(good)
        other = _lane(n, SEC_GL, (j + 1) % n)
        swapped[at], swapped[other] = good[other], good[at]
        for what, strings in (("negated", negated), ("replaced", replaced), ("swapped", swapped)):
            data = _join(k, strings)
            assert data != s.data
            _accepted(gpu_ctx, data, "points")                            # every string still is a point
            for level in ("lagrange", "full"):
                e = _refused(gpu_ctx, data, level)
                assert (e.bits, e.section) == (LAGRANGE, SEC_GL), (what, j, level)
                assert "g_lagrange" in str(e)


@pytest.mark.parametrize("k", KS)
def test_full_catches_a_consistent_but_wrong_srs(gpu_ctx, srs, k):
    from bzh2 import params as Pm
    s = srs(k)
    w, u = C.points_to_array([s.w])[0], C.points_to_array([s.u])[0]
    g = s.g.copy()
    g[[0, 1]] = g[[1, 0]]
    data = Pm.encode(k, g, Pm.group_ifft(gpu_ctx, g), w, u)
    _accepted(gpu_ctx, data, "points")
    _accepted(gpu_ctx, data, "lagrange")                                  # g_lagrange IS the transform of this g
    e = _refused(gpu_ctx, data, "full")
    assert (e.bits, e.section, e.first_bad, e.n_bad) == (GENERATORS, SEC_G, 0, 2)
    assert "g[0]" in str(e)
    data = Pm.encode(k, s.g, s.gl, u, w)                                  # w and u change places
    _accepted(gpu_ctx, data, "lagrange")
    e = _refused(gpu_ctx, data, "full")
    assert (e.bits, e.section, e.first_bad, e.n_bad) == (GENERATORS, SEC_W, 0, 2)


def _bad_strings():
    """three strings from_bytes must refuse here: x >= p, an x with no y on the curve, the identity's 32 zero bytes"""
    p = O.FQ.p                                                            # Vesta's base field
    x = 1
    while pow((x * x * x + 5) % p, (p - 1) // 2, p) == 1:                 # y^2 = x^3 + 5
        x += 1
    return {"x >= p": p.to_bytes(32, "little"), "no y": x.to_bytes(32, "little"), "identity": bytes(32)}


@pytest.mark.parametrize("k", KS)
def test_decode_catches_bad_encodings(gpu_ctx, srs, k):
    s = srs(k)
    n = s.n
    good = _strings(s.data)
    places = [(SEC_G, 0), (SEC_G, n - 1), (SEC_GL, 0), (SEC_GL, n - 1), (SEC_W, 0), (SEC_U, 0)]
    for name, bad in _bad_strings().items():
        for section, index in places:
            strings = list(good)
            strings[_lane(n, section, index)] = bad
            data = _join(k, strings)
            for level in LEVELS:
                e = _refused(gpu_ctx, data, level)
                assert (e.bits, e.section, e.first_bad, e.n_bad) == (DECODE, section, index, 1), (name, section, index, level)


def test_decode_counts_across_workgroups(gpu_ctx, srs):
    """k = 8: 514 lanes, three workgroups of the verdict kernel.  The lowest offender and the count come from different workgroups."""
    k = 8
    s = srs(k)
    n = s.n
    good = _strings(s.data)
    bad = _bad_strings()
    cases = [
        ([(SEC_U, 0, "no y"), (SEC_G, 5, "identity")], (SEC_G, 5, 2)),                            # lane 513 and lane 5
        ([(SEC_GL, n - 1, "x >= p"), (SEC_G, 200, "no y"), (SEC_GL, 3, "identity")], (SEC_G, 200, 3)),   # lanes 511, 200, 259
        ([(SEC_W, 0, "identity"), (SEC_GL, 0, "x >= p"), (SEC_GL, 1, "no y")], (SEC_GL, 0, 3)),          # lanes 512, 256, 257
    ]
    for spots, (section, first, count) in cases:
        strings = list(good)
        for sec, idx, name in spots:
            strings[_lane(n, sec, idx)] = bad[name]
        for level in LEVELS:
            e = _refused(gpu_ctx, _join(k, strings), level)
            assert (e.bits, e.section, e.first_bad, e.n_bad) == (DECODE, section, first, count), (spots, level)


def test_refusal_returns_no_object_and_names_the_point(gpu_ctx, srs):
    """the C ABI itself: BZH_E_RANGE, *out NULL, the verdict filled, bzh_last_error with section and index"""
    import bzh2
    from bzh2 import params as Pm
    k = 4
    s = srs(k)
    strings = _strings(s.data)
    strings[_lane(s.n, SEC_GL, 9)] = bytes(32)
    data = _join(k, strings)
    L = Pm._bind()
    h, v = ctypes.c_void_p(0xdead), np.full(4, 99, dtype=np.uint32)
    rc = L.bzh_params_read(gpu_ctx.handle, data, len(data), 0, Pm.CHECK_POINTS, ctypes.byref(h), ctypes.c_void_p(v.ctypes.data))
    assert rc == Pm.E_RANGE and h.value is None
    assert list(v) == [DECODE, SEC_GL, 9, 1]
    assert "g_lagrange[9]" in bzh2.load().bzh_last_error(gpu_ctx.handle).decode()
    # argument errors leave no object either, and the verdict zero
    for args in ((data, len(data) - 1, 0, Pm.CHECK_FULL), (data, len(data), 0, 3), (data, len(data), -1, Pm.CHECK_FULL)):
        h, v = ctypes.c_void_p(0xdead), np.full(4, 99, dtype=np.uint32)
        assert L.bzh_params_read(gpu_ctx.handle, *args, ctypes.byref(h), ctypes.c_void_p(v.ctypes.data)) == -1
        assert h.value is None and not v.any()
    k0 = struct.pack("<I", 0) + bytes(4 * 32)                             # a well-formed header for k = 0: Params start at k = 1
    assert Pm.file_info(k0) == (0, 1)
    assert L.bzh_params_read(gpu_ctx.handle, k0, len(k0), 0, Pm.CHECK_POINTS, ctypes.byref(h), None) == -1


def test_ctx_works_after_a_refusal(gpu_ctx, oracle_c, srs):
    from bzh2 import params as Pm
    k = 7
    s = srs(k)
    first = Pm.Params.from_bytes(gpu_ctx, s.data, check="full")
    try:
        strings = _strings(s.data)
        strings[_lane(s.n, SEC_G, 77)] = strings[_lane(s.n, SEC_G, 78)]
        for level, bits in (("lagrange", LAGRANGE), ("full", LAGRANGE | GENERATORS)):
            e = _refused(gpu_ctx, _join(k, strings), level)
            assert e.bits == bits
            if level == "full":
                assert (e.section, e.first_bad, e.n_bad) == (SEC_G, 77, 1)
        second = Pm.Params.from_bytes(gpu_ctx, s.data, check="full")
        try:
            a, b = first.points(), second.points()
            assert (a[0] == b[0]).all() and (a[1] == b[1]).all() and a[2:] == b[2:]
            assert second.to_bytes() == first.to_bytes() == s.data
            rng = np.random.default_rng(7)
            sc = np.frombuffer(rng.bytes((s.n + 3) * 32), dtype=np.uint64).reshape(s.n + 3, 4).copy()
            sc[:, 3] &= (1 << 61) - 1
            assert (_affine(gpu_ctx, first.bases_lagrange, sc) == _affine(gpu_ctx, second.bases_lagrange, sc)).all()
        finally:
            second.close()
    finally:
        first.close()


def test_file_round_trip_on_disk(gpu_ctx, srs, tmp_path):
    from bzh2 import params as Pm
    s = srs(4)
    path = tmp_path / "params_k4.bin"
    s.params.to_file(path)
    assert path.read_bytes() == s.data
    p = Pm.Params.from_file(gpu_ctx, path)
    try:
        assert (p.points()[1] == s.gl).all()
    finally:
        p.close()
    with pytest.raises(ValueError):
        Pm.Params.from_bytes(gpu_ctx, s.data, check="everything")
