"""bzh_group_ifft (csrc/params.hip: k_gfft_load, k_gfft_stage, k_gfft_finish, point_scalar_mul) -- the transform that makes
g_lagrange -- on inputs with known discrete logarithms (tests/helpers/group_fft_cases.py): g[i] = [a_i] G, so output j is
[b_j] G with b = intt(a), every one of them compared bit for bit with the C oracle's scalar multiplication.  The named cases
make butterflies add a point to itself, to its negative and to the identity, at stages tests/test_group_fft_cases_cpu.py asserts
from an integer replay of the schedule; the sizes are those where the launch geometry changes: k = 0 (no stage at all), 6 (half a
workgroup of butterflies), 7 (exactly one), 9 and 10 (several workgroups in the load and in the stages).

Known limit: the cache file of Params has no checksum.  A file of the right length, magic and k whose point bytes were changed is
loaded as it is; only the refusals the loader does make are tested here."""
import ctypes
import os

import numpy as np
import pytest

import coracle as C
from helpers import group_fft_cases as GF

pytestmark = pytest.mark.gpu

E_ARG = -1


def _compare(got, want, what):
    """bit for bit, row by row; a row that should be (0, 0) and is not (or the reverse) differs like any other"""
    assert got.shape == want.shape and got.dtype == want.dtype == np.uint64
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, "%s: %d of %d rows differ, the first at index %d: got %s, want %s" % (
        what, bad.size, got.shape[0], bad[0], [hex(int(x)) for x in got[bad[0]]], [hex(int(x)) for x in want[bad[0]]])


def _run(ctx, k, a):
    """(got, want) of one group_ifft call on ([a_i] G)"""
    from bzh2 import params as Pm
    G = GF.generator()
    got = Pm.group_ifft(ctx, GF.input_points(G, a))
    return got, GF.expected_points(G, GF.dlog_ifft(a, k))


@pytest.mark.parametrize("k", GF.GPU_KS_EVERY_OUTPUT)
def test_every_output_on_known_discrete_logs(gpu_ctx, oracle_c, k):
    got, want = _run(gpu_ctx, k, GF.built(k)["uniform"])
    assert want.any(axis=1).all()          # the control has no identity row
    _compare(got, want, "uniform, k = %d" % k)


@pytest.mark.parametrize("k,name", GF.gpu_case_params())
def test_closed_form_and_colliding_inputs(gpu_ctx, oracle_c, k, name):
    a = GF.built(k)[name]
    b = GF.dlog_ifft(a, k)
    got, want = _run(gpu_ctx, k, a)
    zero = np.array([x == 0 for x in b])
    assert (want[zero] == 0).all() and want[~zero].any(axis=1).all()
    assert (got[zero] == 0).all(), "%s, k = %d: %d identity rows are not eight zero limbs" % (name, k, int(got[zero].any(axis=1).sum()))
    _compare(got, want, "%s, k = %d" % (name, k))


def test_walked_table_matches(gpu_ctx, oracle_c):
    """g[i] = [i + 1] G, the table the accumulated-verification tests take their Lagrange bases from"""
    from bzh2 import params as Pm
    k = GF.GPU_K_WALK
    n = 1 << k
    G = GF.generator()
    g = C.point_walk(0, G, n)
    _compare(g[:3], GF.expected_points(G, [1, 2, 3]), "the walk itself")
    _compare(Pm.group_ifft(gpu_ctx, g), GF.expected_points(G, GF.dlog_ifft([i + 1 for i in range(n)], k)), "walked table, k = %d" % k)


def test_input_is_left_as_it_was_and_calls_are_independent(gpu_ctx, oracle_c):
    from bzh2 import params as Pm
    k = 5
    G = GF.generator()
    const, uniform = (GF.input_points(G, GF.built(k)[name]) for name in ("constant", "uniform"))
    const_before, uniform_before = const.copy(), uniform.copy()
    first = Pm.group_ifft(gpu_ctx, const)
    middle = Pm.group_ifft(gpu_ctx, uniform)
    third = Pm.group_ifft(gpu_ctx, const)
    assert (first == third).all()
    assert (const == const_before).all() and (uniform == uniform_before).all()
    _compare(first, GF.expected_points(G, GF.dlog_ifft(GF.built(k)["constant"], k)), "constant, first call")
    _compare(middle, GF.expected_points(G, GF.dlog_ifft(GF.built(k)["uniform"], k)), "uniform, between them")


def test_wrapper_refuses_what_it_cannot_transform(gpu_ctx, oracle_c):
    import bzh2
    from bzh2 import params as Pm
    G = GF.generator()
    for rows in (3, 6, 0):
        with pytest.raises(ValueError):
            Pm.group_ifft(gpu_ctx, np.tile(G, (rows, 1)))
    for shape in ((4, 4), (32,), (2, 2, 8)):
        with pytest.raises(ValueError):
            Pm.group_ifft(gpu_ctx, np.zeros(shape, dtype=np.uint64))
    # the C entry point: a curve other than Vesta, k = 25, NULL pointers
    L, vp = Pm._bind(), ctypes.c_void_p
    g = np.tile(G, (2, 1))
    out = np.full((2, 8), 7, dtype=np.uint64)
    gp, op = vp(g.ctypes.data), vp(out.ctypes.data)
    assert L.bzh_group_ifft(gpu_ctx.handle, bzh2.CURVE_PALLAS, gp, 1, op) == E_ARG
    assert L.bzh_group_ifft(gpu_ctx.handle, bzh2.CURVE_VESTA, gp, 25, op) == E_ARG
    assert L.bzh_group_ifft(None, bzh2.CURVE_VESTA, gp, 1, op) == E_ARG
    assert L.bzh_group_ifft(gpu_ctx.handle, bzh2.CURVE_VESTA, None, 1, op) == E_ARG
    assert L.bzh_group_ifft(gpu_ctx.handle, bzh2.CURVE_VESTA, gp, 1, None) == E_ARG
    assert (out == 7).all()                # a refused call writes nothing
    assert L.bzh_group_ifft(gpu_ctx.handle, bzh2.CURVE_VESTA, gp, 1, op) == 0
    _compare(out, GF.expected_points(G, [1, 0]), "the same arguments, accepted")     # intt([1, 1]) = [1, 0]


def test_cache_file_that_does_not_match_is_regenerated(gpu_ctx, oracle_c, tmp_path):
    """wrong magic, wrong k word, a short read, an empty file: each is refused, the points are made again -- the same -- and the
    file is rewritten so that the next construction loads it"""
    from bzh2 import params as Pm
    k = 3
    n = 1 << k

    def construct():
        p = Pm.Params(gpu_ctx, k, cache_dir=str(tmp_path))
        try:
            return p.points()
        finally:
            p.close()

    def same(x, y):
        return (x[0] == y[0]).all() and (x[1] == y[1]).all() and x[2:4] == y[2:4]

    first = construct()
    assert first[4] is False
    path = os.path.join(str(tmp_path), "params_vesta_k%d_v1.bin" % k)
    good = open(path, "rb").read()
    assert len(good) == 16 + 2 * n * 64 + 128
    assert int.from_bytes(good[8:16], "little") == k
    _compare(first[1], Pm.group_ifft(gpu_ctx, first[0]), "g_lagrange of Params against group_ifft(g)")
    damaged = {"magic": bytes(b ^ 0xff for b in good[:8]) + good[8:],
               "k word": good[:8] + (4).to_bytes(8, "little") + good[16:],
               "short": good[:-64],
               "empty": b""}
    for what, data in damaged.items():
        with open(path, "wb") as f:
            f.write(data)
        again = construct()
        assert again[4] is False, what + ": loaded from a file that does not match"
        assert same(again, first), what
        assert open(path, "rb").read() == good, what + ": the file was not rewritten"
        reloaded = construct()
        assert reloaded[4] is True and same(reloaded, first), what
