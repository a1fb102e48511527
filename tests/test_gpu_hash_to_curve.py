"""csrc/hash_to_curve.hip on the device: k_hash_to_field and k_map_to_curve through bzh_hash_to_curve_batch, bzh_map_to_curve_batch,
bzh_params_generators_device and Params(generators="device") -- byte for byte what the host path (ctx == NULL) of the same call
gives, the oracle on a sample, at n = 1, 255, 256, 257 (a lone lane, the tail guard, a second block), and a Params::new whose
points, cache file, window tables and proof bytes equal the host-made one's."""
import ctypes
import random

import numpy as np
import pytest

from helpers import h2c_cases as K

pytestmark = pytest.mark.gpu
VP, U8P = ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint8)
SIZES = (1, 255, 256, 257)


@pytest.fixture(scope="module")
def lib(gpu_ctx):
    from bzh2 import params as Pm
    return Pm._bind()


def _dev(arr):
    import torch
    return torch.from_numpy(arr.copy()).to("cuda")


def _ints(row):
    import bzh2
    return bzh2.limbs_to_int(row[:4]), bzh2.limbs_to_int(row[4:])


@pytest.mark.parametrize("cid", [0, 1])
def test_block_boundaries_on_the_device(gpu_ctx, cid):
    """every message length and prefix length of the CPU file through the kernels"""
    import bzh2
    from bzh2 import params as Pm
    for prefix, length in [(K.SRS_PREFIX, n) for n in K.LENGTHS] + [(("battlezips:" + "p" * 64)[:n], 5) for n in K.PREFIX_LENGTHS]:
        msgs = K.messages(length, 3, seed=length + len(prefix))
        for form in (bzh2.FORM_CANONICAL, bzh2.FORM_MONTGOMERY):
            host, host_st = Pm.hash_to_curve_batch(None, cid, prefix, msgs, form)
            got, st = Pm.hash_to_curve_batch(gpu_ctx, cid, prefix, msgs, form)
            assert st.tolist() == host_st.tolist() == [0, 0, 0]
            assert got.tobytes() == host.tobytes(), (cid, prefix, length, form)
        assert [_ints(r) for r in Pm.hash_to_curve_batch(gpu_ctx, cid, prefix, msgs)[0]] == [K.hashed(cid, prefix, m) for m in msgs]


@pytest.mark.parametrize("cid", [0, 1])
def test_hash_batch_sizes_host_and_device_memory(gpu_ctx, lib, cid):
    import bzh2
    from bzh2 import params as Pm
    length = 16                                                        # whole 16-byte rows: device buffers are 16-byte aligned
    all_msgs = K.messages(length, 257, seed=cid)
    rng = random.Random(77 + cid)
    for n in SIZES:
        msgs = all_msgs[:n]
        for form in (bzh2.FORM_CANONICAL, bzh2.FORM_MONTGOMERY):
            host, host_st = Pm.hash_to_curve_batch(None, cid, K.SRS_PREFIX, msgs, form)
            got, st = Pm.hash_to_curve_batch(gpu_ctx, cid, K.SRS_PREFIX, msgs, form)          # BZH_MEM_HOST through the kernels
            assert st.tolist() == host_st.tolist() and got.tobytes() == host.tobytes(), (cid, n, form)
            d_in = _dev(np.frombuffer(b"".join(msgs), dtype=np.uint8))
            d_out, d_st = _dev(np.full((n, 8), 3, dtype=np.int64)), _dev(np.full(n, 9, dtype=np.uint8))
            rc = lib.bzh_hash_to_curve_batch(gpu_ctx.handle, cid, K.SRS_PREFIX.encode(), VP(d_in.data_ptr()), length, n, form, bzh2.MEM_DEVICE,
                                             VP(d_out.data_ptr()), ctypes.cast(d_st.data_ptr(), U8P))
            assert rc == bzh2.OK
            gpu_ctx.sync()
            assert d_st.cpu().numpy().tolist() == host_st.tolist() and d_out.cpu().numpy().tobytes() == host.tobytes(), (cid, n, form)
            # status == NULL with device memory: the call waits and reports
            d_out = _dev(np.full((n, 8), 3, dtype=np.int64))
            assert lib.bzh_hash_to_curve_batch(gpu_ctx.handle, cid, K.SRS_PREFIX.encode(), VP(d_in.data_ptr()), length, n, form, bzh2.MEM_DEVICE,
                                               VP(d_out.data_ptr()), None) == bzh2.OK
            assert d_out.cpu().numpy().tobytes() == host.tobytes()
        canon = Pm.hash_to_curve_batch(gpu_ctx, cid, K.SRS_PREFIX, msgs)[0]
        for i in rng.sample(range(n), min(n, 32)):
            assert _ints(canon[i]) == K.hashed(cid, K.SRS_PREFIX, msgs[i]), (cid, n, i)


@pytest.mark.parametrize("cid", [0, 1])
def test_map_alone_on_the_device(gpu_ctx, lib, cid):
    import bzh2
    from bzh2 import params as Pm
    p = K.base_p(cid)
    pairs, want, _ = K.map_cases(cid)
    reps = 257 // len(pairs) + 1
    pairs_all, want_all = (pairs * reps)[:257], (want * reps)[:257]
    for n in SIZES + (len(pairs),):
        want_st = [bzh2.POINT_IDENTITY if w is None else bzh2.POINT_OK for w in want_all[:n]]
        for form in (bzh2.FORM_CANONICAL, bzh2.FORM_MONTGOMERY):
            u = K.pairs_array(pairs_all[:n], p, form)
            host, host_st = Pm.map_to_curve_batch(None, cid, u, form)
            assert host_st.tolist() == want_st and host.tobytes() == K.points_array(want_all[:n], p, form).tobytes()
            got, st = Pm.map_to_curve_batch(gpu_ctx, cid, u, form)
            assert st.tolist() == want_st, (cid, n, form)
            assert got.tobytes() == host.tobytes(), (cid, n, form)
            d_in, d_out, d_st = _dev(u.view(np.int64)), _dev(np.full((n, 8), 3, dtype=np.int64)), _dev(np.full(n, 9, dtype=np.uint8))
            rc = lib.bzh_map_to_curve_batch(gpu_ctx.handle, cid, VP(d_in.data_ptr()), n, form, bzh2.MEM_DEVICE, VP(d_out.data_ptr()),
                                            ctypes.cast(d_st.data_ptr(), U8P))
            assert rc == bzh2.OK
            gpu_ctx.sync()
            assert d_st.cpu().numpy().tolist() == want_st and d_out.cpu().numpy().tobytes() == host.tobytes(), (cid, n, form)
            # in place: the points over their operands
            rc = lib.bzh_map_to_curve_batch(gpu_ctx.handle, cid, VP(d_in.data_ptr()), n, form, bzh2.MEM_DEVICE, VP(d_in.data_ptr()),
                                            ctypes.cast(d_st.data_ptr(), U8P))
            assert rc == bzh2.OK
            gpu_ctx.sync()
            assert d_in.cpu().numpy().tobytes() == host.tobytes()
    # status == NULL: BZH_E_RANGE when a result is the identity, host and device memory; the results still written
    u = K.pairs_array(pairs, p, 0)
    host = Pm.map_to_curve_batch(None, cid, u)[0]
    out = np.full((len(pairs), 8), 3, dtype=np.uint64)
    assert lib.bzh_map_to_curve_batch(gpu_ctx.handle, cid, VP(u.ctypes.data), len(pairs), 0, bzh2.MEM_HOST, VP(out.ctypes.data), None) == bzh2.E_RANGE
    assert out.tobytes() == host.tobytes()
    d_in, d_out = _dev(u.view(np.int64)), _dev(np.full((len(pairs), 8), 3, dtype=np.int64))
    assert lib.bzh_map_to_curve_batch(gpu_ctx.handle, cid, VP(d_in.data_ptr()), len(pairs), 0, bzh2.MEM_DEVICE, VP(d_out.data_ptr()), None) == bzh2.E_RANGE
    assert d_out.cpu().numpy().tobytes() == host.tobytes()
    # a u that is not below p: refused before anything is written from host memory, BZH_POINT_INVALID and zeros per lane on the device
    nc = K.points_array([(1, 2), (p, 2), (3, p + 1), (3, 4)], 1 << 300, 0)
    out, st = np.full((4, 8), 3, dtype=np.uint64), np.full(4, 9, dtype=np.uint8)
    assert lib.bzh_map_to_curve_batch(gpu_ctx.handle, cid, VP(nc.ctypes.data), 4, 0, bzh2.MEM_HOST, VP(out.ctypes.data), st.ctypes.data_as(U8P)) == bzh2.E_RANGE
    assert (out == 3).all() and (st == 9).all()
    d_in, d_out, d_st = _dev(nc.view(np.int64)), _dev(np.full((4, 8), 3, dtype=np.int64)), _dev(np.full(4, 9, dtype=np.uint8))
    assert lib.bzh_map_to_curve_batch(gpu_ctx.handle, cid, VP(d_in.data_ptr()), 4, 0, bzh2.MEM_DEVICE, VP(d_out.data_ptr()),
                                      ctypes.cast(d_st.data_ptr(), U8P)) == bzh2.OK
    gpu_ctx.sync()
    good = Pm.map_to_curve_batch(None, cid, K.pairs_array([(1, 2), (3, 4)], p, 0))[0]
    assert d_st.cpu().numpy().tolist() == [0, 2, 2, 0]
    res = d_out.cpu().numpy().view(np.uint64)
    assert res[0].tobytes() == good[0].tobytes() and res[3].tobytes() == good[1].tobytes() and not res[1:3].any()


def test_refusals_that_need_a_context(gpu_ctx, lib):
    import bzh2
    out = np.full((4, 8), 3, dtype=np.uint64)
    o = VP(out.ctypes.data)
    d = _dev(np.zeros(64, dtype=np.int64))
    st = _dev(np.zeros(16, dtype=np.uint8))
    s = ctypes.cast(st.data_ptr(), U8P)
    H = gpu_ctx.handle
    # misaligned device pointers
    assert lib.bzh_hash_to_curve_batch(H, 0, b"x", VP(d.data_ptr() + 8), 16, 2, 0, bzh2.MEM_DEVICE, VP(d.data_ptr() + 64), s) == bzh2.E_ARG
    assert lib.bzh_hash_to_curve_batch(H, 0, b"x", VP(d.data_ptr()), 16, 2, 0, bzh2.MEM_DEVICE, VP(d.data_ptr() + 72), s) == bzh2.E_ARG
    assert lib.bzh_map_to_curve_batch(H, 0, VP(d.data_ptr() + 4), 2, 0, bzh2.MEM_DEVICE, VP(d.data_ptr() + 256), s) == bzh2.E_ARG
    assert lib.bzh_map_to_curve_batch(H, 0, VP(d.data_ptr()), 2, 0, bzh2.MEM_DEVICE, VP(d.data_ptr() + 264), s) == bzh2.E_ARG
    assert lib.bzh_params_generators_device(H, 0, 2, 0, bzh2.MEM_DEVICE, VP(d.data_ptr() + 8)) == bzh2.E_ARG
    # the message holds the index as a u32
    assert lib.bzh_params_generators_device(H, (1 << 32) - 3, 4, 0, bzh2.MEM_HOST, o) == bzh2.E_RANGE
    assert lib.bzh_params_generators_device(H, 1 << 32, 1, 0, bzh2.MEM_HOST, o) == bzh2.E_RANGE
    assert lib.bzh_params_generators_device(H, 0, 4, 2, bzh2.MEM_HOST, o) == bzh2.E_ARG
    assert lib.bzh_params_generators_device(H, 0, 4, 0, 2, o) == bzh2.E_ARG
    assert lib.bzh_params_generators_device(H, 0, 4, 0, bzh2.MEM_HOST, None) == bzh2.E_ARG
    assert lib.bzh_params_generators_device(H, 0, (1 << 28) + 1, 0, bzh2.MEM_HOST, o) == bzh2.E_ARG
    assert lib.bzh_params_generators_device(H, 5, 0, 0, bzh2.MEM_HOST, None) == bzh2.OK
    h = VP()
    for where in (2, -1):
        assert lib.bzh_params_create_with(H, 4, b"", 0, where, ctypes.byref(h)) == bzh2.E_ARG and not h.value
    assert (out == 3).all()


@pytest.mark.parametrize("first,count", [(0, 512), (250, 12), (65530, 12)])
def test_generators_device_windows(gpu_ctx, first, count):
    """against the host's bzh_params_generators (k = 9 holds the first two windows) / bzh_hash_to_curve; (65530, 12) crosses
    into the third byte of the index"""
    import bzh2
    from bzh2 import params as Pm
    got = Pm.generators_device(gpu_ctx, first, count)
    if first + count <= 512:
        assert got.tobytes() == Pm.generators(9)[0][first:first + count].tobytes()
    else:
        for i in range(count):
            assert _ints(got[i]) == Pm.hash_to_curve(bzh2.CURVE_VESTA, K.SRS_PREFIX, bytes([0]) + (first + i).to_bytes(4, "little")), i
    mont = Pm.generators_device(gpu_ctx, first, count, bzh2.FORM_MONTGOMERY)
    assert mont.tobytes() == K.points_array([_ints(r) for r in got], K.base_p(0), 1).tobytes()


def test_generators_device_large_index_and_device_memory(gpu_ctx, lib):
    import bzh2
    from bzh2 import params as Pm
    first = (1 << 24) - 4
    got = Pm.generators_device(gpu_ctx, first, 4)
    for i in range(4):
        msg = bytes([0]) + (first + i).to_bytes(4, "little")           # the last byte of the index comes into play at 2^24 - 1 + 1
        assert _ints(got[i]) == Pm.hash_to_curve(bzh2.CURVE_VESTA, K.SRS_PREFIX, msg), i
    top = Pm.generators_device(gpu_ctx, (1 << 32) - 2, 2)
    assert _ints(top[1]) == Pm.hash_to_curve(bzh2.CURVE_VESTA, K.SRS_PREFIX, b"\x00\xff\xff\xff\xff")
    d = _dev(np.full((4, 8), 3, dtype=np.int64))
    assert lib.bzh_params_generators_device(gpu_ctx.handle, first, 4, 0, bzh2.MEM_DEVICE, VP(d.data_ptr())) == bzh2.OK
    assert d.cpu().numpy().tobytes() == got.tobytes()


def test_params_with_device_generators_equal_host_made_params(gpu_ctx, oracle_c, tmp_path):
    import os
    from bzh2 import params as Pm
    k = 8
    dirs = [tmp_path / "device", tmp_path / "host"]
    for d in dirs:
        d.mkdir()
    pd = Pm.Params(gpu_ctx, k, cache_dir=str(dirs[0]), generators="device")
    ph = Pm.Params(gpu_ctx, k, cache_dir=str(dirs[1]), generators="host")
    try:
        gd, gld, wd, ud, cached_d = pd.points()
        gh, glh, wh, uh, cached_h = ph.points()
        assert not cached_d and not cached_h
        assert (gd == gh).all() and (gld == glh).all() and (wd, ud) == (wh, uh)
        files = [sorted(os.listdir(d)) for d in dirs]
        assert files[0] == files[1] and len(files[0]) == 1
        assert (dirs[0] / files[0][0]).read_bytes() == (dirs[1] / files[1][0]).read_bytes()
        # the window tables of the two, over their first two rows
        for a, b in ((pd.bases, ph.bases), (pd.bases_lagrange, ph.bases_lagrange)):
            assert gpu_ctx.bases_points(a, 0, 2 * a.n).tobytes() == gpu_ctx.bases_points(b, 0, 2 * b.n).tobytes()
        again = Pm.Params(gpu_ctx, k, cache_dir=str(dirs[0]), generators="device")
        try:
            g2, gl2, w2, u2, cached2 = again.points()
            assert cached2 and (g2 == gd).all() and (gl2 == gld).all() and (w2, u2) == (wd, ud)
        finally:
            again.close()
        with pytest.raises(ValueError):
            Pm.Params(gpu_ctx, k, cache_dir="", generators="gpu")
    finally:
        pd.close()
        ph.close()


def test_one_proof_on_device_made_params(gpu_ctx, oracle_c):
    """the bitify test circuit at k = 6 (tests/test_gpu_params.py): the proof on the device-made params verifies and equals the
    proof on the host-made params under the same rng bytes"""
    import bzh2
    from bzh2 import circuits as Cm, native as N, params as Pm
    from bzh2.game import BinaryValue
    k, bits = 6, 20
    lay = Cm.CircuitLayout(Cm.NUM2BITS_TEST, k, bits)
    proofs = {}
    try:
        blob = lay.blob()
        rng = random.Random(66)
        value = rng.getrandbits(bits)
        adv = lay.synthesize_bitify_test(value, BinaryValue(value))
        rbytes = None
        for where in ("device", "host"):
            prm = Pm.Params(gpu_ctx, k, cache_dir="", generators=where)
            pk = N.NativeProvingKey(gpu_ctx, blob, bzh2.CURVE_VESTA, params=prm)
            try:
                assert not prm.points(want_g=False, want_lagrange=False)[4]
                rbytes = rbytes or bytes(rng.getrandbits(8) for _ in range(pk.rng_bytes))
                proofs[where] = pk.prove_batch(adv, [[]], [rbytes])
                assert pk.verify_batch([[]], proofs[where]) == [True], where
            finally:
                pk.close()
                prm.close()
        assert proofs["device"] == proofs["host"]
    finally:
        lay.close()
