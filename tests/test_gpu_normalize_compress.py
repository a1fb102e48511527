"""csrc/normalize_compress.hip on the device: k_batch_normalize over the three curves, canonical and Montgomery, through
BZH_MEM_HOST and BZH_MEM_DEVICE -- byte for byte what the host path gives, which tests/test_normalize_compress_cpu.py pins to
Python integers.  Shapes come from bzh_batch_normalize_plan: one point per lane at the wave and block edges, then chains of two
and three with a ragged end, identities and invalid lanes placed inside chains, each output alone (the running products then
share that output's slots), the result of a device-resident MSM normalised without leaving HBM, and the enqueue-only contract."""
import ctypes
import functools
import random

import numpy as np
import pytest

import coracle as C
from helpers import normalize_cases as K

pytestmark = pytest.mark.gpu
CAN, MONT = 0, 1


def _dev(arr):
    import torch
    return torch.from_numpy(arr.copy()).to("cuda")


@functools.lru_cache(maxsize=None)
def _case(cid, form, n, with_identities=True):
    """(jac array, places of the planted identities, host-path xy / enc / status) -- computed once per shape"""
    import bzh2
    lanes, _ = bzh2.batch_normalize_plan(n)
    places = []
    if with_identities and lanes > 8:
        own = lambda t: K.chain_indices(n, lanes, t)
        places = [own(1)[0], own(2)[-1]] + own(5)            # the first and the last point of a chain, and a whole chain
    jac = K.jac_array(cid, K.batch(cid, n, seed=n, identities=places), form)
    xy, enc, st = bzh2.batch_normalize(cid, jac, form=form, want_bytes=True, want_status=True)
    for a in (jac, xy, enc, st):
        a.setflags(write=False)
    return jac, places, xy, enc, st


def _on_device(gpu_ctx, cid, form, jac, want_xy=True, want_bytes=True, want_status=True):
    """bzh_batch_normalize on device buffers pre-filled with a pattern: (xy, enc, status) as numpy arrays, None where not asked"""
    import bzh2
    n = jac.shape[0]
    d_in = _dev(jac.view(np.int64))
    d_xy = _dev(np.full((n, 8), 3, dtype=np.int64)) if want_xy else None
    d_enc = _dev(np.full((n, 32), 7, dtype=np.uint8)) if want_bytes else None
    d_st = _dev(np.full(n, 9, dtype=np.uint8)) if want_status else None
    ptr = lambda t: None if t is None else t.data_ptr()
    bzh2.batch_normalize(cid, d_in.data_ptr(), ctx=gpu_ctx, form=form, mem=bzh2.MEM_DEVICE, n=n, out_xy=ptr(d_xy), out32=ptr(d_enc),
                         status=ptr(d_st))
    gpu_ctx.sync()
    assert d_in.cpu().numpy().tobytes() == jac.tobytes()      # the input is read only
    get = lambda t, dt: None if t is None else t.cpu().numpy().view(dt)
    return get(d_xy, np.uint64), get(d_enc, np.uint8), get(d_st, np.uint8)


def _same(got, want, what):
    for g, w, name in zip(got, want, ("xy", "enc", "status")):
        if g is not None:
            assert g.tobytes() == w.tobytes(), (what, name)


@pytest.mark.parametrize("form", [CAN, MONT])
@pytest.mark.parametrize("cid", [0, 1, 2])
def test_device_equals_host_at_wave_and_block_edges(gpu_ctx, cid, form):
    import bzh2
    for n in K.GPU_SIZES:
        assert bzh2.batch_normalize_plan(n) == (n, 1)
        jac, _, *want = _case(cid, form, n)
        assert {0, 1} <= set(want[2].tolist()) or n == 1
        got = bzh2.batch_normalize(cid, jac, ctx=gpu_ctx, form=form, want_bytes=True, want_status=True)       # BZH_MEM_HOST through the kernel
        _same(got, want, (cid, form, n, "host memory"))
        _same(_on_device(gpu_ctx, cid, form, jac), want, (cid, form, n, "device memory"))
        # to_bytes alone: k_affine_compress against the separate host code of bzh_affine_compress
        old = b"".join(bzh2.affine_compress(cid, want[0], form))
        assert bzh2.affine_compress_batch(cid, want[0], ctx=gpu_ctx, form=form).tobytes() == old
        d_xy, d_enc = _dev(want[0].view(np.int64)), _dev(np.full((n, 32), 7, dtype=np.uint8))
        bzh2.affine_compress_batch(cid, d_xy.data_ptr(), ctx=gpu_ctx, form=form, mem=bzh2.MEM_DEVICE, n=n, out32=d_enc.data_ptr())
        gpu_ctx.sync()
        assert d_enc.cpu().numpy().tobytes() == old and old == want[1].tobytes()


def _chain_sizes():
    import bzh2
    n2, n3 = K.smallest_n_with_chain(bzh2.batch_normalize_plan, 2), K.smallest_n_with_chain(bzh2.batch_normalize_plan, 3)
    return n2, n3


@pytest.mark.parametrize("cid,form", [(0, MONT), (1, CAN)])
def test_chains_longer_than_one(gpu_ctx, cid, form):
    import bzh2
    n2, n3 = _chain_sizes()
    for n, chain in ((n2 - 1, 1), (n2, 2), (n2 + 1, 2), (n3 + 5, 3)):
        lanes, got_chain = bzh2.batch_normalize_plan(n)
        assert got_chain == chain
        jac, places, *want = _case(cid, form, n)
        assert len(places) == 2 + len(K.chain_indices(n, lanes, 5)) and (want[2][places] == K.POINT_IDENTITY).all()
        if n in (n2, n3 + 5):
            assert lanes * chain > n                         # a ragged end: the last lanes own one point fewer
        _same(_on_device(gpu_ctx, cid, form, jac), want, (cid, form, n, "device memory"))
    jac, _, *want = _case(cid, form, n3 + 5)
    got = bzh2.batch_normalize(cid, jac, ctx=gpu_ctx, form=form, want_bytes=True, want_status=True)
    _same(got, want, (cid, form, n3 + 5, "host memory"))


@pytest.mark.parametrize("cid", [0, 2])
def test_invalid_lanes_inside_a_chain(gpu_ctx, cid):
    import bzh2
    n = _chain_sizes()[0] + 1
    lanes, chain = bzh2.batch_normalize_plan(n)
    assert chain == 2
    p = K.curve_of(cid).p
    jac, places, *want = _case(cid, CAN, n)
    own = lambda t: K.chain_indices(n, lanes, t)
    bad = {own(3)[0]: (0, p), own(4)[1]: (2, (1 << 256) - 1), own(6)[0]: (1, p + 1), own(6)[1]: (2, p)}    # index -> (coordinate, value)
    assert not set(bad) & set(places) and all(len(own(t)) == 2 for t in (3, 4, 6))
    dirty = jac.copy()
    for i, (coord, v) in bad.items():
        dirty[i, 4 * coord:4 * coord + 4] = np.frombuffer(v.to_bytes(32, "little"), dtype=np.uint64)
    xy, enc, st = (a.copy() for a in want)
    idx = sorted(bad)
    xy[idx], enc[idx], st[idx] = 0, 0, K.POINT_INVALID
    _same(_on_device(gpu_ctx, cid, CAN, dirty), (xy, enc, st), (cid, "invalid lanes"))
    # without a status buffer the call waits for the statuses and reports the invalid lane
    d_in, d_xy = _dev(dirty.view(np.int64)), _dev(np.full((n, 8), 3, dtype=np.int64))
    with pytest.raises(bzh2.BzhError) as e:
        bzh2.batch_normalize(cid, d_in.data_ptr(), ctx=gpu_ctx, form=CAN, mem=bzh2.MEM_DEVICE, n=n, out_xy=d_xy.data_ptr())
    assert e.value.status == bzh2.E_RANGE
    assert d_xy.cpu().numpy().view(np.uint64).tobytes() == xy.tobytes()
    # host operands are refused before the launch
    with pytest.raises(bzh2.BzhError) as e:
        bzh2.batch_normalize(cid, dirty, ctx=gpu_ctx, form=CAN, want_status=True)
    assert e.value.status == bzh2.E_RANGE
    # identities are no error without a status buffer
    d_in = _dev(jac.view(np.int64))
    bzh2.batch_normalize(cid, d_in.data_ptr(), ctx=gpu_ctx, form=CAN, mem=bzh2.MEM_DEVICE, n=n, out_xy=d_xy.data_ptr())
    assert d_xy.cpu().numpy().view(np.uint64).tobytes() == want[0].tobytes()


@pytest.mark.parametrize("cid,form", [(1, MONT), (2, CAN)])
def test_each_output_alone(gpu_ctx, cid, form):
    """the running products wait in out_xy's x slots, or in out32's slots when there is no out_xy"""
    n = _chain_sizes()[0] + 1
    jac, _, *want = _case(cid, form, n)
    _same(_on_device(gpu_ctx, cid, form, jac), want, (cid, form, "both"))
    only_enc = _on_device(gpu_ctx, cid, form, jac, want_xy=False)
    assert only_enc[0] is None
    _same(only_enc, want, (cid, form, "bytes only"))
    only_xy = _on_device(gpu_ctx, cid, form, jac, want_bytes=False)
    assert only_xy[1] is None
    _same(only_xy, want, (cid, form, "points only"))


def test_msm_results_become_a_table_without_leaving_the_device(gpu_ctx):
    import torch
    import bzh2
    import pasta as O
    cid, n, batch = bzh2.CURVE_VESTA, 64, 5
    cv = K.curve_of(cid)
    rng = random.Random(0x6d73)
    bases = C.point_walk(cid, C.points_to_array([cv.random_point(rng)])[0], n)
    sc = [[rng.randrange(O.FP.p) for _ in range(n)] for _ in range(batch)]
    sc[1] = [0] * n                                            # this MSM's result is the identity
    sc_m = np.frombuffer(K.limbs_bytes(K.to_form(s, O.FP.p, MONT) for row in sc for s in row), dtype=np.uint64).reshape(batch, n, 4).copy()
    hb = gpu_ctx.upload_bases(cid, bases)
    tbl = None
    try:
        d_s, d_jac = _dev(sc_m.view(np.int64)), torch.zeros((batch, 12), dtype=torch.int64, device="cuda")
        d_xy, d_st = torch.zeros((batch, 8), dtype=torch.int64, device="cuda"), torch.zeros(batch, dtype=torch.uint8, device="cuda")
        gpu_ctx.msm_device(hb, d_s.data_ptr(), n, batch, d_jac.data_ptr(), form=MONT)
        bzh2.batch_normalize(cid, d_jac.data_ptr(), ctx=gpu_ctx, form=MONT, mem=bzh2.MEM_DEVICE, n=batch, out_xy=d_xy.data_ptr(),
                             status=d_st.data_ptr())
        tbl = gpu_ctx.upload_bases(cid, d_xy.data_ptr(), n=batch, form=MONT, device_ptr=True)
        got = gpu_ctx.bases_points(tbl, 0, batch)
        assert d_st.cpu().numpy().tolist() == [0, 1, 0, 0, 0]
        want = bzh2.jacobian_to_affine(cid, gpu_ctx.msm(hb, sc_m, form=MONT), MONT)
        r_inv = pow(K.R, -1, cv.p)
        want_can = K.limbs_bytes(v * r_inv % cv.p for v in C.array_to_ints(want.reshape(-1, 4)))
        assert got.tobytes() == want_can and not got[1].any() and got[0].any()
        assert C.array_to_point(got[0]) == cv.msm_pippenger(sc[0], [C.array_to_point(b) for b in bases])
    finally:
        if tbl is not None:
            tbl.free()
        hb.free()


def test_enqueue_only_equals_blocking(gpu_ctx):
    import bzh2
    cid, form, n = 0, MONT, 257
    jac, _, *want = _case(cid, form, n)
    d_in = _dev(jac.view(np.int64))
    outs = []
    for with_status in (True, False):
        d_xy, d_enc, d_st = _dev(np.full((n, 8), 3, dtype=np.int64)), _dev(np.full((n, 32), 7, dtype=np.uint8)), _dev(np.full(n, 9, dtype=np.uint8))
        bzh2.batch_normalize(cid, d_in.data_ptr(), ctx=gpu_ctx, form=form, mem=bzh2.MEM_DEVICE, n=n, out_xy=d_xy.data_ptr(),
                             out32=d_enc.data_ptr(), status=d_st.data_ptr() if with_status else None)
        if with_status:
            gpu_ctx.sync()                                     # the call only enqueued
            assert d_st.cpu().numpy().tobytes() == want[2].tobytes()
        outs.append((d_xy.cpu().numpy().tobytes(), d_enc.cpu().numpy().tobytes()))
    assert outs[0] == outs[1] == (want[0].tobytes(), want[1].tobytes())
