"""Accumulated batch verification without a device: bzh_accumulation_weights against bzh_rng_expand and a big-integer wide
reduction, the header / exports agreement for the new calls, and the argument refusals that come before any device use -- a NULL
seed, a batch above the limit -- on a real verifying key read from bytes and made-up table handles a refusal must not read
through."""
import ctypes
import os
import re

import numpy as np
import pytest

from helpers import verify_pass_cases as VP
from helpers import vk_cases as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("bzh_verify_records_accumulated", "bzh_verify_batch_vk_accumulated", "bzh_ipa_check_accumulated")
SEEDS = (bytes(range(32)), bytes(255 - 7 * i & 0xff for i in range(32)))


@pytest.mark.parametrize("curve", [0, 1])
@pytest.mark.parametrize("batch", [1, 5])
@pytest.mark.parametrize("seed", SEEDS)
def test_weights_are_the_wide_reduction_of_the_seeds_draws(curve, batch, seed):
    """w_b = draw b of bzh_rng_expand(seed, ..) as a 512-bit little-endian integer mod the curve's scalar field; draw b depends on
    b alone: the weights of a batch of 1 are a prefix of those of a batch of 5, and draw b is bzh_rng_expand(seed, b, 1)"""
    import bzh2
    from bzh2 import native as N
    r = N.MODULI[bzh2.CURVE_SCALAR_FIELD[curve]]
    stream = N.rng_expand(seed, 0, batch)
    want = [int.from_bytes(stream[64 * b:64 * b + 64], "little") % r for b in range(batch)]
    got = bzh2.accumulation_weights(curve, seed, batch)
    assert got == want and all(0 <= w < r for w in got)
    assert bzh2.accumulation_weights(curve, seed, 5)[:batch] == got
    for b in range(batch):
        assert int.from_bytes(N.rng_expand(seed, b, 1), "little") % r == got[b]
    other = SEEDS[1] if seed == SEEDS[0] else SEEDS[0]
    assert bzh2.accumulation_weights(curve, other, batch) != got


def test_weights_refusals():
    from bzh2 import native as N
    L = N._bind()
    out = np.full(4, 7, dtype=np.uint64)
    vp = ctypes.c_void_p
    assert L.bzh_accumulation_weights(0, None, 1, vp(out.ctypes.data)) == V.E_ARG
    assert L.bzh_accumulation_weights(0, SEEDS[0], 1, None) == V.E_ARG
    assert L.bzh_accumulation_weights(2, SEEDS[0], 1, vp(out.ctypes.data)) == V.E_ARG        # BN254: no Pasta scalar field
    assert (out == 7).all()
    assert L.bzh_accumulation_weights(0, SEEDS[0], 0, None) == 0


def test_header_and_exports_name_the_calls():
    import bzh2
    from bzh2 import native as N
    header = open(os.path.join(ROOT, "include", "bzh2.h")).read()
    for name in CALLS + ("bzh_accumulation_weights",):
        assert re.search(r"\bint %s\(" % name, header) and name in bzh2.EXPORTS, name
        getattr(bzh2.load(), name)
    assert hasattr(N.NativeVerifyingKey, "verify_records_accumulated") and hasattr(N.NativeVerifyingKey, "verify_batch_accumulated")
    sec = header[header.index("int bzh_rng_expand("):header.index("int bzh_accumulation_weights(")]
    assert "SECURITY" in sec and "cryptographically secure" in sec and "fresh per call" in sec and "1/|F|" in sec


def test_argument_refusals_without_a_device():
    """a NULL seed and a batch above 4096 are BZH_E_ARG from both front doors, and so is what the calls they extend refuse; the
    outputs are untouched"""
    from bzh2 import native as N
    L = N._bind()
    vp = ctypes.c_void_p
    fake = vp(0x1000)
    fc, sc = V.oracle_commitments(V.K, 70, 1)
    key = N.NativeVerifyingKey.from_bytes(V.bzv1(V.circuit(V.K, 70, 1)[5], fc, sc))
    try:
        B = 2
        plen = len(VP.oracle_proof(1, 0)[1])
        stride = 144 + plen
        recs = np.zeros(B * stride, dtype=np.uint8)
        res = (ctypes.c_int * B)(7, 7)
        st = np.full(B, 7, dtype=np.uint8)
        path = ctypes.c_int(7)

        def records(**kw):
            a = dict(ctx=fake, vk=key.handle, srs=fake, lag=fake, batch=B, n_inputs=1, records=vp(recs.ctypes.data), stride=stride, g0=None,
                     seed=SEEDS[0], res=res, st=vp(st.ctypes.data), path=ctypes.byref(path))
            a.update(kw)
            return L.bzh_verify_records_accumulated(*a.values())

        for kw in (dict(seed=None), dict(batch=4097), dict(ctx=None), dict(vk=None), dict(srs=None), dict(lag=None), dict(records=None),
                   dict(res=None), dict(n_inputs=0), dict(n_inputs=5), dict(stride=stride - 1)):
            assert records(**kw) == V.E_ARG, kw
        inst = np.zeros((B, 1, 4), dtype=np.uint64)
        proofs = np.zeros((B, plen), dtype=np.uint8)
        lens = (ctypes.c_size_t * B)(plen, plen)
        g0 = np.zeros((3, 8), dtype=np.uint64)

        def batch(**kw):
            a = dict(ctx=fake, vk=key.handle, srs=fake, lag=None, batch=B, inst=vp(inst.ctypes.data), rows=1, proofs=vp(proofs.ctypes.data),
                     stride=plen, lens=lens, g0=vp(g0.ctypes.data), seed=SEEDS[0], res=res, path=ctypes.byref(path))
            a.update(kw)
            return L.bzh_verify_batch_vk_accumulated(*a.values())

        for kw in (dict(seed=None), dict(batch=4097), dict(batch=0), dict(ctx=None), dict(vk=None), dict(srs=None), dict(proofs=None),
                   dict(lens=None), dict(g0=None), dict(res=None)):
            assert batch(**kw) == V.E_ARG, kw
        assert list(res) == [7, 7] and (st == 7).all() and path.value == 7
        ok = ctypes.c_int(7)
        for kw in (dict(weights=None), dict(batch=0), dict(batch=4097), dict(nl=0), dict(ctx=None), dict(bases=None), dict(ok=None)):
            a = dict(ctx=fake, bases=fake, batch=1, nl=1, pts=fake, scal=fake, cu=fake, weights=fake, exclude=None, ok=ctypes.byref(ok))
            a.update(kw)
            assert L.bzh_ipa_check_accumulated(*a.values()) == V.E_ARG, kw
        assert ok.value == 7
    finally:
        key.close()
