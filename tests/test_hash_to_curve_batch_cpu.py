"""Batched hash-to-curve on the host (ctx == NULL): bzh_hash_to_curve_batch and bzh_map_to_curve_batch run the functions of
csrc/hash_to_curve.hpp that the device kernels run one lane per message.  Checked against the oracle (oracle/pasta.py), against
the one-message host function bzh_hash_to_curve (its own streaming expand_message_xmd for messages and prefixes of any length,
then the same map) and the reference's two `generator` known answers, at the BLAKE2b block boundaries of expand_message_xmd and
on the operands of every select of the map."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

from helpers import h2c_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("bzh_hash_to_curve_batch", "bzh_map_to_curve_batch", "bzh_params_generators_device", "bzh_params_create_with")
VP, U8P = ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint8)


@pytest.fixture(scope="module")
def lib():
    import bzh2
    from bzh2 import params as Pm
    return Pm._bind()


def _ints(xy_row):
    import bzh2
    return bzh2.limbs_to_int(xy_row[:4]), bzh2.limbs_to_int(xy_row[4:])


def test_header_declares_and_library_exports_the_entry_points(lib):
    import bzh2
    hdr = open(os.path.join(ROOT, "include", "bzh2.h")).read()
    for name in NEW:
        assert re.search(r"\bint %s\s*\(" % name, hdr), name
        assert name in bzh2.EXPORTS and hasattr(lib, name), name
    assert "BZH_GENERATORS_HOST = 0, BZH_GENERATORS_DEVICE = 1" in hdr


@pytest.mark.parametrize("cid", [0, 1])
def test_host_path_at_every_message_length(cid):
    import bzh2
    from bzh2 import params as Pm
    p = K.base_p(cid)
    for length in K.LENGTHS:
        msgs = K.messages(length, 3, seed=length)
        want = [K.hashed(cid, K.SRS_PREFIX, m) for m in msgs]
        assert want == [Pm.hash_to_curve(cid, K.SRS_PREFIX, m) for m in msgs]       # the one-message host function
        for form in (bzh2.FORM_CANONICAL, bzh2.FORM_MONTGOMERY):
            xy, st = Pm.hash_to_curve_batch(None, cid, K.SRS_PREFIX, msgs, form)
            assert st.tolist() == [bzh2.POINT_OK] * 3
            assert xy.tobytes() == K.points_array(want, p, form).tobytes(), (cid, length, form)


@pytest.mark.parametrize("cid", [0, 1])
def test_host_path_at_the_prefix_lengths_around_one_block(cid):
    import bzh2
    from bzh2 import params as Pm
    p = K.base_p(cid)
    blocks = set()
    for plen in K.PREFIX_LENGTHS:
        prefix = ("battlezips:" + "p" * 64)[:plen]
        blocks.add((64 + 1 + plen + 22 + len(K.CURVES[cid]) + 1 + 127) // 128)
        msgs = K.messages(5, 2, seed=plen)
        want = [K.hashed(cid, prefix, m) for m in msgs]
        assert want == [Pm.hash_to_curve(cid, prefix, m) for m in msgs]
        for form in (bzh2.FORM_CANONICAL, bzh2.FORM_MONTGOMERY):
            xy, _ = Pm.hash_to_curve_batch(None, cid, prefix, msgs, form)
            assert xy.tobytes() == K.points_array(want, p, form).tobytes(), (cid, plen, form)
    assert blocks == {1, 2}       # the second and third hash take one block and two


@pytest.mark.parametrize("cid", [0, 1])
def test_one_message_function_at_lengths_the_batch_plan_cannot_take(cid):
    """bzh_hash_to_curve under a 200-byte domain prefix at message lengths 0, 1, 127, 128, 129 and 300 against the oracle: the
    streaming expand_message_xmd keeps the lengths past the batch plan's 128 bytes; up to 128 bytes the batch gives the same point"""
    import bzh2
    import pasta as O
    from bzh2 import params as Pm
    prefix = ("battlezips:" + "long-domain-prefix/" * 10)[:200]
    assert len(prefix) == 200
    for length in (0, 1, 127, 128, 129, 300):
        msg = K.messages(length, 2, seed=length)[1]
        assert len(msg) == length
        want = K.hashed(cid, prefix, msg)
        assert O.CURVE_BY_ID[cid].is_on_curve(want)
        assert Pm.hash_to_curve(cid, prefix, msg) == want, (cid, length)
        if length <= 128:
            xy, st = Pm.hash_to_curve_batch(None, cid, prefix, [msg])
            assert st.tolist() == [bzh2.POINT_OK] and _ints(xy[0]) == want, (cid, length)


def test_the_references_generators_come_out_as_one_batch_of_two():
    import bzh2
    from bzh2 import params as Pm
    gold = json.load(open(os.path.join(ROOT, "tests", "golden", "fixed_bases.json")))["bases"]
    assert gold["v"]["hash_to_curve"]["domain"] == gold["r"]["hash_to_curve"]["domain"]
    xy, st = Pm.hash_to_curve_batch(None, bzh2.CURVE_PALLAS, gold["v"]["hash_to_curve"]["domain"],
                                    [gold[n]["hash_to_curve"]["message"].encode() for n in ("v", "r")])
    assert st.tolist() == [0, 0]
    assert [_ints(xy[i]) for i in range(2)] == [tuple(int(c, 16) for c in gold[n]["generator"]) for n in ("v", "r")]


@pytest.mark.parametrize("cid", [0, 1])
def test_map_alone_on_the_operands_of_every_select(cid, lib):
    import bzh2
    from bzh2 import params as Pm
    p = K.base_p(cid)
    pairs, want, squares = K.map_cases(cid)
    assert True in squares and False in squares          # both outcomes of the gx1 select are in the random pairs
    want_st = [bzh2.POINT_IDENTITY if w is None else bzh2.POINT_OK for w in want]
    assert [i for i, v in enumerate(want_st) if v == bzh2.POINT_IDENTITY] == [5, 6, 7]   # u1 = p - u0, (1, p - 1) among them
    for form in (bzh2.FORM_CANONICAL, bzh2.FORM_MONTGOMERY):
        u = K.pairs_array(pairs, p, form)
        xy, st = Pm.map_to_curve_batch(None, cid, u, form)
        assert st.tolist() == want_st
        assert xy.tobytes() == K.points_array(want, p, form).tobytes(), (cid, form)
        # status == NULL: BZH_E_RANGE for the identity, the other results still written
        out = np.full((len(pairs), 8), 3, dtype=np.uint64)
        assert lib.bzh_map_to_curve_batch(None, cid, VP(u.ctypes.data), len(pairs), form, bzh2.MEM_HOST, VP(out.ctypes.data), None) == bzh2.E_RANGE
        assert out.tobytes() == xy.tobytes()
        ok = np.ascontiguousarray(u[np.array(want_st) == bzh2.POINT_OK])
        out = np.zeros((ok.shape[0], 8), dtype=np.uint64)
        assert lib.bzh_map_to_curve_batch(None, cid, VP(ok.ctypes.data), ok.shape[0], form, bzh2.MEM_HOST, VP(out.ctypes.data), None) == bzh2.OK
    # the map composed with the oracle's hash_to_field is the hash
    import pasta as O
    msg = b"\x00\x07\x00\x00\x00"
    us = O.hash_to_field(K.CURVES[cid], K.SRS_PREFIX, msg, O.CURVE_BY_ID[cid].base)
    xy, _ = Pm.map_to_curve_batch(None, cid, K.pairs_array([tuple(us)], p, 0))
    assert _ints(xy[0]) == K.hashed(cid, K.SRS_PREFIX, msg)


def test_refusals_leave_the_outputs_untouched(lib):
    import bzh2
    E_ARG, E_RANGE, HOST, DEV = bzh2.E_ARG, bzh2.E_RANGE, bzh2.MEM_HOST, bzh2.MEM_DEVICE
    msgs = np.frombuffer(b"".join(K.messages(5, 2)), dtype=np.uint8).copy()
    out, st = np.full((2, 8), 3, dtype=np.uint64), np.full(2, 9, dtype=np.uint8)
    o, s, m = VP(out.ctypes.data), st.ctypes.data_as(U8P), VP(msgs.ctypes.data)

    def hashb(curve=0, prefix=b"Halo2-Parameters", msgs_=m, msg_len=5, n=2, form=0, mem=HOST, out_=o, st_=s):
        return lib.bzh_hash_to_curve_batch(None, curve, prefix, msgs_, msg_len, n, form, mem, out_, st_)

    assert hashb() == bzh2.OK and (st == 0).all()
    out[:], st[:] = 3, 9
    assert hashb(curve=2) == E_ARG and hashb(curve=7) == E_ARG and hashb(curve=-1) == E_ARG        # BN254 / unknown curve
    big = np.zeros(2 * 129, dtype=np.uint8)
    assert hashb(msgs_=VP(big.ctypes.data), msg_len=129) == E_ARG
    assert hashb(msg_len=128, msgs_=VP(big.ctypes.data)) == bzh2.OK
    out[:], st[:] = 3, 9
    # the DST is prefix + "-vesta_XMD:BLAKE2b_SSWU_RO_" (27 more bytes; 28 on Pallas): 255 bytes pass, 256 do not
    assert hashb(prefix=b"x" * 229) == E_ARG and hashb(curve=1, prefix=b"x" * 228) == E_ARG
    assert hashb(prefix=b"x" * 228) == bzh2.OK and hashb(curve=1, prefix=b"x" * 227) == bzh2.OK
    out[:], st[:] = 3, 9
    assert hashb(prefix=None) == E_ARG
    assert hashb(n=(1 << 28) + 1) == E_ARG
    assert hashb(form=2) == E_ARG and hashb(mem=2) == E_ARG
    assert hashb(mem=DEV) == E_ARG                                  # device memory without a context
    assert hashb(out_=None) == E_ARG and hashb(msgs_=None) == E_ARG
    assert hashb(n=0, out_=None, msgs_=None, st_=None) == bzh2.OK
    assert (out == 3).all() and (st == 9).all()

    p = K.base_p(0)
    u = K.pairs_array([(1, 2), (3, 4)], p, 0)

    def mapb(curve=0, u_=None, n=2, form=0, mem=HOST, out_=o, st_=s):
        return lib.bzh_map_to_curve_batch(None, curve, VP(u.ctypes.data) if u_ is None else u_, n, form, mem, out_, st_)

    assert mapb(curve=2) == E_ARG and mapb(form=5) == E_ARG and mapb(mem=3) == E_ARG and mapb(mem=DEV) == E_ARG
    assert mapb(n=(1 << 28) + 1) == E_ARG and mapb(out_=None) == E_ARG
    assert lib.bzh_map_to_curve_batch(None, 0, None, 2, 0, HOST, o, s) == E_ARG
    assert lib.bzh_map_to_curve_batch(None, 0, None, 0, 0, HOST, None, None) == bzh2.OK
    for bad in (p, p + 1, (1 << 256) - 1):                          # a u that is not below p, in either slot and either form
        for slot in (0, 1):
            for form in (0, 1):
                pair = [1, 2]
                pair[slot] = bad
                nc = K.points_array([(1, 2), tuple(pair)], 1 << 300, 0)
                assert mapb(u_=VP(nc.ctypes.data), form=form) == E_RANGE, (bad, slot, form)
    assert (out == 3).all() and (st == 9).all()
    # entry points that need a context
    h = VP()
    assert lib.bzh_params_generators_device(None, 0, 2, 0, HOST, o) == E_ARG
    assert lib.bzh_params_create_with(None, 4, b"", 0, 1, ctypes.byref(h)) == E_ARG
    assert (out == 3).all() and not h.value
