"""csrc/sqrt_decompress.hip on the device: k_batch_sqrt over all four fields and k_decompress over the three curves, through
BZH_MEM_HOST and BZH_MEM_DEVICE, canonical and Montgomery, at n = 1, 63, 64, 65, 300 (a lone lane, a partial wave, a wave
boundary, a partial block) -- bit for bit what the host path and Python integers give (tests/helpers/sqrt_cases.py) -- and
bzh_verify_batch with the proofs' points decompressed on the device against the host selection and the oracle verifier."""
import ctypes
import random

import numpy as np
import pytest

import coracle as C
import halo2_oracle as H
import pasta as O
import sample_circuit as S
from helpers import sqrt_cases as K
from helpers.real_parity import accelerated_oracle

pytestmark = pytest.mark.gpu
VP, U8P = ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint8)


@pytest.fixture(scope="module")
def lib(gpu_ctx):
    import bzh2
    L = bzh2.load()
    L.bzh_batch_sqrt.argtypes = [VP, ctypes.c_int, VP, ctypes.c_size_t, ctypes.c_int, ctypes.c_int, U8P]
    L.bzh_affine_decompress.argtypes = [VP, ctypes.c_int, VP, ctypes.c_size_t, ctypes.c_int, ctypes.c_int, VP, U8P]
    return L


def _dev(arr):
    import torch
    return torch.from_numpy(arr.copy()).to("cuda")


@pytest.mark.parametrize("fid", [0, 1, 2, 3])
def test_batch_sqrt_on_the_device(gpu_ctx, lib, fid):
    import bzh2
    p = K.FIELDS[fid].p
    cases = K.sqrt_cases(fid)
    assert len(cases) > 300                                   # the full list spans more than one block
    for form in (bzh2.FORM_CANONICAL, bzh2.FORM_MONTGOMERY):
        a_all = np.frombuffer(K.limbs_bytes(K.to_form(u, p, form) for u, _ in cases), dtype=np.uint64).reshape(-1, 4)
        want_all = [K.to_form(u if r is None else r, p, form) for u, r in cases]
        st_all = [0 if r is None else 1 for _, r in cases]
        for n in K.SIZES + (len(cases),):
            a, want, want_st = a_all[:n], K.limbs_bytes(want_all[:n]), st_all[:n]
            host, host_st = bzh2.batch_sqrt(fid, a, form)                       # ctx == NULL: the host path
            assert host.tobytes() == want and host_st.tolist() == want_st
            got, st = bzh2.batch_sqrt(fid, a, form, ctx=gpu_ctx)                # BZH_MEM_HOST through the kernel
            assert st.tolist() == want_st, (fid, form, n)
            assert got.tobytes() == want, (fid, form, n)
            d, dst = _dev(a.view(np.int64)), _dev(np.full(n, 9, dtype=np.uint8))   # BZH_MEM_DEVICE
            rc = lib.bzh_batch_sqrt(gpu_ctx.handle, fid, VP(d.data_ptr()), n, form, bzh2.MEM_DEVICE, ctypes.cast(dst.data_ptr(), U8P))
            assert rc == bzh2.OK
            gpu_ctx.sync()
            assert dst.cpu().numpy().tolist() == want_st and d.cpu().numpy().tobytes() == want, (fid, form, n)
        # status == NULL: BZH_E_RANGE when an element is not a square (host and device memory), the roots still written
        b = a_all.copy()
        assert lib.bzh_batch_sqrt(gpu_ctx.handle, fid, VP(b.ctypes.data), len(cases), form, bzh2.MEM_HOST, None) == bzh2.E_RANGE
        assert b.tobytes() == K.limbs_bytes(want_all)
        d = _dev(a_all.view(np.int64))
        assert lib.bzh_batch_sqrt(gpu_ctx.handle, fid, VP(d.data_ptr()), len(cases), form, bzh2.MEM_DEVICE, None) == bzh2.E_RANGE
        assert d.cpu().numpy().tobytes() == K.limbs_bytes(want_all)
        sq = np.ascontiguousarray(a_all[np.array(st_all, dtype=bool)])
        assert lib.bzh_batch_sqrt(gpu_ctx.handle, fid, VP(sq.ctypes.data), sq.shape[0], form, bzh2.MEM_HOST, None) == bzh2.OK
    assert lib.bzh_batch_sqrt(gpu_ctx.handle, fid, None, 0, 0, bzh2.MEM_DEVICE, None) == bzh2.OK
    assert lib.bzh_batch_sqrt(gpu_ctx.handle, fid, None, 3, 0, bzh2.MEM_DEVICE, None) == bzh2.E_ARG


@pytest.mark.parametrize("cid", [0, 1, 2])
def test_affine_decompress_on_the_device(gpu_ctx, lib, cid):
    import bzh2
    p = K.curve_of(cid).base.p
    strings, pts, mixed, want = K.decompress_cases(cid)
    assert len(mixed) == 300
    for form in (bzh2.FORM_CANONICAL, bzh2.FORM_MONTGOMERY):
        # round trip: compress the points, decompress on the device, the same points come back
        xy = np.frombuffer(K.limbs_bytes(K.to_form(c, p, form) for pt in pts for c in pt), dtype=np.uint64).reshape(-1, 8)
        assert bzh2.affine_compress(cid, xy, form) == strings
        back, st = bzh2.affine_decompress(cid, strings, form, ctx=gpu_ctx)
        assert (st == bzh2.POINT_OK).all() and back.tobytes() == xy.tobytes()
        assert bzh2.affine_decompress(cid, strings, form, ctx=gpu_ctx, check=True)[0].tobytes() == xy.tobytes()
        for n in K.SIZES:
            want_st = [w[0] for w in want[:n]]
            want_xy = K.limbs_bytes(K.to_form(c, p, form) for w in want[:n] for c in w[1:])
            host, host_st = bzh2.affine_decompress(cid, mixed[:n], form)
            assert host.tobytes() == want_xy and host_st.tolist() == want_st
            got, st = bzh2.affine_decompress(cid, mixed[:n], form, ctx=gpu_ctx)
            assert st.tolist() == want_st, (cid, form, n)
            assert got.tobytes() == want_xy, (cid, form, n)
            raw = np.frombuffer(b"".join(mixed[:n]), dtype=np.uint8)
            d_in, d_out, d_st = _dev(raw), _dev(np.full((n, 8), 3, dtype=np.int64)), _dev(np.full(n, 9, dtype=np.uint8))
            rc = lib.bzh_affine_decompress(gpu_ctx.handle, cid, VP(d_in.data_ptr()), n, form, bzh2.MEM_DEVICE, VP(d_out.data_ptr()),
                                           ctypes.cast(d_st.data_ptr(), U8P))
            assert rc == bzh2.OK
            gpu_ctx.sync()
            assert d_st.cpu().numpy().tolist() == want_st and d_out.cpu().numpy().tobytes() == want_xy, (cid, form, n)
        assert {0, 1, 2} == {w[0] for w in want[:63]}       # valid, identity and invalid lanes share the first wave
        # status == NULL gives BZH_E_RANGE, and the valid outputs are still correct
        raw = np.frombuffer(b"".join(mixed), dtype=np.uint8).copy()
        out = np.full((len(mixed), 8), 3, dtype=np.uint64)
        rc = lib.bzh_affine_decompress(gpu_ctx.handle, cid, VP(raw.ctypes.data), len(mixed), form, bzh2.MEM_HOST, VP(out.ctypes.data), None)
        assert rc == bzh2.E_RANGE and out.tobytes() == K.limbs_bytes(K.to_form(c, p, form) for w in want for c in w[1:])
    assert lib.bzh_affine_decompress(gpu_ctx.handle, cid, None, 0, 0, bzh2.MEM_DEVICE, None, None) == bzh2.OK
    assert lib.bzh_affine_decompress(gpu_ctx.handle, cid, None, 2, 0, bzh2.MEM_DEVICE, None, None) == bzh2.E_ARG


def _off_curve_x(cv, rng):
    while True:
        x = rng.randrange(1, cv.base.p)
        if cv.base.sqrt((x * x * x + cv.b) % cv.base.p) is None:
            return x


@pytest.mark.parametrize("k,with_lookup,degree", [(4, False, None), (5, True, None), (6, True, 9)])
@accelerated_oracle
def test_verify_batch_with_device_points_agrees_with_host_and_oracle(gpu_ctx, oracle_c, k, with_lookup, degree):
    """The circuits and proof mutations of test_gpu_native_prover.py::test_native_verify_batch_agrees_with_oracle_verifier, plus a
    first commitment with x >= p and one with x off the curve: results[] under VERIFY_POINTS_DEVICE equal those under
    VERIFY_POINTS_HOST and the oracle verifier's."""
    import bzh2
    from bzh2 import native as N, circuit_data as P
    cv, F = O.VESTA, O.FP
    cs, fixed, copies, adv, inst = S.build(k=k, seed=900 + k, with_lookup=with_lookup, degree=degree)
    rng = random.Random(5000 + k)
    g = [cv.random_point(rng) for _ in range(cs.n)]
    w, u = cv.random_point(rng), cv.random_point(rng)
    keys = H.Keys(cs, H.Domain(cs, F), cv, g, w, u, fixed, copies)
    circ = P.Circuit(cs.k, cs.num_advice, cs.num_fixed, cs.num_instance, cs.gates, cs.perm_columns, cs.lookups, fixed, copies,
                     degree=degree)
    pk = N.NativeProvingKey(gpu_ctx, circ, bzh2.CURVE_VESTA, g, w, u)
    try:
        assert pk.verify_selected() == N.VERIFY_POINTS_HOST                     # every new key's default
        rs = [rng.randrange(F.p) for _ in range(pk.rng_bytes // 64)]
        good = H.create_proof(keys, adv, inst, rs, O.Blake2bTranscript(F))
        cases = [(inst, good)]
        cases.append(([[(inst[0][0] + 1) % F.p]], good))                       # wrong public input
        step = max(1, len(good) // 12)
        for pos in range(5, len(good), step):                                   # one flipped bit per section
            cases.append((inst, good[:pos] + bytes([good[pos] ^ 0x04]) + good[pos + 1:]))
        cases.append((inst, good[:-32]))                                        # truncated
        cases.append((inst, good[:-32] + (F.p + 1).to_bytes(32, "little")))     # non-canonical final scalar
        cases.append((inst, good + b"\x00" * 32))                               # trailing bytes
        cases.append((inst, bytes(32) + good[32:]))                             # an identity commitment
        ipa_start = len(good) - 32 * (2 * k + 3)
        cases.append((inst, good[:ipa_start] + bytes(32) + good[ipa_start + 32:]))   # identity as the IPA's S
        cases.append((inst, (cv.base.p + 2).to_bytes(32, "little") + good[32:]))        # first commitment: x >= p
        cases.append((inst, _off_curve_x(cv, rng).to_bytes(32, "little") + good[32:]))  # first commitment: x off the curve
        cases.append((inst, good[:40]))                                         # ends inside the second point
        want = [H.verify_proof(keys, c[0], c[1], O.Blake2bTranscript(F)) for c in cases]
        assert want[0] is True and not any(want[1:])
        got = {}
        for where in (N.VERIFY_POINTS_DEVICE, N.VERIFY_POINTS_HOST, N.VERIFY_POINTS_DEVICE):
            pk.verify_select(where)
            assert pk.verify_selected() == where
            got[where] = pk.verify_batch([c[0] for c in cases], [c[1] for c in cases])
            assert got[where] == want, where
        with pytest.raises(bzh2.BzhError) as e:
            pk.verify_select(2)
        assert e.value.status == bzh2.E_ARG and pk.verify_selected() == N.VERIFY_POINTS_DEVICE
    finally:
        pk.close()


def test_real_shot_batch_verifies_the_same_through_both_selections(gpu_ctx, oracle_c):
    """ShotCircuit at k = 11 on the Params::new SRS: five proofs, the fourth tampered, verified under both selections."""
    import bzh2
    from bzh2 import circuits as Cm, native as N, params as Pm
    from bzh2.game import BinaryValue
    r = random.Random(0x5407)
    lay = Cm.CircuitLayout(Cm.SHOT, 11)
    prm = Pm.Params(gpu_ctx, 11)
    pk = N.NativeProvingKey(gpu_ctx, lay.blob(), bzh2.CURVE_VESTA, params=prm)
    try:
        _, state = Cm.board_witness([(3, 3, True), (5, 4, False), (0, 1, False), (0, 5, True), (6, 1, False)], None)
        shots = [([3], [5], 1), ([4], [3], 0)] * 2 + [([3], [5], 1)]      # a hit and a miss, a fresh trapdoor each
        circuits = [Cm.ShotCircuit(state, r.randrange(O.FQ.p), Cm.shot_serialize(xs, ys), BinaryValue.from_u8(hit)) for xs, ys, hit in shots]
        adv, insts = lay.synthesize(circuits)
        proofs = pk.prove_batch(adv, insts, None, seeds=[r.randbytes(32) for _ in circuits])
        proofs[3] = proofs[3][:700] + bytes([proofs[3][700] ^ 0x10]) + proofs[3][701:]
        want = [True, True, True, False, True]
        for where in (N.VERIFY_POINTS_HOST, N.VERIFY_POINTS_DEVICE):
            pk.verify_select(where)
            assert pk.verify_batch(insts, proofs) == want, where
    finally:
        pk.close()
        prm.close()
        lay.close()
