"""bzh_ipa_open_batch_device on the GPU: the opening's rounds against a device-resident transcript batch must write the bytes
bzh_ipa_open_batch writes into host transcripts -- and the oracle's restatement of upstream -- leave the transcripts in the same
state, and return the same evaluations; on a window table (paired rounds) and on a plain upload, with and without the generator
collapse, from host operands and from device operands, for one wave of proofs and for a second, partial one (B = 65).
Every transcript is primed first (tests/helpers/ipa_open_device_cases.py), so the block buffer is part-filled, the state is not
the initial one and the proof does not start at offset 0."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import coracle as C
import pasta as O
from helpers import ipa_open_device_cases as K
from helpers.real_parity import accelerated_oracle

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG, E_RANGE = -1, -4
SHAPES = [(k, B) for k in (1, 2, 5) for B in (1, 3, 64, 65)] + [(k, B) for k in (6, 9) for B in (1, 3, 64)]


@functools.lru_cache(maxsize=None)
def oracle_opening(cid, k, B):
    """[(v, proof bytes, one further challenge)] from oracle/pasta.py: ipa_open, proof by proof"""
    cv = O.CURVE_BY_ID[cid]
    F = cv.scalar
    g, w, u = K.srs(cid, k)
    polys, blinds, x3s, rbs = K.operands(cid, k, B)
    out = []
    for b in range(B):
        n = 1 << k
        rs = [O.from_u512(rbs[b][64 * i:64 * (i + 1)], F) for i in range(n + 1 + 2 * k)]
        ot = K.primed_oracle(cid, b)
        v = O.ipa_open(cv, list(g), w, u, polys[b], blinds[b], x3s[b], rs, ot)
        out.append((v, bytes(ot.proof), ot.squeeze_challenge()))
    return out


@pytest.mark.parametrize("precompute", [True, False], ids=["window_table", "plain_upload"])
@pytest.mark.parametrize("k,B", SHAPES)
@pytest.mark.parametrize("cid", [0, 1], ids=["vesta", "pallas"])
@accelerated_oracle
def test_bytes_state_and_values_match_the_host_transcript_path_and_the_oracle(gpu_ctx, cid, k, B, precompute):
    hb = K.upload(gpu_ctx, cid, k, precompute)
    try:
        want = K.host_path(gpu_ctx, hb, cid, k, B)
        got, st, tb_st = K.device_path(gpu_ctx, hb, cid, k, B)
    finally:
        hb.free()
    assert len(got[1][0]) == K.proof_cap(k)
    assert got[1] == want[1]            # the proofs' bytes
    assert got[0] == want[0]            # out_v
    assert got[2] == want[2]            # one further challenge: the state carried over, not only the bytes
    assert not st.any() and not tb_st.any()
    if k <= 5 and B <= 3:
        ora = oracle_opening(cid, k, B)
        assert got[0] == [o[0] for o in ora] and got[1] == [o[1] for o in ora] and got[2] == [o[2] for o in ora]


def test_automatic_collapse_matches_the_host_transcript_path(gpu_ctx):
    """k = 9, B = 8 on a window table: from batch 8 on the opening collapses its generators by itself (jstar), and the restart of
    s is a fill on the device"""
    hb = K.upload(gpu_ctx, 0, 9, True)
    try:
        want = K.host_path(gpu_ctx, hb, 0, 9, 8)
        got, st, tb_st = K.device_path(gpu_ctx, hb, 0, 9, 8)
    finally:
        hb.free()
    assert got == want and not st.any() and not tb_st.any()


def _child(extra):
    env = dict(os.environ)
    for name in ("BZH_IPA_COLLAPSE", "BZH_IPA_TAIL_C"):
        env.pop(name, None)
    env.update(extra)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "helpers", "ipa_open_device_cases.py")], env=env, capture_output=True,
                         text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = dict(ln.split()[:2] for ln in out.stdout.splitlines() if ln.startswith(("PARITY ", "DIGEST ")))
    assert lines.get("PARITY") == "ok", out.stdout[-500:]
    return lines["DIGEST"]


def test_forced_collapse_matches_the_host_transcript_path_in_a_fresh_process():
    """k = 6, B = 3 under BZH_IPA_COLLAPSE=2 (read once per process, hence a child process): the device-transcript path equals
    the host-transcript path under the same setting, and the setting changes no byte"""
    assert _child({"BZH_IPA_COLLAPSE": "2"}) == _child({})


@pytest.mark.parametrize("form", [0, 1], ids=["canonical", "montgomery"])
def test_device_operands_and_a_squeezed_x3_give_the_host_operand_bytes(gpu_ctx, form):
    """the seam end to end: x3 is squeezed into device memory by the batch itself and never leaves it; polys, blinds, rng, out_v
    and status are torch tensors"""
    import torch
    import bzh2
    cid, k, B = 0, 5, 3
    F = O.CURVE_BY_ID[cid].scalar
    n, nrand = 1 << k, (1 << k) + 1 + 2 * k
    polys, blinds, _, rbs = K.operands(cid, k, B)
    conv = (lambda x: x * F.R % F.p) if form == bzh2.FORM_MONTGOMERY else (lambda x: x)
    p_arr = np.stack([C.ints_to_array([conv(c) for c in p]) for p in polys])
    bl_arr = C.ints_to_array([conv(x) for x in blinds])

    def dev(a):
        return torch.from_numpy(np.ascontiguousarray(a).view(np.int64).copy()).to("cuda")

    hb = K.upload(gpu_ctx, cid, k, True)
    try:
        # host operands: the squeezed x3 comes down and goes back up
        trs = K.primed(cid, B)
        with bzh2.TranscriptBatch(cid, B, K.proof_cap(k), gpu_ctx) as tb:
            tb.from_host(trs)
            x3 = tb.squeeze(form=form)
            v_want, st_want = tb.ipa_open(hb, p_arr, bl_arr, x3, list(rbs), form=form)
            want = tb.proofs()
            after_want = tb.squeeze()
        # device operands
        stride = 64 * nrand + 64   # rows further apart than they are long
        raw = np.zeros((B, stride), dtype=np.uint8)
        for b in range(B):
            raw[b, :64 * nrand] = np.frombuffer(rbs[b], dtype=np.uint8)
        d_p, d_bl, d_raw = dev(p_arr), dev(bl_arr), torch.from_numpy(raw).to("cuda")
        d_x3 = torch.zeros((B, 4), dtype=torch.int64, device="cuda")
        d_v = torch.zeros((B, 4), dtype=torch.int64, device="cuda")
        d_st = torch.full((B,), 9, dtype=torch.uint8, device="cuda")
        with bzh2.TranscriptBatch(cid, B, K.proof_cap(k), gpu_ctx) as tb:
            tb.from_host(trs)
            tb.squeeze(form=form, mem=bzh2.MEM_DEVICE, out=d_x3.data_ptr())
            assert tb.ipa_open(hb, d_p.data_ptr(), d_bl.data_ptr(), d_x3.data_ptr(), d_raw.data_ptr(), form=form, mem=bzh2.MEM_DEVICE,
                               out_v=d_v.data_ptr(), status=d_st.data_ptr(), rng_stride=stride) is None
            got = tb.proofs()
            after = tb.squeeze()
            assert not tb.status().any()
        gpu_ctx.sync()
        assert got == want and (after == after_want).all()
        assert (d_v.cpu().numpy().view(np.uint64) == v_want).all()
        assert not d_st.cpu().numpy().any() and not st_want.any()
        # and the evaluation is the polynomial's, at the squeezed point
        x3_int = [bzh2.limbs_to_int(x) for x in x3]
        if form == bzh2.FORM_MONTGOMERY:
            rinv = pow(F.R, -1, F.p)
            x3_int = [x * rinv % F.p for x in x3_int]
            v_int = [bzh2.limbs_to_int(x) * rinv % F.p for x in v_want]
        else:
            v_int = [bzh2.limbs_to_int(x) for x in v_want]
        assert v_int == [O.eval_polynomial(polys[b], x3_int[b], F) for b in range(B)]
        for t in trs:
            t.close()
    finally:
        hb.free()


def test_an_opening_is_accepted_by_ipa_verify_and_rejected_with_another_value(gpu_ctx):
    import bzh2
    cid, k, B = 0, 5, 1
    cv = O.CURVE_BY_ID[cid]
    F = cv.scalar
    g, w, u = K.srs(cid, k)
    polys, blinds, x3s, _ = K.operands(cid, k, B)
    hb = K.upload(gpu_ctx, cid, k, True)
    try:
        (v, proofs, _), st, _ = K.device_path(gpu_ctx, hb, cid, k, B)
        assert not st.any()
        # the commitment from bzh_msm: scalars [poly..., 0 (U), blind (W)]
        jac = gpu_ctx.msm(hb, C.ints_to_array(polys[0] + [0, blinds[0]]))
        P = C.array_to_point(bzh2.jacobian_to_affine(cid, np.asarray(jac).reshape(-1, 12))[0])
        opening = proofs[0][32:]     # after the primed point
        for value, accept in ((v[0], True), ((v[0] + 1) % F.p, False)):
            t = K.primed(cid, 1)[0]
            assert gpu_ctx.ipa_verify(hb, P, x3s[0], value, opening, t, [g[0], u, w]) is accept
            t.close()
    finally:
        hb.free()


def test_refusals_leave_the_batch_as_it_was(gpu_ctx):
    import torch
    import bzh2
    cid, k, B = 0, 2, 3
    n, nrand = 1 << k, (1 << k) + 1 + 2 * k
    polys, blinds, x3s, rbs = K.operands(cid, k, B)
    p_arr = K.poly_array(polys)
    hb = K.upload(gpu_ctx, cid, k, True)
    cap = K.proof_cap(k)

    def batch(curve, size, pcap):
        tb = bzh2.TranscriptBatch(curve, size, pcap, gpu_ctx)
        trs = K.primed(curve, size)
        tb.from_host(trs)
        for t in trs:
            t.close()
        return tb

    def refused(tb, status, call):
        with batch(tb.curve, tb.batch, tb.proof_cap) as twin:
            with pytest.raises(bzh2.BzhError) as e:
                call(tb)
            assert e.value.status == status
            assert tb.proof_len() == 32 and (tb.squeeze() == twin.squeeze()).all()
        tb.close()

    try:
        host_call = lambda tb: tb.ipa_open(hb, p_arr, blinds, x3s, list(rbs))  # noqa: E731
        refused(batch(cid, B + 1, cap), E_ARG, host_call)                       # a batch of another size
        refused(batch(1 - cid, B, cap), E_ARG, host_call)                       # a batch of the other curve
        refused(batch(cid, B, cap - 1), E_RANGE, host_call)                     # proof_cap one byte short
        refused(batch(cid, B, cap), E_ARG, lambda tb: tb.ipa_open(hb, p_arr, blinds, x3s, [r[:-64] for r in rbs]))   # rng_stride too small
        d = torch.zeros(B * n * 4 + B * 12 + B * nrand * 8 + 8, dtype=torch.int64, device="cuda")
        base = d.data_ptr()
        o_bl, o_x3, o_v, o_rng = base + B * n * 32, base + B * n * 32 + B * 32, base + B * n * 32 + B * 64, base + B * n * 32 + B * 96
        for bump in range(5):                                                   # each device pointer in turn 8 bytes off
            ptrs = [base, o_bl, o_x3, o_rng, o_v]
            ptrs[bump] += 8
            refused(batch(cid, B, cap), E_ARG, lambda tb: tb.ipa_open(hb, ptrs[0], ptrs[1], ptrs[2], ptrs[3], form=bzh2.FORM_MONTGOMERY,
                                                                        mem=bzh2.MEM_DEVICE, out_v=ptrs[4], rng_stride=64 * nrand))
        gpu_ctx.sync()
        assert not d.cpu().numpy().any()                                        # nothing was written either
    finally:
        hb.free()
