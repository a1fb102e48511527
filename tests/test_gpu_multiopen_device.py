"""bzh_multiopen_batch_device on the GPU: the multiopen argument against a device-resident transcript batch must write, proof for
proof and byte for byte, what a big-int model composed of oracle pieces writes (tests/helpers/multiopen_cases.py: the multiopen
part of oracle/halo2_oracle.py's create_proof), and leave the transcripts in the same state.  Every transcript is primed first
(tests/helpers/ipa_open_device_cases.py), so the block buffer is part-filled, the state is not the initial one and the proof
does not start at offset 0."""
import copy
import functools

import numpy as np
import pytest

import coracle as C
import pasta as O
from helpers import ipa_open_device_cases as K
from helpers import multiopen_cases as M
from helpers.real_parity import accelerated_oracle

pytestmark = pytest.mark.gpu

E_ARG, E_RANGE = -1, -4


@functools.lru_cache(maxsize=None)
def expected(cid, k, B):
    return M.model(cid, k, B, M.QUERIES, M.operands(cid, k, B))


# k = 4 with B = 1 and k = 6 with B = 3: the smallest sizes at which the opening's collapse-free rounds, a multi-block grid of the
# lane kernels' callees and a batch stride larger than one all occur
@pytest.mark.parametrize("k,B", [(4, 1), (6, 3)])
@pytest.mark.parametrize("cid", [0, 1], ids=["vesta", "pallas"])
@accelerated_oracle
def test_bytes_and_state_match_the_model(gpu_ctx, cid, k, B):
    hb = K.upload(gpu_ctx, cid, k, True)
    try:
        got, st, tb_st = M.device_call(gpu_ctx, hb, cid, k, B, M.QUERIES, M.operands(cid, k, B), M.NSETS)
    finally:
        hb.free()
    want = expected(cid, k, B)
    assert len(got[0][0]) == M.proof_cap(k, M.NSETS)
    for b in range(B):
        assert got[b][0] == want[b][0], "proof %d" % b
        assert got[b][1] == want[b][1], "next challenge of proof %d" % b
    assert not st.any() and not tb_st.any()


@accelerated_oracle
def test_a_group_of_19_polynomials_at_one_point(gpu_ctx):
    """one set, 19 terms in its Horner sum: more than any chunk of 16 an implementation might inherit"""
    cid, k, B, nown = 0, 4, 2, 19
    queries = [(i, 0) for i in range(nown)]
    ops = M.operands(cid, k, B, nown, 0, 1)
    hb = K.upload(gpu_ctx, cid, k, True)
    try:
        got, st, tb_st = M.device_call(gpu_ctx, hb, cid, k, B, queries, ops, 1)
    finally:
        hb.free()
    assert got == M.model(cid, k, B, queries, ops) and not st.any() and not tb_st.any()


@pytest.mark.parametrize("form", [0, 1], ids=["canonical", "montgomery"])
def test_device_operands_give_the_host_operand_bytes(gpu_ctx, form):
    """every operand a torch tensor on the device, in either form: the same bytes, and the status read with one copy at the end"""
    import torch
    import bzh2
    cid, k, B = 0, 4, 3
    F = O.CURVE_BY_ID[cid].scalar
    n, nrand = 1 << k, (1 << k) + 2 + 2 * k
    ops = M.operands(cid, k, B)
    conv = (lambda x: x * F.R % F.p) if form == bzh2.FORM_MONTGOMERY else (lambda x: x)
    p, sh, bl, sbl, pt = M.arrays(ops, conv)

    def dev(a):
        return torch.from_numpy(np.ascontiguousarray(a).view(np.int64).copy()).to("cuda")

    hb = K.upload(gpu_ctx, cid, k, True)
    cap = M.proof_cap(k, M.NSETS)
    try:
        trs = K.primed(cid, B)
        with bzh2.TranscriptBatch(cid, B, cap, gpu_ctx) as tb:
            tb.from_host(trs)
            st_want = tb.multiopen(hb, k, p, bl, pt, M.QUERIES, list(ops[5]), shared=sh, shared_blinds=sbl, form=form)
            want, after_want = tb.proofs(), tb.squeeze()
        stride = 64 * nrand + 64   # rows further apart than they are long
        raw = np.zeros((B, stride), dtype=np.uint8)
        for b in range(B):
            raw[b, :64 * nrand] = np.frombuffer(ops[5][b], dtype=np.uint8)
        d_p, d_sh, d_bl, d_sbl, d_pt, d_raw = dev(p), dev(sh), dev(bl), dev(sbl), dev(pt), torch.from_numpy(raw).to("cuda")
        d_st = torch.full((B,), 9, dtype=torch.uint8, device="cuda")
        with bzh2.TranscriptBatch(cid, B, cap, gpu_ctx) as tb:
            tb.from_host(trs)
            assert tb.multiopen(hb, k, d_p.data_ptr(), d_bl.data_ptr(), d_pt.data_ptr(), M.QUERIES, d_raw.data_ptr(), shared=d_sh.data_ptr(),
                                shared_blinds=d_sbl.data_ptr(), form=form, mem=bzh2.MEM_DEVICE, status=d_st.data_ptr(), rng_stride=stride,
                                npolys_own=M.NOWN, npolys_shared=M.NSHARED, npoints=M.NPOINTS) is None
            got, after = tb.proofs(), tb.squeeze()
            assert not tb.status().any()
        gpu_ctx.sync()
        assert got == want and (after == after_want).all()
        assert not d_st.cpu().numpy().any() and not st_want.any()
        assert got == [w[0] for w in expected(cid, k, B)]                # and they are the model's
        for t in trs:
            t.close()
    finally:
        hb.free()


@accelerated_oracle
def test_coincident_points_flag_one_proof_and_disturb_nothing(gpu_ctx):
    """proof 1's points 0 and 1 are equal: status bit 0 for proof 1 only, proofs 0 and 2 as the model writes them, BZH_OK, and
    the ctx goes on working"""
    import bzh2
    cid, k, B = 0, 4, 3
    cv = O.CURVE_BY_ID[cid]
    ops = list(copy.deepcopy(M.operands(cid, k, B, seed=1)))
    ops[4][1][1] = ops[4][1][0]
    ops = tuple(ops)
    hb = K.upload(gpu_ctx, cid, k, True)
    try:
        got, st, tb_st = M.device_call(gpu_ctx, hb, cid, k, B, M.QUERIES, ops, M.NSETS)
        want = M.model(cid, k, B, M.QUERIES, ops, skip=(1,))
        assert list(st) == [0, 1, 0]
        assert got[0] == want[0] and got[2] == want[2]
        assert len(got[1][0]) == M.proof_cap(k, M.NSETS)
        # a later call on the ctx: one MSM against the oracle's
        g, w, u = K.srs(cid, k)
        sc = [(7 * i + 3) % cv.scalar.p for i in range((1 << k) + 2)]
        jac = gpu_ctx.msm(hb, C.ints_to_array(sc))
        pt = C.array_to_point(bzh2.jacobian_to_affine(cid, np.asarray(jac).reshape(-1, 12))[0])
        assert pt == cv.msm_pippenger(sc, list(g) + [u, w])
    finally:
        hb.free()


def test_refusals_leave_the_batch_as_it_was(gpu_ctx):
    import torch
    import bzh2
    cid, k, B = 0, 4, 3
    n, nrand = 1 << k, (1 << k) + 2 + 2 * k
    ops = M.operands(cid, k, B)
    p, sh, bl, sbl, pt = M.arrays(ops)
    rbs = list(ops[5])
    hb = K.upload(gpu_ctx, cid, k, True)
    hb_small = K.upload(gpu_ctx, cid, k - 1, True)   # a table of n / 2 + 2 points
    cap = M.proof_cap(k, M.NSETS)

    def batch(size, pcap):
        tb = bzh2.TranscriptBatch(cid, size, pcap, gpu_ctx)
        trs = K.primed(cid, size)
        tb.from_host(trs)
        for t in trs:
            t.close()
        return tb

    def refused(tb, status, call):
        with batch(tb.batch, tb.proof_cap) as twin:
            with pytest.raises(bzh2.BzhError) as e:
                call(tb)
            assert e.value.status == status
            assert tb.proof_len() == 32 and (tb.squeeze() == twin.squeeze()).all()
        tb.close()

    try:
        host_call = lambda tb, bases=hb, r=rbs: tb.multiopen(bases, k, p, bl, pt, M.QUERIES, r, shared=sh, shared_blinds=sbl)  # noqa: E731
        refused(batch(B + 1, cap), E_ARG, host_call)                                    # a batch of another size
        refused(batch(B, cap - 1), E_RANGE, host_call)                                  # proof_cap one byte short
        refused(batch(B, cap), E_ARG, lambda tb: host_call(tb, r=[r[:-1] for r in rbs]))   # rng_stride one byte short
        refused(batch(B, cap), E_ARG, lambda tb: host_call(tb, bases=hb_small))         # n + 2 larger than the table
        sizes = [B * M.NOWN * n * 32, B * M.NOWN * 32, B * M.NPOINTS * 32, B * nrand * 64]
        d = torch.zeros(sum(sizes) // 8 + 8, dtype=torch.int64, device="cuda")
        offs = [d.data_ptr() + sum(sizes[:i]) for i in range(4)]
        own_only = [(i, j) for i, j in M.QUERIES if i < M.NOWN]
        for bump in range(4):                                                           # each device pointer in turn 8 bytes off
            ptrs = list(offs)
            ptrs[bump] += 8
            refused(batch(B, cap), E_ARG, lambda tb: tb.multiopen(hb, k, ptrs[0], ptrs[1], ptrs[2], own_only, ptrs[3], form=bzh2.FORM_MONTGOMERY,
                                                                  mem=bzh2.MEM_DEVICE, rng_stride=64 * nrand, npolys_own=M.NOWN,
                                                                  npoints=M.NPOINTS))
        gpu_ctx.sync()
        assert not d.cpu().numpy().any()                                                # nothing was written either
    finally:
        hb.free()
        hb_small.free()
