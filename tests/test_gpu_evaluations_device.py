"""bzh_evaluations_batch_device on the GPU: the evaluation phase against a device-resident transcript batch must write, proof for
proof and byte for byte, what a big-int model composed of oracle pieces writes (tests/helpers/evaluations_cases.py), leave the
transcripts in the same state, and return the model's points, evaluations, h and h_blind.  Every transcript is primed first
(tests/helpers/ipa_open_device_cases.py), so the block buffer is part-filled, the state is not the initial one and the proof does
not start at offset 0.  Chained with bzh_multiopen_batch_device on device operands, with nothing read back in between, the two
calls must write what the model writes when it is carried on through the multiopen argument."""
import numpy as np
import pytest

import pasta as O
from helpers import evaluations_cases as V
from helpers import ipa_open_device_cases as K
from helpers import multiopen_cases as M
from helpers.real_parity import accelerated_oracle

pytestmark = pytest.mark.gpu

E_ARG, E_RANGE = -1, -4
NQ = len(V.QUERIES)


def primed_batch(ctx, cid, B, cap):
    import bzh2
    tb = bzh2.TranscriptBatch(cid, B, cap, ctx)
    trs = K.primed(cid, B)
    tb.from_host(trs)
    for t in trs:
        t.close()
    return tb


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64).copy()).to("cuda")


# k = 0: a single coefficient; k = 4: fewer coefficients than threads; k = 9: two strided Horner steps per thread; B = 3: a real
# batch stride and the all-zero proof.  The rows of the pieces are 3 elements further apart than they are long.
@pytest.mark.parametrize("npieces", [1, 3])
@pytest.mark.parametrize("k,B", [(0, 1), (4, 1), (9, 3)])
@pytest.mark.parametrize("cid", [0, 1], ids=["vesta", "pallas"])
def test_bytes_state_and_outputs_match_the_model(gpu_ctx, cid, k, B, npieces):
    n = 1 << k
    p, sh, hp, hb = V.arrays(V.operands(cid, k, B, npieces), k, npieces, npieces * n + 3)
    with primed_batch(gpu_ctx, cid, B, V.proof_cap(NQ)) as tb:
        pts, ev, h, hbl = tb.evaluations(k, p, V.QUERIES, shared=sh, h_pieces=hp, h_blinds=hb, npieces=npieces)
        proofs, after = tb.proofs(), V.ints(tb.squeeze())
        assert not tb.status().any()
    want = V.model(cid, k, B, npieces)
    assert len(proofs[0]) == V.proof_cap(NQ)
    for b in range(B):
        assert proofs[b] == want[b][0], "proof %d" % b
        assert after[b] == want[b][1], "next challenge of proof %d" % b
        assert V.ints(pts[b]) == want[b][2], "points of proof %d" % b
        assert V.ints(ev[b]) == want[b][3], "evaluations of proof %d" % b
        assert V.ints(h[b]) == want[b][4], "h of proof %d" % b
        assert V.ints(hbl[b]) == want[b][5], "h_blind of proof %d" % b


def test_without_pieces_and_without_out_evals(gpu_ctx):
    """npieces == 0: the h operands are not needed; a device call with out_evals NULL writes the same bytes"""
    import bzh2
    cid, k, B = 0, 4, 3
    p, sh, _, _ = V.arrays(V.operands(cid, k, B, 1), k, 0, 0)
    want = V.model(cid, k, B, 1)
    with primed_batch(gpu_ctx, cid, B, V.proof_cap(NQ)) as tb:
        pts, ev, h, hbl = tb.evaluations(k, p, V.QUERIES, shared=sh)
        assert h is None and hbl is None
        assert tb.proofs() == [w[0] for w in want] and V.ints(pts) == [w[2] for w in want] and V.ints(ev) == [w[3] for w in want]
    d_p, d_sh = dev(p), dev(sh)
    d_pts = dev(np.zeros((B, len(V.ROTATIONS), 4), dtype=np.uint64))
    with primed_batch(gpu_ctx, cid, B, V.proof_cap(NQ)) as tb:
        assert tb.evaluations(k, d_p.data_ptr(), V.QUERIES, shared=d_sh.data_ptr(), mem=bzh2.MEM_DEVICE, out_points=d_pts.data_ptr(),
                              npolys_own=V.NOWN, npolys_shared=V.NSHARED) is None
        assert tb.proofs() == [w[0] for w in want]
    gpu_ctx.sync()
    assert V.ints(d_pts.cpu().numpy().view(np.uint64)) == [w[2] for w in want]


@pytest.mark.parametrize("form", [0, 1], ids=["canonical", "montgomery"])
def test_device_operands_give_the_host_operand_bytes(gpu_ctx, form):
    """every operand and output a torch tensor on the device, in either form: the same bytes, and the outputs read with one copy at
    the end"""
    import torch
    import bzh2
    cid, k, B, npieces = 1, 9, 3, 3
    F = O.CURVE_BY_ID[cid].scalar
    n, nrot = 1 << k, len(V.ROTATIONS)
    stride = npieces * n + 5
    conv = (lambda x: x * F.R % F.p) if form == bzh2.FORM_MONTGOMERY else (lambda x: x)
    back = (lambda x: x * pow(F.R, -1, F.p) % F.p) if form == bzh2.FORM_MONTGOMERY else (lambda x: x)
    p, sh, hp, hb = V.arrays(V.operands(cid, k, B, npieces), k, npieces, stride, conv)
    with primed_batch(gpu_ctx, cid, B, V.proof_cap(NQ)) as tb:
        want_out = tb.evaluations(k, p, V.QUERIES, shared=sh, h_pieces=hp, h_blinds=hb, npieces=npieces, form=form)
        want, after_want = tb.proofs(), tb.squeeze()
    d_p, d_sh, d_hp, d_hb = dev(p), dev(sh), dev(hp), dev(hb)
    sizes = [B * nrot, B * NQ, B * n, B]                     # points | evals | h | h_blind, in elements
    d_out = torch.zeros(sum(sizes) * 4, dtype=torch.int64, device="cuda")
    offs = [d_out.data_ptr() + 32 * sum(sizes[:i]) for i in range(4)]
    with primed_batch(gpu_ctx, cid, B, V.proof_cap(NQ)) as tb:
        assert tb.evaluations(k, d_p.data_ptr(), V.QUERIES, shared=d_sh.data_ptr(), h_pieces=d_hp.data_ptr(), h_blinds=d_hb.data_ptr(),
                              npieces=npieces, h_stride=stride, form=form, mem=bzh2.MEM_DEVICE, out_points=offs[0], out_evals=offs[1],
                              out_h=offs[2], out_h_blind=offs[3], npolys_own=V.NOWN, npolys_shared=V.NSHARED) is None
        got, after = tb.proofs(), tb.squeeze()
        assert not tb.status().any()
    gpu_ctx.sync()
    out = d_out.cpu().numpy().view(np.uint64).reshape(-1, 4)                      # the one copy
    assert got == want and (after == after_want).all()
    model = V.model(cid, k, B, npieces)
    assert got == [w[0] for w in model]                                           # and they are the model's
    at = 0
    for i, (size, host) in enumerate(zip(sizes, want_out)):
        mine = out[at:at + size]
        assert (mine == np.asarray(host).reshape(-1, 4)).all(), "output %d" % i
        at += size
    assert [back(v) for v in V.ints(out[:B * nrot])] == [v for w in model for v in w[2]]
    assert [back(v) for v in V.ints(out[B * nrot + B * NQ:B * nrot + B * NQ + B * n])] == [v for w in model for v in w[4]]


@pytest.mark.parametrize("B", [1, 3])
@accelerated_oracle
def test_chained_with_the_multiopen_on_device_operands(gpu_ctx, B):
    """evaluations, then multiopen, on device operands with nothing read back in between: out_points is the second call's
    `points`, out_h one more own polynomial of its table and out_h_blind that polynomial's blind.  A single proof's out_h and
    out_h_blind ARE the table's last row and the blinds' last entry; a batch's are copied there on the device."""
    import torch
    import bzh2
    cid, k, npieces = 0, 4, 3
    F = O.CURVE_BY_ID[cid].scalar
    n, nrot, MONT = 1 << k, len(V.ROTATIONS), bzh2.FORM_MONTGOMERY
    nrand = n + 2 + 2 * k
    mont = lambda x: x * F.R % F.p   # noqa: E731
    ops = V.operands(cid, k, B, npieces)
    polys, shared, pieces, hblinds = ops
    rng = np.random.default_rng(77 + B)
    blinds = [[int(v) for v in rng.integers(1, 2 ** 62, V.NOWN)] for _ in range(B)]
    sblinds = [int(v) for v in rng.integers(1, 2 ** 62, V.NSHARED)]
    rbs = [rng.bytes(64 * nrand) for _ in range(B)]
    # the multiopen's table: the own polynomials, then h; its queries: every evaluation query at its rotation's number, then h at x
    # (with h as own polynomial NOWN of both calls, the shared ids move up by one)
    # The multiopen needs the points of a set distinct: at n = 16, omega^INT32_MIN is omega^0, so that rotation becomes 5 here.
    ev_queries = [(pid if pid < V.NOWN else pid + 1, 5 if rot == V.INT32_MIN else rot) for pid, rot in V.QUERIES]
    point_of = V.plan(ev_queries, V.NOWN + 1 + V.NSHARED)[1]
    mo_queries = [(pid, pt) for (pid, _), pt in zip(ev_queries, point_of)] + [(V.NOWN, 0)]
    nsets = len(M.oracle_sets(mo_queries)[0])
    cap = V.proof_cap(NQ) + M.proof_growth(k, nsets)
    _, sh, hp, hb = V.arrays(ops, k, npieces, npieces * n + 3, mont)
    table = np.zeros((B, V.NOWN + 1, n, 4), dtype=np.uint64)
    bl = np.zeros((B, V.NOWN + 1, 4), dtype=np.uint64)
    for b in range(B):
        for i in range(V.NOWN):
            table[b, i] = V.lim(polys[b][i], mont)
        bl[b, :V.NOWN] = V.lim(blinds[b], mont)
    d_table, d_bl, d_sh, d_sbl, d_hp, d_hb = dev(table), dev(bl), dev(sh), dev(V.lim(sblinds, mont)), dev(hp), dev(hb)
    d_pts = dev(np.zeros((B, nrot, 4), dtype=np.uint64))
    d_raw = torch.from_numpy(np.frombuffer(b"".join(rbs), dtype=np.uint8).copy()).to("cuda")
    d_st = torch.full((B,), 9, dtype=torch.uint8, device="cuda")
    if B == 1:
        d_h = d_hbl = None
        out_h, out_hbl = d_table.data_ptr() + V.NOWN * n * 32, d_bl.data_ptr() + V.NOWN * 32
    else:
        d_h, d_hbl = dev(np.zeros((B, n, 4), dtype=np.uint64)), dev(np.zeros((B, 4), dtype=np.uint64))
        out_h, out_hbl = d_h.data_ptr(), d_hbl.data_ptr()
    hbases = K.upload(gpu_ctx, cid, k, True)
    try:
        with primed_batch(gpu_ctx, cid, B, cap) as tb:
            # the table's h slot is an own polynomial no evaluation query reads
            tb.evaluations(k, d_table.data_ptr(), ev_queries, shared=d_sh.data_ptr(), h_pieces=d_hp.data_ptr(), h_blinds=d_hb.data_ptr(),
                           npieces=npieces, h_stride=npieces * n + 3, form=MONT, mem=bzh2.MEM_DEVICE, out_points=d_pts.data_ptr(),
                           out_h=out_h, out_h_blind=out_hbl, npolys_own=V.NOWN + 1, npolys_shared=V.NSHARED)
            if B > 1:   # device to device, ordered between the two streams; no byte comes to the host
                gpu_ctx.sync()
                d_table.view(B, V.NOWN + 1, n, 4)[:, V.NOWN] = d_h.view(B, n, 4)
                d_bl.view(B, V.NOWN + 1, 4)[:, V.NOWN] = d_hbl.view(B, 4)
                torch.cuda.synchronize()
            tb.multiopen(hbases, k, d_table.data_ptr(), d_bl.data_ptr(), d_pts.data_ptr(), mo_queries, d_raw.data_ptr(), shared=d_sh.data_ptr(),
                         shared_blinds=d_sbl.data_ptr(), form=MONT, mem=bzh2.MEM_DEVICE, status=d_st.data_ptr(), rng_stride=64 * nrand,
                         npolys_own=V.NOWN + 1, npolys_shared=V.NSHARED, npoints=nrot)
            proofs, after = tb.proofs(), V.ints(tb.squeeze())
            assert not tb.status().any()
        gpu_ctx.sync()
        assert not d_st.cpu().numpy().any()
    finally:
        hbases.free()
    for b in range(B):
        T, points, _, h, h_blind = V.model_transcript(cid, k, b, ev_queries, polys[b] + [[0] * n], shared, pieces[b], hblinds[b])
        V.multiopen_continue(cid, k, T, mo_queries, polys[b] + [h], shared, blinds[b] + [h_blind], sblinds, points, rbs[b])
        assert len(proofs[b]) == cap
        assert proofs[b] == bytes(T.proof), "proof %d" % b
        assert after[b] == T.squeeze_challenge(), "next challenge of proof %d" % b


def test_refusals_leave_the_batch_as_it_was(gpu_ctx):
    import torch
    import bzh2
    cid, k, B, npieces = 0, 4, 3, 3
    n, nrot = 1 << k, len(V.ROTATIONS)
    stride = npieces * n + 3
    p, sh, hp, hb = V.arrays(V.operands(cid, k, B, npieces), k, npieces, stride)
    cap = V.proof_cap(NQ)

    def refused(tb, status, call):
        with primed_batch(gpu_ctx, cid, tb.batch, tb.proof_cap) as twin:
            with pytest.raises(bzh2.BzhError) as e:
                call(tb)
            assert e.value.status == status
            assert tb.proof_len() == 32 and (tb.squeeze() == twin.squeeze()).all()
        tb.close()

    host_call = lambda tb, **kw: tb.evaluations(**{**dict(k=k, polys=p, queries=V.QUERIES, shared=sh, h_pieces=hp, h_blinds=hb,  # noqa: E731
                                                          npieces=npieces), **kw})
    refused(primed_batch(gpu_ctx, cid, B + 1, cap), E_ARG, host_call)                      # a batch of another size
    refused(primed_batch(gpu_ctx, cid, B, cap - 1), E_RANGE, host_call)                    # proof_cap one byte short
    refused(primed_batch(gpu_ctx, cid, B, cap), E_ARG, lambda tb: host_call(tb, h_stride=npieces * n - 1))   # h_stride one short
    # polys | shared | pieces | their blinds | points | evals | h | h_blind, in elements
    sizes = [B * V.NOWN * n, V.NSHARED * n, B * stride, B * npieces, B * nrot, B * NQ, B * n, B]
    d = torch.zeros(sum(sizes) * 4 + 8, dtype=torch.int64, device="cuda")
    offs = [d.data_ptr() + 32 * sum(sizes[:i]) for i in range(8)]
    for bump in range(8):                                                                   # each device pointer in turn 8 bytes off
        a = list(offs)
        a[bump] += 8
        refused(primed_batch(gpu_ctx, cid, B, cap), E_ARG,
                lambda tb: tb.evaluations(k, a[0], V.QUERIES, shared=a[1], h_pieces=a[2], h_blinds=a[3], npieces=npieces, h_stride=stride,
                                          form=bzh2.FORM_MONTGOMERY, mem=bzh2.MEM_DEVICE, out_points=a[4], out_evals=a[5], out_h=a[6],
                                          out_h_blind=a[7], npolys_own=V.NOWN, npolys_shared=V.NSHARED))
    for big_k in (33, 40):                                                                  # k above the two-adicity
        refused(primed_batch(gpu_ctx, cid, B, cap), E_ARG,
                lambda tb: tb.evaluations(big_k, offs[0], V.QUERIES, shared=offs[1], h_pieces=offs[2], h_blinds=offs[3], npieces=npieces,
                                          h_stride=1 << 62, form=bzh2.FORM_MONTGOMERY, mem=bzh2.MEM_DEVICE, out_points=offs[4],
                                          out_evals=offs[5], out_h=offs[6], out_h_blind=offs[7], npolys_own=V.NOWN, npolys_shared=V.NSHARED))
    gpu_ctx.sync()
    assert not d.cpu().numpy().any()                                                        # nothing was written either
