"""bzh_grand_products_batch_device on the GPU: the permutation and lookup grand products against a device-resident transcript
batch must write, proof for proof and byte for byte, what the oracle prover writes (tests/helpers/products_cases.py cuts
halo2_oracle.create_proof's captured state at the grand-product boundary and carries the integer model), leave the transcripts in
the same state and return the oracle's z, its coefficients and its blinds.  The device batch is built by replaying the oracle
proof's prefix through TranscriptBatch with theta, beta, gamma squeezed at their places, so the challenge operands of the device
variant are the squeeze outputs themselves.  Every comparison is exact."""
import numpy as np
import pytest

import pasta as O
from helpers import products_cases as G
from helpers import vanishing_cases as V
from helpers.real_parity import accelerated_oracle

pytestmark = pytest.mark.gpu

E_ARG, E_RANGE = -1, -4
F = O.FP
P = F.p
MONT = lambda x: x * F.R % P          # noqa: E731
UNMONT = lambda x: x * pow(F.R, -1, P) % P   # noqa: E731


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64).copy()).to("cuda")


def xy(pt):
    import bzh2
    x, y = (0, 0) if pt is None else pt
    return np.concatenate([bzh2.int_to_limbs(x), bzh2.int_to_limbs(y)])


def replayed_batch(ctx, bounds, cap, d_ch=None):
    """a device batch after the oracle proofs' prefixes; the squeezes (theta, beta, gamma, in this order) go to the device pointers
    d_ch (Montgomery) or come back as canonical host arrays"""
    import bzh2
    B = len(bounds)
    tb = bzh2.TranscriptBatch(bzh2.CURVE_VESTA, B, cap, ctx)
    host, nsq = [], 0
    for i, (op, _) in enumerate(bounds[0].prefix_ops):
        vals = [s.prefix_ops[i][1] for s in bounds]
        if op == "squeeze":
            if d_ch is None:
                host.append(tb.squeeze())
                assert V.ints(host[-1]) == vals
            else:
                tb.squeeze(form=bzh2.FORM_MONTGOMERY, mem=bzh2.MEM_DEVICE, out=d_ch[nsq])
            nsq += 1
        elif op.endswith("point"):
            getattr(tb, op + "s")(np.stack([xy(v) for v in vals]).reshape(B, 1, 8))
        else:
            getattr(tb, op + "s")(np.stack([bzh2.int_to_limbs(v) for v in vals]).reshape(B, 1, 4))
    assert nsq == 3 and tb.proofs() == [s.prefix_proof for s in bounds]
    return tb, host


def make_key(ctx, case):
    import bzh2
    from bzh2 import native as N
    return N.NativeProvingKey(ctx, case[2], bzh2.CURVE_VESTA, *case[3])


def flat(a):
    return np.asarray(V.ints(a), dtype=object).reshape(-1).tolist()


def run_host(ctx, pk, bounds, shape, cap, ops=None, challenges=None):
    """the call on canonical host operands: ([z, z_polys, z_blinds as flat integer lists, status], proofs, the next squeeze, the
    sticky status).  ops: other operand arrays than the bounds' own; challenges: (beta, gamma) integer lists instead of the squeezed
    ones"""
    ops = G.operand_arrays(bounds) if ops is None else ops
    tb, ch = replayed_batch(ctx, bounds, cap)
    beta, gamma = (ch[1], ch[2]) if challenges is None else (V.lim(challenges[0]), V.lim(challenges[1]))
    with tb:
        z, zp, zb, st = tb.grand_products(pk, *ops, beta, gamma, [s.rng for s in bounds], shape=shape)
        return [flat(z), flat(zp), flat(zb), st], tb.proofs(), V.ints(tb.squeeze()), tb.status()


def run_device(ctx, pk, bounds, shape, cap, ops=None):
    """the call on Montgomery device operands, beta and gamma squeezed straight into the device memory it reads; ops: other operand
    arrays (canonical limbs, as operand_arrays gives them) than the bounds' own"""
    import torch
    import bzh2
    B = len(bounds)
    n, nz, nd = shape[0], shape[5], shape[7]
    if ops is None:
        ops = G.operand_arrays(bounds, MONT)
    else:
        ops = [None if a is None else V.lim([MONT(v) for v in V.ints(a.reshape(-1, 4))]) for a in ops]
    ops = [None if a is None else dev(a) for a in ops]
    d_ch = torch.zeros(3 * B * 4, dtype=torch.int64, device="cuda")
    sizes = [B * nz * n, B * nz * n, B * nz]
    d_out = torch.zeros(sum(sizes) * 4, dtype=torch.int64, device="cuda")
    offs = [d_out.data_ptr() + 32 * sum(sizes[:j]) for j in range(3)]
    d_rng = torch.from_numpy(np.frombuffer(b"".join(s.rng for s in bounds), dtype=np.uint8).copy()).to("cuda")
    d_st = torch.full((B + 1,), 9, dtype=torch.uint8, device="cuda")
    ptr = lambda t: 0 if t is None else t.data_ptr()   # noqa: E731
    tb, _ = replayed_batch(ctx, bounds, cap, [d_ch.data_ptr() + 32 * B * j for j in range(3)])
    with tb:
        assert tb.grand_products(pk, ptr(ops[0]), ptr(ops[1]), ptr(ops[2]), ptr(ops[3]), d_ch.data_ptr() + 32 * B, d_ch.data_ptr() + 64 * B,
                                 d_rng.data_ptr(), form=bzh2.FORM_MONTGOMERY, mem=bzh2.MEM_DEVICE, out_z=offs[0], out_z_polys=offs[1],
                                 out_z_blinds=offs[2], status=d_st.data_ptr() + 1, rng_stride=64 * nd) is None
        proofs, after, sticky = tb.proofs(), V.ints(tb.squeeze()), tb.status()
    ctx.sync()
    vals = [UNMONT(v) for v in V.ints(d_out.cpu().numpy().view(np.uint64).reshape(-1, 4))]
    outs, at = [], 0
    for size in sizes:
        outs.append(vals[at:at + size])
        at += size
    st = d_st.cpu().numpy()
    assert st[0] == 9                                       # the byte before an odd-aligned status array is not touched
    return outs + [st[1:]], proofs, after, sticky


def expect(bounds, want, outs, got, after, only=None):
    """the run's outputs, bytes and next squeeze against the model's, for the proofs in `only` (all of them when None)"""
    B = len(bounds)
    n, nz = len(want[0][2][0]), len(want[0][2])
    for b in range(B) if only is None else only:
        assert got[b] == bounds[b].prefix_proof + want[b][0], "proof %d" % b
        assert after[b] == want[b][1], "squeeze after proof %d" % b
        assert outs[0][b * nz * n:(b + 1) * nz * n] == [v for z in want[b][2] for v in z], "z of proof %d" % b
        assert outs[1][b * nz * n:(b + 1) * nz * n] == [v for c in want[b][3] for v in c], "z_polys of proof %d" % b
        assert outs[2][b * nz:(b + 1) * nz] == want[b][4], "blinds of proof %d" % b
        assert int(outs[3][b]) == want[b][5], "status of proof %d" % b


def both_variants(ctx, case, prove=False):
    cs, keys, _, _, bounds, proofs, want = case
    nz = bounds[0].nz
    cap = len(bounds[0].prefix_proof) + 32 * nz
    for b, s in enumerate(bounds):                           # the model is the oracle proof's own next bytes
        assert want[b][0] == proofs[b][len(s.prefix_proof):cap] and want[b][5] == 0
    pk = make_key(ctx, case)
    try:
        shape = pk.grand_products_plan()
        assert shape[0] == cs.n and shape[5] == nz and shape[7] * 64 == len(bounds[0].rng)
        results = []
        for run in (run_device, run_host):
            outs, got, after, sticky = run(ctx, pk, bounds, shape, cap)
            expect(bounds, want, outs, got, after)
            assert not sticky.any()
            results.append((outs[:3], got, after))
        assert results[0] == results[1]
        if prove:   # the arena is shared and the cached programs undisturbed: bzh_prove_batch on this key still returns the oracle's proof
            n = cs.n
            adv = np.stack([np.stack([V.lim(list(c) + [0] * (n - len(c))) for c in s.v.advice]) for s in bounds])
            assert pk.prove_batch(adv, [s.v.instance for s in bounds], [s.v.rbytes[:pk.rng_bytes] for s in bounds]) == proofs
    finally:
        pk.close()


# (4, no lookup): n = 16, below a workgroup; degree 3 -> one column per set, nsets = 4, the longest carry chain.  (5, lookup, 3
# proofs): sets and a lookup, the per-proof strides and the [b][nz][n] scatter.  (6, degree 9): chunk_len 7, one set with a short
# chunk.  (9, 2 proofs): n = 512, two workgroups of k_gp_factors per (product, proof); taken from the oracle (about 2 s)
@pytest.mark.parametrize("k,with_lookup,degree,B", [(4, False, None, 1), (5, True, None, 3), (6, True, 9, 2), (9, True, None, 2)])
@accelerated_oracle
def test_parity_with_the_oracle(gpu_ctx, oracle_c, k, with_lookup, degree, B):
    both_variants(gpu_ctx, G.case(k, with_lookup, degree, B), prove=k == 5)


@accelerated_oracle
def test_advice_instance_and_fixed_columns_in_the_permutation(gpu_ctx, oracle_c):
    """the sample circuit's permutation has no fixed column: here its table column is in the permutation, with a copy into it; the
    column is read from the key with stride 0 in every proof"""
    case = G.all_kinds_case()
    assert {c[0] for c in case[0].perm_columns} == {"advice", "instance", "fixed"}
    both_variants(gpu_ctx, case)


@accelerated_oracle
def test_a_witness_that_does_not_close(gpu_ctx, oracle_c):
    """B = 3, k = 5 with the lookup: in proof 1 the advice cell that two copy constraints start from is changed.  The call returns
    OK; proof 1's bytes and outputs are the model's and its status and sticky bits are set; proofs 0 and 2 are byte-identical to
    the untouched run and their status is 0.  An unsatisfied witness, not a fault."""
    case = G.case(5, True, None, 3)
    cs, keys, _, _, bounds, _, want = case
    nz = bounds[0].nz
    cap = len(bounds[0].prefix_proof) + 32 * nz
    row = max(1, min(3, cs.usable_rows - 4))                 # sample_circuit: advice 2 at this row is copied to advice 0 and the instance
    cols = dict(bounds[1].cols, advice=[list(c) for c in bounds[1].cols["advice"]])
    cols["advice"][2][row] = (cols["advice"][2][row] + 1) % P
    bad = G.Boundary()
    bad.__dict__.update(bounds[1].__dict__, cols=cols)
    want_bad = G.model(keys, bad, bad.beta, bad.gamma, bad.draws)
    assert want_bad[5] == 1 and want_bad[2][-1] == want[1][2][-1]          # (the lookup's product is not touched)
    mixed = [bounds[0], bad, bounds[2]]
    ops = G.operand_arrays(mixed)
    pk = make_key(gpu_ctx, case)
    try:
        shape = pk.grand_products_plan()
        clean = run_host(gpu_ctx, pk, bounds, shape, cap)
        expect(bounds, want, *clean[:3])
        for run in (run_host, run_device):
            outs, got, after, sticky = run(gpu_ctx, pk, bounds, shape, cap, ops)
            expect(mixed, [want[0], want_bad, want[2]], outs, got, after)
            assert [int(s) for s in outs[3]] == [0, 1, 0] and [int(s) & 1 for s in sticky] == [0, 1, 0]
            assert got[0] == clean[1][0] and got[2] == clean[1][2] and after[0] == clean[2][0] and after[2] == clean[2][2]
    finally:
        pk.close()


@accelerated_oracle
def test_a_zero_denominator(gpu_ctx, oracle_c):
    """host variant, beta and gamma chosen by the caller: advice 0 of proof 0 is -(beta * sigma + gamma) at a row below usable, so
    that row's denominator is 0.  The batch inversion leaves it 0 (upstream's batch_invert): the set's z is 0 from the next row on
    and the sets after it are 0 throughout, exactly as the model says; proof 1 is the model's too, and closes"""
    case = G.case(5, True, None, 2)
    cs, keys, _, _, bounds, _, _ = case
    n, bf, nz = cs.n, cs.blinding_factors, bounds[0].nz
    cap = len(bounds[0].prefix_proof) + 32 * nz
    beta, gamma = [0x1234567 + 11 * b for b in range(2)], [0x7654321 + 13 * b for b in range(2)]
    row = 7
    assert row < cs.usable_rows and cs.perm_columns[0] == ("advice", 0)
    cols = dict(bounds[0].cols, advice=[list(c) for c in bounds[0].cols["advice"]])
    cols["advice"][0][row] = -(beta[0] * keys.sigma[0][row] + gamma[0]) % P
    zero = G.Boundary()
    zero.__dict__.update(bounds[0].__dict__, cols=cols)
    mixed = [zero, bounds[1]]
    want = [G.model(keys, s, beta[b], gamma[b], s.draws) for b, s in enumerate(mixed)]
    assert want[0][2][0][row] != 0 and not any(want[0][2][0][row + 1:n - bf]) and want[0][5] == 1
    assert not any(want[0][2][1][:n - bf]) and all(want[0][2][1][n - bf:])   # the next set starts from 0; its blinding rows are draws
    assert want[1][5] == 0
    pk = make_key(gpu_ctx, case)
    try:
        outs, got, after, sticky = run_host(gpu_ctx, pk, bounds, pk.grand_products_plan(), cap, G.operand_arrays(mixed), (beta, gamma))
        expect(mixed, want, outs, got, after)
        assert [int(s) & 1 for s in sticky] == [1, 0]
    finally:
        pk.close()


@accelerated_oracle
def test_chained_with_the_vanishing_argument(gpu_ctx, oracle_c):
    """k = 5 with the lookup, B = 2, Montgomery device operands: grand_products and then vanishing on one device batch, out_z_polys
    passed as z_polys where it lies; the bytes are the oracle proof's over both phases"""
    import torch
    import bzh2
    case = G.case(5, True, None, 2)
    cs, keys, _, _, bounds, proofs, _ = case
    states = [s.v for s in bounds]
    B, nz = 2, bounds[0].nz
    pk = make_key(gpu_ctx, case)
    try:
        gshape, (vshape, _) = pk.grand_products_plan(), pk.vanishing_plan()
        n, en, _, _, _, _, npieces, vnd = vshape
        cap = len(bounds[0].prefix_proof) + 32 * nz + 32 * (1 + npieces)
        gops = [None if a is None else dev(a) for a in G.operand_arrays(bounds, MONT)]
        vops = [None if a is None else dev(a) for a in V.operand_arrays(states, MONT)[:3]]
        d_ch = torch.zeros(3 * B * 4, dtype=torch.int64, device="cuda")
        theta, beta, gamma = (d_ch.data_ptr() + 32 * B * j for j in range(3))
        sizes = [B * nz * n, B * nz, B * n, B, B * en, B * npieces]
        d_out = torch.zeros(sum(sizes) * 4, dtype=torch.int64, device="cuda")
        zp, zb, rp, rb, h, hb = (d_out.data_ptr() + 32 * sum(sizes[:j]) for j in range(6))
        d_grng = torch.from_numpy(np.frombuffer(b"".join(s.rng for s in bounds), dtype=np.uint8).copy()).to("cuda")
        d_vrng = torch.from_numpy(np.frombuffer(b"".join(s.rng for s in states), dtype=np.uint8).copy()).to("cuda")
        d_st = torch.full((2 * B,), 9, dtype=torch.uint8, device="cuda")
        ptr = lambda t: 0 if t is None else t.data_ptr()   # noqa: E731
        tb, _ = replayed_batch(gpu_ctx, bounds, cap, [theta, beta, gamma])
        with tb:
            tb.grand_products(pk, ptr(gops[0]), ptr(gops[1]), ptr(gops[2]), ptr(gops[3]), beta, gamma, d_grng.data_ptr(), form=bzh2.FORM_MONTGOMERY,
                              mem=bzh2.MEM_DEVICE, out_z=None, out_z_polys=zp, out_z_blinds=zb, status=d_st.data_ptr(), rng_stride=64 * gshape[7])
            tb.vanishing(pk, ptr(vops[0]), ptr(vops[1]), ptr(vops[2]), zp, theta, beta, gamma, d_vrng.data_ptr(), form=bzh2.FORM_MONTGOMERY,
                         mem=bzh2.MEM_DEVICE, out_random=rp, out_random_blind=rb, out_h=h, out_h_blinds=hb, status=d_st.data_ptr() + B,
                         rng_stride=len(states[0].rng))
            got, sticky = tb.proofs(), tb.status()
        gpu_ctx.sync()
        assert len(states[0].rng) >= 64 * vnd
        for b in range(B):
            assert got[b] == proofs[b][:cap], "proof %d" % b
        assert not sticky.any() and not d_st.cpu().numpy().any()
        # without out_z the products were transformed in place: out_z_polys holds the oracle's coefficients
        vals = [UNMONT(v) for v in V.ints(d_out.cpu().numpy().view(np.uint64).reshape(-1, 4)[:B * nz * n])]
        assert vals == [v for s in states for c in s.z_polys for v in c]
    finally:
        pk.close()


@accelerated_oracle
def test_refusals_leave_the_batch_as_it_was(gpu_ctx, oracle_c):
    import torch
    import bzh2
    case = G.case(5, True, None, 3)
    cs, keys, _, _, bounds, _, _ = case
    B, nz = 3, bounds[0].nz
    cap = len(bounds[0].prefix_proof) + 32 * nz
    pk = make_key(gpu_ctx, case)
    try:
        shape = pk.grand_products_plan()
        n, nl, nd = shape[0], shape[4], shape[7]
        na, ni = cs.num_advice, cs.num_instance
        ops = G.operand_arrays(bounds)

        def refused(sts, cap_, status, call):
            tb, ch = replayed_batch(gpu_ctx, sts, cap_)
            twin, _ = replayed_batch(gpu_ctx, sts, cap_)
            with tb, twin:
                before = tb.proof_len()
                with pytest.raises(bzh2.BzhError) as e:
                    call(tb, ch)
                assert e.value.status == status
                assert tb.proof_len() == before and (tb.squeeze() == twin.squeeze()).all()   # nothing was absorbed

        host = lambda rngs: (lambda tb, ch: tb.grand_products(pk, *ops, ch[1], ch[2], rngs, shape=shape))   # noqa: E731
        rngs = [s.rng for s in bounds]
        refused(bounds, cap - 1, E_RANGE, host(rngs))                                    # proof_cap one byte short
        refused(bounds, cap, E_ARG, host([r[:-64] for r in rngs]))                       # rng_stride one draw short
        refused(bounds[:2], cap, E_ARG, host(rngs))                                      # a batch of another size
        sizes = [B * na * n, B * ni * n, B * nl * 2 * n, B * nl * 2 * n, B, B, B * nd * 2, B * nz * n, B * nz * n, B * nz]
        d = torch.zeros(sum(sizes) * 4 + 8, dtype=torch.int64, device="cuda")
        offs = [d.data_ptr() + 32 * sum(sizes[:j]) for j in range(len(sizes))]

        def device_call(p, batch=None):
            return lambda tb, ch: tb.grand_products(pk, p[0], p[1], p[2], p[3], p[4], p[5], p[6], form=bzh2.FORM_MONTGOMERY, mem=bzh2.MEM_DEVICE,
                                                    out_z=p[7], out_z_polys=p[8], out_z_blinds=p[9], rng_stride=64 * nd, batch=batch)

        for bump in range(len(sizes)):                                                   # each device pointer in turn 8 bytes off
            p = list(offs)
            p[bump] += 8
            refused(bounds, cap, E_ARG, device_call(p))
        # batch * nz = 21846 * 3 > 65535: the commitments would not fit one launch's grid.  Refused before anything is read, so the
        # operand pointers need not hold that many proofs
        big = 65535 // nz + 1
        with bzh2.TranscriptBatch(bzh2.CURVE_VESTA, big, 32 * nz, gpu_ctx) as tb:
            with pytest.raises(bzh2.BzhError) as e:
                device_call(offs, big)(tb, None)
            assert e.value.status == E_ARG and tb.proof_len() == 0
        gpu_ctx.sync()
        assert not d.cpu().numpy().any()                                                 # nothing was written either
    finally:
        pk.close()
