"""bzh_vanishing_batch_device on the GPU: the vanishing argument against a device-resident transcript batch must write, proof for
proof and byte for byte, what the oracle prover writes (tests/helpers/vanishing_cases.py takes halo2_oracle.create_proof's state
at the vanishing boundary), leave the transcripts in the same state and return the oracle's h.  The device batch is built by
replaying the oracle proof's prefix through TranscriptBatch with theta, beta, gamma squeezed at their places, so the challenge
operands of the device variant are the squeeze outputs themselves.

Two of the shapes the issue names cannot do what it expects of them, by the call's own contract, and are tested against the
contract instead:
  k = 4 without a lookup has degree 3: its extended domain is 2n = 32 rows, below VM v2's 128-row workgroup, so the key has no
  VM v2 program (bzh_prove_batch folds through VM v1 there) and the call is BZH_E_RANGE with nothing absorbed.  The circuit
  without a lookup is compared with the oracle at k = 6, the smallest size at which it has a VM v2 program (en = 128);
  degrees 3, 5 and 9 give npieces * n == en: there is no coefficient at or above npieces * n and bit 0 can never be set.  The
  unsatisfied witness therefore runs at k = 5 with min_degree 6 (en = 8n = 256, npieces = 5), and the Shot key (degree 9:
  n = 2048, en = 16384, npieces = 8) reports 0 under every flavour."""
import numpy as np
import pytest

import pasta as O
from helpers import vanishing_cases as V
from helpers.real_parity import accelerated_oracle

pytestmark = pytest.mark.gpu

E_ARG, E_RANGE = -1, -4
F = O.FP
MONT = lambda x: x * F.R % F.p          # noqa: E731
UNMONT = lambda x: x * pow(F.R, -1, F.p) % F.p   # noqa: E731


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64).copy()).to("cuda")


def xy(pt):
    import bzh2
    x, y = (0, 0) if pt is None else pt
    return np.concatenate([bzh2.int_to_limbs(x), bzh2.int_to_limbs(y)])


def replayed_batch(ctx, states, cap, d_ch=None):
    """a device batch after the oracle proofs' prefixes; the squeezes (theta, beta, gamma, in this order) go to the device pointers
    d_ch (Montgomery) or come back as canonical host arrays"""
    import bzh2
    B = len(states)
    tb = bzh2.TranscriptBatch(bzh2.CURVE_VESTA, B, cap, ctx)
    host, nsq = [], 0
    for i, (op, _) in enumerate(states[0].prefix_ops):
        vals = [s.prefix_ops[i][1] for s in states]
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
    assert nsq == 3 and tb.proofs() == [s.prefix_proof for s in states]
    return tb, host


def make_key(ctx, case):
    import bzh2
    from bzh2 import native as N
    _, _, circ, (g, w, u), _, _ = case
    return N.NativeProvingKey(ctx, circ, bzh2.CURVE_VESTA, g, w, u)


def run_host(ctx, pk, states, shape, cap, adv=None):
    """the call on canonical host operands: (outputs, proofs, the next squeeze, the sticky status)"""
    a, i, lk, z = V.operand_arrays(states)
    tb, ch = replayed_batch(ctx, states, cap)
    with tb:
        out = tb.vanishing(pk, a if adv is None else adv, i, lk, z, ch[0], ch[1], ch[2], [s.rng for s in states], shape=shape)
        return out, tb.proofs(), V.ints(tb.squeeze()), tb.status()


def run_device(ctx, pk, states, shape, cap, adv=None):
    """the call on Montgomery device operands, the challenges squeezed straight into the device memory it reads; adv: other
    advice polynomials (canonical limbs, as operand_arrays gives them) than the states' own"""
    import torch
    import bzh2
    B = len(states)
    n, en, _, _, _, _, npieces, nd = shape
    ops = [None if x is None else dev(x) for x in V.operand_arrays(states, MONT)]
    if adv is not None:
        ops[0] = dev(V.lim([MONT(v) for v in V.ints(adv.reshape(-1, 4))]))
    d_ch = torch.zeros(3 * B * 4, dtype=torch.int64, device="cuda")
    sizes = [B * n, B, B * en, B * npieces]
    d_out = torch.zeros(sum(sizes) * 4, dtype=torch.int64, device="cuda")
    offs = [d_out.data_ptr() + 32 * sum(sizes[:j]) for j in range(4)]
    d_rng = torch.from_numpy(np.frombuffer(b"".join(s.rng for s in states), dtype=np.uint8).copy()).to("cuda")
    d_st = torch.full((B + 1,), 9, dtype=torch.uint8, device="cuda")
    ptr = lambda t: 0 if t is None else t.data_ptr()   # noqa: E731
    tb, _ = replayed_batch(ctx, states, cap, [d_ch.data_ptr() + 32 * B * j for j in range(3)])
    with tb:
        assert tb.vanishing(pk, ptr(ops[0]), ptr(ops[1]), ptr(ops[2]), ptr(ops[3]), d_ch.data_ptr(), d_ch.data_ptr() + 32 * B,
                            d_ch.data_ptr() + 64 * B, d_rng.data_ptr(), form=bzh2.FORM_MONTGOMERY, mem=bzh2.MEM_DEVICE, out_random=offs[0],
                            out_random_blind=offs[1], out_h=offs[2], out_h_blinds=offs[3], status=d_st.data_ptr() + 1,
                            rng_stride=64 * nd) is None
        proofs, after, sticky = tb.proofs(), V.ints(tb.squeeze()), tb.status()
    ctx.sync()
    flat = [UNMONT(v) for v in V.ints(d_out.cpu().numpy().view(np.uint64).reshape(-1, 4))]
    outs, at = [], 0
    for size in sizes:
        outs.append(flat[at:at + size])
        at += size
    st = d_st.cpu().numpy()
    assert st[0] == 9                                       # the byte before an odd-aligned status array is not touched
    return outs + [st[1:]], proofs, after, sticky


@pytest.mark.parametrize("k,with_lookup,degree,B", [(4, False, None, 1), (6, False, None, 1), (5, True, None, 3), (6, True, 9, 2)])
@accelerated_oracle
def test_parity_with_the_oracle(gpu_ctx, oracle_c, k, with_lookup, degree, B):
    case = V.case(k, with_lookup, degree, B)
    cs, keys, _, _, states, proofs = case
    n, npieces = cs.n, cs.degree - 1
    grow = 32 * (1 + npieces)
    cap = len(states[0].prefix_proof) + grow
    pk = make_key(gpu_ctx, case)
    try:
        if keys.dom.en % 128:          # (k = 4: no VM v2 program on this key; see the module's text)
            import bzh2
            a, i, lk, z = V.operand_arrays(states)
            tb, ch = replayed_batch(gpu_ctx, states, cap)
            twin, _ = replayed_batch(gpu_ctx, states, cap)
            with tb, twin:
                before = tb.proof_len()
                with pytest.raises(bzh2.BzhError) as e:
                    tb.vanishing(pk, a, i, lk, z, ch[0], ch[1], ch[2], [s.rng for s in states],
                                 shape=(n, keys.dom.en, 3, 1, 1, 0, npieces, 0))
                assert e.value.status == E_RANGE
                assert tb.proof_len() == before and (tb.squeeze() == twin.squeeze()).all()   # nothing was absorbed
            return
        shape, _ = pk.vanishing_plan()
        want = [V.model(keys, s) for s in states]
        for b in range(B):                                   # the model is the oracle proof's own next bytes and its x
            at = len(states[b].prefix_proof)
            assert want[b][0] == proofs[b][at:at + grow] and want[b][3] == 0
        results = []
        for run in (run_device, run_host):
            outs, got, after, sticky = run(gpu_ctx, pk, states, shape, cap)
            for b in range(B):
                assert got[b] == states[b].prefix_proof + want[b][0], "proof %d" % b
                assert after[b] == want[b][1], "x of proof %d" % b
            assert not sticky.any() and not np.asarray(outs[4]).any()
            flat = [np.asarray(V.ints(o) if isinstance(o, np.ndarray) else o, dtype=object).reshape(-1).tolist() for o in outs[:4]]
            assert flat[0] == [v for s in states for v in s.random_poly]
            assert flat[1] == [s.random_blind for s in states]
            assert flat[2] == [v for w in want for v in w[2]]
            assert flat[3] == [v for s in states for v in s.h_blinds]
            results.append((flat, got, after))
        assert results[0] == results[1]
        # the arena is shared and the cached programs undisturbed: bzh_prove_batch on this key still returns the oracle's proof
        adv = np.stack([np.stack([V.lim(list(c) + [0] * (n - len(c))) for c in s.advice]) for s in states])
        assert pk.prove_batch(adv, [s.instance for s in states], [s.rbytes[:pk.rng_bytes] for s in states]) == proofs
    finally:
        pk.close()


@accelerated_oracle
def test_one_bad_proof_in_a_batch(gpu_ctx, oracle_c):
    """B = 3, k = 5 (min_degree 6, so that coefficients above npieces * n exist): one advice coefficient of proof 1 changed.  The
    call returns OK, status is [0, 1, 0], proofs 0 and 2 are those of the clean run and proof 1 is the model's, built from the low
    coefficients.  An unsatisfied witness, not a fault."""
    case = V.case(5, True, 6, 3)
    cs, keys, _, _, states, _ = case
    npieces = cs.degree - 1
    assert npieces * cs.n < keys.dom.en
    cap = len(states[0].prefix_proof) + 32 * (1 + npieces)
    pk = make_key(gpu_ctx, case)
    try:
        shape, _ = pk.vanishing_plan()
        clean = run_host(gpu_ctx, pk, states, shape, cap)
        assert not clean[0][4].any() and not clean[3].any()
        assert clean[1] == [s.prefix_proof + V.model(keys, s)[0] for s in states]
        bad_polys = [list(c) for c in states[1].adv_polys]
        bad_polys[1][3] = (bad_polys[1][3] + 1) % F.p
        adv = V.operand_arrays(states)[0].copy()
        adv[1, 1, 3] = V.lim([bad_polys[1][3]])[0]
        want = V.model(keys, states[1], bad_polys)
        assert want[3] == 1
        outs, got, after, sticky = run_host(gpu_ctx, pk, states, shape, cap, adv)
        assert outs[4].tolist() == [0, 1, 0] and [int(s) & 1 for s in sticky] == [0, 1, 0]
        assert got[0] == clean[1][0] and got[2] == clean[1][2] and after[0] == clean[2][0] and after[2] == clean[2][2]
        assert got[1] == states[1].prefix_proof + want[0] and after[1] == want[1]
        assert V.ints(outs[2][1]) == want[2]
        assert (outs[2][0] == clean[0][2][0]).all() and (outs[2][2] == clean[0][2][2]).all()
        # the same on device operands: k_vn_degree's store goes into the caller's own, odd-aligned status array
        d_outs, d_got, d_after, d_sticky = run_device(gpu_ctx, pk, states, shape, cap, adv)
        assert d_outs[4].tolist() == [0, 1, 0] and [int(s) & 1 for s in d_sticky] == [0, 1, 0]
        assert d_got == got and d_after == after
        assert d_outs[2] == [v for row in outs[2] for v in V.ints(row)]
    finally:
        pk.close()


@accelerated_oracle
def test_chained_with_the_evaluation_phase(gpu_ctx, oracle_c):
    """k = 5: out_h (h_stride = en), out_h_blinds, out_random and the polynomials go into TranscriptBatch.evaluations with the
    circuit's query list; the bytes are the oracle proof's up to the end of the evaluations"""
    case = V.case(5, True, None, 3)
    cs, keys, _, _, states, proofs = case
    B, n, npieces = 3, cs.n, cs.degree - 1
    ni, na, nf = cs.num_instance, cs.num_advice, cs.num_fixed
    nsets = len(states[0].perm)
    nz, nl = len(states[0].z_polys), len(cs.lookups)
    z0, l0 = ni + na + 1, ni + na + 1 + nz
    nown = l0 + 2 * nl
    last_rot = -(cs.blinding_factors + 1)
    q = [(c, r) for c, r in cs.instance_queries] + [(ni + c, r) for c, r in cs.advice_queries] + [(nown + c, r) for c, r in cs.fixed_queries]
    q += [(ni + na, 0)] + [(nown + nf + j, 0) for j in range(len(cs.perm_columns))]
    for i in range(nsets):
        q += [(z0 + i, 0), (z0 + i, 1)] + ([(z0 + i, last_rot)] if i != nsets - 1 else [])
    for li in range(nl):
        q += [(z0 + nsets + li, 0), (z0 + nsets + li, 1), (l0 + 2 * li, 0), (l0 + 2 * li, -1), (l0 + 2 * li + 1, 0)]
    grow = 32 * (1 + npieces) + 32 * len(q)
    cap = len(states[0].prefix_proof) + grow
    pk = make_key(gpu_ctx, case)
    try:
        shape, _ = pk.vanishing_plan()
        a, i, lk, z = V.operand_arrays(states)
        tb, ch = replayed_batch(gpu_ctx, states, cap)
        with tb:
            rp, _, h, hb, st = tb.vanishing(pk, a, i, lk, z, ch[0], ch[1], ch[2], [s.rng for s in states], shape=shape)
            assert not st.any()
            polys = np.concatenate([i, a, rp.reshape(B, 1, n, 4), z, lk.reshape(B, 2 * nl, n, 4)], axis=1)
            shared = np.stack([V.lim(c) for c in keys.fixed_polys + keys.sigma_polys])
            tb.evaluations(cs.k, polys, q, shared=shared, h_pieces=h, h_blinds=hb, npieces=npieces, h_stride=shape[1])
            got = tb.proofs()
        for b in range(B):
            assert got[b] == proofs[b][:cap], "proof %d" % b
    finally:
        pk.close()


def _shot_key(ctx, params):
    import bzh2
    from bzh2 import circuits as Cm, native as N
    lay = Cm.CircuitLayout(Cm.SHOT, 11)
    blob = lay.blob()
    lay.close()
    return N.NativeProvingKey(ctx, blob, bzh2.CURVE_VESTA, params=params)


def test_flavours_agree_on_the_shot_key(gpu_ctx, monkeypatch):
    """the Shot circuit's key at k = 11 (en = 16384: the unsaturated builtin kernel's conditions hold), B = 2, seeded random
    polynomials as operands: bytes, out_h and status are identical under the interpreter, the unsaturated builtin kernel and the
    saturated builtin kernel (and a module, were one set) -- this is what covers the fe29 constant slots on the device; the
    interpreter is anchored to the oracle by the parity test.
    That the unsaturated kernel is what runs under QUOTIENT_BUILTIN is read off the key: a second key of the same circuit made
    under BZH_QUOTIENT_SATURATED=1 has no fe29 kernel and therefore no fe29 planes of its columns, so it owns less device memory;
    a key that owns the planes has the kernel (bzh_pk_create drops the one with the other), and with BUILTIN selected,
    en % 128 == 0 and ek = 14 every condition of the Prover's q29 holds."""
    import bzh2
    from bzh2 import native as N
    from bzh2.params import Params
    params = Params(gpu_ctx, 11)
    monkeypatch.delenv("BZH_QUOTIENT_SATURATED", raising=False)
    monkeypatch.delenv("BZH_QUOTIENT_V1", raising=False)
    pk = _shot_key(gpu_ctx, params)
    monkeypatch.setenv("BZH_QUOTIENT_SATURATED", "1")        # read by bzh_pk_create alone
    try:
        pk_sat = _shot_key(gpu_ctx, params)
    finally:
        monkeypatch.delenv("BZH_QUOTIENT_SATURATED")
    try:
        assert pk.quotient_selected()[1] and pk_sat.quotient_selected()[1]      # both have the builtin kernel ...
        assert pk.device_bytes()[0] > pk_sat.device_bytes()[0]                  # ... and this one its fe29 flavour and planes
        shape, _ = pk.vanishing_plan()
        n, en, na, ni, nz, nl, npieces, nd = shape
        assert (n, en, npieces) == (2048, 16384, 8)
        B = 2
        rng = np.random.default_rng(2026)

        def elems(*s):
            a = np.frombuffer(rng.bytes(int(np.prod(s)) * 32), dtype=np.uint64).reshape(*s, 4).copy()
            a[..., 3] &= (1 << 60) - 1
            return a
        ops = [elems(B, na, n), elems(B, ni, n), elems(B, nl, 2, n), elems(B, nz, n)]
        ch = [elems(B) for _ in range(3)]
        rbs = [rng.bytes(64 * nd) for _ in range(B)]
        results = {}
        for name, key, flavour in (("interpreter", pk, N.QUOTIENT_INTERPRETER), ("builtin, fe29", pk, N.QUOTIENT_BUILTIN),
                                   ("builtin, saturated", pk_sat, N.QUOTIENT_BUILTIN), ("module", pk, N.QUOTIENT_MODULE)):
            try:
                key.quotient_select(flavour)
            except bzh2.BzhError as e:
                assert e.status == E_RANGE and flavour == N.QUOTIENT_MODULE   # no module was set on this key
                continue
            assert key.quotient_selected()[0] == flavour
            with bzh2.TranscriptBatch(bzh2.CURVE_VESTA, B, 32 * (1 + npieces), gpu_ctx) as tb:
                out = tb.vanishing(key, *ops, *ch, rbs)              # (shape: the key's own plan)
                results[name] = (tb.proofs(), tb.squeeze().tolist(), out[2].tobytes(), out[4].tolist(), tb.status().tolist())
        assert set(results) >= {"interpreter", "builtin, fe29", "builtin, saturated"}
        first = results["interpreter"]
        for name, r in results.items():
            assert r == first, name
        assert first[3] == [0, 0]        # npieces * n == en on this key: no coefficient to flag (the module's text)
        assert any(first[2])
    finally:
        pk.close()
        pk_sat.close()
        params.close() if hasattr(params, "close") else None


@accelerated_oracle
def test_refusals_leave_the_batch_as_it_was(gpu_ctx, oracle_c):
    import torch
    import bzh2
    case = V.case(5, True, None, 3)
    cs, keys, _, _, states, _ = case
    B, npieces = 3, cs.degree - 1
    cap = len(states[0].prefix_proof) + 32 * (1 + npieces)
    pk = make_key(gpu_ctx, case)
    try:
        shape, _ = pk.vanishing_plan()
        n, en, na, ni, nz, nl, _, nd = shape
        a, i, lk, z = V.operand_arrays(states)

        def refused(sts, cap_, status, call, cid=bzh2.CURVE_VESTA):
            if cid == bzh2.CURVE_VESTA:
                tb, ch = replayed_batch(gpu_ctx, sts, cap_)
                twin, _ = replayed_batch(gpu_ctx, sts, cap_)
            else:
                tb, twin = (bzh2.TranscriptBatch(cid, len(sts), cap_, gpu_ctx) for _ in range(2))
                ch = [np.zeros((len(sts), 4), dtype=np.uint64)] * 3
            with tb, twin:
                before = tb.proof_len()
                with pytest.raises(bzh2.BzhError) as e:
                    call(tb, ch)
                assert e.value.status == status
                assert tb.proof_len() == before and (tb.squeeze() == twin.squeeze()).all()

        host = lambda rngs: (lambda tb, ch: tb.vanishing(pk, a, i, lk, z, ch[0], ch[1], ch[2], rngs, shape=shape))   # noqa: E731
        rngs = [s.rng for s in states]
        refused(states, cap, E_ARG, host([r[:-64] for r in rngs]))                       # rng_stride one draw short
        refused(states, cap - 1, E_RANGE, host(rngs))                                    # proof_cap one byte short
        refused(states[:2], cap, E_ARG, lambda tb, ch: tb.vanishing(pk, a, i, lk, z, ch[0], ch[1], ch[2], rngs, shape=shape))   # another size
        refused(states, cap, E_ARG, host(rngs), cid=bzh2.CURVE_PALLAS)                   # a batch on the other curve
        sizes = [B * na * n, B * ni * n, B * nl * 2 * n, B * nz * n, B, B, B, B * nd * 2, B * n, B, B * en, B * npieces]
        d = torch.zeros(sum(sizes) * 4 + 8, dtype=torch.int64, device="cuda")
        offs = [d.data_ptr() + 32 * sum(sizes[:j]) for j in range(len(sizes))]
        for bump in range(len(sizes)):                                                   # each device pointer in turn 8 bytes off
            p = list(offs)
            p[bump] += 8
            refused(states, cap, E_ARG, lambda tb, ch: tb.vanishing(pk, p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7], form=bzh2.FORM_MONTGOMERY,
                                                                    mem=bzh2.MEM_DEVICE, out_random=p[8], out_random_blind=p[9], out_h=p[10],
                                                                    out_h_blinds=p[11], rng_stride=64 * nd))
        gpu_ctx.sync()
        assert not d.cpu().numpy().any()                                                 # nothing was written either
    finally:
        pk.close()
