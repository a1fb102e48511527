"""bzh_commitments_batch_device on the GPU: the instance, advice and lookup commitments against a device-resident transcript
batch must write, proof for proof and byte for byte, what the oracle prover writes (tests/helpers/commitments_cases.py cuts
halo2_oracle.create_proof's captured state at the head and carries the integer model), leave the transcripts in the same state,
squeeze the oracle's theta, beta, gamma and return the oracle's columns, coefficients and blinds.  The last test runs the whole
chain -- commitments, grand products, vanishing, evaluations, multiopen with the opening -- on one device batch, device operands
throughout, and compares whole proofs with the oracle's and with bzh_prove_batch's.  Every comparison is exact."""
import numpy as np
import pytest

import pasta as O
from helpers import commitments_cases as K
from helpers import vanishing_cases as V
from helpers.real_parity import accelerated_oracle

pytestmark = pytest.mark.gpu

E_ARG, E_RANGE = -1, -4
F = O.FP
P = F.p
MONT = lambda x: x * F.R % P          # noqa: E731
UNMONT = lambda x: x * pow(F.R, -1, P) % P   # noqa: E731
ID = lambda x: x                      # noqa: E731


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64).copy()).to("cuda")


def fresh_batch(ctx, bounds, cap):
    """a device batch that has absorbed the key's vk_repr, as every batch does before its first leaf"""
    import bzh2
    B = len(bounds)
    tb = bzh2.TranscriptBatch(bzh2.CURVE_VESTA, B, cap, ctx)
    (op, v), = bounds[0].prefix_ops
    assert op == "common_scalar"
    tb.common_scalars(np.stack([bzh2.int_to_limbs(v)] * B).reshape(B, 1, 4))
    return tb


def make_key(ctx, case):
    import bzh2
    from bzh2 import native as N
    return N.NativeProvingKey(ctx, case[2], bzh2.CURVE_VESTA, *case[3])


def sizes_of(shape, B):
    n, _, _, na, ni, nl = shape[:6]
    return {"advice": B * na * n, "instance": B * ni * n, "lookup_compressed": B * nl * 2 * n, "lookup_permuted": B * nl * 2 * n,
            "advice_polys": B * na * n, "instance_polys": B * ni * n, "lookup_polys": B * nl * 2 * n, "advice_blinds": B * na,
            "lookup_blinds": B * nl * 2, "theta": B, "beta": B, "gamma": B}


def run_host(ctx, pk, bounds, shape, cap, advice=None, rows=None):
    """the call on canonical host operands: ({name: flat integer list}, status, proofs, the next squeeze, the sticky status)"""
    adv, inst = K.operand_arrays(bounds, shape[0], advice=advice)
    if rows is not None:
        inst = inst[:, :, :rows]
    with fresh_batch(ctx, bounds, cap) as tb:
        res, st = tb.commitments(pk, adv, inst if inst.shape[2] else None, [s.rng for s in bounds], shape=shape, instance_rows=inst.shape[2])
        outs = {nm: np.asarray(V.ints(a.reshape(-1, 4)), dtype=object).tolist() for nm, a in res.items()}
        return outs, st, tb.proofs(), V.ints(tb.squeeze()), tb.status()


def run_device(ctx, pk, bounds, shape, cap, form, advice=None):
    """the call on device operands in `form`; the status array starts at an odd address"""
    import torch
    import bzh2
    B = len(bounds)
    conv, back = (MONT, UNMONT) if form == bzh2.FORM_MONTGOMERY else (ID, ID)
    adv, inst = K.operand_arrays(bounds, shape[0], conv, advice=advice)
    d_adv, d_inst = dev(adv), dev(inst)
    sizes = sizes_of(shape, B)
    d_out = torch.zeros(sum(sizes.values()) * 4 + 4, dtype=torch.int64, device="cuda")
    ptrs, at = {}, 0
    for nm in K.OUT:
        ptrs[nm] = d_out.data_ptr() + 32 * at if sizes[nm] else None
        at += sizes[nm]
    d_rng = torch.from_numpy(np.frombuffer(b"".join(s.rng for s in bounds), dtype=np.uint8).copy()).to("cuda")
    d_st = torch.full((B + 1,), 9, dtype=torch.uint8, device="cuda")
    with fresh_batch(ctx, bounds, cap) as tb:
        assert tb.commitments(pk, d_adv.data_ptr(), d_inst.data_ptr(), d_rng.data_ptr(), form=form, mem=bzh2.MEM_DEVICE, out=ptrs,
                              status=d_st.data_ptr() + 1, instance_rows=inst.shape[2], rng_stride=len(bounds[0].rng)) is None
        proofs, after, sticky = tb.proofs(), V.ints(tb.squeeze()), tb.status()
    ctx.sync()
    vals = V.ints(d_out.cpu().numpy().view(np.uint64).reshape(-1, 4))
    outs, at = {}, 0
    for nm in K.OUT:
        chunk = vals[at:at + sizes[nm]]
        outs[nm] = chunk if nm in ("theta", "beta", "gamma") and form != bzh2.FORM_MONTGOMERY else [back(v) for v in chunk]
        at += sizes[nm]
    assert vals[at] == 0                                      # the element after the last output is not touched
    st = d_st.cpu().numpy()
    assert st[0] == 9                                         # nor the byte before an odd-aligned status array
    return outs, st[1:], proofs, after, sticky


def expect(bounds, want, outs, st, got, after, only=None):
    """the run's outputs, bytes and next squeeze against the model's, for the proofs in `only` (all of them when None)"""
    B = len(bounds)
    for b in range(B) if only is None else only:
        assert got[b] == bounds[b].prefix_proof + want[b]["bytes"], "proof %d" % b
        assert after[b] == want[b]["after"], "squeeze after proof %d" % b
        for nm in K.OUT:
            per = len(outs[nm]) // B
            assert outs[nm][b * per:(b + 1) * per] == K.flat(want[b], nm), "%s of proof %d" % (nm, b)
        assert int(st[b]) == 0, "status of proof %d" % b


def all_variants(ctx, case, pk=None):
    import bzh2
    cs, keys, _, _, bounds, proofs, want = case
    cap = len(want[0]["bytes"])
    for b in range(len(bounds)):                             # the model is the oracle proof's own first bytes
        assert want[b]["bytes"] == proofs[b][:cap]
    own = pk is None
    pk = make_key(ctx, case) if own else pk
    try:
        shape = pk.commitments_plan()
        assert shape == K.plan(cs) and shape[6] * 64 == len(bounds[0].rng) and shape[7] == cap
        results = []
        for run in (lambda: run_host(ctx, pk, bounds, shape, cap), lambda: run_device(ctx, pk, bounds, shape, cap, bzh2.FORM_MONTGOMERY),
                    lambda: run_device(ctx, pk, bounds, shape, cap, bzh2.FORM_CANONICAL)):
            outs, st, got, after, sticky = run()
            expect(bounds, want, outs, st, got, after)
            assert not sticky.any()
            results.append((outs, got, after))
        assert results[0] == results[1] == results[2]
        return results[0]
    finally:
        if own:
            pk.close()


# (4, no lookup): n = 16, below a workgroup.  (5, lookup, 3 proofs): the per-proof strides of every layout.  (6, degree 9): more
# blinding-independent shape, another usable.  (9, 2 proofs): n = 512, two workgroups of k_cm_place per (column, proof)
@pytest.mark.parametrize("k,with_lookup,degree,B", [(4, False, None, 1), (5, True, None, 3), (6, True, 9, 2), (9, True, None, 2)])
@accelerated_oracle
def test_parity_with_the_oracle(gpu_ctx, oracle_c, k, with_lookup, degree, B):
    all_variants(gpu_ctx, K.case(k, with_lookup, degree, B))


@accelerated_oracle
def test_two_column_lookup_with_a_rotation(gpu_ctx, oracle_c):
    """k = 5, B = 2: both sides of the lookup have two expressions, so theta -- read from where it was squeezed -- enters the
    compressed columns: they must be the oracle's Horner in theta (expect compares lookup_compressed with the model, which
    test_commitments_device_cpu checks against the closed form)"""
    case = K.two_column_case()
    outs = all_variants(gpu_ctx, case)[0]
    assert any(outs["lookup_compressed"]) and outs["lookup_compressed"] != outs["lookup_permuted"]


@accelerated_oracle
def test_a_circuit_without_instance_and_without_lookup(gpu_ctx, oracle_c):
    """k = 4, B = 2, ni = 0 and nl = 0: `instances` and the instance and lookup members of the outputs are NULL in every variant,
    and no launch may touch them; the advice commitments, theta, beta, gamma are the oracle's"""
    case = K.no_instance_case()
    assert case[0].num_instance == 0 and not case[0].lookups
    outs = all_variants(gpu_ctx, case)[0]
    assert outs["instance"] == [] and outs["lookup_polys"] == [] and any(outs["advice_polys"])


class _Lagrange:
    """(g_lagrange | u | w) for a case's explicit SRS, with its window table"""

    def __init__(self, ctx, case):
        import bzh2
        import coracle as C
        from bzh2 import params as Pm
        g, w, u = case[3]
        self.bases = ctx.upload_bases(bzh2.CURVE_VESTA, np.concatenate([Pm.group_ifft(ctx, C.points_to_array(g)), C.points_to_array([u, w])])).precompute(0)


@pytest.mark.parametrize("k,B", [(5, 3), (9, 2)])
@accelerated_oracle
def test_a_key_with_g_lagrange_gives_the_same_bytes_and_outputs(gpu_ctx, oracle_c, k, B):
    """the commitments are made in the basis the key offers: with bzh_pk_set_lagrange the evaluations are committed against
    g_lagrange (rows evals | 0 | blind from device blinds), without it the coefficients against the SRS -- same bytes, outputs"""
    case = K.case(k, True, None, B)
    lag = _Lagrange(gpu_ctx, case)
    pk = make_key(gpu_ctx, case)
    try:
        plain = all_variants(gpu_ctx, case, pk)
        pk.set_lagrange(lag.bases)
        with_table = all_variants(gpu_ctx, case, pk)
        assert plain == with_table
        pk.set_lagrange(None)
    finally:
        pk.close()
        lag.bases.free()


@accelerated_oracle
def test_a_lookup_input_that_is_not_in_the_table(gpu_ctx, oracle_c):
    """B = 3, k = 5: in proof 1 the looked-up advice cell holds a value the table does not.  The call returns OK; proof 1's status
    bit and sticky bit are set; proofs 0 and 2 are byte-identical to the untouched run, outputs included.  An unsatisfied
    witness, not a fault."""
    import bzh2
    case = K.case(5, True, None, 3)
    cs, keys, _, _, bounds, _, want = case
    cap = len(want[0]["bytes"])
    rows = [r for r in range(cs.usable_rows) if keys.fixed[3][r]]          # sample_circuit: q_lookup * advice 0 is looked up
    assert rows
    advice = [[list(c) for c in b.advice] for b in bounds]
    advice[1][0][rows[0]] = 1 << 40                                        # the table holds 0 .. 7
    pk = make_key(gpu_ctx, case)
    try:
        shape = pk.commitments_plan()
        clean = run_host(gpu_ctx, pk, bounds, shape, cap)
        expect(bounds, want, *clean[:4])
        for run in (lambda: run_host(gpu_ctx, pk, bounds, shape, cap, advice=advice),
                    lambda: run_device(gpu_ctx, pk, bounds, shape, cap, bzh2.FORM_MONTGOMERY, advice=advice)):
            outs, st, got, after, sticky = run()
            assert [int(s) for s in st] == [0, 1, 0] and [int(s) & 1 for s in sticky] == [0, 1, 0]
            expect(bounds, want, outs, st, got, after, only=(0, 2))
            assert got[0] == clean[2][0] and got[2] == clean[2][2] and after[0] == clean[3][0] and after[2] == clean[3][2]
            assert len(got[1]) == cap and got[1] != clean[2][1]            # the failed proof still gets all its messages
    finally:
        pk.close()


@accelerated_oracle
def test_instance_rows_and_the_callers_blinding_rows(gpu_ctx, oracle_c):
    """instance_rows 0, 1 and usable: the instance is padded with zeros (0 rows: `instances` is not read).  Rows from `usable` on
    of the caller's advice, filled with 0xff bytes, reach no output"""
    case = K.case(5, True, None, 3)
    cs, keys, _, _, bounds, _, want = case
    n, usable, cap = cs.n, cs.usable_rows, len(want[0]["bytes"])
    pk = make_key(gpu_ctx, case)
    try:
        shape = pk.commitments_plan()
        # 1 row is the case's own instance; `usable` rows: the same column with explicit zeros
        padded = []
        for b in bounds:
            c = K.Boundary()
            c.__dict__.update(b.__dict__, instance=[list(col) + [0] * (usable - len(col)) for col in b.instance])
            padded.append(c)
        assert all(len(col) == 1 for b in bounds for col in b.instance)
        for bs in (bounds, padded):
            outs, st, got, after, _ = run_host(gpu_ctx, pk, bs, shape, cap)
            expect(bounds, want, outs, st, got, after)
        # 0 rows: the model with an empty instance (the witness no longer satisfies the copy constraint; this phase does not care)
        want0 = [K.model(keys, b, instance=[[] for _ in b.instance]) for b in bounds]
        outs, st, got, after, _ = run_host(gpu_ctx, pk, bounds, shape, cap, rows=0)
        expect(bounds, want0, outs, st, got, after)
        assert not any(outs["instance"])
        # 0xff in the caller's blinding rows (not even a field element)
        adv, inst = K.operand_arrays(bounds, n)
        adv[:, :, usable:] = np.uint64(0xffffffffffffffff)
        with fresh_batch(gpu_ctx, bounds, cap) as tb:
            res, st = tb.commitments(pk, adv, inst, [s.rng for s in bounds], shape=shape)
            outs = {nm: np.asarray(V.ints(a.reshape(-1, 4)), dtype=object).tolist() for nm, a in res.items()}
            expect(bounds, want, outs, st, tb.proofs(), V.ints(tb.squeeze()))
    finally:
        pk.close()


@accelerated_oracle
def test_the_whole_chain_gives_the_oracles_and_prove_batchs_proofs(gpu_ctx, oracle_c):
    """k = 5 with the lookup, B = 3, Montgomery device operands: new batch, common_scalars(vk_repr), commitments, grand products,
    vanishing, evaluations, multiopen (with the opening) on one device batch; one 64-byte draw stream per proof, cut at the
    leaves' draw counts.  Between the calls only device-to-device copies arrange the operands.  tb.proofs() equals, byte for byte
    and in length, the oracle's whole proofs and bzh_prove_batch's on the same key with the same rng; bzh_verify_batch accepts."""
    import torch
    import bzh2
    case = K.case(5, True, None, 3)
    cs, keys, _, _, bounds, proofs, _ = case
    B, n, k = 3, cs.n, cs.k
    ni, na, nf, nl, m = cs.num_instance, cs.num_advice, cs.num_fixed, len(cs.lookups), len(cs.perm_columns)
    MO = bzh2.FORM_MONTGOMERY
    pk = make_key(gpu_ctx, case)
    try:
        cshape, gshape, (vshape, _) = pk.commitments_plan(), pk.grand_products_plan(), pk.vanishing_plan()
        nsets, nz, en, npieces = gshape[3], gshape[5], vshape[1], vshape[6]
        nd_c, nd_g, nd_v, nd_m = cshape[6], gshape[7], vshape[7], n + 2 + 2 * k
        total = nd_c + nd_g + nd_v + nd_m
        assert 64 * total == pk.rng_bytes
        streams = [s.v.rbytes[:64 * total] for s in bounds]
        d_rng = torch.from_numpy(np.frombuffer(b"".join(streams), dtype=np.uint8).copy()).to("cuda")
        at = lambda draws: d_rng.data_ptr() + 64 * draws   # noqa: E731
        # the polynomial table of the evaluations and the multiopen: instance, advice, random, z, lookups, h; then the key's
        z0, l0 = ni + na + 1, ni + na + 1 + nz
        nown = l0 + 2 * nl + 1
        hid = nown - 1
        last_rot = -(cs.blinding_factors + 1)
        q = [(c, r) for c, r in cs.instance_queries] + [(ni + c, r) for c, r in cs.advice_queries] + [(nown + c, r) for c, r in cs.fixed_queries]
        q += [(ni + na, 0)] + [(nown + nf + j, 0) for j in range(m)]
        for i in range(nsets):
            q += [(z0 + i, 0), (z0 + i, 1)] + ([(z0 + i, last_rot)] if i != nsets - 1 else [])
        for li in range(nl):
            q += [(z0 + nsets + li, 0), (z0 + nsets + li, 1), (l0 + 2 * li, 0), (l0 + 2 * li, -1), (l0 + 2 * li + 1, 0)]
        rotations = bzh2.evaluations_plan(q, nown + nf + m)[0]
        pt = rotations.index
        mq = [(c, pt(r)) for c, r in cs.instance_queries] + [(ni + c, pt(r)) for c, r in cs.advice_queries]
        for i in range(nsets):
            mq += [(z0 + i, pt(0)), (z0 + i, pt(1))] + ([(z0 + i, pt(last_rot))] if i != nsets - 1 else [])
        for li in range(nl):
            lz, la, ls = z0 + nsets + li, l0 + 2 * li, l0 + 2 * li + 1
            mq += [(lz, pt(0)), (la, pt(0)), (ls, pt(0)), (la, pt(-1)), (lz, pt(1))]
        mq += [(nown + c, pt(r)) for c, r in cs.fixed_queries] + [(nown + nf + j, pt(0)) for j in range(m)] + [(hid, pt(0)), (ni + na, pt(0))]
        cap = len(proofs[0])
        assert all(len(p) == cap for p in proofs)

        z64 = lambda *shape: torch.zeros(shape + (4,), dtype=torch.int64, device="cuda")   # noqa: E731
        sizes = sizes_of(cshape, B)
        c_out = {nm: z64(sizes[nm]) for nm in K.OUT}
        zp, zb = z64(B, nz, n), z64(B, nz)
        rp, rb, h, hb = z64(B, 1, n), z64(B, 1), z64(B, en), z64(B, npieces)
        table, blinds = z64(B, nown, n), z64(B, nown)
        pts, d_h, d_hbl = z64(B, len(rotations)), z64(B, n), z64(B)
        one = torch.from_numpy(V.lim([MONT(1)]).view(np.int64).copy()).to("cuda")
        shared = dev(np.stack([V.lim(c, MONT) for c in keys.fixed_polys + keys.sigma_polys]))
        shared_blinds = dev(V.lim([MONT(1)] * (nf + m)))
        d_st = torch.full((4 * B,), 9, dtype=torch.uint8, device="cuda")
        adv, inst = K.operand_arrays(bounds, n, MONT)
        d_adv, d_inst = dev(adv), dev(inst)
        p = lambda t: t.data_ptr()   # noqa: E731
        stride = 64 * total
        with fresh_batch(gpu_ctx, bounds, cap) as tb:
            tb.commitments(pk, p(d_adv), p(d_inst), at(0), form=MO, mem=bzh2.MEM_DEVICE, out={nm: p(t) for nm, t in c_out.items()},
                           status=p(d_st), instance_rows=inst.shape[2], rng_stride=stride)
            tb.grand_products(pk, p(c_out["advice"]), p(c_out["instance"]), p(c_out["lookup_compressed"]), p(c_out["lookup_permuted"]),
                              p(c_out["beta"]), p(c_out["gamma"]), at(nd_c), form=MO, mem=bzh2.MEM_DEVICE, out_z=None, out_z_polys=p(zp),
                              out_z_blinds=p(zb), status=p(d_st) + B, rng_stride=stride)
            tb.vanishing(pk, p(c_out["advice_polys"]), p(c_out["instance_polys"]), p(c_out["lookup_polys"]), p(zp), p(c_out["theta"]),
                         p(c_out["beta"]), p(c_out["gamma"]), at(nd_c + nd_g), form=MO, mem=bzh2.MEM_DEVICE, out_random=p(rp),
                         out_random_blind=p(rb), out_h=p(h), out_h_blinds=p(hb), status=p(d_st) + 2 * B, rng_stride=stride)
            gpu_ctx.sync()                                    # device to device, ordered between the two streams; no byte comes to the host
            parts = [c_out["instance_polys"].view(B, ni, n, 4), c_out["advice_polys"].view(B, na, n, 4), rp, zp,
                     c_out["lookup_polys"].view(B, 2 * nl, n, 4)]
            table[:, :hid] = torch.cat(parts, dim=1)
            blinds[:, :hid] = torch.cat([one.view(1, 1, 4).expand(B, ni, 4), c_out["advice_blinds"].view(B, na, 4), rb, zb,
                                         c_out["lookup_blinds"].view(B, 2 * nl, 4)], dim=1)
            torch.cuda.synchronize()
            tb.evaluations(k, p(table), q, shared=p(shared), h_pieces=p(h), h_blinds=p(hb), npieces=npieces, h_stride=en, form=MO,
                           mem=bzh2.MEM_DEVICE, out_points=p(pts), out_h=p(d_h), out_h_blind=p(d_hbl), npolys_own=nown, npolys_shared=nf + m)
            gpu_ctx.sync()
            table[:, hid] = d_h
            blinds[:, hid] = d_hbl
            torch.cuda.synchronize()
            tb.multiopen(pk.bases, k, p(table), p(blinds), p(pts), mq, at(nd_c + nd_g + nd_v), shared=p(shared), shared_blinds=p(shared_blinds),
                         form=MO, mem=bzh2.MEM_DEVICE, status=p(d_st) + 3 * B, rng_stride=stride, npolys_own=nown, npolys_shared=nf + m,
                         npoints=len(rotations))
            got, sticky = tb.proofs(), tb.status()
        gpu_ctx.sync()
        assert not sticky.any() and not d_st.cpu().numpy().any()
        for b in range(B):
            assert len(got[b]) == len(proofs[b]) and got[b] == proofs[b], "proof %d against the oracle" % b
        adv_c, _ = K.operand_arrays(bounds, n)
        instances = [s.instance for s in bounds]
        assert pk.prove_batch(adv_c, instances, streams) == got
        assert pk.verify_batch(instances, got) == [True] * B
    finally:
        pk.close()


@accelerated_oracle
def test_refusals_leave_the_batch_as_it_was(gpu_ctx, oracle_c):
    import torch
    import bzh2
    case = K.case(5, True, None, 3)
    cs, keys, _, _, bounds, _, want = case
    B, cap = 3, len(want[0]["bytes"])
    pk = make_key(gpu_ctx, case)
    try:
        shape = pk.commitments_plan()
        n, usable, _, na, ni, nl, nd, _ = shape
        adv, inst = K.operand_arrays(bounds, n)
        rngs = [s.rng for s in bounds]

        def refused(sts, cap_, status, call):
            with fresh_batch(gpu_ctx, sts, cap_) as tb, fresh_batch(gpu_ctx, sts, cap_) as twin:
                before = tb.proof_len()
                with pytest.raises(bzh2.BzhError) as e:
                    call(tb)
                assert e.value.status == status
                assert tb.proof_len() == before and (tb.squeeze() == twin.squeeze()).all() and not tb.status().any()   # nothing was absorbed

        host = lambda r, i=inst, rows=None: (lambda tb: tb.commitments(pk, adv, i, r, shape=shape, instance_rows=rows))   # noqa: E731
        refused(bounds, cap - 1, E_RANGE, host(rngs))                                    # proof_cap one byte short
        refused(bounds, cap, E_ARG, host([r[:-64] for r in rngs]))                       # rng_stride one draw short
        refused(bounds[:2], cap, E_ARG, host(rngs))                                      # a batch of another size
        wide = np.zeros((B, ni, usable + 1, 4), dtype=np.uint64)
        refused(bounds, cap, E_ARG, host(rngs, wide))                                    # instance_rows > usable
        refused(bounds, cap, E_ARG, host(rngs, None, 1))                                 # instance rows without an instance
        with bzh2.TranscriptBatch(bzh2.CURVE_PALLAS, B, cap, gpu_ctx) as tb:             # a batch of another curve
            with pytest.raises(bzh2.BzhError) as e:
                host(rngs)(tb)
            assert e.value.status == E_ARG and tb.proof_len() == 0
        sizes = sizes_of(shape, B)
        order = ["adv_in", "inst_in", "rng"] + list(K.OUT)
        elems = dict(sizes, adv_in=B * na * n, inst_in=B * ni, rng=B * nd * 2)
        d = torch.zeros(sum(elems.values()) * 4 + 8, dtype=torch.int64, device="cuda")
        offs, at = {}, 0
        for nm in order:
            offs[nm] = d.data_ptr() + 32 * at
            at += elems[nm]

        def device_call(p, batch=None, drop=None):
            out = {nm: p[nm] for nm in K.OUT if nm != drop}
            return lambda tb: tb.commitments(pk, p["adv_in"], p["inst_in"], p["rng"], form=bzh2.FORM_MONTGOMERY, mem=bzh2.MEM_DEVICE, out=out,
                                             instance_rows=1, rng_stride=64 * nd, batch=batch)

        for bump in order:                                                               # each device pointer in turn 8 bytes off
            p = dict(offs)
            p[bump] += 8
            refused(bounds, cap, E_ARG, device_call(p))
        for drop in K.OUT:                                                               # each required output member in turn NULL
            refused(bounds, cap, E_ARG, device_call(offs, drop=drop))
        # batch * max(na, ni, 2 nl) = 21846 * 3 > 65535: the commitments would not fit one launch's grid.  Refused before anything is
        # read, so the operand pointers need not hold that many proofs
        big = 65535 // max(na, ni, 2 * nl) + 1
        with bzh2.TranscriptBatch(bzh2.CURVE_VESTA, big, cap, gpu_ctx) as tb:
            with pytest.raises(bzh2.BzhError) as e:
                device_call(offs, big)(tb)
            assert e.value.status == E_ARG and tb.proof_len() == 0
        gpu_ctx.sync()
        assert not d.cpu().numpy().any()                                                 # nothing was written either
    finally:
        pk.close()
