"""bzh_permute_expression_pair_batch (csrc/lookup_permute.hip) against oracle/pasta.py: permute_expression_pair, row by row,
and the prover with the lookup argument's permutation on the device against the host selection.

Inputs are drawn from the table unless a case says otherwise; every case first runs the oracle on the CPU side, so an
oracle failure (an input value missing from the table) is asserted there and never reaches the device unintended.

Sizes: the general path sorts 1024-key tiles in LDS and merges runs of 1024, 2048, 4096, ... keys, so besides the listed
sizes the cases take 1025, 4097 and 8193 (one key past a tile / run boundary); the small-key path counts 4096 values per
histogram pass, so its cases put values on both sides of 4095 | 4096 and 65535 | 65536."""
import random

import numpy as np
import pytest

import pasta as O
from helpers import field_edges as FE

pytestmark = pytest.mark.gpu

R = 1 << 256
LIFT = 1 << 250          # added to small values to send a pair down the general path with the same order structure


def _arr(rows, stride, p, form, fill=0xFF):
    """(batch, stride, 4) uint64 from lists of ints; rows past each list are filled with `fill` bytes"""
    out = np.full((len(rows), stride, 4), np.uint64(int.from_bytes(bytes([fill]) * 8, "little")), dtype=np.uint64)
    for b, vals in enumerate(rows):
        if form:
            vals = [v * R % p for v in vals]
        out[b, :len(vals)] = FE.ints_to_array(vals)
    return out


def _oracle(pairs, usable, fid):
    return [O.permute_expression_pair(a, t, usable, O.FIELD_BY_ID[fid]) for a, t in pairs]


def _run(ctx, fid, pairs, usable, stride=None, form=0, mem=0, check=True):
    """-> (A', S', status) as uint64 arrays (batch, stride, 4); outputs prefilled with 0xff bytes, inputs checked unchanged"""
    import bzh2
    p = FE.MODULI[fid]
    stride = stride or usable
    a = _arr([x[0] for x in pairs], stride, p, form)
    t = _arr([x[1] for x in pairs], stride, p, form)
    if mem == bzh2.MEM_HOST:
        a0, t0 = a.copy(), t.copy()
        oa = np.full_like(a, np.uint64(0xFFFFFFFFFFFFFFFF))
        ot = np.full_like(a, np.uint64(0xFFFFFFFFFFFFFFFF))
        _, _, st = ctx.permute_expression_pair_batch(fid, a, t, usable, form, check=check, out=(oa, ot))
        assert (a == a0).all() and (t == t0).all()
        return oa, ot, st
    import torch
    da, dt = torch.from_numpy(a.view(np.int64)).cuda(), torch.from_numpy(t.view(np.int64)).cuda()
    doa, dot = torch.full_like(da, -1), torch.full_like(dt, -1)
    torch.cuda.synchronize()
    st = ctx.permute_expression_pair_batch_device(fid, da.data_ptr(), dt.data_ptr(), stride, usable, len(pairs), doa.data_ptr(), dot.data_ptr(),
                                                  form, check=check)
    assert (da.cpu().numpy().view(np.uint64) == a).all() and (dt.cpu().numpy().view(np.uint64) == t).all()
    return doa.cpu().numpy().view(np.uint64), dot.cpu().numpy().view(np.uint64), st


def _check(got, want, usable, fid, form, only=None):
    """row by row against the oracle's (A', S') per pair; rows usable .. stride must read zero"""
    oa, ot, st = got
    p = FE.MODULI[fid]
    for b, pair in enumerate(want):
        if only is not None and b not in only:
            continue
        wa, ws = pair
        assert st[b] == 0, (b, st)
        for name, g, w in (("A'", oa[b], wa), ("S'", ot[b], ws)):
            exp = FE.ints_to_array([v * R % p for v in w] if form else w)
            bad = np.nonzero((g[:usable] != exp).any(axis=1))[0]
            assert bad.size == 0, "%s pair %d: %d rows differ, first at row %d: got %s want %#x" % (
                name, b, bad.size, bad[0], [hex(int(x)) for x in g[bad[0]]], (w[bad[0]] * R % p) if form else w[bad[0]])
            assert not g[usable:].any(), "%s pair %d: rows past usable are not zero" % (name, b)


def _draw(rng, table, usable):
    return [table[rng.randrange(len(table))] for _ in range(usable)]


GENERAL_SIZES = (1, 2, 7, 63, 64, 65, 1000, 1025, 2047, 2048, 2049, 4097, 4099, 8193)


@pytest.mark.parametrize("mem", [0, 1], ids=["host", "device"])
@pytest.mark.parametrize("form", [0, 1], ids=["canonical", "montgomery"])
@pytest.mark.parametrize("fid", [0, 1, 2])
def test_general_keys_match_the_oracle(gpu_ctx, fid, form, mem):
    p = FE.MODULI[fid]
    rng = random.Random(1000 + 10 * fid + 2 * form + mem)
    for usable in GENERAL_SIZES:
        table = [rng.randrange(p) for _ in range(usable)]
        pairs = [(_draw(rng, table, usable), table)]
        _check(_run(gpu_ctx, fid, pairs, usable, form=form, mem=mem), _oracle(pairs, usable, fid), usable, fid, form)


@pytest.mark.parametrize("fid", [0, 1, 2])
def test_comparator_orders_by_canonical_value_limb_3_first(gpu_ctx, fid):
    p = FE.MODULI[fid]
    rng = random.Random(2000 + fid)
    edges = FE.edge_values(p)
    assert len(edges) == 256 and 0 in edges and p - 1 in edges
    base = rng.randrange(1 << 180) | (1 << 100)
    cases = {
        "edge operands": edges,
        "only limb 3 differs": [base + (j << 192) for j in rng.sample(range(1 << 20), 200)],
        "only limb 0 differs": [(base & ~((1 << 64) - 1)) + (j << 17) for j in rng.sample(range(1 << 46), 200)],
        "upper 224 bits equal": [(base & ~0xFFFFFFFF) + j for j in rng.sample(range(1 << 32), 200)],
        "0 and p - 1": [p - 1, 0],
    }
    for name, table in cases.items():
        assert all(0 <= v < p for v in table) and len(set(table)) == len(table), name
        usable = len(table)
        for form in (0, 1):
            pairs = [(_draw(rng, table, usable), table), (rng.sample(table, usable), table)]
            _check(_run(gpu_ctx, fid, pairs, usable, form=form), _oracle(pairs, usable, fid), usable, fid, form)


@pytest.mark.parametrize("lift", [0, LIFT], ids=["small", "general"])
def test_run_structures(gpu_ctx, lift):
    fid, usable = 0, 1500
    rng = random.Random(3000)
    distinct = [lift + v for v in rng.sample(range(1, 60000), usable)]
    lo, hi = min(distinct), max(distinct)
    pairs = [
        ([lift + rng.randrange(16) for _ in range(usable)], [lift + i % 16 for i in range(usable)]),     # table i % 16
        ([lift + 7] * usable, [lift + 7] * usable),                                                       # all equal: m = usable - 1
        (rng.sample(distinct, usable), distinct),                                                         # a permutation: m = 0
        ([distinct[5]] * usable, distinct),                                                               # one value repeated
        ([lo] * usable, distinct),                                                                        # ... the smallest
        ([hi] * usable, distinct),                                                                        # ... the largest
    ]
    want = _oracle(pairs, usable, fid)
    assert want[1][1] == [lift + 7] * usable and want[2][0] == want[2][1] == sorted(distinct)
    _check(_run(gpu_ctx, fid, pairs, usable), want, usable, fid, 0)


def test_path_boundaries(gpu_ctx):
    import bzh2
    fid, usable = 1, 3000
    rng = random.Random(4000)
    for big in (65535, 65536):
        for where in ("input", "table", "both"):
            for with_zero in (True, False):
                table = [(0 if with_zero else 1) + i % 1000 for i in range(usable)]
                table[1::7] = [4095 + i % 3 for i in range(len(table[1::7]))]       # both sides of a histogram pass boundary
                inp = _draw(rng, table, usable)
                if where != "input":
                    table[-1] = big
                if where != "table":
                    inp[0] = big
                pairs = [(inp, table)]
                if where == "input":                                                # the largest value has no table copy
                    with pytest.raises(ValueError):
                        _oracle(pairs, usable, fid)
                    _, _, st = _run(gpu_ctx, fid, pairs, usable, check=False)
                    assert list(st) == [bzh2.E_RANGE], (big, where)
                else:
                    _check(_run(gpu_ctx, fid, pairs, usable), _oracle(pairs, usable, fid), usable, fid, 0)


def test_both_paths_give_the_same_rows_for_the_same_content(gpu_ctx):
    """one value >= 2^16 appended to the input and the table sends the pair down the general path; being the largest it lands
    on the last row of A' and S' and leaves the other rows as the small-key path wrote them"""
    fid, usable = 0, 2500
    rng = random.Random(5000)
    table = [i % 300 + 4000 for i in range(usable)]
    inp = _draw(rng, table, usable)
    small = _run(gpu_ctx, fid, [(inp, table)], usable)
    _check(small, _oracle([(inp, table)], usable, fid), usable, fid, 0)
    big = 1 << 200
    general = _run(gpu_ctx, fid, [(inp + [big], table + [big])], usable + 1)
    _check(general, _oracle([(inp + [big], table + [big])], usable + 1, fid), usable + 1, fid, 0)
    for s, g in zip(small[:2], general[:2]):
        assert (s[0] == g[0, :usable]).all()
        assert FE.array_to_ints(g[0, usable:]) == [big]


def _reference_pair(rng, usable):
    table = [i % 1024 for i in range(usable)]
    inp = [0] * usable
    for r in rng.sample(range(usable), 2399):
        inp[r] = rng.randrange(1, 1024)
    return inp, table


@pytest.mark.parametrize("mem", [0, 1], ids=["host", "device"])
def test_reference_shape_k14_range_table(gpu_ctx, mem):
    """the reference's lookup at the bench default: 2^14 rows, 10-bit range table, input non-zero on 2 399 rows"""
    fid, usable = 0, 16378
    rng = random.Random(6000)
    pairs = [_reference_pair(rng, usable) for _ in range(3)]
    assert len({tuple(a) for a, _ in pairs}) == 3 and all(sum(1 for v in a if v) == 2399 for a, _ in pairs)
    _check(_run(gpu_ctx, fid, pairs, usable, stride=1 << 14, form=1, mem=mem), _oracle(pairs, usable, fid), usable, fid, 1)


def test_k17_shape_general_keys(gpu_ctx):
    """usable = 131 066 (k = 17), full-width keys, batch 2 -- and the k = 14 shape on the same ctx right after (one call
    has one usable_rows; the second call runs in the workspace the first one grew)"""
    fid = 0
    p = FE.MODULI[fid]
    rng = random.Random(7000)
    for usable in (131066, 16378):
        pairs = []
        for _ in range(2):
            table = [rng.randrange(p) for _ in range(usable)]
            pairs.append((_draw(rng, table, usable), table))
        _check(_run(gpu_ctx, fid, pairs, usable, stride=usable + 6), _oracle(pairs, usable, fid), usable, fid, 0)


@pytest.mark.parametrize("mem", [0, 1], ids=["host", "device"])
@pytest.mark.parametrize("lift", [0, LIFT], ids=["small", "general"])
def test_batch_and_stride(gpu_ctx, lift, mem):
    fid, usable = 2, 1234
    rng = random.Random(8000)
    pairs = []
    for b in range(5):
        table = [lift + rng.randrange(50 * (b + 1)) for _ in range(usable)]
        pairs.append((_draw(rng, table, usable), table))
    assert len({tuple(a) for a, _ in pairs}) == 5
    # _run prefills the outputs with 0xff bytes and the input rows past `usable` too; _check wants rows usable .. stride zero
    for form in (0, 1):
        _check(_run(gpu_ctx, fid, pairs, usable, stride=usable + 6, form=form, mem=mem), _oracle(pairs, usable, fid), usable, fid, form)


@pytest.mark.parametrize("missing", ["below", "above", "between"])
@pytest.mark.parametrize("lift", [0, LIFT], ids=["small", "general"])
def test_missing_input_value_fails_its_pair_only(gpu_ctx, lift, missing):
    import bzh2
    fid, usable = 0, 2100
    rng = random.Random(9000)
    pairs = []
    for b in range(4):
        table = [lift + 10 + 2 * rng.randrange(500) for _ in range(usable)]      # even values in [10, 1010)
        pairs.append((_draw(rng, table, usable), table))
    bad = {"below": lift + 3, "above": lift + 5000, "between": lift + 501}[missing]
    tbl = pairs[2][1]
    assert bad not in tbl and {"below": bad < min(tbl), "above": bad > max(tbl), "between": min(tbl) < bad < max(tbl)}[missing]
    pairs[2][0][usable // 2] = bad
    with pytest.raises(ValueError):
        _oracle(pairs[2:3], usable, fid)
    want = _oracle(pairs[:2], usable, fid) + [None] + _oracle(pairs[3:], usable, fid)
    with pytest.raises(bzh2.BzhError) as e:
        _run(gpu_ctx, fid, pairs, usable)
    assert e.value.status == bzh2.E_RANGE
    got = _run(gpu_ctx, fid, pairs, usable, check=False)
    assert list(got[2]) == [0, 0, bzh2.E_RANGE, 0]
    _check(got, want, usable, fid, 0, only=(0, 1, 3))
    ok = pairs[:2]                                                                # the next call on the same ctx succeeds
    _check(_run(gpu_ctx, fid, ok, usable), want[:2], usable, fid, 0)


def test_argument_errors(gpu_ctx):
    import bzh2
    a = np.zeros((1, 8, 4), dtype=np.uint64)
    for usable in (0, 9):
        with pytest.raises(bzh2.BzhError) as e:
            gpu_ctx.permute_expression_pair_batch(0, a, a, usable)
        assert e.value.status == bzh2.E_ARG


# ---- the prover ------------------------------------------------------------------------------------------------------------
def _eval(e, adv, fixed, row, n, p):
    tag = e[0]
    if tag == "const":
        return e[1] % p
    if tag in ("advice", "fixed", "instance"):
        assert tag != "instance"
        col = adv[e[1]] if tag == "advice" else fixed[e[1]]
        return col[(row + e[2]) % n]
    if tag == "neg":
        return -_eval(e[1], adv, fixed, row, n, p) % p
    if tag == "scale":
        return _eval(e[1], adv, fixed, row, n, p) * e[2] % p
    x, y = _eval(e[1], adv, fixed, row, n, p), _eval(e[2], adv, fixed, row, n, p)
    return (x + y) % p if tag == "add" else x * y % p


def _advice_queries(e, out):
    if e[0] == "advice":
        out.append((e[1], e[2]))
    elif e[0] in ("neg", "scale"):
        _advice_queries(e[1], out)
    elif e[0] in ("add", "mul"):
        _advice_queries(e[1], out)
        _advice_queries(e[2], out)
    return out


def test_prover_gives_the_same_proofs_with_the_lookup_on_host_and_device(gpu_ctx):
    """The reference's ShotCircuit (k = 11, 10-bit range lookup), batch of 3, seeded: identical proof bytes under both
    selections, both verify; a witness whose lookup input leaves the table (one cell of the running-sum column the lookup
    reads, on a row where the lookup is enabled, pushed out of range) is BZH_E_RANGE under both."""
    import blob as Bm
    import bzh2
    from bzh2 import circuits as Cm, native as N, params as Pm
    from helpers import real_parity as RP
    lay = Cm.CircuitLayout(Cm.SHOT, 11)
    prm = Pm.Params(gpu_ctx, 11)
    pk = N.NativeProvingKey(gpu_ctx, lay.blob(), bzh2.CURVE_VESTA, params=prm)
    try:
        circuits = RP.shot_circuits(Cm, 77, 3)
        adv, insts = lay.synthesize(circuits)
        seeds = [bytes([17 + b]) * 32 for b in range(3)]
        proofs = {}
        for where in (N.LOOKUP_HOST, N.LOOKUP_DEVICE):
            pk.lookup_select(where)
            assert pk.lookup_selected() == where
            proofs[where] = pk.prove_batch(adv, insts, None, seeds=seeds)
            assert pk.verify_batch(insts, proofs[where]) == [True] * 3
        assert proofs[N.LOOKUP_HOST] == proofs[N.LOOKUP_DEVICE] and len(set(proofs[N.LOOKUP_HOST])) == 3
        with pytest.raises(bzh2.BzhError) as e:
            pk.lookup_select(2)
        assert e.value.status == bzh2.E_ARG and pk.lookup_selected() == N.LOOKUP_DEVICE
        # push one lookup input of proof 1 out of the table
        circ = Bm.decode(lay.blob())
        p, n, usable = O.FP.p, circ.n, pk.usable_rows
        (ins, tabs), = circ.lookups
        assert len(ins) == 1
        cols = [FE.array_to_ints(adv[1, c]) for c in range(adv.shape[1])]
        table = {_eval(tabs[0], cols, circ.fixed, r, n, p) for r in range(usable)}
        values = [_eval(ins[0], cols, circ.fixed, r, n, p) for r in range(usable)]
        assert all(v in table for v in values)
        row = next(r for r in range(usable) if values[r])                # the lookup is enabled here
        col = next(c for c, rot in _advice_queries(ins[0], []) if rot == 0)
        cols[col][row] = (cols[col][row] + (1 << 100)) % p
        assert _eval(ins[0], cols, circ.fixed, row, n, p) not in table
        bad = adv.copy()
        bad[1, col, row] = FE.ints_to_array([cols[col][row]])[0]
        for where in (N.LOOKUP_HOST, N.LOOKUP_DEVICE):
            pk.lookup_select(where)
            with pytest.raises(bzh2.BzhError) as e:
                pk.prove_batch(bad, insts, None, seeds=seeds)
            assert e.value.status == bzh2.E_RANGE, where
            assert pk.prove_batch(adv, insts, None, seeds=seeds) == proofs[where]     # the ctx and the key are fine afterwards
    finally:
        pk.close()
        prm.close()
        lay.close()
