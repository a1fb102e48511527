"""Accumulated batch verification on the device.

The leaf (bzh_ipa_check_accumulated: k_ipa_acc_weights, k_ipa_acc_s, k_ipa_acc_scale, two MSMs, k_ipa_acc_result) on a table made
by bzh_bases_walk, G_i = [i + 1] G: every discrete logarithm is known, so whether an opening is valid -- and whether a weighted
sum of openings is -- is integer arithmetic mod r.  k = 5 (odd; n = 32, below one workgroup) and k = 6; batches of 1, 3 and 65;
nl = 16 with (0,0) padding under non-zero scalars in the last slots.

The two front doors against the calls they extend (bzh_verify_records_device, bzh_verify_batch_vk_with under the device pass) on
the k = 5 sample circuit and on Shot at k = 11: results and status equal, path as the issue's table says."""
import random

import numpy as np
import pytest

import coracle as C
import pasta as O
from helpers import verify_pass_cases as VP
from helpers import vk_cases as V
from test_gpu_verify_records import Side, _Srs, _game_side, _input, _sample_proofs

pytestmark = pytest.mark.gpu
NL, POOL = 16, 30                                                        # (the k = 5 table holds 34 points)
SEED_A, SEED_B = bytes(range(1, 33)), bytes((11 * i + 5) & 0xff for i in range(32))


class Walk:
    """a walked table of n + 2 points on one curve, its first POOL points on the host, and the scalar field"""

    def __init__(self, ctx, cid, k):
        import bzh2
        from bzh2 import native as N
        self.ctx, self.cid, self.k, self.n = ctx, cid, k, 1 << k
        self.r = N.MODULI[bzh2.CURVE_SCALAR_FIELD[cid]]
        self.g = C.points_to_array([O.CURVE_BY_ID[cid].random_point(random.Random(40 + cid))])[0]
        self.bases = ctx.bases_walk(cid, self.g, self.n + 2)
        self.pool = ctx.bases_points(self.bases, 0, POOL)                  # pool[m - 1] = [m] G

    def close(self):
        self.bases.free()

    def right(self, c, us):
        """the discrete logarithm of < c s(u), G >: sum_i c prod_{j: bit (k-1-j) of i} u_j * (i + 1)"""
        r, k, total = self.r, self.k, 0
        for i in range(self.n):
            s = c
            for j in range(k):
                if (i >> (k - 1 - j)) & 1:
                    s = s * us[j] % r
            total = (total + s * (i + 1)) % r
        return total

    def opening(self, rng, off=0, twin=None):
        """(multiples m[NL] (0 = padding), scalars[NL], cu[k + 1]) with sum scal m = right(c, u) + off mod r.  The last two slots
        are (0,0) padding under non-zero scalars; slot NL - 3 closes the equation.  twin = e: slots 0 and 1 hold the same point
        with scalars e and r - e."""
        r = self.r
        cu = [rng.randrange(1, r) for _ in range(self.k + 1)]
        m = [rng.randrange(1, POOL + 1) for _ in range(NL - 2)] + [0, 0]
        sc = [rng.randrange(r) for _ in range(NL)]
        if twin is not None:
            m[1] = m[0]
            sc[0], sc[1] = twin % r, (r - twin) % r
        part = sum(sc[j] * m[j] for j in range(NL - 3)) % r
        sc[NL - 3] = (self.right(cu[0], cu[1:]) + off - part) * pow(m[NL - 3], -1, r) % r
        return m, sc, cu

    def check(self, openings, weights, exclude=None):
        pts = np.zeros((len(openings), NL, 8), dtype=np.uint64)
        for b, (m, _, _) in enumerate(openings):
            for j, mj in enumerate(m):
                if mj:
                    pts[b, j] = self.pool[mj - 1]
        return self.check_points(pts, [sc for _, sc, _ in openings], [c for _, _, c in openings], weights, exclude)

    def check_points(self, pts, scalars, cus, weights, exclude=None):
        """pts: (B, NL, 8) canonical affine points; scalars: B lists of NL ints; cus: B lists of k + 1 ints"""
        from bzh2 import native as N
        import ctypes
        B = len(scalars)
        pts = np.ascontiguousarray(pts, dtype=np.uint64)
        scal = np.ascontiguousarray(np.stack([C.ints_to_array(sc) for sc in scalars]))
        cu = np.ascontiguousarray(np.stack([C.ints_to_array(c) for c in cus]))
        w = np.ascontiguousarray(C.ints_to_array([int(x) % self.r for x in weights]))
        ex = np.ascontiguousarray(np.array(exclude, dtype=np.uint8)) if exclude is not None else None
        ok = ctypes.c_int(7)
        vp = ctypes.c_void_p
        rc = N._bind().bzh_ipa_check_accumulated(self.ctx.handle, self.bases.handle, B, NL, vp(pts.ctypes.data), vp(scal.ctypes.data),
                                                 vp(cu.ctypes.data), vp(w.ctypes.data), vp(ex.ctypes.data) if ex is not None else None,
                                                 ctypes.byref(ok))
        self.ctx._check(rc, "bzh_ipa_check_accumulated")
        assert ok.value in (0, 1)
        return bool(ok.value)

    def weights(self, seed, B):
        import bzh2
        return bzh2.accumulation_weights(self.cid, seed, B)


@pytest.fixture(scope="module")
def walks(gpu_ctx):
    w = {(0, 5): Walk(gpu_ctx, 0, 5), (0, 6): Walk(gpu_ctx, 0, 6), (1, 5): Walk(gpu_ctx, 1, 5)}
    yield w
    for x in w.values():
        x.close()


@pytest.mark.parametrize("k", [5, 6])
@pytest.mark.parametrize("batch", [1, 3, 65])
def test_leaf_valid_invalid_and_excluded(walks, k, batch):
    """all valid: ok; one invalid opening first, in the middle, last: not ok; the same with its exclude byte set: ok"""
    wk = walks[(0, k)]
    rng = random.Random(1000 * k + batch)
    good = [wk.opening(rng) for _ in range(batch)]
    w = wk.weights(SEED_A, batch)
    assert wk.check(good, w)
    assert wk.check(good, w, exclude=[0] * batch)
    for pos in sorted({0, batch // 2, batch - 1}):
        bad = list(good)
        bad[pos] = wk.opening(rng, off=1 + pos)
        assert not wk.check(bad, w), pos
        ex = [0] * batch
        ex[pos] = 1
        assert wk.check(bad, w, exclude=ex), pos
        # an excluded opening's rows are meaningless: garbage there changes nothing
        m, sc, cu = bad[pos]
        bad[pos] = (m, [wk.r - 1] * NL, [wk.r - 2] * (k + 1))
        assert wk.check(bad, w, exclude=ex), pos


@pytest.mark.parametrize("k", [5, 6])
def test_leaf_cancelling_pair_needs_the_weights(walks, k):
    """two openings whose left sides are off by +D and -D pass with weights (1, 1) and fail with the seeded weights: the weights
    reach both sides"""
    wk = walks[(0, k)]
    rng = random.Random(77 + k)
    D = rng.randrange(1, wk.r)
    pair = [wk.opening(rng, off=D), wk.opening(rng, off=wk.r - D)]
    assert wk.check(pair, [1, 1])
    w = wk.weights(SEED_A, 2)
    assert w[0] != w[1]
    assert not wk.check(pair, w)
    assert not wk.check(pair, [1, 2])
    valid = [wk.opening(rng), wk.opening(rng)]
    assert wk.check(valid, w) and wk.check(valid, [1, 1])


def test_leaf_forced_doubling_and_cancellation(walks):
    """two identical valid openings under equal weights put P + P into every bucket they touch; one opening that holds the same
    point with scalars e and r - e puts P + (-P) there"""
    wk = walks[(0, 5)]
    rng = random.Random(5)
    one = wk.opening(rng)
    assert wk.check([one, one], [1, 1])
    assert wk.check([one, one], [3, 3])
    assert wk.check([one, one, one], wk.weights(SEED_B, 3))
    for e in (1, 2, rng.randrange(wk.r), wk.r - 1):
        assert wk.check([wk.opening(rng, twin=e)], [1]), e
        assert not wk.check([wk.opening(rng, twin=e, off=1)], [1]), e
    assert not wk.check([one, wk.opening(rng, off=9)], [1, 1])


def test_leaf_on_the_other_pasta_curve(walks):
    wk = walks[(1, 5)]
    rng = random.Random(15)
    good = [wk.opening(rng) for _ in range(3)]
    w = wk.weights(SEED_B, 3)
    assert wk.check(good, w)
    bad = [good[0], wk.opening(rng, off=4), good[2]]
    assert not wk.check(bad, w)
    assert wk.check(bad, w, exclude=[0, 1, 0])


def test_leaf_agrees_with_ipa_verify_on_one_opening(walks):
    """B = 1, weight 1: a real opening made by bzh_ipa_open against the walked table, verified by bzh_ipa_verify and, with its
    left side assembled here from the proof bytes and a replayed transcript as ipa_verify assembles it -- L_j (u_j^-1), R_j (u_j),
    P (1), G_0 (-v), S (xi), U (-c b_0 z), W (-f) --, by the accumulated leaf: the same verdict, for the valid opening and for a
    changed c, a changed f, another x3 and another v"""
    import bzh2
    wk = walks[(0, 5)]
    ctx, k, n, r = wk.ctx, wk.k, wk.n, wk.r
    rng = random.Random(505)
    table = C.point_walk(0, wk.g, n + 2)                                   # the table bzh_bases_walk made, on the host
    poly = [rng.randrange(r) for _ in range(n)]
    blind, x3 = rng.randrange(r), rng.randrange(r)
    rbytes = np.random.default_rng(5).bytes(64 * (n + 1 + 2 * k))
    P = C.array_to_point(C.msm(0, C.ints_to_array(poly + [0, blind]), table, 1))
    hb = ctx.upload_bases(0, table).precompute()                           # the same points with a window table, for the opening
    t = bzh2.Transcript(bzh2.FIELD_FP)
    v = ctx.ipa_open(hb, C.ints_to_array(poly), blind, x3, rbytes, t)
    proof = t.proof()
    assert len(proof) == 32 * (1 + 2 * k + 2)
    g0_u_w = [C.array_to_point(table[i]) for i in (0, n, n + 1)]

    def scalar(pr, at, add):
        val = (int.from_bytes(pr[at:at + 32], "little") + add) % r
        return pr[:at] + val.to_bytes(32, "little") + pr[at + 32:]

    def leaf(pr, x3_, v_):
        xy, st = bzh2.affine_decompress(0, [pr[32 * i:32 * i + 32] for i in range(1 + 2 * k)])
        assert (st == 0).all()
        tr = bzh2.Transcript(bzh2.FIELD_FP)
        tr.common_point(C.array_to_point(xy[0]))
        xi, z = tr.squeeze_challenge(), tr.squeeze_challenge()
        us = []
        for j in range(k):
            tr.common_point(C.array_to_point(xy[1 + 2 * j]))
            tr.common_point(C.array_to_point(xy[2 + 2 * j]))
            us.append(tr.squeeze_challenge())
        tr.close()
        c = int.from_bytes(pr[32 + 64 * k:64 + 64 * k], "little")
        f = int.from_bytes(pr[64 + 64 * k:96 + 64 * k], "little")
        b0 = 1
        for j in range(k):
            b0 = b0 * (1 + us[j] * pow(x3_, 1 << (k - 1 - j), r)) % r
        pts = np.zeros((1, NL, 8), dtype=np.uint64)
        sc = [0] * NL
        for j in range(k):
            pts[0, 2 * j], pts[0, 2 * j + 1] = xy[1 + 2 * j], xy[2 + 2 * j]
            sc[2 * j], sc[2 * j + 1] = pow(us[j], -1, r), us[j]
        o = 2 * k
        for point, s_ in ((C.points_to_array([P])[0], 1), (table[0], -v_), (xy[0], xi), (table[n], -c * b0 * z), (table[n + 1], -f)):
            pts[0, o], sc[o] = point, s_ % r
            o += 1
        assert o == NL - 1                                                  # 2k + 5 = 15 slots, one of padding
        sc[o] = 3
        return wk.check_points(pts, [sc], [[c] + us], [1])

    def reference(pr, x3_, v_):
        tr = bzh2.Transcript(bzh2.FIELD_FP)
        try:
            return bool(ctx.ipa_verify(hb, P, x3_, v_, pr, tr, g0_u_w))
        finally:
            tr.close()

    cases = [("valid", proof, x3, v, True), ("c + 1", scalar(proof, 32 + 64 * k, 1), x3, v, False),
             ("f + 1", scalar(proof, 64 + 64 * k, 1), x3, v, False), ("x3 + 1", proof, (x3 + 1) % r, v, False),
             ("v + 1", proof, x3, (v + 1) % r, False)]
    try:
        for name, pr, x3_, v_, want in cases:
            ref = reference(pr, x3_, v_)
            assert ref is want, name
            assert leaf(pr, x3_, v_) is ref, name
    finally:
        hb.free()


# ---- the two front doors -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sample(gpu_ctx):
    from bzh2 import native as N
    srs5 = _Srs(gpu_ctx, V.K)
    pk, insts, proofs = _sample_proofs(gpu_ctx, srs5, V.K, 1, 3)
    side = Side(gpu_ctx, srs5, N.NativeVerifyingKey.from_pk(pk), 1, insts, proofs, g0_u_w=srs5.g0_u_w)
    pk.close()
    yield side
    side.vk.close()
    srs5.close()


@pytest.fixture(scope="module")
def shot(gpu_ctx):
    side, prm = _game_side(gpu_ctx, "shot", 11, 3)
    yield side
    side.vk.close()
    prm.close()


def _flip(s, b):
    """record b with the low bit of the opening's last scalar f flipped: every point still decompresses and every scalar is
    canonical, so the pass rejects nothing and only the opening check fails"""
    proof = s.pairs[b][1]
    at = len(proof) - 32
    return s.record(s.pairs[b][0][0], proof[:at] + bytes([proof[at] ^ 1]) + proof[at + 1:], index=b)


def _both(s, records, want_path, name=""):
    """the accumulated call under two seeds against bzh_verify_records_device on the same records"""
    ref_res, ref_st = s.run(records)
    for seed in (SEED_A, SEED_B):
        res, st, path = s.vk.verify_records_accumulated(s.ctx, s.tables, records, s.n_inputs, seed=seed, g0_u_w=s.g0)
        assert res == ref_res and list(st) == list(ref_st), (name, res, ref_res, list(st), list(ref_st))
        assert path == want_path, (name, path)
    return ref_res, list(ref_st)


def _cases(s):
    B = len(s.valid)
    assert _both(s, list(s.valid), 0, "all valid") == ([True] * B, [0] * B)
    for pos in (0, B // 2, B - 1):
        recs = list(s.valid)
        recs[pos] = _flip(s, pos)
        want = [b != pos for b in range(B)]
        assert s.run(recs)[0] == want                                       # the existing call rejects exactly that record
        assert _both(s, recs, 1, "flipped %d" % pos) == (want, [0] * B)
    p = O.FP.p
    recs = [s.valid[0], _input(s.valid[1], 0, p), s.valid[2]]
    assert _both(s, recs, 0, "non-canonical input") == ([True, False, True], [0, 1, 0])
    short = s.record(s.pairs[1][0][0], s.pairs[1][1][:-32])
    assert _both(s, [s.valid[0], short, s.valid[2]], 0, "wrong length") == ([True, False, True], [0, 1, 0])
    assert _both(s, [short, _input(s.valid[0], 0, p)], 0, "every record refused") == ([False, False], [1, 1])
    assert _both(s, [s.valid[1]], 0, "B = 1") == ([True], [0])
    assert _both(s, [_flip(s, 1)], 1, "B = 1 flipped") == ([False], [0])


def _shift_f(s, b, delta):
    """record b with delta added to the opening's last scalar f: its left side moves by -[delta] W, nothing else changes"""
    r = O.FP.p
    proof = s.pairs[b][1]
    at = len(proof) - 32
    f = (int.from_bytes(proof[at:], "little") + delta) % r
    return s.record(s.pairs[b][0][0], proof[:at] + f.to_bytes(32, "little"), index=b)


@pytest.mark.parametrize("g0", [True, False])
def test_the_seeds_weights_reach_the_device_through_the_records_door(sample, g0):
    """The front door's weights are bzh_accumulation_weights(seed), exactly: two records forged for a KNOWN seed -- f_0 + w_1 t and
    f_1 - w_0 t, so that w_0 (-w_1 t W) + w_1 (w_0 t W) = 0 -- pass the accumulated check under that seed (what the SECURITY
    paragraph warns of: a seed the author can predict) and only under it.  Weights that arrive changed, zeroed or shifted by
    one record make the pair fail and the call fall back; under any other seed the pair is rejected as the per-record call
    rejects it.  With and without g0_u_w (the weights lie behind it in the upload), among valid neighbours, and in a batch of 65."""
    import bzh2
    s = sample
    r = O.FP.p
    kw = dict(g0_u_w=s.g0) if g0 else {}
    for B, (i, j) in ((2, (0, 1)), (3, (0, 2)), (65, (7, 64))):
        w = bzh2.accumulation_weights(bzh2.CURVE_VESTA, SEED_A, B)
        t = 0x1234567 + B
        recs = [s.valid[b % 3] for b in range(B)]
        recs[i], recs[j] = _shift_f(s, i % 3, w[j] * t % r), _shift_f(s, j % 3, -w[i] * t % r)
        honest = [b not in (i, j) for b in range(B)]
        assert s.run(recs)[0] == honest                                     # each of the two is invalid on its own
        res, st, path = s.vk.verify_records_accumulated(s.ctx, s.tables, recs, 1, seed=SEED_A, **kw)
        assert path == 0 and res == [True] * B, (B, path, res)             # the forged pair cancels: these ARE the seed's weights
        res, st, path = s.vk.verify_records_accumulated(s.ctx, s.tables, recs, 1, seed=SEED_B, **kw)
        assert path == 1 and res == honest, (B, path, res)
        # the same pair forged for the weights of the neighbouring positions does not cancel
        recs[i], recs[j] = _shift_f(s, i % 3, w[i] * t % r), _shift_f(s, j % 3, -w[j] * t % r)
        res, st, path = s.vk.verify_records_accumulated(s.ctx, s.tables, recs, 1, seed=SEED_A, **kw)
        assert path == 1 and res == honest, (B, path, res)


def test_the_seeds_weights_reach_the_device_through_the_batch_door(sample):
    import bzh2
    s = sample
    r = O.FP.p
    insts, proofs = [p[0] for p in s.pairs], [p[1] for p in s.pairs]
    w = bzh2.accumulation_weights(bzh2.CURVE_VESTA, SEED_B, 3)
    t = 0x7654321

    def shift(pr, delta):
        f = (int.from_bytes(pr[-32:], "little") + delta) % r
        return pr[:-32] + f.to_bytes(32, "little")

    pp = [shift(proofs[0], w[2] * t % r), proofs[1], shift(proofs[2], -w[0] * t % r)]
    assert s.vk.verify_batch_accumulated(s.ctx, s.tables, insts, pp, seed=SEED_B, g0_u_w=s.g0) == ([True] * 3, 0)
    assert s.vk.verify_batch_accumulated(s.ctx, s.tables, insts, pp, seed=SEED_A, g0_u_w=s.g0) == ([False, True, False], 1)


def test_records_sample_circuit(sample):
    _cases(sample)


def test_records_shot_k11(shot):
    _cases(shot)


def test_records_65_at_k5_and_the_existing_call_afterwards(sample):
    s = sample
    recs = [s.valid[b % 3] for b in range(65)]
    assert _both(s, recs, 0, "65 valid")[0] == [True] * 65
    recs[64] = _flip(s, 64 % 3)
    want = [True] * 64 + [False]
    assert _both(s, recs, 1, "65, the last flipped")[0] == want
    # a damaged proof the pass rejects (a point off the curve, ..) is excluded, not a fallback
    bad = [s.record(s.pairs[1][0][0], pr) for _, pr, _ in VP.damaged(1, s.pairs[1][1], s.pairs[1][1])]
    ref = s.run([s.valid[0]] + bad + [s.valid[2]])
    got = s.vk.verify_records_accumulated(s.ctx, s.tables, [s.valid[0]] + bad + [s.valid[2]], 1, seed=SEED_A, g0_u_w=s.g0)
    assert got[0] == ref[0] and list(got[1]) == list(ref[1]) and got[0][0] and got[0][-1]
    # the existing call after an accumulated one that fell back, same key and ctx: shared workspace, in-place conversion
    assert s.run(recs)[0] == want
    assert s.run(list(s.valid)) [0] == [True] * 3
    assert s.vk.verify_records_accumulated(s.ctx, s.tables, list(s.valid), 1, g0_u_w=s.g0)[2] == 0     # seed = None: os.urandom


@pytest.mark.parametrize("lagrange", [True, False])
def test_batch_door_against_the_device_pass(sample, lagrange):
    from bzh2 import native as N
    s = sample
    insts, proofs = [p[0] for p in s.pairs], [p[1] for p in s.pairs]

    def both(ii, pp, want_path, name):
        ref = s.vk.verify_batch(s.ctx, s.tables, ii, pp, lagrange=lagrange, g0_u_w=s.g0, pass_where=N.VERIFY_PASS_DEVICE)
        for seed in (SEED_A, SEED_B):
            res, path = s.vk.verify_batch_accumulated(s.ctx, s.tables, ii, pp, seed=seed, lagrange=lagrange, g0_u_w=s.g0)
            assert res == ref and path == want_path, (name, res, ref, path)
        return ref

    assert both(insts, proofs, 0, "all valid") == [True] * 3
    for pos in range(3):
        pr = proofs[pos]
        pp = list(proofs)
        pp[pos] = pr[:-32] + bytes([pr[-32] ^ 1]) + pr[-31:]
        assert both(insts, pp, 1, "flipped") == [b != pos for b in range(3)]
    assert both(insts, [proofs[0], proofs[1][:-32], proofs[2]], 0, "wrong length") == [True, False, True]
    assert both(insts[:2], [proofs[0][:-1], proofs[1] + b"\0"], 0, "every proof refused") == [False, False]
    assert both([insts[1]], [proofs[1]], 0, "B = 1") == [True]
    assert both([insts[1], insts[0], insts[2]], proofs, 1, "instances swapped") == [False, False, True]
    ii, pp = [insts[b % 3] for b in range(65)], [proofs[b % 3] for b in range(65)]
    assert both(ii, pp, 0, "65 valid") == [True] * 65
    assert s.vk.verify_batch(s.ctx, s.tables, insts, proofs, g0_u_w=s.g0, pass_where=N.VERIFY_PASS_DEVICE) == [True] * 3
