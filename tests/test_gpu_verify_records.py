"""bzh_verify_records_device (verify_board / verify_shot over a batch of binary records, device-resident) against
bzh_record_decode followed by bzh_verify_batch_vk_with under BZH_VERIFY_PASS_HOST and under BZH_VERIFY_PASS_DEVICE on the same
records: results[] equal both, record by record, and status bit 0 marks exactly the records refused before verification (decode
refuses them, or they carry another n_inputs or another proof length than the call's key).  Shot at k = 11 with batches of 1, 3
and 65 (one full wave and one lane on every one-lane kernel), Board at k = 12 with a batch of 2, and tests/helpers/vk_cases.py's
k = 5 sample circuit for the 65-wide sweep of the damaged proofs of tests/helpers/verify_pass_cases.py.  Proofs come from
bzh_prove_batch_seeded, records from bzh_record_encode; tampered inputs and headers are patched into the encoded bytes.  One
Params, one key and one vk per circuit for the module; a reference decision is computed once per distinct record."""
import ctypes
import struct

import numpy as np
import pytest

import coracle as C
import pasta as O
from helpers import real_parity as R
from helpers import verify_pass_cases as VP
from helpers import vk_cases as V

pytestmark = pytest.mark.gpu
E_ARG = -1
P = O.FP.p
HEADER = 144


def _patch(rec: bytes, at: int, new: bytes) -> bytes:
    return rec[:at] + new + rec[at + len(new):]


def _input(rec: bytes, i: int, value: int) -> bytes:
    return _patch(rec, 16 + 32 * i, int(value).to_bytes(32, "little"))


class Side:
    """one circuit: tables, vk, the proof length of its key, valid (instances, proof) pairs, and the reference decisions"""

    def __init__(self, ctx, tables, vk, n_inputs, insts, proofs, g0_u_w=None):
        from bzh2 import wire as W
        self.ctx, self.tables, self.vk, self.n_inputs, self.g0 = ctx, tables, vk, n_inputs, g0_u_w
        self.plen = len(proofs[0])
        assert all(len(p) == self.plen for p in proofs)
        self.cap = self.plen + 96                                          # room for the longer proofs of the damage list
        self.stride = W.record_stride(self.cap)
        self.pairs = list(zip(insts, proofs))
        self.valid = [self.record(i[0], p, index=b) for b, (i, p) in enumerate(self.pairs)]
        self.known = {}

    def record(self, inputs, proof, kind=1, index=0) -> bytes:
        from bzh2 import wire as W
        return W.BattleZipsRecord([int(v) for v in inputs], proof, kind, index).to_fixed(self.cap)

    def expect(self, records):
        """(results, status) by decode + bzh_verify_batch_vk_with, host pass and device pass, once per distinct record"""
        from bzh2 import native as N, wire as W
        new = [r for r in dict.fromkeys(records) if r not in self.known]
        decoded = []
        for r in new:
            try:
                d = W.BattleZipsRecord.from_fixed(r)
            except ValueError:
                self.known[r] = (False, 1)
                continue
            decoded.append((r, d))
        if decoded:
            insts = [[list(d.commitment)] for _, d in decoded]
            proofs = [d.proof for _, d in decoded]
            kw = dict(g0_u_w=self.g0) if self.g0 is not None else {}
            host = self.vk.verify_batch(self.ctx, self.tables, insts, proofs, pass_where=N.VERIFY_PASS_HOST, **kw)
            dev = self.vk.verify_batch(self.ctx, self.tables, insts, proofs, pass_where=N.VERIFY_PASS_DEVICE, **kw)
            assert host == dev
            for (r, d), ok in zip(decoded, host):
                early = len(d.commitment) != self.n_inputs or len(d.proof) != self.plen
                assert not (early and ok)                                  # what the call refuses early the verifier rejects
                self.known[r] = (ok, 1 if early else 0)
        return [self.known[r][0] for r in records], [self.known[r][1] for r in records]

    def run(self, records, **kw):
        return self.vk.verify_records(self.ctx, self.tables, records, self.n_inputs, g0_u_w=self.g0, **kw)

    def check(self, records, name=""):
        want_res, want_st = self.expect(records)
        res, st = self.run(records)
        assert res == want_res, (name, res, want_res)
        assert list(st) == want_st, (name, list(st), want_st)
        return res, list(st)


class _Srs:
    """the k = 5 sample circuit's tables (as tests/test_gpu_verify_pass.py builds them)"""

    def __init__(self, ctx, k):
        import bzh2
        from bzh2 import params as Pm
        g, w, u = V.srs(k)
        self.g, self.w, self.u = g, w, u
        garr = C.points_to_array(g)
        uw = C.points_to_array([u, w])
        self.bases = ctx.upload_bases(bzh2.CURVE_VESTA, np.concatenate([garr, uw])).precompute(0)
        self.bases_lagrange = ctx.upload_bases(bzh2.CURVE_VESTA, np.concatenate([Pm.group_ifft(ctx, garr), uw])).precompute(0)
        self.g0_u_w = np.ascontiguousarray(np.stack([garr[0], uw[0], uw[1]]))

    def close(self):
        self.bases.free()
        self.bases_lagrange.free()


def _sample_proofs(ctx, srs, k, num_instance, count):
    import bzh2
    from bzh2 import native as N
    cases = [V.circuit(k, 70 + b, num_instance) for b in range(count)]
    pk = N.NativeProvingKey(ctx, cases[0][5], bzh2.CURVE_VESTA, srs.g, srs.w, srs.u)
    n = 1 << k
    adv = np.stack([np.stack([C.ints_to_array(list(col) + [0] * (n - len(col))) for col in cse[3]]) for cse in cases])
    insts = [[list(col) for col in cse[4]] for cse in cases]
    seeds = [R.rng_stream("vrec-%d-%d-%d" % (k, num_instance, b), 32) for b in range(count)]
    return pk, insts, pk.prove_batch(adv, insts, None, seeds=seeds)


def _game_side(ctx, kind, k, count):
    import bzh2
    from bzh2 import circuits as Cm, native as N, params as Pm
    shot = kind == "shot"
    lay = Cm.CircuitLayout(Cm.SHOT if shot else Cm.BOARD, k)
    prm = Pm.Params(ctx, k)
    pk = N.NativeProvingKey(ctx, lay.blob(), bzh2.CURVE_VESTA, params=prm)
    adv, insts = lay.synthesize((R.shot_circuits if shot else R.board_circuits)(Cm, 977, count))
    proofs = pk.prove_batch(adv, insts, None, seeds=[R.rng_stream("vrec-%s-%d" % (kind, b), 32) for b in range(count)])
    vk = N.NativeVerifyingKey.from_pk(pk)
    pk.close()
    lay.close()
    return Side(ctx, prm, vk, 4 if shot else 2, insts, proofs), prm


@pytest.fixture(scope="module")
def shot(gpu_ctx):
    side, prm = _game_side(gpu_ctx, "shot", 11, 3)
    yield side
    side.vk.close()
    prm.close()


@pytest.fixture(scope="module")
def board(gpu_ctx):
    side, prm = _game_side(gpu_ctx, "board", 12, 2)
    yield side
    side.vk.close()
    prm.close()


@pytest.fixture(scope="module")
def sample(gpu_ctx):
    """the k = 5 sample circuit: the one-instance-column side, vks with 0 and 2 instance columns, one k = 6 proof"""
    from bzh2 import native as N
    srs5, srs6 = _Srs(gpu_ctx, V.K), _Srs(gpu_ctx, 6)
    pk6, _, proofs6 = _sample_proofs(gpu_ctx, srs6, 6, 1, 1)
    pk6.close()
    srs6.close()
    pk, insts, proofs = _sample_proofs(gpu_ctx, srs5, V.K, 1, 3)
    side = Side(gpu_ctx, srs5, N.NativeVerifyingKey.from_pk(pk), 1, insts, proofs, g0_u_w=srs5.g0_u_w)
    pk.close()
    others = {}
    for ni in (0, 2):
        pko, _, _ = _sample_proofs(gpu_ctx, srs5, V.K, ni, 1)
        others[ni] = N.NativeVerifyingKey.from_pk(pko)
        pko.close()
    yield side, others, proofs6[0]
    for v in others.values():
        v.close()
    side.vk.close()
    srs5.close()


def _tampered_shot(s):
    """[(name, record)] from the first valid Shot record: none verifies; the canonical ones reach the verifier"""
    (cx, cy, sh, hit), proof = s.pairs[0][0][0], s.pairs[0][1]
    base = s.valid[0]
    moved = sh << 1 if sh < (1 << 99) else sh >> 1
    return [("hit flipped", _input(base, 3, hit ^ 1)), ("shot moved to another cell", _input(base, 2, moved)),
            ("the commitment's y replaced by p - y", _input(base, 1, P - cy)), ("an input equal to p - 1", _input(base, 2, P - 1)),
            ("an input equal to p", _input(base, 2, P)), ("an input equal to 2^256 - 1", _input(base, 3, (1 << 256) - 1)),
            ("all inputs zero", _patch(base, 16, bytes(128)))]


def _corrupt_headers(s):
    base = s.valid[0]
    short = s.record(s.pairs[0][0][0], s.pairs[0][1][:-32])
    return [("proof_len above the stride", _patch(base, 0, struct.pack("<I", s.cap + 1))), ("proof_len different from the key's", short),
            ("n_inputs of 5", _patch(base, 4, b"\x05")), ("n_inputs of 2 in a Shot batch", _patch(base, 4, b"\x02")),
            ("a reserved byte set", _patch(base, 6, b"\x01")), ("the reserved word set", _patch(base, 12, b"\x01"))]


@pytest.mark.parametrize("batch", [1, 3, 65])
def test_shot_records(shot, batch):
    """valid records, the tampered inputs and the corrupt headers at lane 0, at lane 64 and between valid neighbours"""
    s = shot
    bad = _tampered_shot(s) + _corrupt_headers(s)
    if batch == 1:
        for rec in [s.valid[0]] + [r for _, r in bad]:
            s.check([rec])
        return
    if batch == 3:
        assert s.check(list(s.valid))[0] == [True] * 3
        for name, rec in bad:
            res, st = s.check([s.valid[0], rec, s.valid[2]], name)
            assert res == [True, False, True] and st[0] == st[2] == 0, name
        res, st = s.check([bad[4][1], s.valid[1], s.valid[2]])
        assert res == [False, True, True] and st == [1, 0, 0]
        return
    recs = [s.valid[b % 3] for b in range(65)]
    want = [True] * 65
    lanes = [0, 64] + list(range(2, 2 * len(bad) - 2, 2))
    for lane, (_, rec) in zip(lanes, bad):
        recs[lane], want[lane] = rec, False
    res, st = s.check(recs)
    assert res == want
    assert s.run(recs, want_status=False) == (want, None)                   # status = NULL


def test_tampered_inputs_decide_as_the_issue_says(shot):
    """p - 1 is canonical and reaches the verifier (status 0, rejected); p and 2^256 - 1 are refused (status bit 0); all inputs zero
    commits to W itself: rejected, status 0, the neighbours accepted"""
    s = shot
    t = dict(_tampered_shot(s))
    res, st = s.check([s.valid[1], t["an input equal to p - 1"], t["an input equal to p"], t["an input equal to 2^256 - 1"],
                       t["all inputs zero"], s.valid[2]])
    assert res == [True, False, False, False, False, True] and st == [0, 0, 1, 1, 0, 0]
    for name in ("hit flipped", "shot moved to another cell", "the commitment's y replaced by p - y"):
        assert s.check([t[name]], name) == ([False], [0])
    h = dict(_corrupt_headers(s))
    assert s.check(list(h.values())) == ([False] * len(h), [1] * len(h))   # every record of a batch refused


def test_board_records(board):
    s = board
    assert s.check(list(s.valid)) == ([True, True], [0, 0])
    cy = s.pairs[1][0][0][1]
    res, st = s.check([s.valid[0], _input(s.valid[1], 1, P - cy)])
    assert res == [True, False] and st == [0, 0]
    assert s.check([_input(s.valid[0], 0, P), s.valid[1]]) == ([False, True], [1, 0])


def test_damaged_proofs_sweep_one_wave_and_one_lane(sample):
    """the damaged proofs of verify_pass_cases at lane 0, at lane 64 and at every other lane between valid neighbours"""
    s, _, k6 = sample
    inputs = s.pairs[1][0][0]
    bad = [s.record(inputs, pr) for _, pr, _ in VP.damaged(1, s.pairs[1][1], k6)]
    recs = [s.valid[b % 3] for b in range(65)]
    want = [True] * 65
    lanes = [0, 64] + list(range(2, 2 * len(bad) - 2, 2))
    for lane, rec in zip(lanes, bad):
        recs[lane], want[lane] = rec, False
    recs[40], recs[41] = s.record(s.pairs[(41 % 3)][0][0], s.pairs[40 % 3][1]), s.record(s.pairs[40 % 3][0][0], s.pairs[41 % 3][1])
    want[40] = want[41] = False                                             # two neighbours' inputs swapped
    res, st = s.check(recs)
    assert res == want
    assert sum(st) == 3                                                     # one byte short, one byte long, the k = 6 proof
    for rec in (bad[0], bad[5], bad[10]):
        s.check([rec])


def test_arguments_and_housekeeping(gpu_ctx, sample):
    from bzh2 import BzhError, native as N
    s, others, _ = sample
    L = N._bind()
    for ni, vk in others.items():                                           # a vk with 0 and with 2 instance columns
        with pytest.raises(BzhError) as e:
            vk.verify_records(gpu_ctx, s.tables, list(s.valid), 1)
        assert e.value.status == E_ARG, ni

    class NoLagrange:
        bases = s.tables.bases
    with pytest.raises(BzhError) as e:                                      # NULL g_lagrange
        s.vk.verify_records(gpu_ctx, NoLagrange, list(s.valid), 1)
    assert e.value.status == E_ARG
    with pytest.raises(BzhError) as e:                                      # a stride too short for the key's proof length
        s.vk.verify_records(gpu_ctx, s.tables, list(s.valid), 1, record_stride=HEADER + s.plen - 1)
    assert e.value.status == E_ARG
    for n_inputs in (0, 5):
        with pytest.raises(BzhError) as e:
            s.vk.verify_records(gpu_ctx, s.tables, list(s.valid), n_inputs)
        assert e.value.status == E_ARG
    swapped = np.ascontiguousarray(s.g0[[0, 2, 1]])                         # U and W exchanged: not this SRS's points
    with pytest.raises(BzhError) as e:
        s.vk.verify_records(gpu_ctx, s.tables, list(s.valid), 1, g0_u_w=swapped)
    assert e.value.status == E_ARG
    res, st = s.vk.verify_records(gpu_ctx, s.tables, list(s.valid), 1)      # g0_u_w = NULL: the table's own points
    assert res == [True] * 3 and list(st) == [0] * 3
    # batch = 0 touches nothing
    res0 = (ctypes.c_int * 1)(7)
    st0 = np.full(1, 7, dtype=np.uint8)
    buf = np.zeros(16, dtype=np.uint8)
    vp = ctypes.c_void_p
    assert L.bzh_verify_records_device(gpu_ctx.handle, s.vk.handle, s.tables.bases.handle, s.tables.bases_lagrange.handle, 0, 1,
                                       vp(buf.ctypes.data), s.stride, None, res0, vp(st0.ctypes.data)) == 0
    assert res0[0] == 7 and st0[0] == 7
    # two calls in a row on one ctx with different batch sizes: the workspace is reused, the answers stay
    bad = s.record(s.pairs[0][0][0], s.pairs[1][1])
    big = [s.valid[b % 3] for b in range(9)] + [bad]
    small = [bad, s.valid[1]]
    first = s.check(big)
    assert s.check(small) == ([False, True], [0, 0])
    assert s.check(big) == first
    # the vk is usable by bzh_verify_batch_vk afterwards
    insts, proofs = [p[0] for p in s.pairs], [p[1] for p in s.pairs]
    assert s.vk.verify_batch(gpu_ctx, s.tables, insts, proofs, g0_u_w=s.g0) == [True] * 3
