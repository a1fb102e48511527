"""TEST HELPER (pure Python + numpy, no GPU): schedules, operands and expected results for bzh_transcript_batch_*.

A schedule is a list of (op, count): op is one of OPS, count the items every transcript of the batch takes in that call (1 for a
squeeze).  The expected challenges and proof bytes come from oracle/pasta.py's Blake2bTranscript -- hashlib.blake2b --, one per
transcript; run_host_objects gives the library's own second opinion, the host bzh_transcript objects fed the same items.

A point costs 65 bytes, a scalar 33, a squeeze 1; the block is 128 bytes.  The schedules are built from that arithmetic and the
arithmetic is asserted here (trace), so that a schedule that stops reaching its edge fails in the helper, not silently."""
from __future__ import annotations

import functools
import random

import numpy as np

import pasta as O
from helpers import normalize_cases as K

OPS = ("common_points", "write_points", "common_scalars", "write_scalars", "squeeze")
ITEM_BYTES = {"common_points": 65, "write_points": 65, "common_scalars": 33, "write_scalars": 33, "squeeze": 1}
BLOCK = 128
POINT_OK, POINT_IDENTITY, POINT_INVALID = 0, 1, 2


def trace(schedule):
    """[(op, item index in its call, first byte, one past the last byte)] for every item of one transcript, in order"""
    out, pos = [], 0
    for op, count in schedule:
        assert op in OPS and count >= 1 and (op != "squeeze" or count == 1)
        for i in range(count):
            out.append((op, i, pos, pos + ITEM_BYTES[op]))
            pos += ITEM_BYTES[op]
    return out


def far_sides(schedule):
    """for every item that straddles a block edge: (op, bytes on the far side)"""
    return [(op, end % BLOCK) for op, _, start, end in trace(schedule) if start // BLOCK != (end - 1) // BLOCK]


@functools.lru_cache(maxsize=None)
def block_edge_schedule():
    """one point, one scalar, 31 squeezes: 65 + 33 + 30 = 128.  The 30th squeeze finalises a FULL last block; the 31st first has
    to compress that block as a non-last one (the lazy rule of csrc/blake2b.hpp)."""
    sched = (("write_points", 1), ("write_scalars", 1)) + (("squeeze", 1),) * 31
    tr = trace(sched)
    sq = [t for t in tr if t[0] == "squeeze"]
    assert sq[29][3] == BLOCK                                  # after the 30th squeeze's byte the buffer holds exactly one full block
    assert sq[30][2] == BLOCK and sq[30][3] == BLOCK + 1       # the 31st adds a byte to a full buffer: compress, then one byte
    assert not far_sides(sched)                                # nothing straddles: the edge is met exactly
    return sched


def _filler(residue):
    """the shortest (scalars, points, squeezes) with 33 a + 65 b + c = residue mod 128"""
    best = None
    for a in range(8):
        for b in range(8):
            c = (residue - 33 * a - 65 * b) % BLOCK
            if best is None or a + b + c < sum(best):
                best = (a, b, c)
    return best


@functools.lru_cache(maxsize=None)
def straddle_schedule():
    """items that straddle a block edge with 1, 7, 8, 9, 63 and 64 bytes on the far side -- one byte, the last byte of a word, a
    whole word, a word and a byte, and about half of a point (64 is all of a point but its first byte) --, each behind the
    shortest prefix of scalars, points and squeezes that puts it there, and each followed by a squeeze"""
    targets = ((1, "write_scalars"), (7, "write_points"), (8, "common_scalars"), (9, "common_points"), (63, "write_points"),
               (64, "common_points"), (1, "common_points"), (8, "write_points"))
    sched, pos = [], 0
    for far, op in targets:
        L = ITEM_BYTES[op]
        assert 0 < far < L
        a, b, c = _filler((far - L - pos) % BLOCK)
        for fop, cnt in (("write_scalars", a), ("common_points", b)):
            if cnt:
                sched.append((fop, cnt))
        sched += [("squeeze", 1)] * c
        sched += [(op, 1), ("squeeze", 1)]
        pos = trace(sched)[-1][3]
    sched = tuple(sched)
    got = far_sides(sched)
    for far, op in targets:
        assert (op, far) in got, (op, far)
    assert {f for _, f in got} >= {1, 7, 8, 9, 63, 64}
    return sched


@functools.lru_cache(maxsize=None)
def proof_schedule():
    """shaped like one Board proof (about 60 points, 60 scalars, the IPA's 14 rounds of two points and a challenge, and the
    challenges between): what tools/ubench_transcript.py times"""
    import importlib.util
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))), "tools", "ubench_transcript.py")
    spec = importlib.util.spec_from_file_location("ubench_transcript", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    s = tuple(mod.SCHEDULE)
    assert sum(s[j:j + 2] == (("write_points", 2), ("squeeze", 1)) for j in range(len(s))) >= 14      # the IPA's rounds
    n_pts = sum(c for op, c in s if op.endswith("points"))
    n_sc = sum(c for op, c in s if op.endswith("scalars"))
    assert 55 <= n_pts <= 65 and 55 <= n_sc <= 65 and len(far_sides(s)) > 40
    return s


SCHEDULES = {"block_edge": block_edge_schedule, "straddle": straddle_schedule, "proof": proof_schedule}


def proof_bytes(schedule) -> int:
    return 32 * sum(c for op, c in schedule if op.startswith("write"))


# ---- operands ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def operands(cid: int, name: str, batch: int):
    """per call of the schedule: None (a squeeze) or [transcript][item] of canonical operands -- (x, y) for a point, an int for a
    scalar.  Every transcript gets its own seeded uniform values; every fourth item (shifted by the transcript's index) is one of
    the hand-placed values instead: coordinates and scalars 0, 1 and p - 1, a point next to its negation.  In the first and in
    the largest point call the transcripts with b % 4 = 1, 2, 3 get the identity (0, 0) as the first, a middle and the last item."""
    sched = SCHEDULES[name]()
    cv = K.curve_of(cid)
    p, r = cv.p, cv.scalar.p
    pts = K.affine_points(cid)
    point_calls = [j for j, (op, _) in enumerate(sched) if op.endswith("points")]
    id_calls = {point_calls[0], max(point_calls, key=lambda j: sched[j][1])}
    special_pts = [(0, 1), (1, 0), (p - 1, p - 1), (1, p - 1), "pair"]
    special_sc = [0, 1, r - 1]
    seen = set()
    calls = [None if op == "squeeze" else [[None] * cnt for _ in range(batch)] for op, cnt in sched]
    for b in range(batch):
        rng = random.Random((0x7472 + 977 * cid + 31 * batch) * 1000003 + b)
        k, pending = 0, None
        for j, (op, cnt) in enumerate(sched):
            if op == "squeeze":
                continue
            for i in range(cnt):
                special = (k + b) % 4 == 0
                if op.endswith("points"):
                    v = (rng.randrange(p), rng.randrange(p))
                    if pending is not None:
                        v, pending = pending, None
                        seen.add("negation")
                    elif special:
                        v = special_pts[((k + b) // 4) % len(special_pts)]
                        if v == "pair":
                            v = pts[(k + b) % len(pts)]
                            pending = cv.neg(v)
                        else:
                            seen.add(v)
                    ident = {1: 0, 2: cnt // 2, 3: cnt - 1}.get(b % 4)
                    if j in id_calls and ident == i:
                        v = (0, 0)
                        seen.add(("identity", b % 4))
                else:
                    v = rng.randrange(r)
                    if special:
                        v = special_sc[((k + b) // 4) % len(special_sc)]
                        seen.add(("scalar", v))
                calls[j][b][i] = v
                k += 1
    if batch >= 65 and name == "proof":
        want = {(0, 1), (1, 0), (p - 1, p - 1), (1, p - 1), "negation", ("identity", 1), ("identity", 2), ("identity", 3),
                ("scalar", 0), ("scalar", 1), ("scalar", r - 1)}
        assert want <= seen, want - seen
    if batch > 1:
        firsts = [next(c for c in calls if c is not None)[b] for b in range(batch)]
        assert len({repr(f) for f in firsts}) > 1              # the transcripts do not share their data
    return calls


def expected_status(cid: int, name: str, batch: int):
    st = [POINT_OK] * batch
    for (op, _), call in zip(SCHEDULES[name](), operands(cid, name, batch)):
        if call is not None and op.endswith("points"):
            for b in range(batch):
                if (0, 0) in call[b]:
                    st[b] = POINT_IDENTITY
    return st


def as_array(cid: int, op: str, call, form: int) -> np.ndarray:
    """one call's operands as (batch, count, limbs) uint64 in `form`"""
    cv = K.curve_of(cid)
    if op.endswith("points"):
        ints = (K.to_form(c, cv.p, form) for row in call for pt in row for c in pt)
        limbs = 8
    else:
        ints = (K.to_form(s, cv.scalar.p, form) for row in call for s in row)
        limbs = 4
    return np.frombuffer(K.limbs_bytes(ints), dtype=np.uint64).reshape(len(call), len(call[0]), limbs).copy()


def _oracle_apply(tr, cv, op, item):
    if op.endswith("points"):
        pt = None if item == (0, 0) else item
        (tr.write_point if op.startswith("write") else tr.common_point)(cv, pt)
    else:
        (tr.write_scalar if op.startswith("write") else tr.common_scalar)(item)


def oracle_run(cid: int, sched, calls, skip=()):
    """(challenges: one list of `batch` ints per squeeze, proofs: `batch` byte strings) from the oracle transcript; the calls
    whose index is in `skip` are left out"""
    cv = K.curve_of(cid)
    batch = len(next(c for c in calls if c is not None))
    trs = [O.Blake2bTranscript(cv.scalar) for _ in range(batch)]
    chal = []
    for j, ((op, _), call) in enumerate(zip(sched, calls)):
        if j in skip:
            continue
        if op == "squeeze":
            chal.append([t.squeeze_challenge() for t in trs])
            continue
        for b, t in enumerate(trs):
            for item in call[b]:
                _oracle_apply(t, cv, op, item)
    return chal, [bytes(t.proof) for t in trs]


@functools.lru_cache(maxsize=None)
def expected(cid: int, name: str, batch: int):
    """the oracle's (challenges, proofs) for a named schedule: computed once, shared by every test that needs it"""
    return oracle_run(cid, SCHEDULES[name](), operands(cid, name, batch))


def host_objects_feed(bzh2, trs, cid, op, call):
    """one call's items into the host bzh_transcript objects `trs`; a squeeze returns their challenges"""
    if op == "squeeze":
        return [t.squeeze_challenge() for t in trs]
    for b, t in enumerate(trs):
        for item in call[b]:
            if op == "write_points":
                t.write_point(cid, item)
            elif op == "common_points":
                t.common_point(item)
            elif op == "write_scalars":
                t.write_scalar(item)
            else:
                t.common_scalar(item)
    return None


def run_host_objects(bzh2, cid: int, sched, calls):
    trs = [bzh2.Transcript(bzh2.CURVE_SCALAR_FIELD[cid]) for _ in range(len(next(c for c in calls if c is not None)))]
    try:
        chal = []
        for (op, _), call in zip(sched, calls):
            got = host_objects_feed(bzh2, trs, cid, op, call)
            if got is not None:
                chal.append(got)
        return chal, [t.proof() for t in trs]
    finally:
        for t in trs:
            t.close()


def challenge_ints(cid: int, arr: np.ndarray, form: int):
    """a squeeze's (batch, 4) limbs in `form` as canonical ints"""
    r = K.curve_of(cid).scalar.p
    inv = pow(K.R, -1, r) if form == 1 else 1
    return [int.from_bytes(row.tobytes(), "little") * inv % r for row in arr]


def run_batch(tb, cid: int, sched, calls, form: int, feed=None, squeeze=None, first=0, last=None):
    """calls [first, last) of a schedule through a TranscriptBatch: the challenges as canonical ints, one list per squeeze.
    feed(op, array) absorbs one call's operands (default: host arrays); squeeze() returns a (batch, 4) array in `form`."""
    feed = feed or (lambda op, arr: getattr(tb, op)(arr, form=form))
    squeeze = squeeze or (lambda: tb.squeeze(form=form))
    chal = []
    for (op, _), call in list(zip(sched, calls))[first:last]:
        if op == "squeeze":
            chal.append(challenge_ints(cid, squeeze(), form))
        else:
            feed(op, as_array(cid, op, call, form))
    return chal
