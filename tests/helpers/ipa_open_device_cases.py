"""Shared pieces of tests/test_gpu_ipa_open_device.py: seeded openings, primed transcripts, and the two paths -- bzh_ipa_open_batch
on host transcripts, bzh_ipa_open_batch_device on a device-resident batch loaded from identically primed host transcripts.
Run as a program it is ONE process = one setting of BZH_IPA_COLLAPSE / BZH_IPA_TAIL_C (read once per process): it opens k = 6,
B = 3 on a window table both ways and prints PARITY and a digest of the bytes."""
import functools
import hashlib
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (os.path.join(ROOT, "battlezips-halo2_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402

import coracle as C  # noqa: E402
import pasta as O  # noqa: E402


@functools.lru_cache(maxsize=None)
def srs(cid, k):
    """(g, w, u) as tests/test_gpu_ipa.py's setup_case draws them"""
    from test_gpu_ipa import setup_case
    return setup_case(cid, k, 100 * cid + k)[2:5]


@functools.lru_cache(maxsize=None)
def operands(cid, k, B, seed=0):
    """B openings: polys (ints), blinds, x3s, the 64-byte draws; proof 1 of a batch opens the zero polynomial"""
    F = O.CURVE_BY_ID[cid].scalar
    rng = random.Random(7000 + 100 * cid + 10 * k + B + seed)
    n = 1 << k
    polys = [[rng.randrange(F.p) for _ in range(n)] for _ in range(B)]
    if B > 1:
        polys[1] = [0] * n
    blinds = [rng.randrange(F.p) for _ in range(B)]
    x3s = [rng.randrange(F.p) for _ in range(B)]
    rbs = [rng.randbytes(64 * (n + 1 + 2 * k)) for _ in range(B)]
    return polys, blinds, x3s, rbs


def prime_args(cid, b):
    """what every transcript absorbs before the opening: a written point, a common point, a scalar, then one squeeze -- the block
    buffer is part-filled (65 + 65 + 33 + 1 = 164 = 128 + 36 bytes), the state is not the initial one and the proof is not empty"""
    cv = O.CURVE_BY_ID[cid]
    rng = random.Random(31 * cid + b)
    return cv.random_point(rng), cv.random_point(rng), rng.randrange(cv.scalar.p)


def primed(cid, B):
    import bzh2
    trs = []
    for b in range(B):
        p1, p2, s = prime_args(cid, b)
        t = bzh2.Transcript(bzh2.CURVE_SCALAR_FIELD[cid])
        t.write_point(cid, p1)
        t.common_point(p2)
        t.common_scalar(s)
        t.squeeze_challenge()
        trs.append(t)
    return trs


def primed_oracle(cid, b):
    cv = O.CURVE_BY_ID[cid]
    p1, p2, s = prime_args(cid, b)
    ot = O.Blake2bTranscript(cv.scalar)
    ot.write_point(cv, p1)
    ot.common_point(cv, p2)
    ot.common_scalar(s)
    ot.squeeze_challenge()
    return ot


def proof_cap(k):
    return 32 + 32 * (1 + 2 * k) + 64   # the primed point, then S, (L_j, R_j), c, f


def upload(ctx, cid, k, precompute):
    g, w, u = srs(cid, k)
    hb = ctx.upload_bases(cid, C.points_to_array(list(g) + [u, w]))
    if precompute:
        hb.precompute()
    return hb


def poly_array(polys):
    return np.stack([C.ints_to_array(p) for p in polys])


def host_path(ctx, hb, cid, k, B, seed=0):
    """bzh_ipa_open_batch on primed host transcripts: (v ints, proofs, one further challenge each)"""
    polys, blinds, x3s, rbs = operands(cid, k, B, seed)
    trs = primed(cid, B)
    v = ctx.ipa_open_batch(hb, poly_array(polys), blinds, x3s, list(rbs), trs)
    out = v, [t.proof() for t in trs], [t.squeeze_challenge() for t in trs]
    for t in trs:
        t.close()
    return out


def device_path(ctx, hb, cid, k, B, seed=0):
    """bzh_ipa_open_batch_device (host operands) on a device batch loaded from primed host transcripts: the same triple, the
    opening's status bytes and the batch's own"""
    import bzh2
    polys, blinds, x3s, rbs = operands(cid, k, B, seed)
    trs = primed(cid, B)
    with bzh2.TranscriptBatch(cid, B, proof_cap(k), ctx) as tb:
        tb.from_host(trs)
        v, st = tb.ipa_open(hb, poly_array(polys), blinds, x3s, list(rbs))
        proofs = tb.proofs()
        tb_st = tb.status()
        tb.to_host(trs)
    out = [bzh2.limbs_to_int(x) for x in v], proofs, [t.squeeze_challenge() for t in trs]
    for t in trs:
        t.close()
    return out, st, tb_st


def main():
    import bzh2
    ctx = bzh2.Context(0)
    cid, k, B = 0, 6, 3
    hb = upload(ctx, cid, k, True)
    want = host_path(ctx, hb, cid, k, B)
    got, st, tb_st = device_path(ctx, hb, cid, k, B)
    hb.free()
    ctx.close()
    ok = got == want and not st.any() and not tb_st.any()
    print("PARITY", "ok" if ok else "MISMATCH")
    print("DIGEST", hashlib.sha256(b"".join(want[1])).hexdigest())


if __name__ == "__main__":
    main()
