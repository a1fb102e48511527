"""TEST HELPER (pure Python + numpy, no GPU, no library): Jacobian inputs and expected outputs for bzh_batch_normalize and
bzh_affine_compress_batch, from Python integers over oracle/pasta.py's curves (x = X / Z^2, y = Y / Z^3, and its to_bytes rule).

A case is a list of canonical integer triples (X, Y, Z).  They are built from known affine points -- small multiples of the
generator through the oracle's group law -- as (x Z^2, y Z^3, Z), so the expected affine point is known twice over: from the
construction and from the division."""
from __future__ import annotations

import functools
import random

import numpy as np

import pasta as O

R = 1 << 256
POINT_OK, POINT_IDENTITY, POINT_INVALID = 0, 1, 2
GENERATORS = {0: (O.VESTA.p - 1, 2), 1: (O.PALLAS.p - 1, 2), 2: (1, 2)}
CPU_SIZES = (1, 2, 7, 64, 257)
GPU_SIZES = (1, 63, 64, 65, 255, 256, 257)


def curve_of(cid: int):
    return O.CURVE_BY_ID[cid]


@functools.lru_cache(maxsize=None)
def affine_points(cid: int):
    """[k] G for k = 1 .. 40 (oracle group law); both parities of y occur"""
    cv, g = curve_of(cid), GENERATORS[cid]
    assert cv.is_on_curve(g)
    pts, acc = [], None
    for _ in range(40):
        acc = cv.add(acc, g)
        pts.append(acc)
    assert all(cv.is_on_curve(pt) for pt in pts) and {pt[1] & 1 for pt in pts} == {0, 1}
    return pts


def lift(pt, z: int, p: int):
    """the Jacobian triple of an affine point under Z = z"""
    return (pt[0] * z * z % p, pt[1] * z * z * z % p, z % p)


def full_words(p: int) -> int:
    """a value below p whose eight 32-bit words are all non-zero"""
    v = int.from_bytes(bytes(range(0x11, 0x31)), "little") % (1 << (p.bit_length() - 1))
    assert v < p and all((v >> (32 * i)) & 0xFFFFFFFF for i in range(8))
    return v


@functools.lru_cache(maxsize=None)
def edge_set(cid: int):
    """The hand-placed part: Z in {1, 2, p - 1, all words non-zero} on a point of each parity; a point and its negation side by
    side; one point under two different Z; Z = 0 with arbitrary X and Y (also X = Y = 0); then points under random Z."""
    cv = curve_of(cid)
    p, pts = cv.p, affine_points(cid)
    rng = random.Random(0x6e6f + cid)
    even = next(pt for pt in pts if pt[1] & 1 == 0)
    odd = next(pt for pt in pts if pt[1] & 1 == 1)
    out = []
    for z in (1, 2, p - 1, full_words(p)):
        out += [lift(even, z, p), lift(odd, z, p)]
    z = rng.randrange(1, p)
    out += [lift(pts[4], z, p), lift(cv.neg(pts[4]), z, p)]
    out += [lift(pts[5], rng.randrange(1, p), p), lift(cv.neg(pts[5]), rng.randrange(1, p), p)]
    out += [lift(pts[6], rng.randrange(1, p), p), lift(pts[6], rng.randrange(1, p), p)]
    out += [(rng.randrange(p), rng.randrange(p), 0), (0, 0, 0), (p - 1, 1, 0)]
    out += [lift(pt, rng.randrange(1, p), p) for pt in pts]
    return out


def batch(cid: int, n: int, seed: int = 0, identities=()):
    """n triples: the edge set cycled -- from the second round on under a fresh random Z --, then Z = 0 (arbitrary X, Y) at the
    indices in `identities`"""
    p, es = curve_of(cid).p, edge_set(cid)
    rng = random.Random(0x6a61 + 31 * cid + seed)
    out = []
    for i in range(n):
        X, Y, Z = es[i % len(es)]
        if i >= len(es) and Z:
            s = rng.randrange(1, p)                      # (X, Y, Z) ~ (X s^2, Y s^3, Z s)
            X, Y, Z = X * s * s % p, Y * s * s * s % p, Z * s % p
        out.append((X, Y, Z))
    for i in identities:
        out[i] = (rng.randrange(p), rng.randrange(p), 0)
    return out


def expected(cid: int, triples):
    """[(status, x, y, to_bytes)] by integer division in the base field"""
    cv = curve_of(cid)
    p, out = cv.p, []
    for X, Y, Z in triples:
        if Z % p == 0:
            out.append((POINT_IDENTITY, 0, 0, cv.compress(None)))
            continue
        zi = cv.base.inv(Z)
        pt = (X * zi * zi % p, Y * zi * zi * zi % p)
        out.append((POINT_OK, pt[0], pt[1], cv.compress(pt)))
    return out


def to_form(v: int, p: int, form: int) -> int:
    """canonical integer -> the integer whose limbs the library reads / writes in `form` (1 = Montgomery)"""
    return v * R % p if form == 1 else v


def limbs_bytes(ints) -> bytes:
    return b"".join(int(v).to_bytes(32, "little") for v in ints)


def jac_array(cid: int, triples, form: int) -> np.ndarray:
    p = curve_of(cid).p
    raw = limbs_bytes(to_form(c, p, form) for t in triples for c in t)
    return np.frombuffer(raw, dtype=np.uint64).reshape(-1, 12).copy()


def want_xy_bytes(cid: int, exp, form: int) -> bytes:
    p = curve_of(cid).p
    return limbs_bytes(to_form(c, p, form) for e in exp for c in e[1:3])


def want_enc_bytes(exp) -> bytes:
    return b"".join(e[3] for e in exp)


def want_status(exp) -> list:
    return [e[0] for e in exp]


def smallest_n_with_chain(plan, c: int) -> int:
    """the smallest n with plan(n).chain >= c, by bisection (the chain is monotone in n: test_normalize_compress_cpu.py)"""
    lo, hi = 1, 2
    while plan(hi)[1] < c:
        hi *= 2
        assert hi <= 1 << 28, "no n reaches chain %d" % c
    while lo < hi:
        mid = (lo + hi) // 2
        if plan(mid)[1] >= c:
            hi = mid
        else:
            lo = mid + 1
    return lo


def chain_indices(n: int, lanes: int, t: int) -> list:
    """the points lane t owns"""
    return list(range(t, n, lanes))
