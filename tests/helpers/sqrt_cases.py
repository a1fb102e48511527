"""TEST HELPER (pure Python, no GPU, no library): expected values and inputs for bzh_batch_sqrt and bzh_affine_decompress,
from Python integers over oracle/pasta.py's fields and curves.

The root is the one pasta_curves 0.4.1's `sqrt` returns: with p - 1 = 2^S T, g = gen^T and t in [0, 2^S) such that
u^T g^t = 1 (t is even exactly when u is a square), it is u^((T+1)/2) g^(t/2).  `ref_sqrt` finds t bit by bit."""
from __future__ import annotations

import functools
import random

import pasta as O
from helpers import field_edges as E

FIELDS = {0: O.FP, 1: O.FQ, 2: O.BN_FR, 3: O.BN_FQ}
SIZES = (1, 63, 64, 65, 300)
POINT_OK, POINT_IDENTITY, POINT_INVALID = 0, 1, 2


def sylow_log(F, u: int) -> int:
    """t in [0, 2^S) with u^T g^t = 1, bit by bit from the bottom (u != 0)"""
    p, S = F.p, F.S
    cur, t = pow(u, (p - 1) >> S, p), 0
    for i in range(S):
        if pow(cur, 1 << (S - 1 - i), p) != 1:
            t |= 1 << i
            cur = cur * pow(F.root, 1 << i, p) % p
    assert cur == 1
    return t


def ref_sqrt(F, u: int):
    """the root, or None for a non-square"""
    p = F.p
    if u % p == 0:
        return 0
    t = sylow_log(F, u)
    if t & 1:
        return None
    T = (p - 1) >> F.S
    r = pow(u, (T + 1) // 2, p) * pow(F.root, t >> 1, p) % p
    assert r * r % p == u % p
    return r


@functools.lru_cache(maxsize=None)
def sqrt_cases(fid: int):
    """[(u, root or None)]: the squares of the issue's list, then gen * a for each of them (all non-squares), shuffled with a
    fixed seed so that squares and non-squares share waves"""
    F = FIELDS[fid]
    p, S, g = F.p, F.S, F.root
    T = (p - 1) >> S
    rng = random.Random(0x5157 + fid)

    def odd_order():
        return pow(rng.randrange(2, p), 1 << S, p)

    squares = [1, 4]
    for j in range(S):                                   # every bit position is the lowest set bit of t once
        squares.append(pow(pow(g, 1 << j, p) * odd_order() % p, 2, p))
    mask = (1 << (S - 1)) - 1
    for h in sorted({mask, 0x55555555 & mask, 0x2aaaaaaa & mask}):   # t / 2 = h: u = (g^e c)^2 with 2 e T = -2 h mod 2^S
        e = (-h * pow(T, -1, 1 << S)) % (1 << S)
        u = pow(pow(g, e, p) * odd_order() % p, 2, p)
        assert sylow_log(F, u) == 2 * h
        squares.append(u)
    squares += [a * a % p for a in E.edge_values(p)]
    uniform = [rng.randrange(p) for _ in range(64)]
    squares = [a for a in dict.fromkeys(squares) if a]
    vals = [0, p - 1, F.g] + squares + uniform + [F.g * a % p for a in squares]
    cases = [(u, ref_sqrt(F, u)) for u in dict.fromkeys(vals)]
    assert all(r is not None for u, r in cases if u in set(squares)) and ref_sqrt(F, F.g) is None
    assert all(ref_sqrt(F, F.g * a % p) is None for a in squares[:8])
    nonsq = sum(1 for _, r in cases if r is None)
    assert nonsq >= len(squares) and len(cases) - nonsq >= len(squares)
    rng.shuffle(cases)
    return cases


def curve_of(cid: int):
    return O.CURVE_BY_ID[cid]


def ref_decompress(cid: int, raw: bytes):
    """(status, x, y) of pasta_curves from_bytes on 32 bytes"""
    cv = curve_of(cid)
    F, p = cv.base, cv.base.p
    v = int.from_bytes(raw, "little")
    sign, x = v >> 255, v & ((1 << 255) - 1)
    if x == 0:
        return (POINT_INVALID, 0, 0) if sign else (POINT_IDENTITY, 0, 0)
    if x >= p:
        return POINT_INVALID, 0, 0
    y = ref_sqrt(F, (x * x * x + cv.b) % p)
    if y is None:
        return POINT_INVALID, 0, 0
    if (y & 1) != sign:
        y = p - y
    return POINT_OK, x, y


@functools.lru_cache(maxsize=None)
def decompress_cases(cid: int):
    """(strings, points, expected): `points` are the random points whose compression opens `strings` (both parities); then the
    identity, zeros with the sign bit, x = p, p + 1, 2^255 - 1 (with and without the sign bit), and x off the curve; shuffled
    with a fixed seed, the special strings spread over the first 60 places, so that valid and invalid lanes share a wave.  expected[i] = (status, x, y)."""
    cv = curve_of(cid)
    F, p = cv.base, cv.base.p
    rng = random.Random(0xdec0 + cid)
    pts = []
    while len(pts) < 162 or len({y & 1 for _, y in pts}) < 2:
        x = rng.randrange(1, p)
        y = ref_sqrt(F, (x * x * x + cv.b) % p)
        if y is None:
            continue
        pts.append((x, y if rng.getrandbits(1) else p - y))
    strings = [(x | ((y & 1) << 255)).to_bytes(32, "little") for x, y in pts]
    extra = [bytes(32), (1 << 255).to_bytes(32, "little")]
    for x in (p, p + 1, (1 << 255) - 1):
        extra += [x.to_bytes(32, "little"), (x | (1 << 255)).to_bytes(32, "little")]
    off = []
    while len(off) < 130:
        x = rng.randrange(1, p)
        if ref_sqrt(F, (x * x * x + cv.b) % p) is None:
            off.append((x | (rng.getrandbits(1) << 255)).to_bytes(32, "little"))
    mixed = strings + off
    rng.shuffle(mixed)
    for j, e in enumerate(extra):          # the special strings sit among the first 60, so every wave size of SIZES but 1 has them
        mixed.insert(3 + 7 * j, e)
    return strings, pts, mixed, [ref_decompress(cid, s) for s in mixed]


def limbs_bytes(ints) -> bytes:
    return b"".join(int(v).to_bytes(32, "little") for v in ints)


def to_form(v: int, p: int, form: int) -> int:
    """canonical integer -> the integer whose limbs the library reads / writes in `form` (1 = Montgomery)"""
    return v * E.R % p if form == 1 else v
