"""TEST HELPER (pure Python, no GPU, no library): the adversarial operand set for the 8 x 32-bit-limb field arithmetic of
csrc/field.cuh and its big-int reference.

The device routines are inline-assembly carry chains; a defect in one of them needs a limb equal to 0, to 0xffffffff or to the
modulus's own limb to show, which operands drawn uniformly below the modulus meet with probability about 2^-32.  `edge_values`
puts those limbs there on purpose; `reference` says what the device computes on raw Montgomery-form bits (R = 2^256);
`targeted_products` makes the structure appear on the OUTPUT side of the Montgomery product.
"""
from __future__ import annotations

import random

R = 1 << 256
M32 = 0xFFFFFFFF
N_EDGE = 256

# field id -> modulus (include/bzh2.h: BZH_FIELD_FP, _FQ, _BN254_FR, _BN254_FQ)
MODULI = {
    0: 0x40000000000000000000000000000000224698fc094cf91b992d30ed00000001,
    1: 0x40000000000000000000000000000000224698fc0994a8dd8c46eb2100000001,
    2: 0x30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000001,
    3: 0x30644e72e131a029b85045b68181585d97816a916871ca8d3c208c16d87cfd47,
}


def limbs(x: int) -> list:
    return [(x >> (32 * i)) & M32 for i in range(8)]


def _structured(p: int) -> list:
    """the listed special values, in a fixed order, each in [0, p), duplicates removed"""
    out, seen = [], set()

    def put(v):
        if 0 <= v < p and v not in seen:
            seen.add(v)
            out.append(v)

    for v in (0, 1, 2, p - 1, p - 2, (p - 1) // 2, (p + 1) // 2, R % p, R * R % p):
        put(v)
    for i in range(1, 8):
        for d in (-1, 0, 1):
            put((1 << (32 * i)) + d)
    put((1 << (p.bit_length() - 1)) - 1)                      # the largest 2^j - 1 below p
    top_mask = (1 << (p.bit_length() - 1 - 224)) - 1          # top limb of an all-ones value that stays below p
    all_ones = ((1 << 224) - 1) | (top_mask << 224)
    for i in range(8):
        put(M32 << (32 * i) if i < 7 else top_mask << 224)    # only limb i set
        put(all_ones & ~(M32 << (32 * i)))                    # every limb set except limb i
    for i in range(1, 8):
        low = p % (1 << (32 * i))                             # the modulus's own low limbs
        for v in (low, low - 1, low + 1, p - (1 << (32 * i))):
            put(v)
    for v in list(out):                                       # closure: a + b in {p, p - 1, p + 1} for every value above
        for w in (p - v, p - v - 1, p - v + 1):
            put(w)
    return out


def edge_values(p: int) -> list:
    """256 distinct values in [0, p): the structured ones first, then seeded uniform values (deterministic)."""
    out = _structured(p)
    assert len(out) <= N_EDGE, "structured part outgrew the set: %d" % len(out)
    seen = set(out)
    rng = random.Random(p & 0xFFFFFFFFFFFF)
    while len(out) < N_EDGE:
        v = rng.randrange(p)
        if v not in seen:
            seen.add(v)
            out.append(v)
    return out


def reference(op: str, a: int, b: int, p: int) -> int:
    """what the device computes on raw Montgomery-form bits a, b < p"""
    if op == "add":
        return (a + b) % p
    if op == "sub":
        return (a - b) % p
    if op == "neg":
        return (-a) % p
    if op == "mul":
        return a * b * pow(R, -1, p) % p
    raise ValueError(op)


def product_targets(p: int) -> list:
    out = []
    for t in [1, 2, (1 << 32) - 1] + [1 << (32 * i) for i in range(1, 8)] + [p - 1, p - 2] + \
            [p % (1 << (32 * i)) for i in range(1, 8)]:
        if 0 < t < p and t not in out:
            out.append(t)
    return out


def targeted_products(p: int, rng: random.Random, per_target: int = 64) -> list:
    """[(x, y, t)]: x random, y = t R x^-1 mod p, so that the Montgomery product x y R^-1 is exactly t -- the accumulator
    before the final conditional subtraction is t or t + p."""
    out = []
    for t in product_targets(p):
        for _ in range(per_target):
            x = rng.randrange(1, p)
            out.append((x, t * R * pow(x, -1, p) % p, t))
    return out


def all_pairs(vals: list):
    """columns A, B of len(vals)^2 rows holding every ordered pair once: A = each value repeated, B = the list tiled"""
    n = len(vals)
    return [v for v in vals for _ in range(n)], list(vals) * n


def pair_statistics(vals: list, p: int) -> dict:
    """counts of ordered pairs (a, b) that reach the corners of the add / sub carry chains"""
    lo4 = (1 << 128) - 1
    st = {"sum_is_p": 0, "sum_is_p_minus_1": 0, "sum_is_p_plus_1": 0, "equal": 0, "sum_ge_2_255": 0, "borrow_low4_equal": 0}
    for a in vals:
        for b in vals:
            s = a + b
            st["sum_is_p"] += s == p
            st["sum_is_p_minus_1"] += s == p - 1
            st["sum_is_p_plus_1"] += s == p + 1
            st["equal"] += a == b
            st["sum_ge_2_255"] += s >= 1 << 255
            st["borrow_low4_equal"] += a < b and (a & lo4) == (b & lo4)
    return st


def ints_to_array(xs):
    import numpy as np
    return np.frombuffer(b"".join(int(x).to_bytes(32, "little") for x in xs), dtype=np.uint64).reshape(-1, 4).copy()


def array_to_ints(a):
    import numpy as np
    b = np.ascontiguousarray(a, dtype=np.uint64).tobytes()
    return [int.from_bytes(b[i:i + 32], "little") for i in range(0, len(b), 32)]


def first_mismatch(got: list, want: list, a: list, b: list, what: str):
    """None if equal, else a message naming the first failing operand pair in hex"""
    if got == want:
        return None
    i = next(k for k in range(len(want)) if got[k] != want[k])
    bad = sum(1 for g, w in zip(got, want) if g != w)
    return "%s: %d of %d rows differ; first at row %d: a=%#066x b=%#066x got=%#066x want=%#066x" % (
        what, bad, len(want), i, a[i], b[i] if b is not None else 0, got[i], want[i])
