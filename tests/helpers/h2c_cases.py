"""Cases shared by tests/test_hash_to_curve_batch_cpu.py and tests/test_gpu_hash_to_curve.py: message and prefix lengths at the
BLAKE2b block boundaries of expand_message_xmd, operands for every select of the map, and what the oracle (oracle/pasta.py)
gives for them."""
import functools

import numpy as np

import pasta as O
import randutil

CURVES = {0: "vesta", 1: "pallas"}
SRS_PREFIX = "Halo2-Parameters"
# After the zero block the first hash takes len + 3 + len(dst_prime) bytes: len + 47 on Vesta and len + 48 on Pallas with the
# SRS prefix, so 81 (Vesta) and 80 (Pallas) fill the second block exactly and one byte more opens a third.
LENGTHS = (0, 1, 5, 79, 80, 81, 82, 128)
# 64 + 1 + len(dst_prime) is 128 for a 35-character prefix on Vesta (34 on Pallas) and 129 for one character more: the
# one-block and the two-block case of the second and third hash.
PREFIX_LENGTHS = (34, 35, 36)
R = 1 << 256


def base_p(cid):
    return O.CURVE_BY_ID[cid].base.p


def messages(length, n, seed=0):
    return [bytes((seed + 31 * i + 7 * j + (i * j) % 5) % 256 for j in range(length)) for i in range(n)]


def to_form(v, p, form):
    return v * R % p if form == 1 else v


def points_array(points, p, form):
    """[(x, y) | None] -> (n, 8) uint64 in `form`, zeros for None"""
    out = np.zeros((len(points), 8), dtype=np.uint64)
    for i, pt in enumerate(points):
        if pt is not None:
            for c in range(2):
                v = to_form(pt[c], p, form)
                out[i, 4 * c:4 * c + 4] = [(v >> (64 * j)) & 0xFFFFFFFFFFFFFFFF for j in range(4)]
    return out


def pairs_array(pairs, p, form):
    return points_array(pairs, p, form)


@functools.lru_cache(maxsize=None)
def hashed(cid, prefix, msg):
    return O.hash_to_curve(CURVES[cid], prefix, msg)


@functools.lru_cache(maxsize=None)
def map_cases(cid):
    """(pairs, wanted points with None for the identity, gx1-is-a-square flags of the random pairs' u0)"""
    p = base_p(cid)
    rnd = randutil.uniform_below(np.random.default_rng(0xC0FFEE + cid), 128, p)
    vals = [sum(int(rnd[i, j]) << (64 * j) for j in range(4)) for i in range(128)]
    random_pairs = [(vals[2 * i], vals[2 * i + 1]) for i in range(64)]
    pairs = [(0, 5), (5, 0), (0, 0),            # ta == 0
             (7, 7), (vals[0], vals[0]),          # doubling
             (9, p - 9), (vals[1], p - vals[1]),  # opposite points: the identity
             (1, p - 1),                          # ... and u = 1 with u = p - 1
             (1, 2), (p - 1, 2), (p - 1, p - 1)] + random_pairs
    iso, mp = O._ISO_CURVES[CURVES[cid]], O.iso_map(CURVES[cid])
    want = [O.iso_map_apply(iso.add(O.map_to_curve_simple_swu(a, iso), O.map_to_curve_simple_swu(b, iso)), mp, iso) for a, b in pairs]
    return pairs, want, [gx1_is_square(cid, a) for a, _ in random_pairs]


def gx1_is_square(cid, u):
    iso = O._ISO_CURVES[CURVES[cid]]
    F, p = iso.base, iso.base.p
    zu2 = O.SWU_Z * u * u % p
    ta = (zu2 * zu2 + zu2) % p
    x1 = iso.b * F.inv(O.SWU_Z * iso.a % p) % p if ta == 0 else (-iso.b) * F.inv(iso.a) % p * (1 + F.inv(ta)) % p
    return F.sqrt((x1 * x1 * x1 + iso.a * x1 + iso.b) % p) is not None
