"""The adversarial operand set of tests/helpers/field_edges.py has the properties the GPU tests rely on (pure Python: no GPU, no
library).  The floors below are the counts the generator produces, counted here; a change to the generator that loses corner
pairs fails this test instead of silently thinning the GPU coverage."""
import random

import pytest

from helpers import field_edges as E

# ordered pairs (a, b) of the 256 x 256 table, per field id.  BN254: 2p < 2^255, so no sum reaches 2^255 there.
FLOORS = {
    0: {"sum_is_p": 104, "sum_is_p_minus_1": 101, "sum_is_p_plus_1": 101, "equal": 256, "sum_ge_2_255": 1715, "borrow_low4_equal": 308},
    1: {"sum_is_p": 104, "sum_is_p_minus_1": 101, "sum_is_p_plus_1": 101, "equal": 256, "sum_ge_2_255": 1715, "borrow_low4_equal": 308},
    2: {"sum_is_p": 128, "sum_is_p_minus_1": 127, "sum_is_p_plus_1": 125, "equal": 256, "sum_ge_2_255": 0, "borrow_low4_equal": 556},
    3: {"sum_is_p": 128, "sum_is_p_minus_1": 127, "sum_is_p_plus_1": 125, "equal": 256, "sum_ge_2_255": 0, "borrow_low4_equal": 556},
}


def test_moduli_are_the_oracles():
    import pasta as O
    assert {f: O.FIELD_BY_ID[f].p for f in range(4)} == E.MODULI


@pytest.mark.parametrize("fid", [0, 1, 2, 3])
def test_edge_set_is_256_distinct_reduced_values_and_deterministic(fid):
    p = E.MODULI[fid]
    v = E.edge_values(p)
    assert len(v) == 256 and len(set(v)) == 256 and all(0 <= x < p for x in v)
    assert v == E.edge_values(p)


@pytest.mark.parametrize("fid", [0, 1, 2, 3])
def test_edge_set_contains_the_listed_values(fid):
    p = E.MODULI[fid]
    s = set(E.edge_values(p))
    must = [0, 1, 2, p - 1, p - 2, (p - 1) // 2, (p + 1) // 2, E.R % p, E.R * E.R % p, (1 << (p.bit_length() - 1)) - 1]
    for i in range(1, 8):
        must += [(1 << (32 * i)) - 1, 1 << (32 * i), (1 << (32 * i)) + 1]
        low = p % (1 << (32 * i))
        must += [low, low - 1, low + 1, p - (1 << (32 * i))]
    for x in must:
        assert 0 <= x < p and x in s, hex(x)
    top = (1 << (p.bit_length() - 1 - 224)) - 1
    for i in range(8):
        only = [0] * 8
        only[i] = E.M32 if i < 7 else top
        must.append(sum(l << (32 * k) for k, l in enumerate(only)))
        allbut = [E.M32] * 7 + [top]
        allbut[i] = 0
        must.append(sum(l << (32 * k) for k, l in enumerate(allbut)))
    for x in must:                                           # the values themselves, and the closure x -> p - x, p - x +- 1
        assert x in s, hex(x)
        for w in (p - x, p - x - 1, p - x + 1):
            assert not (0 <= w < p) or w in s, (hex(x), hex(w))


@pytest.mark.parametrize("fid", [0, 1, 2, 3])
def test_pair_table_reaches_the_carry_chain_corners(fid):
    p = E.MODULI[fid]
    st = E.pair_statistics(E.edge_values(p), p)
    for key, floor in FLOORS[fid].items():
        assert st[key] >= floor, (key, st[key], floor)
    a, b = E.all_pairs(E.edge_values(p))
    assert len(a) == len(b) == 65536 and len(set(zip(a, b))) == 65536


@pytest.mark.parametrize("fid", [0, 1, 2, 3])
def test_targeted_pairs_multiply_to_their_targets(fid):
    p = E.MODULI[fid]
    trip = E.targeted_products(p, random.Random(5 + fid))
    targets = E.product_targets(p)
    assert len(trip) == 64 * len(targets) and len(targets) == (15 if fid < 2 else 19)   # the Pasta low parts coincide
    assert {1, 2, (1 << 32) - 1, 1 << 32, 1 << 224, p - 1, p - 2, p % (1 << 32), p % (1 << 224)} <= set(targets)
    for x, y, t in trip:
        assert 0 < x < p and 0 <= y < p and E.reference("mul", x, y, p) == t


def test_reference_is_montgomery_arithmetic_on_raw_bits():
    for p in E.MODULI.values():
        rng = random.Random(p % 1000)
        for _ in range(50):
            x, y = rng.randrange(p), rng.randrange(p)
            xm, ym = x * E.R % p, y * E.R % p
            assert E.reference("mul", xm, ym, p) == x * y * E.R % p
            assert E.reference("add", xm, ym, p) == (x + y) * E.R % p
            assert E.reference("sub", xm, ym, p) == (x - y) * E.R % p
            assert E.reference("neg", xm, 0, p) == (-x) * E.R % p


@pytest.mark.parametrize("cid", [0, 1])
def test_c_oracle_msm_handles_colliding_bases(oracle_c, cid):
    """the GPU tests compare MSMs over repeated, negated and identity bases with the C oracle: the C oracle itself against the
    affine big-int definition on a 256-point case of the same construction"""
    import numpy as np
    import pasta as O
    from randutil import SCALAR_MODULUS, uniform_below
    from helpers.msm_edges import colliding_bases, colliding_scalar_vectors
    cv = O.CURVE_BY_ID[cid]
    rng = random.Random(9 + cid)
    pts = colliding_bases(cv, 256, rng, distinct=16)
    assert pts.count(None) == 4 and len({p for p in pts if p}) == 32
    batch = colliding_scalar_vectors(SCALAR_MODULUS[cid], 256, 11, 4, rng, np.random.default_rng(cid), uniform_below)
    arr = oracle_c.points_to_array(pts)
    for k, v in enumerate(batch):
        got = oracle_c.array_to_point(oracle_c.msm(cid, np.ascontiguousarray(v), arr, 4))
        assert got == oracle_c.array_to_point(oracle_c.msm_naive(cid, np.ascontiguousarray(v), arr)), k
        if k in ((0, 2) if cid == 0 else (0,)):          # the big-int definition is slow: the all-equal and the boundary vector
            assert got == cv.msm_naive(oracle_c.array_to_ints(v), pts), k


@pytest.mark.parametrize("count", [64, 640, 2048])
@pytest.mark.parametrize("c", range(3, 16))
def test_boundary_scalars_cover_every_window_value(c, count):
    """every window position of a vector, short ones included, sees each of the six raw values (the top window those that keep
    the scalar below r) at least floor(assembled / 6) times; the fixed scalars are there as far as they fit"""
    from helpers.msm_edges import boundary_scalars, window_values
    r = E.MODULI[0]
    sc = boundary_scalars(c, r, random.Random(c), count)
    assert len(sc) == count and all(0 <= s < r for s in sc)
    assert {r - 1, r - 2, (r - 1) // 2, 1, 1 << 254} <= set(sc)
    if count >= 2 * 258:
        assert {1 << j for j in range(255)} <= set(sc)
    n_asm = count - min(count // 2, 258)
    assert n_asm >= count // 2 >= 32
    asm = sc[:n_asm]
    nwin = (255 + c - 1) // c
    want = window_values(c)
    assert len(want) == 6
    floor = n_asm // len(want)
    assert floor >= 5
    for w in range(nwin):
        seen = [(s >> (w * c)) & ((1 << c) - 1) for s in asm]
        for v in (want if w < nwin - 1 else [v for v in want if v < (r >> (w * c))]):
            assert seen.count(v) >= floor, (c, w, v)
    assert sc == boundary_scalars(c, r, random.Random(c), count)


def test_boundary_scalar_vectors_differ_per_width():
    from helpers.msm_edges import boundary_scalars
    r = E.MODULI[0]
    vecs = [tuple(boundary_scalars(c, r, random.Random(1), 64)[:32]) for c in range(3, 16)]
    assert len(set(vecs)) == 13
