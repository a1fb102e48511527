"""TEST HELPER (pure Python + numpy, no GPU, no library): inputs and expected outputs for the vector primitives of
csrc/polyops.hip at launch shapes a single small proof never produces -- capped batch-inversion launches, hundreds of scanned
vectors, every (threads, L, S) regime of kate_division, batched inner products, folds and evaluations.

Every builder returns numpy uint64 arrays (4 little-endian limbs per element), inputs and expected outputs alike, so that a
test compares a million elements with one array comparison.  The big cases are assembled from a small number of distinct
vectors whose expected outputs come from the big-int definitions of oracle/pasta.py; only those few vectors ever exist as
Python integers.  Neighbouring vectors of a batch are always different ones, so a result stitched from the wrong vector, span
or chain cannot agree with the expectation by accident."""
from __future__ import annotations

import functools
import random

import numpy as np

import pasta as O
from helpers import field_edges as E

R = 1 << 256
TABLE = 4099                      # prime: the tiling never lines up with a power-of-two launch shape
FIRST_ZERO = 400                  # table position of the first planted zero: it and its two companions miss the 256 edge values
N_SCAN, N_KATE = 11, 7            # distinct vectors behind scan_case / kate_case
N_VEC, N_PT = 7, 11               # distinct vectors and points behind the inner-product / fold / evaluation builders

ints_to_array, array_to_ints = E.ints_to_array, E.array_to_ints


def field_of(p: int) -> O.FieldSpec:
    return next(f for f in O.FIELD_BY_ID.values() if f.p == p)


def uniform(rng: random.Random, n: int, p: int) -> list:
    return [rng.randrange(p) for _ in range(n)]


def first_difference(got: np.ndarray, want: np.ndarray):
    """None if the two element arrays agree bit for bit, else (index of the first differing element, how many differ)"""
    g, w = np.ascontiguousarray(got, dtype=np.uint64).reshape(-1, 4), np.ascontiguousarray(want, dtype=np.uint64).reshape(-1, 4)
    assert g.shape == w.shape, (g.shape, w.shape)
    bad = np.flatnonzero((g != w).any(axis=1))
    return None if bad.size == 0 else (int(bad[0]), int(bad.size))


def hex_of(a: np.ndarray, i: int) -> str:
    return "%#066x" % E.array_to_ints(np.ascontiguousarray(a, dtype=np.uint64).reshape(-1, 4)[i:i + 1])[0]


# ---- batch inversion ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def inverse_table(p: int):
    """(values, inverses): the 256 edge values of helpers/field_edges.py, then seeded uniform values, TABLE in all; the inverse
    of zero is zero (ff::BatchInvert)"""
    vals = list(E.edge_values(p))
    rng = random.Random(0x7ab1e ^ (p & 0xFFFFFFFF))
    vals += uniform(rng, TABLE - len(vals), p)
    assert len(vals) == TABLE
    return vals, [pow(x, -1, p) if x else 0 for x in vals]


def tiled_inverse_case(p: int, count: int, nthreads: int, montgomery: bool = False):
    """(input, expected, info) for a batch inversion of `count` elements run by `nthreads` threads, thread t owning the chain
    t, t + nthreads, ...  Inversion is element-wise, so the input is the table of `inverse_table` repeated to `count` and the
    expectation its inverses repeated the same way.  Zeros: three table positions nthreads apart (mod TABLE), so that some
    chain meets three zeros in a row wherever the tiling puts them; elements 0 and count - 1; and the whole chain of thread
    info["zero_chain"].  montgomery: the input bits stand for x R^-1, so the expected bits are x^-1 R^2."""
    vals, invs = inverse_table(p)
    vals, invs = list(vals), list(invs)
    d = nthreads % TABLE
    planted = sorted({(FIRST_ZERO + k * d) % TABLE for k in range(3)})
    for pos in planted:
        vals[pos] = invs[pos] = 0
    if montgomery:
        invs = [y * R * R % p for y in invs]
    idx = np.arange(count) % TABLE
    v, want = ints_to_array(vals)[idx], ints_to_array(invs)[idx]
    t0 = nthreads // 3
    for a in (v, want):
        a[0] = 0
        a[count - 1] = 0
        a[t0::nthreads] = 0
    return v, want, {"planted": planted, "zero_chain": t0, "table": (vals, invs)}


# ---- grand-product scan ---------------------------------------------------------------------------------------------------
def scan_zero_positions(n: int):
    """where the two zero-carrying vectors have their zero: the last element of the first 2048-element tile and the first of
    the second one, or, in a vector too short for that, its middle and its last element"""
    return (2047 if n > 2047 else n // 2), (2048 if n > 2048 else n - 1)


@functools.lru_cache(maxsize=None)
def scan_vectors(p: int, n: int):
    """the N_SCAN distinct vectors and their exclusive running products (O.prefix_product): 7 uniform ones, all ones, all
    p - 1 (the product alternates 1, p - 1), and two uniform ones with a single zero (everything after it is zero)"""
    F = field_of(p)
    rng = random.Random(0x5ca9 + 31 * n + (p & 0xFFFF))
    vecs = [uniform(rng, n, p) for _ in range(7)] + [[1] * n, [p - 1] * n]
    for z in scan_zero_positions(n):
        v = [rng.randrange(1, p) for _ in range(n)]
        v[z] = 0
        vecs.append(v)
    assert len(vecs) == N_SCAN
    want = [O.prefix_product(v, F) for v in vecs]
    return np.stack([ints_to_array(v) for v in vecs]), np.stack([ints_to_array(w) for w in want])


def scan_pick(batch: int) -> np.ndarray:
    """which distinct vector sits at each place of the batch: in rotation, except that the zero-carrying vectors take places
    63, 64 and 65 -- the last thread of the first 64-thread block of the totals scan and the first two of the second"""
    pick = np.arange(batch) % N_SCAN
    for place, which in ((63, 9), (64, 10), (65, 9)):
        if place < batch:
            pick[place] = which
    return pick


def scan_case(p: int, n: int, batch: int):
    """(input, expected, pick), input and expected of shape (batch, n, 4)"""
    vecs, want = scan_vectors(p, n)
    pick = scan_pick(batch)
    return vecs[pick], want[pick], pick


# ---- kate_division --------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def kate_pairs(p: int, n: int):
    """[(coefficients, x, quotient)] as integers, N_KATE pairs; the quotient is O.kate_division, exact.
    Polynomials: uniform (three of them), the top third of the coefficients zero, all zero, all p - 1, only the constant term
    non-zero.  Points: 0, 1, p - 1, 2 and three uniform values.  The pairing puts a point whose powers are all different next
    to a polynomial with a non-trivial quotient in the first three pairs, which are all that a batch of one to three sees: at
    x = 0 the recurrence r <- r x + c forgets every carried value, and at x = 1 or p - 1 every power of x is 1 or p - 1."""
    F = field_of(p)
    rng = random.Random(0x4a7e + 17 * n + (p & 0xFFFF))
    uni = [uniform(rng, n, p) for _ in range(3)]
    top_zero = uniform(rng, n, p)
    for i in range(n - n // 3, n):
        top_zero[i] = 0
    const_only = [rng.randrange(1, p)] + [0] * (n - 1)
    u = [rng.randrange(3, p - 1) for _ in range(3)]
    pairs = [(uni[0], u[0]), (top_zero, 2), ([p - 1] * n, u[1]), (uni[1], p - 1), (uni[2], 1), ([0] * n, u[2]), (const_only, 0)]
    assert len(pairs) == N_KATE
    return [(c, x, O.kate_division(c, x, F)) for c, x in pairs]


def kate_case(p: int, n: int, batch: int):
    """(coefficients (batch, n, 4), the batch's points as integers, expected quotients (batch, n - 1, 4)): the pairs of
    `kate_pairs` in rotation over the batch"""
    pairs = kate_pairs(p, n)
    pick = np.arange(batch) % N_KATE
    coeffs = np.stack([ints_to_array(c) for c, _, _ in pairs])
    quot = np.stack([ints_to_array(q).reshape(n - 1, 4) for _, _, q in pairs])
    return coeffs[pick], [pairs[k][1] for k in pick], quot[pick]


def kate_multiplied_back(c, x: int, q, p: int) -> bool:
    """q(X) (X - x) + p(x) == p(X), coefficient by coefficient with integers"""
    n = len(c)
    rem = O.eval_polynomial(c, x, field_of(p))
    back = [0] * n
    for i, qi in enumerate(q):
        back[i + 1] = (back[i + 1] + qi) % p
        back[i] = (back[i] - qi * x) % p
    back[0] = (back[0] + rem) % p
    return back == [ci % p for ci in c]


# ---- inner product, fold, evaluation ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _vectors(p: int, n: int, how_many: int, seed: int):
    rng = random.Random(seed + 131 * n + (p & 0xFFFF))
    return [uniform(rng, n, p) for _ in range(how_many)]


def inner_product_case(p: int, n: int, batch: int):
    """(a, b, expected): a, b of shape (batch, n, 4), expected (batch, 4).  Vector v of a is one of N_VEC uniform vectors, of b
    one of N_PT others, in rotation: N_VEC * N_PT different pairs, each summed once with integers (O.inner_product)"""
    F = field_of(p)
    av, bv = _vectors(p, n, N_VEC, 0x1a), _vectors(p, n, N_PT, 0x1b)
    ia, ib = np.arange(batch) % N_VEC, np.arange(batch) % N_PT
    memo = {}
    want = [memo.setdefault((i, j), O.inner_product(av[i], bv[j], F)) for i, j in zip(ia.tolist(), ib.tolist())]
    return np.stack([ints_to_array(v) for v in av])[ia], np.stack([ints_to_array(v) for v in bv])[ib], ints_to_array(want)


def fold_case(p: int, half: int, batch: int, nu: int):
    """(v, u, expected): v of shape (batch, 2 * half, 4) laid out [lo | hi], u (nu, 4) with nu = 1 or batch, expected
    (batch, half, 4) = lo + u_b hi (O.fold_scalars); every vector and every u uniform and different"""
    assert nu in (1, batch)
    F = field_of(p)
    rng = random.Random(0xf01d + 131 * half + 7 * batch + nu + (p & 0xFFFF))
    vs = [uniform(rng, 2 * half, p) for _ in range(batch)]
    us = uniform(rng, nu, p)
    want = [O.fold_scalars(v, us[b if nu > 1 else 0], F) for b, v in enumerate(vs)]
    return (np.stack([ints_to_array(v) for v in vs]), ints_to_array(us),
            np.stack([ints_to_array(w).reshape(half, 4) for w in want]))


def eval_case(p: int, n: int, batch: int, nx: int):
    """(coefficients (batch, n, 4), points (nx, 4), expected (batch, 4)), nx = 1 or batch: N_VEC uniform polynomials and, for
    nx = batch, N_PT uniform points in rotation; each different (polynomial, point) pair evaluated once (O.eval_polynomial)"""
    assert nx in (1, batch)
    F = field_of(p)
    polys = _vectors(p, n, N_VEC, 0xe7a1)
    pts = uniform(random.Random(0xe7a2 + n + (p & 0xFFFF)), N_PT, p)
    ip = np.arange(batch) % N_VEC
    ix = np.arange(nx) % N_PT
    memo = {}
    want = [memo.setdefault((i, j), O.eval_polynomial(polys[i], pts[j], F))
            for i, j in zip(ip.tolist(), (ix if nx > 1 else np.zeros(batch, dtype=np.int64)).tolist())]
    return np.stack([ints_to_array(c) for c in polys])[ip], ints_to_array([pts[j] for j in ix.tolist()]), ints_to_array(want)
