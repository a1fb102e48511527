"""TEST HELPER (pure Python + numpy): MSM inputs that sit on the corners of the signed-digit recoding (k_msm_digits) and of the
bucket accumulation -- scalars assembled window by window from the raw window values where the recoding changes behaviour, and
base sets made of few distinct points, so that additions into a bucket are doublings, cancellations or identities."""
from __future__ import annotations

import numpy as np

from helpers.field_edges import ints_to_array as _ints_to_array

WINDOW_VALUES = 6


def window_values(c: int) -> list:
    """the raw window values where the signed-digit recoding changes behaviour: 0 (the digit a borrow turns into -2^(c-1)), 1,
    the largest positive digit 2^(c-1) - 1, the first values that borrow 2^(c-1) and 2^(c-1) + 1, and the all-ones window that
    a carry turns into 0"""
    half = 1 << (c - 1)
    return sorted({0, 1, half - 1, half, half + 1, (1 << c) - 1})


def boundary_scalars(c: int, r: int, rng, count: int) -> list:
    """`count` scalars below r for window width c.  The first half (rounded up) is assembled window by window: at every window
    position the values of `window_values(c)` in turn, in an order shuffled per position, so that each of them occurs at
    every position at least floor(count / 2 / 6) times (the top window takes those that keep the scalar below r).  The rest
    is fixed: r - 1, r - 2, (r - 1) / 2, then the single-bit scalars 2^j -- every j < bits(r) if they fit, otherwise evenly
    spaced ones with the top bit among them; what is left over is filled with more assembled scalars."""
    bits = r.bit_length()
    nwin = (bits + c - 1) // c
    choices = window_values(c)
    top_shift = (nwin - 1) * c
    top_choices = [v for v in choices if v < (r >> top_shift)]      # strictly below r's own top window: any low part fits
    assert top_choices
    n_asm = (count + 1) // 2
    n_fixed = count - n_asm
    fixed = [r - 1, r - 2, (r - 1) // 2][:n_fixed]
    room = n_fixed - len(fixed)
    if room >= bits:
        fixed += [1 << j for j in range(bits)]
    elif room == 1:
        fixed.append(1 << (bits - 1))
    elif room > 1:
        fixed += [1 << ((bits - 1) * i // (room - 1)) for i in range(room)]
    n_asm = count - len(fixed)

    def column(values):
        col = (values * (n_asm // len(values) + 1))[:n_asm]
        rng.shuffle(col)
        return col

    cols = [column(choices) for _ in range(nwin - 1)] + [column(top_choices)]
    out = []
    for i in range(n_asm):
        s = 0
        for w in range(nwin):
            s |= cols[w][i] << (w * c)
        assert s < r
        out.append(s)
    return out + fixed


def colliding_bases(curve, n: int, rng, distinct: int = 64) -> list:
    """n affine points (None = identity): `distinct` random points repeated in order, every third repeat negated, and the
    identity at a few places"""
    pts = [curve.random_point(rng) for _ in range(distinct)]
    out = []
    for i in range(n):
        rep, k = divmod(i, distinct)
        out.append(curve.neg(pts[k]) if rep % 3 == 2 else pts[k])
    for i in (5, distinct + 5, n // 2, n - 1):
        if i < n:
            out[i] = None
    return out


def colliding_scalar_vectors(r: int, n: int, c: int, nvec: int, rng, np_rng, uniform_below) -> np.ndarray:
    """(nvec, n, 4): all-equal vectors (every addition into a bucket after the first is a doubling or a cancellation), i mod 2,
    boundary scalars of width c, uniform -- the four kinds in turn"""
    equal_values = [r - 1, 1, (1 << (c - 1)) + (1 << (2 * c - 1)), rng.randrange(r), (r - 1) // 2, 1 << (c - 1), 2]
    vecs = []
    for v in range(nvec):
        kind = v % 4
        if kind == 0:
            vecs.append(_ints_to_array([equal_values[(v // 4) % len(equal_values)]] * n))
        elif kind == 1:
            vecs.append(_ints_to_array([(i + v // 4) % 2 for i in range(n)]))
        elif kind == 2:
            vecs.append(_ints_to_array(boundary_scalars(c, r, rng, n)))
        else:
            vecs.append(uniform_below(np_rng, n, r))
    return np.stack(vecs)
