"""TEST HELPER (plain Python + the C oracle, no GPU): the group FFT behind g_lagrange (csrc/params.hip: k_gfft_load, k_gfft_stage,
k_gfft_finish) on inputs whose discrete logarithms are known.  With g[i] = [a_i] G for one fixed G, output j of the inverse group
FFT is [b_j] G with b = intt(a) in the Vesta scalar field -- integer arithmetic -- and the a_i can be chosen so that a butterfly
adds a point to itself, to its negative or to the identity at a known stage.  `replay` mirrors the kernels' schedule on the
discrete logs and counts those meetings, so that a test can assert which branch of the group law an input reaches.

The row (0, 0) is the identity, a discrete log of 0."""
from __future__ import annotations

import functools
import random

import numpy as np

import coracle as C
import pasta as O

F = O.FP            # the Vesta scalar field
R = F.p
VESTA, FIELD_FP = 0, 0    # the C oracle's ids


@functools.lru_cache(maxsize=None)
def _generator_bytes() -> bytes:
    base = C.points_to_array([(O.Q - 1, 2)])      # Vesta's generator (-1, 2); G is a multiple of it with no special coordinate
    g = C.msm_naive(VESTA, C.ints_to_array([0x1f3a5c7e9b2d4f60718293a4b5c6d7e8f9]), base)
    assert O.VESTA.is_on_curve(C.array_to_point(g)) and C.array_to_point(g) is not None
    return g.tobytes()


def generator() -> np.ndarray:
    """the fixed point G, 8 canonical limbs"""
    return np.frombuffer(_generator_bytes(), dtype=np.uint64).copy()


def dlog_ifft(a, k: int) -> list:
    """b = intt(a): output j of the inverse group FFT of ([a_i] G) is [b_j] G"""
    n = 1 << k
    assert len(a) == n
    return C.array_to_ints(C.ntt(FIELD_FP, C.ints_to_array([x % R for x in a]), F.omega(k), inverse=True))


def expected_points(G: np.ndarray, b) -> np.ndarray:
    """([b_j] G) as an (n, 8) array of canonical limbs, (0, 0) where b_j == 0: one scalar multiplication of the C oracle per
    distinct b_j"""
    G = np.ascontiguousarray(G, dtype=np.uint64).reshape(1, 8)
    out = np.zeros((len(b), 8), dtype=np.uint64)
    seen = {}
    for j, s in enumerate(b):
        s %= R
        if s == 0:
            continue
        if s not in seen:
            seen[s] = C.msm_naive(VESTA, C.ints_to_array([s]), G)
        out[j] = seen[s]
    return out


def input_points(G: np.ndarray, a) -> np.ndarray:
    """([a_i] G) as an (n, 8) array, (0, 0) where a_i == 0"""
    return expected_points(G, a)


def _bitrev(i: int, k: int) -> int:
    return int(format(i, "0%db" % k)[::-1], 2) if k else 0


def replay(a, k: int):
    """What the kernels do, on discrete logs: the bit-reversed load, then the decimation-in-time stages m = 1, 2, ..., n / 2 with
    butterflies (i0, i0 + m), i0 = grp * 2m + j, twiddle omega^(-j * n / (2m)) applied to the upper operand only for j != 0, and
    s = a + t, d = a - t.  Returns (final, counters): final is the vector before k_gfft_finish scales it (n * dlog_ifft(a, k)),
    counters = {"stages": [one dict per stage], "zero_finals": rows k_gfft_finish sees as the identity}.  A stage's dict counts
    its butterflies, with t taken after the twiddle:
      eq            a == t != 0   -- s = a + t is a doubling, d = a + (-t) a cancellation
      eq_twiddled   ... of them with j != 0 (t came out of point_scalar_mul)
      neg           a == -t != 0  -- s is a cancellation, d a doubling
      neg_twiddled  ... of them with j != 0
      a_zero        a == 0 (t anything),   a_zero_only   a == 0 != t  (xyzz_add takes the other operand)
      t_zero        t == 0 (a anything),   t_zero_only   t == 0 != a  (xyzz_add returns at once)
      twiddle_on_zero   j != 0 and t == 0  (point_scalar_mul of the identity)"""
    n = 1 << k
    assert len(a) == n
    w_inv = F.inv(F.omega(k))
    work = [0] * n
    for i in range(n):
        work[_bitrev(i, k)] = a[i] % R
    stages = []
    m = 1
    while m < n:
        stride = n // (2 * m)
        c = dict(m=m, eq=0, eq_twiddled=0, neg=0, neg_twiddled=0, a_zero=0, a_zero_only=0, t_zero=0, t_zero_only=0, twiddle_on_zero=0)
        for idx in range(n // 2):
            grp, j = divmod(idx, m)
            i0 = grp * 2 * m + j
            i1 = i0 + m
            x, t = work[i0], work[i1]
            if j:
                c["twiddle_on_zero"] += t == 0
                t = t * pow(w_inv, j * stride, R) % R
            c["a_zero"] += x == 0
            c["t_zero"] += t == 0
            c["a_zero_only"] += x == 0 and t != 0
            c["t_zero_only"] += t == 0 and x != 0
            if x and x == t:
                c["eq"] += 1
                c["eq_twiddled"] += j != 0
            elif x and (x + t) % R == 0:
                c["neg"] += 1
                c["neg_twiddled"] += j != 0
            work[i0], work[i1] = (x + t) % R, (x - t) % R
        stages.append(c)
        m *= 2
    return work, {"stages": stages, "zero_finals": sum(1 for v in work if v == 0)}


def doublings(stage: dict) -> int:
    """butterflies of a stage in which xyzz_add_impl takes its doubling branch (in s or in d)"""
    return stage["eq"] + stage["neg"]


def cancellations(stage: dict) -> int:
    """butterflies of a stage in which xyzz_add_impl returns the identity (in d or in s): the same butterflies as `doublings`"""
    return stage["eq"] + stage["neg"]


IMPULSES = ("impulse_first", "impulse_second", "impulse_middle", "impulse_last")


def impulse_index(name: str, k: int) -> int:
    n = 1 << k
    return {"impulse_first": 0, "impulse_second": 1, "impulse_middle": n // 2, "impulse_last": n - 1}[name]


def case_names(k: int) -> tuple:
    """the cases that exist at size 2^k: the four impulse positions {0, 1, n/2, n-1} are two at k = 1; late_doubling needs a last
    stage with a j != 0 and quarter_zero a quarter of at least one row (k >= 2); at k = 0 there is no butterfly at all"""
    if k == 0:
        return ("uniform", "all_zero", "constant")
    names = ("uniform", "all_zero", "constant", "alternating", "impulse_first", "impulse_last", "equal_halves", "opposite_halves")
    if k >= 2:
        names += ("impulse_second", "impulse_middle", "late_doubling", "quarter_zero")
    return names


def _nonzero(rng) -> int:
    return rng.randrange(1, R)


def _late_doubling(k: int, rng) -> list:
    """a vector whose LAST stage meets a == t at one butterfly j != 0: choose the state X before that stage with
    X[j] = omega^-j X[j + n/2], everything else random, and undo the earlier stages -- they are two unnormalised inverse DFTs of
    size n/2 (root omega^2), of the even-indexed inputs into X[:n/2] and of the odd-indexed ones into X[n/2:]"""
    n, h = 1 << k, 1 << (k - 1)
    omega = F.omega(k)
    X = [_nonzero(rng) for _ in range(n)]
    j = rng.randrange(1, h)
    X[j] = X[j + h] * pow(F.inv(omega), j, R) % R
    h_inv = F.inv(h)
    w2 = omega * omega % R
    even = [v * h_inv % R for v in O.ntt(X[:h], w2, F)]
    odd = [v * h_inv % R for v in O.ntt(X[h:], w2, F)]
    a = [0] * n
    a[0::2], a[1::2] = even, odd
    return a


def cases(k: int, rng) -> dict:
    """name -> discrete-log vector of length 2^k, for the names of case_names(k); c is one random non-zero scalar"""
    n, h = 1 << k, (1 << k) // 2
    c = _nonzero(rng)
    out = {"uniform": [_nonzero(rng) for _ in range(n)], "all_zero": [0] * n, "constant": [c] * n}
    if k == 0:
        return out
    out["alternating"] = [c if i % 2 == 0 else R - c for i in range(n)]
    for name in IMPULSES:
        if name in case_names(k):
            v = [0] * n
            v[impulse_index(name, k)] = c
            out[name] = v
    half = [_nonzero(rng) for _ in range(h)]
    out["equal_halves"] = half + half
    half = [_nonzero(rng) for _ in range(h)]
    out["opposite_halves"] = half + [R - x for x in half]
    if k >= 2:
        out["late_doubling"] = _late_doubling(k, rng)
        v = [_nonzero(rng) for _ in range(n)]
        for i in rng.sample(range(n), n // 4):
            v[i] = 0
        out["quarter_zero"] = v
    assert tuple(sorted(out)) == tuple(sorted(case_names(k)))
    return out


GPU_KS_EVERY_OUTPUT = (0, 1, 2, 5, 6, 7, 10)     # tests/test_gpu_group_fft.py: the uniform case, all outputs compared
GPU_KS_CASES = (1, 2, 6, 7, 9)                   # ... every case of case_names(k)
GPU_K_WALK = 8                                   # ... the walked table g[i] = [i + 1] G


def gpu_case_params() -> list:
    """the (k, name) pairs the GPU test runs: what a size cannot have is left out here"""
    return [(k, name) for k in GPU_KS_CASES for name in case_names(k)]


@functools.lru_cache(maxsize=None)
def built(k: int) -> dict:
    """cases(k) on a seed fixed per k: every test that names (case, k) sees the same vector.  Not to be written to."""
    return cases(k, random.Random(0x6f7 + k))
