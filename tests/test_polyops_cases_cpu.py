"""No device needed: the launch plans of bzh_batch_invert and bzh_kate_division (bzh_batch_invert_plan, bzh_kate_division_plan,
the functions the drivers in csrc/polyops.hip call) pinned to their values; a guard that the case table of
tests/test_gpu_polyops_geometry.py reaches every regime of those plans it claims to; and the case builders of
tests/helpers/polyops_cases.py checked against definitions other than the ones they were built from."""
import ctypes

import numpy as np
import pytest

import pasta as O
import test_gpu_polyops_geometry as G
from helpers import field_edges as E
from helpers import polyops_cases as K

KATE_PLANS = {
    (2, 1): (64, 4, 1), (258, 3): (128, 4, 1), (514, 3): (256, 4, 1), (1025, 1): (256, 4, 1), (1026, 1): (256, 4, 2),
    (2050, 256): (256, 9, 1), (4097, 64): (256, 4, 4), (4098, 64): (256, 5, 4), (8193, 40): (256, 5, 7), (32769, 2): (256, 4, 32),
    (32770, 2): (256, 5, 26),
}
INVERT_PLANS = {63: 63, 64: 64, 1024: 64, 1025: 65, 1 << 20: 65536, (1 << 20) + 1: 65536, 1245201: 65536}


@pytest.fixture(scope="module")
def bzh2_lib():
    import bzh2
    bzh2.load()
    return bzh2


def test_kate_division_plan_values(bzh2_lib):
    for (n, batch), want in KATE_PLANS.items():
        assert bzh2_lib.kate_division_plan(n, batch) == want, (n, batch)


def test_batch_invert_plan_values(bzh2_lib):
    for count, want in INVERT_PLANS.items():
        assert bzh2_lib.batch_invert_plan(count) == want, count
    assert G.CAPPED_COUNT == 1245201
    assert bzh2_lib.batch_invert_plan(0) == 0                                 # nothing is launched


def test_plans_cover_their_input_and_refuse_what_the_drivers_refuse(bzh2_lib):
    for n in list(range(2, 40)) + [255, 256, 257, 258, 1024, 1025, 1026, 4097, 32769, 32770, 131072, (1 << 20) + 5]:
        for batch in (1, 2, 3, 7, 8, 9, 40, 64, 255, 256, 257, 65535):
            threads, L, S = bzh2_lib.kate_division_plan(n, batch)
            m = n - 1
            assert threads in (64, 128, 256) and L >= 4 and 1 <= S <= 32, (n, batch)
            assert (S - 1) * threads * L < m <= S * threads * L, (n, batch)    # every span but the last is full, the last not empty
    for count in list(range(1, 200)) + [1023, 1024, 1025, 1 << 20, (1 << 20) + 1, 1 << 24]:
        t = bzh2_lib.batch_invert_plan(count)
        assert 1 <= t <= min(count, 65536), count                              # no thread without an element
    L = bzh2_lib.load()
    szp = ctypes.POINTER(ctypes.c_size_t)
    L.bzh_batch_invert_plan.argtypes = [ctypes.c_size_t, szp]
    L.bzh_kate_division_plan.argtypes = [ctypes.c_size_t, ctypes.c_size_t, ctypes.POINTER(ctypes.c_uint), szp, szp]
    assert L.bzh_batch_invert_plan(5, None) == bzh2_lib.E_ARG
    th, seg, sp = ctypes.c_uint(), ctypes.c_size_t(), ctypes.c_size_t()
    ok = (ctypes.byref(th), ctypes.byref(seg), ctypes.byref(sp))
    assert L.bzh_kate_division_plan(100, 1, *ok) == bzh2_lib.OK
    for k in range(3):
        args = list(ok)
        args[k] = None
        assert L.bzh_kate_division_plan(100, 1, *args) == bzh2_lib.E_ARG
    for n, batch in ((0, 1), (1, 1), (100, 0), (100, 65536)):
        assert L.bzh_kate_division_plan(n, batch, *ok) == bzh2_lib.E_ARG, (n, batch)
    with pytest.raises(bzh2_lib.BzhError):
        bzh2_lib.kate_division_plan(100, 65536)


def test_gpu_case_table_reaches_every_regime(bzh2_lib):
    """tests/test_gpu_polyops_geometry.py's own tables against the library's plans"""
    assert set(G.KATE_CASES_OTHER_FIELDS) <= set(G.KATE_CASES)
    plans = {(n, b): bzh2_lib.kate_division_plan(n, b) for n, b in G.KATE_CASES}
    for key, want in KATE_PLANS.items():
        assert key in plans and plans[key] == want
    some = lambda pred: [k for k, (t, L, S) in plans.items() if pred(k[0] - 1, t, L, S)]
    assert some(lambda m, t, L, S: S == 1 and L > 4)
    assert some(lambda m, t, L, S: 1 < S < 32 and L > 4)
    assert some(lambda m, t, L, S: S == 32)
    assert some(lambda m, t, L, S: S > 1 and m == S * t * L)                   # an exact fit: every span full
    assert some(lambda m, t, L, S: S > 1 and m - (S - 1) * t * L == 1)         # a last span of one coefficient
    assert some(lambda m, t, L, S: m <= (t - 1) * L + (S - 1) * t * L)         # threads with an empty segment (k0 == m)
    for threads in (64, 128, 256):
        assert some(lambda m, t, L, S: t == threads), threads
    sub = [plans[k] for k in G.KATE_CASES_OTHER_FIELDS]                        # the other fields: both regimes with L > 4
    assert any(S == 1 and L > 4 for _, L, S in sub) and any(S > 1 and L > 4 for _, L, S in sub)
    counts = [G.CAPPED_COUNT] + G.STEP_COUNTS + G.ALL_ZERO_COUNTS
    threads = {c: bzh2_lib.batch_invert_plan(c) for c in counts}
    assert threads[G.CAPPED_COUNT] == 65536 and G.CAPPED_COUNT > 16 * 65536
    lens = {len(range(t, G.CAPPED_COUNT, 65536)) for t in (0, 16, 17, 65535)}
    assert lens == {19, 20}
    assert {threads[c] for c in G.STEP_COUNTS} >= {64, 65, 65536}
    assert threads[1 << 20] * 16 == 1 << 20 and threads[(1 << 20) + 1] * 16 < (1 << 20) + 1   # the last uncapped count, the first capped one
    # scan: more than one 64-thread block of k_scan_totals with more than one tile; more than one 65 535-vector chunk
    assert all(n > 2048 and batch > 64 for n, batch in G.SCAN_CASES) and any(batch > 128 for _, batch in G.SCAN_CASES)
    assert G.SCAN_SECOND_CHUNK[1] > 65535 + 1


@pytest.mark.parametrize("fid", [0, 1, 2])
def test_tiled_inverse_against_the_oracle(fid):
    F = O.FIELD_BY_ID[fid]
    p = F.p
    count, nthreads = G.CAPPED_COUNT, 65536
    v, want, info = K.tiled_inverse_case(p, count, nthreads)
    assert v.shape == want.shape == (count, 4)
    planted, t0 = info["planted"], info["zero_chain"]
    assert len(planted) == 3
    # a 10 000-element slice with the planted zeros (the table is shorter than that), the edge values and the zeroed chain in it
    lo = K.TABLE - 100
    sl = slice(lo, lo + 10000)
    assert all(any((i % K.TABLE) == z for i in range(lo, lo + 10000)) for z in planted)
    ints = E.array_to_ints(v[sl])
    assert E.array_to_ints(want[sl]) == O.batch_invert(ints, F)
    assert ints.count(0) >= 2 * 3 + 2
    # three zeros in a row in one chain: the elements i, i + nthreads, i + 2 nthreads for the first i on the first planted position
    i0 = next(i for i in range(count) if i % K.TABLE == K.FIRST_ZERO)
    assert i0 + 2 * nthreads < count and not v[[i0, i0 + nthreads, i0 + 2 * nthreads]].any()
    assert v[i0 + 3 * nthreads].any()
    # the ends and one whole chain
    assert not v[0].any() and not v[count - 1].any() and not v[t0::nthreads].any() and not want[t0::nthreads].any()
    # zeros in, zeros out, and nothing else is zero
    assert ((v == 0).all(axis=1) == (want == 0).all(axis=1)).all()
    # Montgomery form: x stands for x R^-1, the result for x^-1 R^2
    vm, wm, _ = K.tiled_inverse_case(p, 5000, 65, montgomery=True)
    rinv = pow(E.R, -1, p)
    canon = [x * rinv % p for x in E.array_to_ints(vm)]
    assert E.array_to_ints(wm) == [y * E.R % p for y in O.batch_invert(canon, F)]
    # the small counts keep their planted zeros inside the input
    for cnt, nt in ((1024, 64), (1025, 65), (1040, 65)):
        vs, _, inf = K.tiled_inverse_case(p, cnt, nt)
        assert all(z < cnt for z in inf["planted"]) and not vs[inf["planted"]].any()
        assert inf["planted"][1] - inf["planted"][0] == nt


@pytest.mark.parametrize("fid", [0, 1, 2])
def test_kate_pairs_multiply_back(fid):
    p = O.FIELD_BY_ID[fid].p
    for n in sorted({n for n, _ in G.KATE_CASES if n <= 514}):
        pairs = K.kate_pairs(p, n)
        assert len(pairs) == K.N_KATE and len({x for _, x, _ in pairs}) == K.N_KATE
        assert {0, 1, 2, p - 1} <= {x for _, x, _ in pairs}
        for c, x, q in pairs:
            assert len(q) == n - 1 and K.kate_multiplied_back(c, x, q, p), (n, x)
        # a batch of one to three meets only points whose powers differ and quotients that are not trivial
        for c, x, q in pairs[:3]:
            assert x not in (0, 1, p - 1) and any(q)
    coeffs, xs, want = K.kate_case(p, 258, 10)
    assert coeffs.shape == (10, 258, 4) and want.shape == (10, 257, 4) and len(xs) == 10
    assert xs[7] == xs[0] and (coeffs[7] == coeffs[0]).all() and (coeffs[1] != coeffs[0]).any()
    assert E.array_to_ints(want[8]) == O.kate_division(E.array_to_ints(coeffs[8]), xs[8], O.FIELD_BY_ID[fid])


def test_scan_case_layout():
    F = O.FP
    p = F.p
    v, want, pick = K.scan_case(p, 2049, 130)
    assert v.shape == want.shape == (130, 2049, 4)
    assert set(pick.tolist()) == set(range(K.N_SCAN)) and (pick[1:] != pick[:-1]).all()      # neighbours always differ
    assert list(pick[63:66]) == [9, 10, 9]
    assert not v[63][2047].any() and v[63][2046].any() and not v[64][2048].any() and v[64][2047].any()
    assert want[63][2047].any() and not want[63][2048].any()                                  # zero from the element after the zero on
    assert want[64][2048].any()                                                               # a zero in the last element changes no output
    for b in (0, 7, 8, 63, 64, 129):
        assert E.array_to_ints(want[b]) == O.prefix_product(E.array_to_ints(v[b]), F)
    ones, minus = E.array_to_ints(want[7]), E.array_to_ints(want[8])
    assert set(ones) == {1} and minus[:4] == [1, p - 1, 1, p - 1]
    short, swant, spick = K.scan_case(p, 3, 70000)
    assert short.shape == (70000, 3, 4) and (spick[1:] != spick[:-1]).all()
    for b in (65534, 65535, 65536, 69999):
        assert E.array_to_ints(swant[b]) == O.prefix_product(E.array_to_ints(short[b]), F)
    assert len({short[b].tobytes() for b in (65534, 65535, 65536)}) == 3


def test_inner_product_fold_eval_builders():
    F = O.BN_FR
    p = F.p
    a, b, want = K.inner_product_case(p, 257, 300)
    assert a.shape == b.shape == (300, 257, 4) and want.shape == (300, 4)
    for k in (0, 1, 76, 77, 299):
        assert E.array_to_ints(want[k:k + 1]) == [O.inner_product(E.array_to_ints(a[k]), E.array_to_ints(b[k]), F)]
    assert len({want[k].tobytes() for k in range(77)}) == 77
    for nu in (1, 37):
        v, u, want = K.fold_case(p, 255, 37, nu)
        assert v.shape == (37, 510, 4) and u.shape == (nu, 4) and want.shape == (37, 255, 4)
        us = E.array_to_ints(u)
        for k in (0, 1, 36):
            assert E.array_to_ints(want[k]) == O.fold_scalars(E.array_to_ints(v[k]), us[k if nu > 1 else 0], F)
    for nx in (1, 300):
        c, x, want = K.eval_case(p, 513, 300, nx)
        assert c.shape == (300, 513, 4) and x.shape == (nx, 4) and want.shape == (300, 4)
        xs = E.array_to_ints(x)
        for k in (0, 1, 150, 299):
            assert E.array_to_ints(want[k:k + 1]) == [O.eval_polynomial(E.array_to_ints(c[k]), xs[k if nx > 1 else 0], F)]


def test_first_difference_names_the_first_element():
    a = np.arange(40, dtype=np.uint64).reshape(10, 4)
    b = a.copy()
    assert K.first_difference(a, b) is None
    b[6, 3] += 1
    b[8, 0] += 1
    assert K.first_difference(a, b) == (6, 2)
    assert K.hex_of(a, 1) == "%#066x" % (4 + (5 << 64) + (6 << 128) + (7 << 192))
