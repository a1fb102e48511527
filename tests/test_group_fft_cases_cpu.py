"""The model and the inputs of tests/test_gpu_group_fft.py, checked without a GPU (tests/helpers/group_fft_cases.py): the expected
points against the definition of the inverse group FFT computed another way, the integer replay of the kernels' schedule against
the inverse NTT, and -- a condition on the inputs, not a measurement -- that every named case meets the branch of the group law
it is named for, at every size the GPU test runs it, while the uniform case meets none."""
import random

import numpy as np
import pytest

import coracle as C
import pasta as O
from helpers import group_fft_cases as GF

F, R = GF.F, GF.R


@pytest.fixture(scope="module", autouse=True)
def _oracle(oracle_c):
    return oracle_c


def _stages(a, k):
    return GF.replay(a, k)[1]["stages"]


@pytest.mark.parametrize("k", [0, 1, 3])
@pytest.mark.parametrize("name", ["uniform", "quarter_zero"])
def test_expected_points_equal_the_definition(k, name):
    """out[i] = sum_j c_ij g[j], c_i = intt(e_i), by the pure-Python curve on the points themselves (no discrete logs).
    quarter_zero has no zero row below k = 2: there a vector with one zero row stands in."""
    rng = random.Random(31 + k)
    n = 1 << k
    if name in GF.case_names(k):
        a = GF.cases(k, rng)[name]
    else:
        a = [GF._nonzero(rng) for _ in range(n)]
        a[n - 1] = 0
    G = GF.generator()
    g_arr = GF.input_points(G, a)
    g = [C.array_to_point(g_arr[i]) for i in range(n)]
    assert [p is None for p in g] == [x == 0 for x in a]
    assert all(O.VESTA.is_on_curve(p) for p in g)
    got = GF.expected_points(G, GF.dlog_ifft(a, k))
    omega = F.omega(k)
    for i in range(n):
        e = [0] * n
        e[i] = 1
        want = O.VESTA.msm_naive(O.intt(e, omega, F), g)
        assert C.array_to_point(got[i]) == want, i


def test_expected_points_rows():
    """[0] G is the row of eight zero limbs, [1] G is G, [r - 1] G is -G, equal scalars give equal rows"""
    G = GF.generator()
    x, y = C.array_to_point(G)
    out = GF.expected_points(G, [0, 1, R - 1, 5, 5, R])
    assert not out[0].any() and not out[5].any()
    assert (out[1] == G).all()
    assert C.array_to_point(out[2]) == (x, O.Q - y)
    assert (out[3] == out[4]).all() and C.array_to_point(out[3]) == O.VESTA.mul(5, (x, y))


@pytest.mark.parametrize("k", [1, 3, 6])
def test_replay_equals_n_times_the_inverse_ntt(k):
    n = 1 << k
    cs = GF.cases(k, random.Random(77 + k))
    assert tuple(cs) and set(cs) == set(GF.case_names(k))
    for name, a in cs.items():
        b = GF.dlog_ifft(a, k)
        assert b == O.intt(a, F.omega(k), F), name
        final, counters = GF.replay(a, k)
        assert final == [n * x % R for x in b], name
        assert counters["zero_finals"] == sum(1 for x in b if x == 0), name
        assert len(counters["stages"]) == k and [s["m"] for s in counters["stages"]] == [1 << i for i in range(k)]


@pytest.mark.parametrize("k", sorted(set(GF.GPU_KS_CASES)))
def test_closed_forms(k):
    """the outputs the cases are built to have, from the formula b_j = n^-1 sum_i a_i omega^(-ij)"""
    n = 1 << k
    cs = GF.built(k)
    c = cs["constant"][0]
    w_inv = F.inv(F.omega(k))
    assert GF.dlog_ifft(cs["all_zero"], k) == [0] * n
    assert GF.dlog_ifft(cs["constant"], k) == [c] + [0] * (n - 1)
    assert GF.dlog_ifft(cs["alternating"], k) == [c if j == n // 2 else 0 for j in range(n)]
    for name in GF.IMPULSES:
        if name in cs:
            i = GF.impulse_index(name, k)
            assert GF.dlog_ifft(cs[name], k) == [c * F.inv(n) * pow(w_inv, i * j, R) % R for j in range(n)], name
    b = GF.dlog_ifft(cs["equal_halves"], k)
    assert all(b[j] == 0 for j in range(1, n, 2)) and all(b[j] for j in range(0, n, 2))
    b = GF.dlog_ifft(cs["opposite_halves"], k)
    assert all(b[j] == 0 for j in range(0, n, 2)) and all(b[j] for j in range(1, n, 2))


def _special(stage):
    return {key: v for key, v in stage.items() if key != "m" and v}


@pytest.mark.parametrize("k", sorted(set(GF.GPU_KS_EVERY_OUTPUT) | set(GF.GPU_KS_CASES)))
def test_the_uniform_case_is_the_control(k):
    """no butterfly of the uniform case adds equal, opposite or identity operands, and no output is the identity"""
    stages, zero_finals = GF.replay(GF.built(k)["uniform"], k)[1].values()
    assert [_special(s) for s in stages] == [{}] * k and zero_finals == 0


def test_the_walked_table_is_generic_too():
    k = GF.GPU_K_WALK
    stages, zero_finals = GF.replay([i + 1 for i in range(1 << k)], k)[1].values()
    assert [_special(s) for s in stages] == [{}] * k and zero_finals == 0


@pytest.mark.parametrize("k,name", GF.gpu_case_params())
def test_each_case_reaches_the_branch_it_is_named_for(k, name):
    n = 1 << k
    a = GF.built(k)[name]
    assert len(a) == n and all(0 <= x < R for x in a)
    counters = GF.replay(a, k)[1]
    st, zero_finals = counters["stages"], counters["zero_finals"]
    if name == "uniform":
        assert not any(_special(s) for s in st)
    elif name == "all_zero":
        # every operand of every butterfly, every twiddled operand and every row of k_gfft_finish is the identity
        assert all(s["a_zero"] == s["t_zero"] == n // 2 and s["twiddle_on_zero"] == n // 2 - n // (2 * s["m"]) for s in st)
        assert zero_finals == n
    elif name == "constant":
        # stage 1: every butterfly doubles in s and cancels in d; from then on the j = 0 butterflies go on doubling and the
        # others add identities
        assert st[0]["eq"] == n // 2 and st[0]["neg"] == 0
        assert GF.doublings(st[0]) == GF.cancellations(st[0]) == n // 2
        assert all(s["eq"] == n // (2 * s["m"]) and s["a_zero"] == s["t_zero"] == n // 2 - s["eq"] for s in st[1:])
        assert zero_finals == n - 1
    elif name == "alternating":
        # the bit-reversed load pairs a_i with a_(i + n/2) in stage 1: opposite at k = 1, equal from k = 2 on.  Either way
        # stage 1 cancels (in s or in d); the last stage meets a == -t, the cancellation in s itself
        assert GF.cancellations(st[0]) == n // 2
        assert (st[0]["neg"], st[0]["eq"]) == ((1, 0) if k == 1 else (0, n // 2))
        if k >= 2:
            assert GF.doublings(st[1]) >= 1
        assert st[-1]["neg"] == 1 and st[-1]["eq"] == 0
        assert zero_finals == n - 1
    elif name in GF.IMPULSES:
        # one operand of a butterfly is the identity and the other is not; at k >= 2 the all-identity butterflies count for
        # both sides.  Which side the impulse is on is a bit of its bit-reversed index: see the test of all four below.  By
        # stage m it has spread over m rows, the m butterflies of one half-group
        assert [s["a_zero_only"] + s["t_zero_only"] for s in st] == [s["m"] for s in st]
        if k >= 2:
            assert sum(s["a_zero"] for s in st) >= 1 and sum(s["t_zero"] for s in st) >= 1
        # a twiddle meets the identity wherever a j != 0 butterfly has no part of the impulse in its upper operand: everywhere
        # from k = 3 on; at k = 2 the only twiddled butterfly is (1, 3) of stage 2, empty for the impulses loaded below index 2
        reached = sum(s["twiddle_on_zero"] for s in st) > 0
        assert reached == (k >= 3 or (k == 2 and name in ("impulse_first", "impulse_middle")))
        assert zero_finals == 0 and not any(s["eq"] or s["neg"] for s in st)
    elif name == "equal_halves":
        assert st[0]["eq"] == n // 2 and zero_finals == n // 2
    elif name == "opposite_halves":
        assert st[0]["neg"] == n // 2 and zero_finals == n // 2
    elif name == "late_doubling":
        # exactly one butterfly of the whole transform is special: a == t, after the twiddle, in the last stage
        assert not any(_special(s) for s in st[:-1])
        assert _special(st[-1]) == {"eq": 1, "eq_twiddled": 1}
        assert zero_finals == 1
    elif name == "quarter_zero":
        assert sum(1 for x in a if x == 0) == n // 4
        assert st[0]["a_zero"] + st[0]["t_zero"] >= 1 and zero_finals == 0
    else:
        raise AssertionError("a case without a reach condition: " + name)


@pytest.mark.parametrize("k", sorted(set(GF.GPU_KS_CASES)))
def test_the_impulses_together_put_the_identity_on_either_side(k):
    """a == 0 != t (xyzz_add takes the other operand) and t == 0 != a (it returns at once), and at k >= 2 a twiddle on the
    identity: each met by at least one of the impulses of a size"""
    cs = GF.built(k)
    st = [s for name in GF.IMPULSES if name in cs for s in _stages(cs[name], k)]
    assert sum(s["a_zero_only"] for s in st) >= 1 and sum(s["t_zero_only"] for s in st) >= 1
    assert (sum(s["twiddle_on_zero"] for s in st) >= 1) == (k >= 2)


def test_wrapper_refuses_before_it_loads_anything():
    """bzh2.params.group_ifft on a row count that is no power of two, or on another shape: ValueError before the library or the
    context is touched (ctx = None would fail otherwise)"""
    from bzh2 import params as Pm
    for shape in ((3, 8), (6, 8), (0, 8), (4, 4), (8,), (2, 2, 8)):
        with pytest.raises(ValueError):
            Pm.group_ifft(None, np.zeros(shape, dtype=np.uint64))
