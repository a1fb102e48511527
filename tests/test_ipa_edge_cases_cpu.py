"""tests/helpers/ipa_edge_cases.py without a GPU: the builders' invariants, and the reference's own check on reference strings it
has never folded -- the accelerated oracle (C MSMs and generator folds, the reference of tests/test_gpu_ipa_edges.py) emits the
big-int oracle's bytes on a periodic and on a dead-column string, identities and cancelling points included."""
import random

import pytest

import accel
import pasta as O
from helpers import ipa_edge_cases as E


def _first(**want):
    return next(c for c in E.CASES if all(getattr(c, k) == v for k, v in want.items()))


@pytest.mark.parametrize("case", [_first(k=3, family="periodic", cid=0), _first(k=3, family="dead", cid=1)], ids=lambda c: c.name)
def test_accelerated_oracle_emits_the_bigint_oracles_bytes(oracle_c, case):
    want = E.reference(case.name)
    with accel.accelerated(threads=2):
        got = E.reference(case.name)
    assert got == want
    assert all(len(proof) == 32 + 32 * (1 + 2 * case.k + 2) for _, proof in want)


def test_pool_points_are_distinct_and_u_w_are_outside():
    for cid in (0, 1):
        cv = O.CURVE_BY_ID[cid]
        pts, u, w = E.pool(cid)
        xs = {q[0] for q in pts}
        assert len(pts) == E.POOL == len(xs)                  # distinct x: no point equals another or its negative
        assert u[0] not in xs and w[0] not in xs and u[0] != w[0]
        assert all(cv.is_on_curve(q) for q in (pts[0], pts[-1], u, w))


@pytest.mark.parametrize("case", [c for c in E.CASES if c.family != "plain"], ids=lambda c: c.name)
def test_periodic_and_dead_strings_repeat_negate_and_vanish_as_documented(case):
    cv = O.CURVE_BY_ID[case.cid]
    n, m = 1 << case.k, case.m
    g, w, u = E.srs(case)
    base = E.pool(case.cid)[0][:m]
    assert len(g) == n and w is not None and u is not None
    ids = set(E.periodic_identities(n, m))
    for i in range(n):
        col, t = i % m, i // m
        if col in case.dead or i in ids:
            assert g[i] is None
        else:
            assert g[i] == (cv.neg(base[col]) if t % 3 == 2 else base[col])
    live = [c for c in range(m) if c not in case.dead]
    assert live and all(g[c] is not None for c in live)       # t = 0 is never an identity repeat
    if n // m >= 3:                                           # far enough for a negated repeat: a column holds P, P and -P
        for c in live:
            col = [g[c + t * m] for t in range(n // m)]
            assert cv.neg(base[c]) in col and col.count(base[c]) >= 2 - (1 if (m + c) in ids else 0)


@pytest.mark.parametrize("case", [_first(k=3, family="dead", cid=0), _first(k=6, family="dead", cid=1),
                                  _first(k=6, family="periodic", cid=0)], ids=lambda c: c.name)
def test_folded_generators_of_the_model_are_upstreams_and_dead_columns_fold_to_the_identity(oracle_c, case):
    """G'[i] = sum_t s_t G[i + t m'] with s^(j+1)[2t + beta] = s^(j)[t] u_j^beta (csrc/ipa.hip's header) equals upstream's round by
    round fold, at every round; on the dead family G'[i] is the identity for every i = i0 mod m, and no live column folds to it.
    Big-int group arithmetic at k = 3; at k = 6 (some 300 scalar multiplications) the C oracle's, which the first test pins."""
    if case.k > 3:
        with accel.accelerated(threads=2):
            return _check_folds(case)
    _check_folds(case)


def _check_folds(case):
    cv = O.CURVE_BY_ID[case.cid]
    p = cv.scalar.p
    n = 1 << case.k
    g, _, _ = E.srs(case)
    rng = random.Random(case.name)
    s, folded = [1], list(g)
    for j in range(1, case.k):
        uj = rng.randrange(1, p)
        s = [x * (uj if beta else 1) % p for x in s for beta in (0, 1)]
        folded = O.fold_bases(cv, folded, uj)
        mj = n >> j
        model = [cv.msm_naive(s, [g[i + t * mj] for t in range(1 << j)]) for i in range(mj)]
        assert model == folded
        if mj >= case.m:
            for i in range(mj):
                assert (model[i] is None) == (i % case.m in case.dead)
