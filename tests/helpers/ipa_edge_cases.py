"""Case builders of tests/test_gpu_ipa_edges.py and tests/test_ipa_edge_cases_cpu.py: openings whose reference strings and
operands sit where the generator collapse (k_collapse_generators, k_expand_rows_shared_inverse in csrc/msm.hip) and the round
kernels of csrc/ipa.hip can go wrong -- generators that repeat with period m, so that every folded generator sums one point with
itself and with its negative; columns of identities, so that a folded generator IS the identity; polynomials with a zero half,
x3 in {0, 1, p - 1, a root of unity}, zero blinds, and 64-byte draws at the bounds of k_reduce_wide.

Run as a program (`ipa_edge_cases.py SETTING`) it is ONE process = one setting of BZH_IPA_COLLAPSE / BZH_IPA_TAIL_C /
BZH_ACC_SATURATED (read once per process; the PARENT puts them into the environment): it opens every case of SETTINGS[SETTING]
with Context.ipa_open_batch under profiling and prints one JSON line per case -- the proofs, the v's, and the bucket additions
and launch counts of that case alone.  The reference (oracle/pasta.py: ipa_open, upstream's collapsing algorithm) is computed
by the parent, never here."""
import collections
import functools
import json
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (os.path.join(ROOT, "battlezips-halo2_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import coracle as C  # noqa: E402
import pasta as O  # noqa: E402
from helpers import ipa_open_device_cases as K  # noqa: E402

POOL = 1024   # distinct points per curve: the plain family at k = 10 takes them all


# ---------------------------------------------------------------------------
# reference strings
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def pool(cid):
    """(POOL distinct random points, U, W): U and W are drawn after the pool and differ from every pool point and its negative"""
    cv = O.CURVE_BY_ID[cid]
    rng = random.Random(0x1BA0 + cid)
    pts, seen = [], set()
    while len(pts) < POOL + 2:
        q = cv.random_point(rng)
        if q[0] not in seen:          # a new x: neither a pool point nor the negative of one
            seen.add(q[0])
            pts.append(q)
    return tuple(pts[:POOL]), pts[POOL], pts[POOL + 1]


def srs_plain(cid, n):
    return list(pool(cid)[0][:n])


def periodic_identities(n, m):
    """the few repeats (t >= 1, so no column loses its t = 0 entry) that are the identity"""
    return sorted({i for i in (m, 5 * m + min(3, m - 1), n - 1) if m <= i < n})


def srs_periodic(cid, n, m):
    """G[i + t m] = +-G[i]: every third repeat (t mod 3 = 2) negated, a few repeats the identity (None).  Every output of a
    collapse to m' = n >> j >= m points, G'[i'] = sum_t' s_t' G[i' + t' m'], then sums +-(the same pool point)."""
    base = pool(cid)[0][:m]
    cv = O.CURVE_BY_ID[cid]
    out = [cv.neg(base[i % m]) if (i // m) % 3 == 2 else base[i % m] for i in range(n)]
    for i in periodic_identities(n, m):
        out[i] = None
    return out


def srs_dead(cid, n, m, dead):
    """the periodic set with G[i0 + t m] the identity for all t and every i0 in `dead`: G'[i'] is the identity exactly for every
    i' = i0 mod m, whatever the scalars"""
    out = srs_periodic(cid, n, m)
    for i in range(n):
        if i % m in dead:
            out[i] = None
    return out


# ---------------------------------------------------------------------------
# operands: every kind is named, so that a test can look a proof up by what it is
# ---------------------------------------------------------------------------
POLYS = ["zero", "upper_zero", "lower_zero", "last_only", "all_minus_one", "alternating", "uniform"]
X3S = ["zero", "one", "minus_one", "omega_n", "uniform"]
BLINDS = ["uniform", "zero", "minus_one", "uniform"]
DRAWS = ["uniform", "uniform", "uniform", "uniform", "all_ff", "uniform", "uniform", "uniform", "uniform", "bounds", "uniform"]


def make_poly(kind, n, F, rng):
    p, h = F.p, n // 2
    if kind == "zero":
        return [0] * n
    if kind == "upper_zero":
        return [rng.randrange(p) for _ in range(h)] + [0] * (n - h)
    if kind == "lower_zero":
        return [0] * h + [rng.randrange(p) for _ in range(n - h)]
    if kind == "last_only":
        return [0] * (n - 1) + [rng.randrange(1, p)]
    if kind == "all_minus_one":
        return [p - 1] * n
    if kind == "alternating":
        x = rng.randrange(1, p)
        return [x if i % 2 == 0 else p - x for i in range(n)]
    assert kind == "uniform"
    return [rng.randrange(p) for _ in range(n)]


def make_x3(kind, k, F, rng):
    return {"zero": 0, "one": 1, "minus_one": F.p - 1, "omega_n": F.omega(k), "uniform": rng.randrange(F.p)}[kind]


def make_blind(kind, F, rng):
    return {"zero": 0, "minus_one": F.p - 1, "uniform": rng.randrange(F.p)}[kind]


def make_draws(kind, nrand, F, rng):
    """nrand 64-byte draws, each read as a 512-bit little-endian integer and reduced mod p (k_reduce_wide): all 0xff is the
    largest input; p, 2^256 - 1 and 2^256 are a low half that reduces to 0, the largest low half, and the smallest high half"""
    if kind == "all_ff":
        return b"\xff" * (64 * nrand)
    if kind == "bounds":
        vals = [F.p, (1 << 256) - 1, 1 << 256]
        return b"".join(vals[i % 3].to_bytes(64, "little") for i in range(nrand))
    assert kind == "uniform"
    return rng.randbytes(64 * nrand)


# ---------------------------------------------------------------------------
# cases.  c: the window width of the table (bzh_bases_precompute), 0 = the library's own choice, None = no table.
# family: "plain" | "periodic" | "dead"; m: the period; dead: the dead columns; recipes: (poly, x3, blind, draws) per proof
# ---------------------------------------------------------------------------
Case = collections.namedtuple("Case", "name cid k B c family m dead recipes")
WIDTHS = [4, 5, 8, 15]     # nwin = 64, 52, 32, 18; h = c / 2 = 2, 2, 4, 7: even and odd splits of the collapse's digits
# the period per k: the smallest m at which every forced round (m' = n >> j >= m) still sees repeats, and at which t runs far
# enough for a negated repeat (t = 2): k = 2 -> (+, id, -, id) on one point; k = 3 -> (+, +, -, +) on two; k = 6 -> 16 repeats of 4
PERIOD = {2: 1, 3: 2, 6: 4}
# the dead family's period and columns: k = 2 has two columns only, one stays alive
DEAD = {2: (2, (1,)), 3: (4, (1, 3)), 6: (4, (1, 2))}


def _build_cases():
    cases, q = [], 0

    def rotate(B):
        nonlocal q
        out = []
        for _ in range(B):
            out.append((POLYS[q % len(POLYS)], X3S[q % len(X3S)], BLINDS[q % len(BLINDS)], DRAWS[q % len(DRAWS)]))
            q += 1
        return tuple(out)

    idx = 0
    for cid in (0, 1):
        for k in (2, 3, 6):
            for family in ("plain", "periodic", "dead"):
                c = WIDTHS[idx % 4]
                idx += 1
                m, dead = (0, ()) if family == "plain" else (PERIOD[k], ()) if family == "periodic" else DEAD[k]
                cases.append(Case("%s_k%d_c%d_%s" % (O.CURVE_BY_ID[cid].name, k, c, family), cid, k, 3, c, family, m, dead, rotate(3)))
    # no window table: `paired` is false, the rounds run k_ipa_round_vectors and msm_run on 2 B vectors
    cases.append(Case("vesta_k3_notable_periodic", 0, 3, 3, None, "periodic", 2, (), rotate(3)))
    # the three proofs the verifiers also see: the zero polynomial, x3 = 0, all of them on a dead column
    cases.append(Case("vesta_k3_c5_dead_verify", 0, 3, 3, 5, "dead", 4, (1, 3),
                      (("zero", "uniform", "uniform", "uniform"), ("uniform", "uniform", "uniform", "uniform"),
                       ("uniform", "zero", "uniform", "uniform"))))
    # B = 8, k = 9: the cost model collapses by itself
    cases.append(Case("vesta_k9_b8_plain", 0, 9, 8, 0, "plain", 0, (), rotate(8)))
    cases.append(Case("vesta_k9_b8_periodic", 0, 9, 8, 0, "periodic", 4, (), rotate(8)))
    # k = 10, B = 2: half = 512 in round 0 (k_ipa_inner2 strides twice), cnt = 512 at half = 1 in round 9 without a collapse
    cases.append(Case("vesta_k10_b2_plain", 0, 10, 2, 0, "plain", 0, (), rotate(2)))
    return cases


CASES = _build_cases()
BY_NAME = {c.name: c for c in CASES}
SMALL = [c.name for c in CASES if c.k <= 6]
K9 = [c.name for c in CASES if c.k == 9]
K10 = [c.name for c in CASES if c.k == 10]

# one child process per setting: (environment, the cases it opens).  COLLAPSE=0 opens every case: its additions are what
# every other setting's are compared with.  "COLLAPSE = k - 2" is one setting per k (the variable is read once per process):
# 1 at k = 3, 4 at k = 6 -- m = 4 folded generators both times; at k = 2 it is COLLAPSE=0 itself.
SETTINGS = {
    "default": ({}, SMALL + K9),
    "collapse0": ({"BZH_IPA_COLLAPSE": "0"}, SMALL + K9 + K10),
    "collapse1": ({"BZH_IPA_COLLAPSE": "1"}, SMALL),
    "collapse2_tail4": ({"BZH_IPA_COLLAPSE": "2", "BZH_IPA_TAIL_C": "4"}, SMALL),
    "collapse1_tail13": ({"BZH_IPA_COLLAPSE": "1", "BZH_IPA_TAIL_C": "13"}, [n for n in SMALL if BY_NAME[n].k == 3]),
    "collapse4_tail13": ({"BZH_IPA_COLLAPSE": "4", "BZH_IPA_TAIL_C": "13"}, [n for n in SMALL if BY_NAME[n].k == 6]),
    "collapse2_tail7_saturated": ({"BZH_IPA_COLLAPSE": "2", "BZH_IPA_TAIL_C": "7", "BZH_ACC_SATURATED": "1"}, SMALL),
    "collapse3": ({"BZH_IPA_COLLAPSE": "3"}, K10),
}
ENV_NAMES = ("BZH_IPA_COLLAPSE", "BZH_IPA_TAIL_C", "BZH_ACC_SATURATED")


def srs(case):
    """(g, w, u): n generators (None = the identity), then the blinding and the inner-product base"""
    n = 1 << case.k
    _, u, w = pool(case.cid)
    if case.family == "plain":
        g = srs_plain(case.cid, n)
    elif case.family == "periodic":
        g = srs_periodic(case.cid, n, case.m)
    else:
        g = srs_dead(case.cid, n, case.m, case.dead)
    return g, w, u


@functools.lru_cache(maxsize=None)
def operands(name):
    """(polys, blinds, x3s, draws) of a case, from its recipes and a seed of its own"""
    case = BY_NAME[name]
    F = O.CURVE_BY_ID[case.cid].scalar
    n, nrand = 1 << case.k, (1 << case.k) + 1 + 2 * case.k
    rng = random.Random("ipa-edges/" + name)
    polys, blinds, x3s, rbs = [], [], [], []
    for poly, x3, blind, draws in case.recipes:
        polys.append(make_poly(poly, n, F, rng))
        x3s.append(make_x3(x3, case.k, F, rng))
        blinds.append(make_blind(blind, F, rng))
        rbs.append(make_draws(draws, nrand, F, rng))
    return polys, blinds, x3s, rbs


def reference(name):
    """[(v, proof bytes)] per proof: upstream's collapsing algorithm on a transcript primed as the child's.  Call it inside
    accel.accelerated(...) for the C oracle's MSMs and folds, outside for the big-int ones."""
    case = BY_NAME[name]
    cv = O.CURVE_BY_ID[case.cid]
    g, w, u = srs(case)
    polys, blinds, x3s, rbs = operands(name)
    nrand = (1 << case.k) + 1 + 2 * case.k
    out = []
    for b in range(case.B):
        rs = [O.from_u512(rbs[b][64 * i:64 * (i + 1)], cv.scalar) for i in range(nrand)]
        ot = K.primed_oracle(case.cid, b)
        v = O.ipa_open(cv, list(g), w, u, polys[b], blinds[b], x3s[b], rs, ot)
        out.append((v, bytes(ot.proof)))
    return out


def upload(ctx, case):
    g, w, u = srs(case)
    hb = ctx.upload_bases(case.cid, C.points_to_array(list(g) + [u, w]))
    if case.c is not None:
        hb.precompute(case.c)
    return hb


def open_case(ctx, name):
    """one bzh_ipa_open_batch under profiling: (v's, proofs, bucket additions, launches per timer) of this case alone"""
    case = BY_NAME[name]
    polys, blinds, x3s, rbs = operands(name)
    hb = upload(ctx, case)
    trs = K.primed(case.cid, case.B)
    try:
        ctx.profile(True)          # resets the timers and the additions counter
        v = ctx.ipa_open_batch(hb, K.poly_array(polys), blinds, x3s, list(rbs), trs)
        additions = ctx.msm_additions()
        launches = {timer: t["launches"] for timer, t in ctx.timings().items() if t["launches"]}
        ctx.profile(False)
        proofs = [t.proof() for t in trs]
    finally:
        for t in trs:
            t.close()
        hb.free()
    return v, proofs, additions, launches


def main(setting):
    import bzh2
    env, names = SETTINGS[setting]
    for name in ENV_NAMES:   # the parent sets the environment; a child that ran under another one would prove nothing
        assert os.environ.get(name) == env.get(name), "%s: %s is %r" % (setting, name, os.environ.get(name))
    ctx = bzh2.Context(0)
    for name in names:
        try:
            v, proofs, additions, launches = open_case(ctx, name)
        except Exception:
            print("FAILED in case %s %r" % (name, BY_NAME[name].recipes), file=sys.stderr)   # any library error: exit non-zero
            raise
        print(json.dumps({"case": name, "v": ["%064x" % x for x in v], "proofs": [p.hex() for p in proofs], "additions": additions,
                          "launches": launches}), flush=True)
    ctx.close()


if __name__ == "__main__":
    main(sys.argv[1])
