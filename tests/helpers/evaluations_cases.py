"""Shared pieces of the evaluation-phase tests (bzh_evaluations_plan, bzh_evaluations_batch_device): the query pattern, seeded
operands, and a big-int model of what the call must write and return, composed only of oracle pieces -- pasta.Blake2bTranscript
primed as tests/helpers/ipa_open_device_cases.py primes it, the field's omega(k) and eval_polynomial.  multiopen_continue carries
the same oracle transcript on through the multiopen argument (the steps of tests/helpers/multiopen_cases.py: model_proof, on a
transcript that is handed in), for the test that chains the two device calls."""
import functools
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (os.path.join(ROOT, "battlezips-halo2_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402

import coracle as C  # noqa: E402
import halo2_oracle as H  # noqa: E402
import pasta as O  # noqa: E402
from helpers import ipa_open_device_cases as K  # noqa: E402
from helpers import multiopen_cases as M  # noqa: E402

# 7 own polynomials (ids 0-6) and 2 shared ones (7, 8).  Own polynomials at {0}, {0, 1}, {0, 1, -1} and {0, -5}; own polynomial 4 at
# 8 distinct rotations, the smallest int32 among them (two passes of the kernel, 5 + 3 points); a repeated query; the shared ones
# at {0}; own polynomial 5 is never queried; own polynomial 6 at 4 rotations, so that a pass of every size from 1 to 5 occurs.
NOWN, NSHARED = 7, 2
INT32_MIN = -2 ** 31
QUERIES = [(0, 0), (1, 0), (1, 1), (2, 0), (2, 1), (2, -1), (3, 0), (4, 2), (3, -5), (1, 0), (7, 0), (4, 0), (4, 1), (4, -1), (4, -2),
           (6, 1), (4, 3), (4, INT32_MIN), (6, 0), (4, -5), (6, -5), (8, 0), (6, 3)]
ROTATIONS = [0, 1, -1, 2, -5, -2, 3, INT32_MIN]   # first-seen order
ROT_COUNT = [1, 2, 3, 2, 8, 0, 4, 1, 1]
POLY_ORDER = [0, 1, 2, 3, 4, 7, 6, 8]


def plan(queries, npolys):
    """bzh_evaluations_plan in a few lines: (rotations, point_of_query, poly_order, rot_count)"""
    rotations, point, order, rots_of = [], [], [], [set() for _ in range(npolys)]
    for pid, rot in queries:
        if rot not in rotations:
            rotations.append(rot)
        point.append(rotations.index(rot))
        if pid not in order:
            order.append(pid)
        rots_of[pid].add(rot)
    return rotations, point, order, [len(s) for s in rots_of]


def proof_cap(nqueries):
    return 32 + 32 * nqueries   # the primed point first


@functools.lru_cache(maxsize=None)
def operands(cid, k, B, npieces, seed=0):
    """own polynomials (B x NOWN x n ints; proof 1 of a batch of three has all-zero own polynomials), shared ones, the pieces of
    h (B x npieces x n) and their blinds"""
    F = O.CURVE_BY_ID[cid].scalar
    rng = random.Random(12000 + 1000 * seed + 100 * cid + 10 * k + 3 * B + npieces)
    n = 1 << k
    polys = [[[rng.randrange(F.p) for _ in range(n)] for _ in range(NOWN)] for _ in range(B)]
    if B == 3:
        polys[1] = [[0] * n for _ in range(NOWN)]
    shared = [[rng.randrange(F.p) for _ in range(n)] for _ in range(NSHARED)]
    pieces = [[[rng.randrange(F.p) for _ in range(n)] for _ in range(npieces)] for _ in range(B)]
    hblinds = [[rng.randrange(F.p) for _ in range(npieces)] for _ in range(B)]
    return polys, shared, pieces, hblinds


def model_transcript(cid, k, b, queries, polys_b, shared, pieces_b, hblinds_b):
    """proof b up to the last written evaluation: (the oracle transcript, points, evaluations, h, h_blind)"""
    F = O.CURVE_BY_ID[cid].scalar
    p, n = F.p, 1 << k
    w = F.omega(k)
    poly_of = lambda i: polys_b[i] if i < len(polys_b) else shared[i - len(polys_b)]   # noqa: E731
    T = K.primed_oracle(cid, b)
    x = T.squeeze_challenge()
    evals = []
    for pid, rot in queries:
        evals.append(O.eval_polynomial(poly_of(pid), x * pow(w, rot, p) % p, F))
        T.write_scalar(evals[-1])
    points = [x * pow(w, rot, p) % p for rot in plan(queries, len(polys_b) + len(shared))[0]]
    xn = pow(x, n, p)
    h, h_blind = [0] * n, 0
    for piece, blind in zip(reversed(pieces_b), reversed(hblinds_b)):
        h = [(a * xn + c) % p for a, c in zip(h, piece)]
        h_blind = (h_blind * xn + blind) % p
    return T, points, evals, h, h_blind


@functools.lru_cache(maxsize=None)
def model(cid, k, B, npieces):
    """per proof: (proof bytes, the next challenge, points, evaluations, h, h_blind) on QUERIES and operands()"""
    polys, shared, pieces, hblinds = operands(cid, k, B, npieces)
    out = []
    for b in range(B):
        T, points, evals, h, h_blind = model_transcript(cid, k, b, QUERIES, polys[b], shared, pieces[b], hblinds[b])
        out.append((bytes(T.proof), T.squeeze_challenge(), points, evals, h, h_blind))
    return out


def multiopen_continue(cid, k, T, queries, polys_b, shared, blinds_b, sblinds, points_b, rb):
    """the multiopen part of halo2_oracle.create_proof on the transcript T, which is left after the opening's last message"""
    cv = O.CURVE_BY_ID[cid]
    F = cv.scalar
    p, n = F.p, 1 << k
    g, w, u = K.srs(cid, k)
    nown = len(polys_b)
    rnd = iter(O.from_u512(rb[64 * i:64 * (i + 1)], F) for i in range(n + 2 + 2 * k))
    poly_of = lambda i: polys_b[i] if i < nown else shared[i - nown]        # noqa: E731
    blind_of = lambda i: blinds_b[i] if i < nown else sblinds[i - nown]     # noqa: E731
    x1 = T.squeeze_challenge()
    x2 = T.squeeze_challenge()
    point_sets, groups = M.oracle_sets(queries)
    q_polys, q_blinds, q_evalsets, pt_values = [], [], [], []
    for key, grp in zip(point_sets, groups):
        pts = [points_b[j] for j in key]
        poly, blind, evs = [0] * n, 0, [0] * len(pts)
        for i in grp:
            cp, cb = poly_of(i), blind_of(i)
            poly = [(a * x1 + c) % p for a, c in zip(poly, cp)]
            blind = (blind * x1 + cb) % p
            evs = [(e * x1 + O.eval_polynomial(cp, ptv, F)) % p for e, ptv in zip(evs, pts)]
        q_polys.append(poly), q_blinds.append(blind), q_evalsets.append(evs), pt_values.append(pts)
    f_poly = None
    for pts, evs, poly in zip(pt_values, q_evalsets, q_polys):
        r_poly = H.lagrange_interpolate(pts, evs, F)
        pl = list(poly)
        for i, rv in enumerate(r_poly):
            pl[i] = (pl[i] - rv) % p
        for ptv in pts:
            pl = O.kate_division(pl, ptv, F)
        pl = pl + [0] * (n - len(pl))
        f_poly = pl if f_poly is None else [(a * x2 + c) % p for a, c in zip(f_poly, pl)]
    f_blind = next(rnd)
    T.write_point(cv, M.commit(cv, g, w, f_poly, f_blind))
    x3 = T.squeeze_challenge()
    for poly in q_polys:
        T.write_scalar(O.eval_polynomial(poly, x3, F))
    x4 = T.squeeze_challenge()
    p_poly, p_blind = f_poly, f_blind
    for poly, blind in zip(q_polys, q_blinds):
        p_poly = [(a * x4 + c) % p for a, c in zip(p_poly, poly)]
        p_blind = (p_blind * x4 + blind) % p
    O.ipa_open(cv, list(g), w, u, p_poly, p_blind, x3, list(rnd), T)


def lim(values, conv=lambda x: x):
    return C.ints_to_array([conv(x) for x in values])


def arrays(ops, k, npieces, h_stride, conv=lambda x: x):
    """the operands as uint64 limb arrays: polys (B, NOWN, n, 4), shared (NSHARED, n, 4), the pieces in rows of h_stride elements
    (B, h_stride, 4) whose tail past npieces * n holds 7s, the pieces' blinds (B, npieces, 4); the last two None without pieces"""
    polys, shared, pieces, hblinds = ops
    n = 1 << k
    p = np.stack([np.stack([lim(c, conv) for c in pb]) for pb in polys])
    sh = np.stack([lim(c, conv) for c in shared])
    if not npieces:
        return p, sh, None, None
    hp = np.full((len(polys), h_stride, 4), 7, dtype=np.uint64)
    hp[:, :, 1:] = 0
    for b, pb in enumerate(pieces):
        for i, c in enumerate(pb):
            hp[b, i * n:(i + 1) * n] = lim(c, conv)
    return p, sh, hp, np.stack([lim(v, conv) for v in hblinds])


def ints(a):
    """a (.., 4) limb array as nested lists of ints"""
    import bzh2
    a = np.asarray(a)
    if a.ndim == 1:
        return bzh2.limbs_to_int(a)
    return [ints(x) for x in a]
