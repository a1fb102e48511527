"""Shared pieces of the grand-product tests (bzh_grand_products_plan, bzh_grand_products_batch_device): the state of an oracle
proof at the grand-product boundary, derived from helpers.vanishing_cases.capture's State (the oracle is not instrumented again),
and the model: a direct integer implementation of halo2_oracle.create_proof's permutation and lookup products
(oracle/halo2_oracle.py:363-401) with inv(0) = 0, which is upstream's batch_invert.  Whenever the operands are the captured ones
the model is asserted against what the oracle computed.  Call inside helpers.real_parity's accelerated_oracle."""
import random

import numpy as np

import halo2_oracle as H
import pasta as O
import sample_circuit as S
from helpers import vanishing_cases as V

CV, F = V.CV, V.F
P = F.p


class Boundary:
    """one proof at the grand-product boundary: prefix_ops / prefix_proof (beta and gamma are its last two squeezes), beta, gamma,
    the operands over the domain (cols: {'advice' | 'instance': [column]}, lk: [{'a_c', 's_c', 'a', 's'}]), the phase's draws as
    bytes (rng) and as integers (draws), and the vanishing State it was cut from (v)"""


def boundary(keys, st):
    cs, dom = keys.cs, keys.dom
    n, bf = cs.n, cs.blinding_factors
    nz = len(st.perm) + len(st.lk)
    b = Boundary()
    b.v, b.nz, b.beta, b.gamma = st, nz, st.beta, st.gamma
    assert all(op == "write_point" for op, _ in st.prefix_ops[len(st.prefix_ops) - nz:])
    b.prefix_ops, b.prefix_proof = st.prefix_ops[:len(st.prefix_ops) - nz], st.prefix_proof[:len(st.prefix_proof) - 32 * nz]
    assert b.prefix_ops[-2:] == [("squeeze", st.beta), ("squeeze", st.gamma)]
    last = st.used - (n + 1)                                   # (the random polynomial and its blind follow the products' draws)
    b.rng = st.rbytes[64 * (last - nz * (bf + 1)):64 * last]
    b.draws = [O.from_u512(b.rng[64 * i:64 * (i + 1)], F) for i in range(nz * (bf + 1))]
    # the advice over the domain with its blinding rows: the captured polynomials evaluated back
    adv = [O.ntt(list(c), dom.omega, F) for c in st.adv_polys]
    usable = cs.usable_rows
    assert all(list(col[:usable]) == [v % P for v in (list(src) + [0] * n)[:usable]] for col, src in zip(adv, st.advice))
    b.cols = {"advice": adv, "instance": [list(c) + [0] * (n - len(c)) for c in st.instance]}
    b.lk = [{nm: list(d[nm]) for nm in ("a_c", "s_c", "a", "s")} for d in st.lk]
    return b


def inv0(x):
    return pow(x, P - 2, P)                                    # 0 for 0


def products(keys, cols, lk, beta, gamma, draws):
    """(z, blinds, status): every product over the domain in the order they are made -- permutation sets, then lookups --, the
    draws taken in upstream's order; status: the last set's z[usable] or a lookup's z[usable] is not 1"""
    cs, dom = keys.cs, keys.dom
    n, bf, usable = cs.n, cs.blinding_factors, cs.usable_rows
    rnd = iter(draws)
    lag = dict(cols, fixed=keys.fixed)
    nsets = (len(cs.perm_columns) + cs.chunk_len - 1) // cs.chunk_len if cs.perm_columns else 0
    zs, blinds, last_z, status = [], [], 1, 0
    wpow = [pow(dom.omega, r, P) for r in range(n)]

    def finish(z):
        for r in range(n - bf, n):
            z[r] = next(rnd)
        zs.append(z)
        blinds.append(next(rnd))

    for i in range(nsets):
        z = [last_z]
        for r in range(n - 1):
            num = den = 1
            for j, c in enumerate(cs.perm_columns[i * cs.chunk_len:(i + 1) * cs.chunk_len], i * cs.chunk_len):
                v = lag[c[0]][c[1]][r]
                den = den * ((beta * keys.sigma[j][r] + gamma + v) % P) % P
                num = num * ((pow(dom.delta, j, P) * wpow[r] % P * beta + gamma + v) % P) % P
            z.append(z[-1] * num % P * inv0(den) % P)
        last_z = z[usable]
        finish(z)
    status |= int(nsets > 0 and last_z != 1)
    for d in lk:
        z = [1]
        for r in range(n - 1):
            nu = (d["a_c"][r] + beta) * (d["s_c"][r] + gamma) % P
            de = (d["a"][r] + beta) * (d["s"][r] + gamma) % P
            z.append(z[-1] * nu % P * inv0(de) % P)
        status |= int(z[usable] != 1)
        finish(z)
    return zs, blinds, status


def model(keys, operands, beta, gamma, draws):
    """what the leaf must write and return for one proof: (the proof bytes it appends, the next squeeze, z, z_polys, the blinds,
    the status bit).  operands: a Boundary (its cols, lk and prefix_ops are read); when beta, gamma, the draws and the operands
    are the captured ones, the result is checked against the oracle's own values"""
    dom = keys.dom
    zs, blinds, status = products(keys, operands.cols, operands.lk, beta, gamma, draws)
    polys = [dom.lagrange_to_coeff(z) for z in zs]
    T = V.replay(operands.prefix_ops)
    for poly, blind in zip(polys, blinds):
        T.write_point(CV, keys.commit(poly, blind))
    return bytes(T.proof[len(operands.prefix_proof):]), T.squeeze_challenge(), zs, polys, blinds, status


def check_captured(keys, b):
    """the model on the captured operands is the oracle: z, polynomial and blind of every product, the bytes, a closed witness"""
    st = b.v
    got = model(keys, b, b.beta, b.gamma, b.draws)
    want = [(d["z"], d["poly"], d["blind"]) for d in st.perm] + [(d["z"], d["z_poly"], d["z_blind"]) for d in st.lk]
    assert [list(z) for z in got[2]] == [list(w[0]) for w in want]
    assert [list(c) for c in got[3]] == [list(w[1]) for w in want] and got[4] == [w[2] for w in want]
    assert got[0] == st.prefix_proof[len(b.prefix_proof):] and got[5] == 0
    return got


_CASES = {}


def case(k, with_lookup, degree, B):
    """helpers.vanishing_cases.case cut at the grand-product boundary: (cs, keys, circuit, (g, w, u), [Boundary], [whole proofs],
    [model on the captured operands])"""
    key = (k, with_lookup, degree, B)
    if key not in _CASES:
        cs, keys, circ, gwu, states, proofs = V.case(k, with_lookup, degree, B)
        bounds = [boundary(keys, s) for s in states]
        _CASES[key] = (cs, keys, circ, gwu, bounds, proofs, [check_captured(keys, b) for b in bounds])
    return _CASES[key]


def all_kinds_case(k=5, B=2):
    """the sample circuit with its lookup table column added to the permutation and one copy into it, so that the permutation has
    an advice, an instance and a fixed column: same tuple as case().  advice 1, row 0 is 1 in every witness (the first power of
    two of the bit decomposition) and the table column holds its row number in its first rows"""
    key = ("kinds", k, B)
    if key not in _CASES:
        from bzh2 import circuit_data as Pd
        built = [S.build(k=k, seed=900 + 7 * b, with_lookup=True) for b in range(B)]
        cs0, fixed, copies = built[0][:3]
        assert fixed[2][1] == 1 and all(bt[3][1][0] == 1 for bt in built)
        perm = list(cs0.perm_columns) + [("fixed", 2)]
        copies = list(copies) + [((1, 0), (len(perm) - 1, 1))]
        cs = H.ConstraintSystem(cs0.k, cs0.num_advice, cs0.num_fixed, cs0.num_instance, cs0.gates, perm, cs0.lookups)
        rng = random.Random(4100 + k)
        g = [CV.random_point(rng) for _ in range(cs.n)]
        w, u = CV.random_point(rng), CV.random_point(rng)
        keys = H.Keys(cs, H.Domain(cs, F), CV, g, w, u, fixed, copies)
        circ = Pd.Circuit(cs.k, cs.num_advice, cs.num_fixed, cs.num_instance, cs.gates, cs.perm_columns, cs.lookups, fixed, copies)
        bounds, proofs = [], []
        for b in range(B):
            rbytes = bytes(rng.getrandbits(8) for _ in range(64 * V.draws_per_proof(cs)))
            st, proof = V.capture(keys, built[b][3], built[b][4], rbytes)
            assert H.verify_proof(keys, built[b][4], proof, O.Blake2bTranscript(F))
            bounds.append(boundary(keys, st)), proofs.append(proof)
        _CASES[key] = (cs, keys, circ, (g, w, u), bounds, proofs, [check_captured(keys, b) for b in bounds])
    return _CASES[key]


def operand_arrays(bounds, conv=lambda x: x):
    """the leaf's operands as uint64 limb arrays: advice (B, na, n, 4), instance (B, ni, n, 4), lookup_compressed and
    lookup_permuted (B, nl, 2, n, 4) or None"""
    stack = lambda rows: np.stack([np.stack([V.lim(c, conv) for c in r]) for r in rows])  # noqa: E731
    adv = stack([b.cols["advice"] for b in bounds])
    inst = stack([b.cols["instance"] for b in bounds])
    if not bounds[0].lk:
        return adv, inst, None, None
    pair = lambda x, y: np.stack([np.stack([np.stack([V.lim(d[x], conv), V.lim(d[y], conv)]) for d in b.lk]) for b in bounds])  # noqa: E731
    return adv, inst, pair("a_c", "s_c"), pair("a", "s")
