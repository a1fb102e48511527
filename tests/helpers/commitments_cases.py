"""Shared pieces of the witness-commitment tests (bzh_commitments_plan, bzh_commitments_batch_device): the state of an oracle
proof at the theta / beta / gamma boundary, cut from helpers.vanishing_cases.capture's State (the oracle is not instrumented
again), and the model: a direct integer implementation of halo2_oracle.create_proof's instance, advice and lookup phases
(oracle/halo2_oracle.py:328-362).  Whenever the operands are the captured ones the model is asserted against what the oracle
computed.  Call inside helpers.real_parity's accelerated_oracle."""
import random

import numpy as np

import halo2_oracle as H
import pasta as O
import sample_circuit as S
from helpers import products_cases as G
from helpers import vanishing_cases as V

CV, F = V.CV, V.F
P = F.p
OUT = ("advice", "instance", "lookup_compressed", "lookup_permuted", "advice_polys", "instance_polys", "lookup_polys", "advice_blinds",
       "lookup_blinds", "theta", "beta", "gamma")


def plan(cs):
    """what bzh_commitments_plan must say for this constraint system"""
    bf, na, ni, nl = cs.blinding_factors, cs.num_advice, cs.num_instance, len(cs.lookups)
    return (cs.n, cs.usable_rows, bf, na, ni, nl, na * (bf + 1) + na + nl * (2 * (bf + 1) + 2), 32 * (na + 2 * nl))


class Boundary:
    """one proof at the head of create_proof: prefix_ops (common_scalar(vk_repr) alone) / prefix_proof (empty), the witness
    (advice, instance: the caller's columns), the phase's draws as bytes (rng) and integers (draws), and the State it was cut
    from (v)"""


def boundary(keys, st):
    b = Boundary()
    b.v = st
    assert st.prefix_ops[0] == ("common_scalar", keys.vk_repr)
    b.prefix_ops, b.prefix_proof = st.prefix_ops[:1], b""
    nd = plan(keys.cs)[6]
    b.rng = st.rbytes[:64 * nd]
    b.draws = [O.from_u512(b.rng[64 * i:64 * (i + 1)], F) for i in range(nd)]
    b.advice, b.instance = st.advice, st.instance
    return b


def fold(terms, ch):
    acc = 0
    for t in terms:
        acc = (acc * ch + t) % P
    return acc


def model(keys, operands, advice=None, instance=None, draws=None):
    """what the leaf must write and return for one proof: a dict with 'bytes' (the proof bytes it appends), 'after' (the next
    squeeze) and the outputs by the names of OUT -- columns as lists of integer lists, lookup_* as [lookup][2] columns.  advice /
    instance / draws: others than the Boundary's own; with its own the result is checked against the oracle's values"""
    cs, dom = keys.cs, keys.dom
    n, bf, usable = cs.n, cs.blinding_factors, cs.usable_rows
    captured = advice is None and instance is None and draws is None
    advice = operands.advice if advice is None else advice
    instance = operands.instance if instance is None else instance
    rnd = iter(operands.draws if draws is None else draws)
    T = V.replay(operands.prefix_ops)
    inst = [[v % P for v in c] + [0] * (n - len(c)) for c in instance]
    inst_polys = [dom.lagrange_to_coeff(c) for c in inst]
    for poly in inst_polys:
        T.common_point(CV, keys.commit(poly, 1))
    adv = [([v % P for v in c] + [0] * n)[:n] for c in advice]
    for col in adv:
        for r in range(usable, n):
            col[r] = next(rnd)
    adv_blinds = [next(rnd) for _ in adv]
    adv_polys = [dom.lagrange_to_coeff(c) for c in adv]
    for poly, bl in zip(adv_polys, adv_blinds):
        T.write_point(CV, keys.commit(poly, bl))
    theta = T.squeeze_challenge()
    lag = {"advice": adv, "fixed": keys.fixed, "instance": inst}
    comp, perm, polys, blinds = [], [], [], []
    for ins, tabs in cs.lookups:
        side = lambda es: [fold([H.expr_eval(e, lambda t, c, r, row=row: lag[t][c][(row + r) % n], P) for e in es], theta)  # noqa: E731
                           for row in range(n)]
        a_c, s_c = side(ins), side(tabs)
        a_p, s_p = O.permute_expression_pair(a_c, s_c, usable, F)
        a_p = list(a_p) + [next(rnd) for _ in range(bf + 1)]
        s_p = list(s_p) + [next(rnd) for _ in range(bf + 1)]
        bl = [next(rnd), next(rnd)]
        pp = [dom.lagrange_to_coeff(a_p), dom.lagrange_to_coeff(s_p)]
        T.write_point(CV, keys.commit(pp[0], bl[0]))
        T.write_point(CV, keys.commit(pp[1], bl[1]))
        comp.append([a_c, s_c]), perm.append([a_p, s_p]), polys.append(pp), blinds.append(bl)
    beta = T.squeeze_challenge()
    gamma = T.squeeze_challenge()
    m = {"bytes": bytes(T.proof[len(operands.prefix_proof):]), "after": T.squeeze_challenge(), "advice": adv, "instance": inst,
         "lookup_compressed": comp, "lookup_permuted": perm, "advice_polys": adv_polys, "instance_polys": inst_polys, "lookup_polys": polys,
         "advice_blinds": adv_blinds, "lookup_blinds": blinds, "theta": theta, "beta": beta, "gamma": gamma}
    if captured:
        st = operands.v
        assert (theta, beta, gamma) == (st.theta, st.beta, st.gamma)
        assert [list(c) for c in adv_polys] == [list(c) for c in st.adv_polys] and [list(c) for c in inst_polys] == [list(c) for c in st.inst_polys]
        for l, d in enumerate(st.lk):
            assert comp[l] == [list(d["a_c"]), list(d["s_c"])] and perm[l] == [list(d["a"]), list(d["s"])]
            assert polys[l] == [list(d["a_poly"]), list(d["s_poly"])] and blinds[l] == [d["a_blind"], d["s_blind"]]
        assert m["bytes"] == st.prefix_proof[:len(m["bytes"])] and len(m["bytes"]) == plan(cs)[7]
    return m


def flat(m, name):
    """one output of the model as a flat integer list in the leaf's layout"""
    v = m[name]
    if name in ("theta", "beta", "gamma"):
        return [v]
    if name in ("advice_blinds",):
        return list(v)
    if name == "lookup_blinds":
        return [x for pair in v for x in pair]
    if name.startswith("lookup_"):
        return [x for pair in v for col in pair for x in col]
    return [x for col in v for x in col]


_CASES = {}


def case(k, with_lookup, degree, B):
    """helpers.products_cases.case cut at the head: (cs, keys, circuit, (g, w, u), [Boundary], [whole proofs], [model on the
    captured operands])"""
    key = (k, with_lookup, degree, B)
    if key not in _CASES:
        cs, keys, circ, gwu, gbounds, proofs, _ = G.case(k, with_lookup, degree, B)
        bounds = [boundary(keys, g.v) for g in gbounds]
        _CASES[key] = (cs, keys, circ, gwu, bounds, proofs, [model(keys, b) for b in bounds])
    return _CASES[key]


def two_column_case(k=5, B=2):
    """the sample circuit with its lookup replaced by ([3 * A(0), A(1) at rotation 1], [Fx(2), Fx(3)]): two expressions a side,
    so theta enters the compressed columns, and a rotation that reads advice 1's first blinding row from the last usable row.
    The table (fixed 2, 3) lists every pair the B witnesses look up, that row's pair with the drawn value included: the draws
    are the test's own bytes, so they are known before the key is built.  Same tuple as case()."""
    key = ("two", k, B)
    if key not in _CASES:
        from bzh2 import circuit_data as Pd
        built = [S.build(k=k, seed=1300 + 7 * b, with_lookup=True) for b in range(B)]
        cs0, fixed, copies = built[0][:3]
        A = lambda c, r=0: ("advice", c, r)   # noqa: E731
        Fx = lambda c: ("fixed", c, 0)        # noqa: E731
        lookups = [([("scale", A(0), 3), A(1, 1)], [Fx(2), Fx(3)])]
        cs = H.ConstraintSystem(cs0.k, cs0.num_advice, cs0.num_fixed, cs0.num_instance, cs0.gates, cs0.perm_columns, lookups)
        n, usable, bf = cs.n, cs.usable_rows, cs.blinding_factors
        assert (usable, bf) == (cs0.usable_rows, cs0.blinding_factors)
        rng = random.Random(4200 + k)
        g = [CV.random_point(rng) for _ in range(n)]
        w, u = CV.random_point(rng), CV.random_point(rng)
        rbytes = [bytes(rng.getrandbits(8) for _ in range(64 * V.draws_per_proof(cs))) for _ in range(B)]
        pairs = []
        for b in range(B):
            adv = built[b][3]
            first_blind = O.from_u512(rbytes[b][64 * (bf + 1):64 * (bf + 2)], F)      # advice 1, row `usable`: draw 1 * (bf + 1) + 0
            a1 = ([v % P for v in adv[1]] + [0] * n)[:usable] + [first_blind]
            for r in range(usable):
                pr = (3 * adv[0][r] % P if r < len(adv[0]) else 0, a1[r + 1])
                if pr not in pairs:
                    pairs.append(pr)
        assert len(pairs) <= usable and len(pairs) > 3
        fixed = [list(c) for c in fixed]
        for r in range(n):
            fixed[2][r], fixed[3][r] = pairs[r % len(pairs)] if r < usable else (0, 0)
        keys = H.Keys(cs, H.Domain(cs, F), CV, g, w, u, fixed, copies)
        circ = Pd.Circuit(cs.k, cs.num_advice, cs.num_fixed, cs.num_instance, cs.gates, cs.perm_columns, cs.lookups, fixed, copies)
        bounds, proofs = [], []
        for b in range(B):
            st, proof = V.capture(keys, built[b][3], built[b][4], rbytes[b])
            assert H.verify_proof(keys, built[b][4], proof, O.Blake2bTranscript(F))
            bounds.append(boundary(keys, st)), proofs.append(proof)
        _CASES[key] = (cs, keys, circ, (g, w, u), bounds, proofs, [model(keys, b) for b in bounds])
    return _CASES[key]


def no_instance_case(k=4, B=2):
    """the sample circuit without its lookup and without its instance column (the permutation keeps the three advice columns, the
    copy into the instance is dropped): ni = 0 and nl = 0, so the leaf's instance and lookup members are all NULL.  Same tuple as
    case()."""
    key = ("noinst", k, B)
    if key not in _CASES:
        from bzh2 import circuit_data as Pd
        built = [S.build(k=k, seed=1700 + 7 * b, with_lookup=False) for b in range(B)]
        cs0, fixed, copies = built[0][:3]
        copies = [c for c in copies if c[0][0] < 3 and c[1][0] < 3]
        cs = H.ConstraintSystem(cs0.k, cs0.num_advice, cs0.num_fixed, 0, cs0.gates, list(cs0.perm_columns[:3]), [])
        rng = random.Random(4300 + k)
        g = [CV.random_point(rng) for _ in range(cs.n)]
        w, u = CV.random_point(rng), CV.random_point(rng)
        keys = H.Keys(cs, H.Domain(cs, F), CV, g, w, u, fixed, copies)
        circ = Pd.Circuit(cs.k, cs.num_advice, cs.num_fixed, cs.num_instance, cs.gates, cs.perm_columns, cs.lookups, fixed, copies)
        bounds, proofs = [], []
        for b in range(B):
            rbytes = bytes(rng.getrandbits(8) for _ in range(64 * V.draws_per_proof(cs)))
            st, proof = V.capture(keys, built[b][3], [], rbytes)
            assert H.verify_proof(keys, [], proof, O.Blake2bTranscript(F))
            bounds.append(boundary(keys, st)), proofs.append(proof)
        _CASES[key] = (cs, keys, circ, (g, w, u), bounds, proofs, [model(keys, b) for b in bounds])
    return _CASES[key]


def operand_arrays(bounds, n, conv=lambda x: x, advice=None):
    """the leaf's operands as uint64 limb arrays: advice (B, na, n, 4) -- rows the witness does not fill are 0 -- and instances
    (B, ni, rows, 4); advice: other per-proof columns than the bounds' own"""
    cols = [b.advice for b in bounds] if advice is None else advice
    adv = np.stack([np.stack([V.lim((list(c) + [0] * n)[:n], conv) for c in w]) for w in cols])
    if not bounds[0].instance:
        return adv, np.zeros((len(bounds), 0, 0, 4), dtype=np.uint64)
    inst = np.stack([np.stack([V.lim(list(c), conv) for c in b.instance]) for b in bounds])
    return adv, inst
