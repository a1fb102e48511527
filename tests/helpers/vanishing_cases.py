"""Shared pieces of the vanishing-argument tests (bzh_vanishing_plan, bzh_vanishing_batch_device): the model.  It runs
halo2_oracle.create_proof on sample_circuit.build(...) and takes the prover's state at the vanishing boundary -- the coefficient
polynomials of every column, grand product and lookup, theta, beta, gamma, the draws consumed so far and every transcript
operation so far -- by substituting halo2_oracle.quotient_evals for the duration of the call (restored in a `finally`, the way
oracle/accel.py substitutes that function) and by handing create_proof a transcript that keeps a log and a draw iterator that
counts.  The expected values are the oracle's own: quotient_evals -> extended_to_coeff for h, Keys.commit for the points,
pasta.Blake2bTranscript for y and for the squeeze that follows.  Call inside accel.accelerated(...) (helpers.real_parity's
accelerated_oracle): the oracle's transforms and sums then run in the C oracle."""
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
import sample_circuit as S  # noqa: E402

CV, F = O.VESTA, O.FP


class LoggingTranscript(O.Blake2bTranscript):
    """pasta.Blake2bTranscript that also lists its operations: ('common_scalar', s), ('common_point', pt), ('write_point', pt),
    ('write_scalar', s), ('squeeze', challenge)"""

    def __init__(self, field):
        super().__init__(field)
        self.log = []

    def common_point(self, curve, pt):
        self.log.append(("common_point", pt))
        O.Blake2bTranscript.common_point(self, curve, pt)

    def common_scalar(self, s):
        self.log.append(("common_scalar", s))
        O.Blake2bTranscript.common_scalar(self, s)

    def write_point(self, curve, pt):
        self.log.append(("write_point", pt))
        O.Blake2bTranscript.common_point(self, curve, pt)
        self.proof += curve.compress(pt)

    def write_scalar(self, s):
        self.log.append(("write_scalar", s))
        O.Blake2bTranscript.common_scalar(self, s)
        self.proof += O.to_repr(s)

    def squeeze_challenge(self):
        c = O.Blake2bTranscript.squeeze_challenge(self)
        self.log.append(("squeeze", c))
        return c


class CountingDraws:
    def __init__(self, values):
        self.values, self.used = values, 0

    def __iter__(self):
        return self

    def __next__(self):
        if self.used >= len(self.values):
            raise StopIteration
        self.used += 1
        return self.values[self.used - 1]


class State:
    """one proof at the vanishing boundary"""


def capture(keys, advice, instance, rbytes):
    """create_proof on the oracle with the state at the vanishing boundary taken on the way: (State, the whole proof)"""
    cs, dom = keys.cs, keys.dom
    n, npieces = cs.n, cs.degree - 1
    draws = CountingDraws([O.from_u512(rbytes[64 * i:64 * (i + 1)], F) for i in range(len(rbytes) // 64)])
    T = LoggingTranscript(F)
    st = State()
    inner = H.quotient_evals

    def spy(keys_, cosets, perm, lk, beta, gamma, theta, y):
        st.cosets, st.perm, st.lk = cosets, perm, lk
        st.theta, st.beta, st.gamma, st.y = theta, beta, gamma, y
        st.used, st.nlog, st.proof_len = draws.used, len(T.log) - 2, len(T.proof) - 32   # before the random polynomial's commitment
        return inner(keys_, cosets, perm, lk, beta, gamma, theta, y)

    H.quotient_evals = spy
    try:
        proof = H.create_proof(keys, advice, instance, draws, T)
    finally:
        H.quotient_evals = inner
    assert T.log[st.nlog][0] == "write_point" and T.log[st.nlog + 1] == ("squeeze", st.y)
    st.prefix_ops, st.prefix_proof = T.log[:st.nlog], bytes(T.proof[:st.proof_len])
    st.rbytes, st.advice, st.instance = rbytes, advice, instance
    first = st.used - (n + 1)
    st.rng = rbytes[64 * first:64 * (st.used + npieces)]
    st.random_poly, st.random_blind = draws.values[first:first + n], draws.values[first + n]
    st.h_blinds = draws.values[st.used:st.used + npieces]
    # the coefficient polynomials: of the instance columns from the instance, of the advice columns (whose blinding rows are draws)
    # back from their cosets
    st.inst_polys = [dom.lagrange_to_coeff(list(c) + [0] * (n - len(c))) for c in instance]
    st.adv_polys = [dom.extended_to_coeff(c)[:n] for c in st.cosets["advice"]]
    st.lookup_polys = [[d["a_poly"], d["s_poly"]] for d in st.lk]
    st.z_polys = [d["poly"] for d in st.perm] + [d["z_poly"] for d in st.lk]
    return st, proof


def replay(ops):
    """the oracle transcript after `ops`"""
    T = O.Blake2bTranscript(F)
    for op, v in ops:
        if op == "squeeze":
            assert T.squeeze_challenge() == v
        elif op.endswith("point"):
            getattr(T, op)(CV, v)
        else:
            getattr(T, op)(v)
    return T


def model(keys, st, adv_polys=None):
    """what the leaf must write and return for one proof: (the proof bytes it appends, the next squeeze, h -- en coefficients --,
    the status bit).  adv_polys: other advice polynomials than the captured ones (an unsatisfied witness)"""
    cs, dom = keys.cs, keys.dom
    n, npieces = cs.n, cs.degree - 1
    T = replay(st.prefix_ops)
    T.write_point(CV, keys.commit(st.random_poly, st.random_blind))
    y = T.squeeze_challenge()
    cosets = st.cosets
    if adv_polys is None:
        assert y == st.y
    else:
        cosets = dict(st.cosets, advice=[dom.coeff_to_extended(c) for c in adv_polys])
    h = dom.extended_to_coeff(H.quotient_evals(keys, cosets, st.perm, st.lk, st.beta, st.gamma, st.theta, y))
    for i in range(npieces):
        T.write_point(CV, keys.commit(h[i * n:(i + 1) * n], st.h_blinds[i]))
    return bytes(T.proof[len(st.prefix_proof):]), T.squeeze_challenge(), h, int(any(h[npieces * n:]))


_CASES = {}


def case(k, with_lookup, degree, B):
    """the sample circuit at this shape, B witnesses: (cs, keys, circuit for NativeProvingKey, (g, w, u), [State], [whole proofs])"""
    key = (k, with_lookup, degree, B)
    if key not in _CASES:
        from bzh2 import circuit_data as P
        built = [S.build(k=k, seed=500 + 11 * b + k, with_lookup=with_lookup, degree=degree) for b in range(B)]
        cs, fixed, copies = built[0][:3]
        rng = random.Random(4000 + k)
        g = [CV.random_point(rng) for _ in range(cs.n)]
        w, u = CV.random_point(rng), CV.random_point(rng)
        keys = H.Keys(cs, H.Domain(cs, F), CV, g, w, u, fixed, copies)
        circ = P.Circuit(cs.k, cs.num_advice, cs.num_fixed, cs.num_instance, cs.gates, cs.perm_columns, cs.lookups, fixed, copies, degree=degree)
        ndraws = draws_per_proof(cs)
        states, proofs = [], []
        for b in range(B):
            rbytes = bytes(rng.getrandbits(8) for _ in range(64 * ndraws))
            st, proof = capture(keys, built[b][3], built[b][4], rbytes)
            states.append(st), proofs.append(proof)
        _CASES[key] = (cs, keys, circ, (g, w, u), states, proofs)
    return _CASES[key]


def draws_per_proof(cs):
    """more draws than create_proof takes at these sizes (it takes them in order and leaves the rest)"""
    return 3 * cs.n + 64 * (cs.num_advice + 4 * len(cs.lookups) + len(cs.perm_columns)) + 2 * cs.k + 64


def lim(values, conv=lambda x: x):
    return C.ints_to_array([conv(x) for x in values])


def operand_arrays(states, conv=lambda x: x):
    """the leaf's operands as uint64 limb arrays: advice (B, na, n, 4), instance (B, ni, n, 4), lookups (B, nl, 2, n, 4) or None,
    grand products (B, nz, n, 4)"""
    stack = lambda rows: np.stack([np.stack([lim(c, conv) for c in r]) for r in rows])  # noqa: E731
    adv = stack([s.adv_polys for s in states])
    inst = stack([s.inst_polys for s in states])
    lk = np.stack([np.stack([np.stack([lim(c, conv) for c in pair]) for pair in s.lookup_polys]) for s in states]) if states[0].lookup_polys else None
    z = stack([s.z_polys for s in states])
    return adv, inst, lk, z


def ints(a):
    import bzh2
    a = np.asarray(a)
    if a.ndim == 1:
        return bzh2.limbs_to_int(a)
    return [ints(x) for x in a]
