"""The verifying key on the device: keygen_vk (bzh_vk_create), pk.get_vk() (bzh_vk_from_pk) and bzh_verify_batch_vk against
bzh_verify_batch, element for element, on valid and damaged proofs, with the instance columns committed in the Lagrange basis
(the prefix MSM) and in the coefficient basis.  Proofs come from the library's own prover (bzh_prove_batch); the bytes of a key
are compared with the ones tests/helpers/vk_cases.py builds in Python from the oracle's commitments."""
import os
import subprocess
import sys
import threading

import coracle as C
import numpy as np
import pytest

from helpers import real_parity as R
from helpers import vk_cases as V

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _Srs:
    """explicit tables for the synthetic circuits: (g | u | w) and (g_lagrange | u | w), both with window tables"""

    def __init__(self, ctx, k):
        import bzh2
        from bzh2 import params as Pm
        g, w, u = V.srs(k)
        self.g, self.w, self.u = g, w, u
        garr = C.points_to_array(g)
        uw = C.points_to_array([u, w])
        self.bases = ctx.upload_bases(bzh2.CURVE_VESTA, np.concatenate([garr, uw])).precompute(0)
        self.bases_lagrange = ctx.upload_bases(bzh2.CURVE_VESTA, np.concatenate([Pm.group_ifft(ctx, garr), uw])).precompute(0)
        self.g0_u_w = np.ascontiguousarray(np.stack([garr[0], uw[0], uw[1]]))

    def close(self):
        self.bases.free()
        self.bases_lagrange.free()


@pytest.fixture(scope="module")
def srs5(gpu_ctx):
    s = _Srs(gpu_ctx, V.K)
    yield s
    s.close()


def _prove(ctx, srs, num_instance, count, instance_rows=None):
    """(pk, blob, instances, proofs) for `count` witnesses of vk_cases.circuit(num_instance=...)"""
    import bzh2
    from bzh2 import circuit_data as P, native as N
    cases = [V.circuit(V.K, 70 + b, num_instance) for b in range(count)]
    circ = cases[0][5]
    pk = N.NativeProvingKey(ctx, circ, bzh2.CURVE_VESTA, srs.g, srs.w, srs.u)
    n = 1 << V.K
    adv = np.stack([np.stack([C.ints_to_array(list(col) + [0] * (n - len(col))) for col in cse[3]]) for cse in cases])
    insts = [[list(col) for col in cse[4]] for cse in cases]
    if instance_rows is not None:    # zero rows after the cells the circuit constrains
        insts = [[col + [0] * (instance_rows - len(col)) for col in cols] for cols in insts]
    rbs = [R.rng_stream("vk-%d-%d" % (num_instance, b), pk.rng_bytes) for b in range(count)]
    proofs = pk.prove_batch(adv, insts, rbs)
    return pk, P.serialize_circuit(circ, V.O.FP.p), insts, proofs


def _damaged(info, insts, proofs):
    """the issue's list over three valid proofs: (instances, proofs) pairs, each a batch of 3"""
    cs, _, _, _, _, circ = V.circuit()
    nl, nsets, npieces = len(cs.lookups), -(-len(cs.perm_columns) // circ.chunk_len), circ.degree - 1
    evals_at = 32 * (cs.num_advice + 3 * nl + nsets + 1 + npieces)
    ln = len(proofs[1])
    flip = lambda pr, at: pr[:at] + bytes([pr[at] ^ 0x10]) + pr[at + 1:]
    batches = [("three valid proofs", insts, proofs)]
    for name, at in (("an advice commitment", 37), ("an evaluation", evals_at + 32 * 2 + 5), ("an L_j", ln - 64 - 64 * V.K + 64 + 3),
                     ("the final scalars", ln - 40)):
        batches.append(("a flipped byte inside " + name, insts, [proofs[0], flip(proofs[1], at), proofs[2]]))
    batches.append(("truncated by 1 and by 32 bytes", insts, [proofs[0][:-1], proofs[1], proofs[2][:-32]]))
    batches.append(("instances swapped with the neighbour's", [insts[1], insts[0], insts[2]], proofs))
    batches.append(("an empty proof", insts, [proofs[0], b"", proofs[2]]))
    return batches


def test_synthetic_circuit_bytes_and_results(gpu_ctx, srs5):
    from bzh2 import native as N
    pk, blob, insts, proofs = _prove(gpu_ctx, srs5, 1, 3)
    try:
        vk_c = N.NativeVerifyingKey.create(gpu_ctx, srs5.bases, blob)
        vk_p = N.NativeVerifyingKey.from_pk(pk)
        # keygen_vk, pk.get_vk() and the Python-built bytes with the ORACLE's commitments are the same bytes
        assert vk_c.to_bytes() == vk_p.to_bytes() == V.golden()
        assert vk_c.info()["max_proof_bytes"] == pk.max_proof_bytes and all(len(p) <= pk.max_proof_bytes for p in proofs)
        vk = N.NativeVerifyingKey.from_bytes(vk_c.to_bytes())
        seen = []
        for name, ii, pp in _damaged(vk.info(), insts, proofs):
            want = pk.verify_batch(ii, pp)
            seen.append(want)
            for lagrange in (True, False):
                got = vk.verify_batch(gpu_ctx, srs5, ii, pp, lagrange=lagrange, g0_u_w=srs5.g0_u_w)
                assert got == want, (name, lagrange, got, want)
        assert seen[0] == [True] * 3 and all(s != [True] * 3 for s in seen[1:]) and all(s[0] for s in seen[:-3])
        for k_ in (vk, vk_c, vk_p):
            k_.close()
    finally:
        pk.close()


_CHILD = r"""
import sys
sys.path[:0] = sys.argv[2:]
import bzh2
from bzh2 import native as N
key = N.NativeVerifyingKey.from_bytes(open(sys.argv[1], "rb").read())
open(sys.argv[1] + ".back", "wb").write(key.to_bytes())
key.close()
"""


def test_a_vk_that_never_saw_a_pk(gpu_ctx, srs5, tmp_path):
    from bzh2 import native as N
    pk, blob, insts, proofs = _prove(gpu_ctx, srs5, 1, 3)
    bad = [proofs[0], proofs[1][:100] + b"\x01" + proofs[1][101:], proofs[2]]
    recorded = [pk.verify_batch(insts, proofs), pk.verify_batch(insts, bad)]
    path = tmp_path / "key.bzv1"
    vk0 = N.NativeVerifyingKey.from_pk(pk)
    path.write_bytes(vk0.to_bytes())
    vk0.close()
    pk.close()
    # a fresh process reads the key and writes it again: no ctx, no device, no keygen there
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    out = subprocess.run([sys.executable, "-c", _CHILD, str(path), os.path.join(ROOT, "battlezips-halo2_amd")], capture_output=True, text=True,
                         timeout=120, env=env)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    vk = N.NativeVerifyingKey.from_bytes((tmp_path / "key.bzv1.back").read_bytes())
    assert vk.device_bytes() == (0, 0)
    assert [vk.verify_batch(gpu_ctx, srs5, insts, proofs, g0_u_w=srs5.g0_u_w), vk.verify_batch(gpu_ctx, srs5, insts, bad, g0_u_w=srs5.g0_u_w)] == recorded
    assert recorded[0] == [True] * 3 and recorded[1] == [True, False, True]
    assert vk.device_bytes()[0] == 0 and vk.device_bytes()[1] > 0     # the workspace of this (key, ctx) pair, not the key's
    vk.close()


@pytest.mark.parametrize("num_instance", [0, 1, 2])
def test_instance_shapes(gpu_ctx, srs5, num_instance):
    from bzh2 import native as N
    usable = V.circuit(V.K, 70, num_instance)[5].usable_rows
    for rows in (0, 1, 4, usable):       # (a column keeps the cells the circuit constrains: rows below that length leave it as it is)
        pk, blob, insts, proofs = _prove(gpu_ctx, srs5, num_instance, 2, rows)
        try:
            vk = N.NativeVerifyingKey.from_pk(pk)
            swapped = [insts[1], insts[0]]
            nothing = [[[] for _ in cols] for cols in insts]       # instance_rows = 0 whatever the circuit has
            for ii in (insts, swapped, nothing):
                want = pk.verify_batch(ii, proofs)
                lag = vk.verify_batch(gpu_ctx, srs5, ii, proofs, lagrange=True, g0_u_w=srs5.g0_u_w)
                coeff = vk.verify_batch(gpu_ctx, srs5, ii, proofs, lagrange=False, g0_u_w=srs5.g0_u_w)
                assert lag == coeff == want, (num_instance, rows, lag, coeff, want)
            assert pk.verify_batch(insts, proofs) == [True, True], (num_instance, rows)
            vk.close()
        finally:
            pk.close()


def test_the_references_shot_circuit_and_the_digest(gpu_ctx):
    import bzh2
    from bzh2 import circuits as Cm, native as N, params as Pm
    lay = Cm.CircuitLayout(Cm.SHOT, 11)
    prm = Pm.Params(gpu_ctx, 11)
    keys = []
    try:
        circuits = R.shot_circuits(Cm, 911, 2)
        adv, insts = lay.synthesize(circuits)
        seeds = [R.rng_stream("vk-shot-%d" % b, 32) for b in range(2)]
        pk = N.NativeProvingKey(gpu_ctx, lay.blob(), bzh2.CURVE_VESTA, params=prm)
        keys.append(pk)
        proofs = pk.prove_batch(adv, insts, None, seeds=seeds)
        flipped = [insts[0], [list(c) for c in insts[1]]]
        flipped[1][0][3] = 1 - int(flipped[1][0][3])                     # `hit` of the second proof
        vk = N.NativeVerifyingKey.create(gpu_ctx, prm, lay.blob())
        keys.append(vk)
        assert vk.to_bytes() == N.NativeVerifyingKey.from_pk(pk).to_bytes() and vk.vk_repr() == (V.PLACEHOLDER, True)
        for ii in (insts, flipped):
            want = pk.verify_batch(ii, proofs)
            assert vk.verify_batch(gpu_ctx, prm, ii, proofs) == want == [True, ii is insts]
            assert vk.verify_batch(gpu_ctx, prm, ii, proofs, lagrange=False) == want
        # a key with a real digest carries it; proofs made under the placeholder are rejected by it, and the other way round
        lay.set_vk_repr(V.OTHER_REPR)
        pk2 = N.NativeProvingKey(gpu_ctx, lay.blob(), bzh2.CURVE_VESTA, params=prm)
        keys.append(pk2)
        vk2 = N.NativeVerifyingKey.create(gpu_ctx, prm, lay.blob())
        keys.append(vk2)
        assert vk2.vk_repr() == (V.OTHER_REPR, False) and N.NativeVerifyingKey.from_bytes(vk2.to_bytes()).vk_repr() == (V.OTHER_REPR, False)
        proofs2 = pk2.prove_batch(adv, insts, None, seeds=seeds)
        assert vk2.verify_batch(gpu_ctx, prm, insts, proofs2) == [True, True] and vk.verify_batch(gpu_ctx, prm, insts, proofs2) == [False, False]
        assert vk2.verify_batch(gpu_ctx, prm, insts, proofs) == [False, False]
    finally:
        for k_ in keys:
            k_.close()
        prm.close()
        lay.close()


def test_wrong_srs(gpu_ctx, srs5):
    import bzh2
    from bzh2 import native as N
    pk, blob, insts, proofs = _prove(gpu_ctx, srs5, 1, 2)
    srs6 = _Srs(gpu_ctx, 6)
    short = gpu_ctx.upload_bases(bzh2.CURVE_VESTA, np.concatenate([C.points_to_array(srs5.g[:-1]), C.points_to_array([srs5.u, srs5.w])])).precompute(0)
    try:
        vk = N.NativeVerifyingKey.from_pk(pk)
        for args in ((srs5, srs6.g0_u_w),        # G_0, U, W of another k: refused, as bzh_verify_batch refuses them
                     (short, srs5.g0_u_w),       # an srs shorter than n + 2
                     (srs6, srs6.g0_u_w)):       # an srs of another k
            with pytest.raises(bzh2.BzhError) as e:
                vk.verify_batch(gpu_ctx, args[0], insts, proofs, lagrange=False, g0_u_w=args[1])
            assert e.value.status == bzh2.E_ARG
        with pytest.raises(bzh2.BzhError) as e:
            pk._g0_u_w = srs6.g0_u_w
            pk.verify_batch(insts, proofs)
        assert e.value.status == bzh2.E_ARG
        # proofs of a k = 6 key against the k = 5 vk: rejected, not an error
        cases6 = V.circuit(6, 70)
        pk6 = N.NativeProvingKey(gpu_ctx, cases6[5], bzh2.CURVE_VESTA, srs6.g, srs6.w, srs6.u)
        adv6 = np.stack([np.stack([C.ints_to_array(list(col) + [0] * (64 - len(col))) for col in cases6[3]])])
        proofs6 = pk6.prove_batch(adv6, [cases6[4]], [R.rng_stream("vk-k6", pk6.rng_bytes)])
        assert pk6.verify_batch([cases6[4]], proofs6) == [True]
        pk6.close()
        assert vk.verify_batch(gpu_ctx, srs5, [cases6[4]] * 2, proofs6 * 2, g0_u_w=srs5.g0_u_w) == [False, False]
        vk.close()
    finally:
        pk.close()
        short.free()
        srs6.close()


def test_two_threads_share_one_vk_and_free_waits(gpu_ctx, srs5):
    """Two host threads verify on ONE bzh_vk through two ctxs and get the single-thread results; then bzh_vk_free keeps being
    asked for while one long call runs on another ctx: every answer during the call is a refusal (tests/test_gpu_shared_key.py
    does the same for bzh_pk_free)."""
    import time
    import bzh2
    from bzh2 import native as N
    pk, blob, insts, proofs = _prove(gpu_ctx, srs5, 1, 3)
    bad = [proofs[0], proofs[1][:-1], proofs[2]]
    want = [pk.verify_batch(insts, proofs), pk.verify_batch(insts, bad)]
    vk = N.NativeVerifyingKey.from_pk(pk)
    pk.close()
    ctxs = [bzh2.Context(0) for _ in range(2)]
    try:
        got, errors = [None, None], []

        def work(wi):
            try:
                for _ in range(3):
                    got[wi] = [vk.verify_batch(ctxs[wi], srs5, insts, proofs, g0_u_w=srs5.g0_u_w),
                               vk.verify_batch(ctxs[wi], srs5, insts, bad, lagrange=wi == 0, g0_u_w=srs5.g0_u_w)]
            except BaseException as e:  # noqa: BLE001
                errors.append(e)
        ths = [threading.Thread(target=work, args=(wi,)) for wi in range(2)]
        for t in ths:
            t.start()
        for t in ths:
            t.join()
        assert not errors, errors
        assert got == [want, want] and want == [[True] * 3, [True, False, True]]
        # one long call (768 proofs) on ctxs[0]; the main thread asks for the key to be freed until it is over
        state = {"running": False, "done": False, "res": None, "error": None}

        def long_call():
            try:
                state["running"] = True
                state["res"] = vk.verify_batch(ctxs[0], srs5, insts * 256, proofs * 256, g0_u_w=srs5.g0_u_w)
            except BaseException as e:  # noqa: BLE001
                state["error"] = e
            finally:
                state["done"] = True
        th = threading.Thread(target=long_call)
        th.start()
        while not state["running"]:
            time.sleep(0)
        time.sleep(0.002)      # let the call take the key
        refused = 0
        while not state["done"] and vk.handle is not None:
            try:
                vk.close()
                th.join(timeout=1.0)     # allowed only once the call has left the library (its thread ends right after)
                if th.is_alive():
                    state["error"] = AssertionError("bzh_vk_free went through while a verification was running")
            except bzh2.BzhError as e:
                assert e.status == bzh2.E_ARG
                refused += 1
        th.join()
        assert state["error"] is None, state["error"]
        assert refused >= 1 and state["res"] == [True] * 768
    finally:
        for c in ctxs:
            c.close()
        vk.close()


def test_context_churn_on_one_key(gpu_ctx, srs5):
    """Eight contexts, one after the other, verify the same three proofs (one corrupted) on ONE bzh_vk and ONE bzh_pk and are
    closed again.  A key files its per-ctx workspace under the ctx's serial number, so a new context never inherits the workspace
    of a destroyed one whose address it got back: the results are the first iteration's every time, the verifying key owns no
    device memory of its own throughout, and both keys can be closed once the contexts are gone."""
    import bzh2
    from bzh2 import native as N
    pk, blob, insts, proofs = _prove(gpu_ctx, srs5, 1, 3)
    bad = [proofs[0], proofs[1][:100] + b"\x01" + proofs[1][101:], proofs[2]]
    vk = N.NativeVerifyingKey.from_pk(pk)
    try:
        first = None
        for it in range(8):
            ctx = bzh2.Context(0)
            try:
                got = [vk.verify_batch(ctx, srs5, insts, bad, g0_u_w=srs5.g0_u_w), pk.verify_batch(insts, bad, ctx=ctx)]
            finally:
                ctx.close()
            if first is None:
                first = got
            assert got == first == [[True, False, True]] * 2, (it, got)
            assert vk.device_bytes()[0] == 0 and vk.device_bytes()[1] > 0, it
    finally:
        vk.close()
        pk.close()
    assert vk.handle is None and pk.handle is None


def test_no_key_columns_on_the_device(gpu_ctx, srs5):
    import bzh2
    from bzh2 import native as N
    circ = V.circuit()[5]
    blob = N.serialize_circuit(circ, V.O.FP.p)
    vk = N.NativeVerifyingKey.create(gpu_ctx, srs5.bases, blob)
    gpu_ctx.sync()
    assert vk.device_bytes() == (0, 0)
    pk = N.NativeProvingKey(gpu_ctx, circ, bzh2.CURVE_VESTA, srs5.g, srs5.w, srs5.u)
    n, en = 1 << V.K, 1 << circ.extended_k
    # at least the fixed and permutation columns in Lagrange, coefficient and extended-coset form
    assert pk.device_bytes()[0] >= 32 * ((circ.num_fixed + len(circ.perm_columns)) * (2 * n + en))
    pk.close()
    vk.close()
