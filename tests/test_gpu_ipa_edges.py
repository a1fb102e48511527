"""The inner-product opening (csrc/ipa.hip) and its generator collapse (msm_collapse_table, csrc/msm.hip) on adversarial reference
strings and operands, byte for byte against the oracle's restatement of upstream's collapsing prover (oracle/pasta.py: ipa_open,
per proof), under every setting of BZH_IPA_COLLAPSE / BZH_IPA_TAIL_C / BZH_ACC_SATURATED that changes the path taken.  The cases
are tests/helpers/ipa_edge_cases.py's; one child process per setting (the variables are read once per process), one after the
other, each under its own timeout; after a child that exits abnormally no further child is started.

Collapse witness: the bucket additions ctx.msm_additions() reports for a case (non-zero window digits of the MSMs plus the
collapse's own mixed additions).  Without a collapse every round is an MSM over the n original points; with one, the rounds from
j on run over n >> j points and the collapse adds its items: the count differs.  WHETHER a case collapses under a setting is
stated below by hand (COLLAPSES), not derived from the library's rule; the test asserts it against the same case's count under
BZH_IPA_COLLAPSE=0, and against the launches ctx.timings() counts under the accumulate timer (one more with a collapse)."""
import functools
import json
import os
import subprocess
import sys
import time

import pytest

import accel
import pasta as O
from helpers import ipa_edge_cases as E
from helpers import ipa_open_device_cases as K
from helpers.real_parity import THREADS

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = os.path.join(ROOT, "tests", "helpers", "ipa_edge_cases.py")
CHILD_TIMEOUT = 240

# Does a case on a window table collapse?  By setting and k, written down by hand.  A forced round j is taken when rounds remain
# after it (j <= k - 2) and its item lists fit the LDS cap (they do at every width here: 2^j <= 16, nwin <= 64); k = 2 has no
# such round; the default collapses from B = 8, k = 9 on.  The case without a window table never collapses.
COLLAPSES = {
    "default": {2: False, 3: False, 6: False, 9: True},
    "collapse0": {2: False, 3: False, 6: False, 9: False, 10: False},
    "collapse1": {2: False, 3: True, 6: True},
    "collapse2_tail4": {2: False, 3: False, 6: True},
    "collapse1_tail13": {3: True},             # k - 2 at k = 3: m = 4 folded generators
    "collapse4_tail13": {6: True},             # k - 2 at k = 6: m = 4 folded generators
    "collapse2_tail7_saturated": {2: False, 3: False, 6: True},
    "collapse3": {10: True},
}
NO_TABLE = "vesta_k3_notable_periodic"

_children = {}
_abnormal = []


def child(setting):
    """the child's lines by case name; run once per session"""
    if setting in _children:
        return _children[setting]
    if _abnormal:
        pytest.fail("no further child after %s exited abnormally" % _abnormal[0])
    env = dict(os.environ)
    for name in E.ENV_NAMES:
        env.pop(name, None)
    env.update(E.SETTINGS[setting][0])
    t0 = time.perf_counter()
    try:
        out = subprocess.run([sys.executable, CHILD, setting], env=env, capture_output=True, text=True, timeout=CHILD_TIMEOUT)
    except subprocess.TimeoutExpired:
        _abnormal.append(setting)
        raise
    if out.returncode != 0:
        _abnormal.append(setting)
        pytest.fail("child %s: exit %d\n%s\n%s" % (setting, out.returncode, out.stdout[-1000:], out.stderr[-2000:]))
    print("child %s: %.2f s" % (setting, time.perf_counter() - t0))
    lines = [json.loads(ln) for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert [ln["case"] for ln in lines] == E.SETTINGS[setting][1]
    _children[setting] = {ln["case"]: ln for ln in lines}
    return _children[setting]


@functools.lru_cache(maxsize=None)
def reference(name):
    t0 = time.perf_counter()
    with accel.accelerated(THREADS):
        ref = E.reference(name)
    print("reference %s: %.2f s" % (name, time.perf_counter() - t0))
    return ref


@pytest.mark.parametrize("setting", list(E.SETTINGS))
def test_openings_equal_the_oracle_and_collapse_exactly_where_stated(setting):
    base = child("collapse0")
    got = child(setting)
    for name in E.SETTINGS[setting][1]:
        case, line, ref = E.BY_NAME[name], got[name], reference(name)
        assert [int(v, 16) for v in line["v"]] == [r[0] for r in ref], name
        assert [bytes.fromhex(p) for p in line["proofs"]] == [r[1] for r in ref], name
        expected = False if name == NO_TABLE else COLLAPSES[setting][case.k]
        print("%s %s: additions %d (COLLAPSE=0: %d), launches %s, collapse expected: %s"
              % (setting, name, line["additions"], base[name]["additions"], line["launches"], expected))
        assert line["additions"] > 0
        accumulates, accumulates0 = line["launches"]["msm_accumulate"], base[name]["launches"]["msm_accumulate"]
        if expected:
            assert line["additions"] != base[name]["additions"], "%s under %s did not collapse" % (name, setting)
            assert accumulates == accumulates0 + 1       # k_collapse_generators runs under the accumulate timer, once
        else:
            assert line["additions"] == base[name]["additions"], "%s under %s collapsed" % (name, setting)
            assert accumulates == accumulates0


def test_both_verifiers_accept_three_edge_proofs_and_reject_another_value(gpu_ctx):
    """the zero polynomial, a uniform one and x3 = 0, all on a reference string with two dead columns: bzh_ipa_verify and the
    oracle's verifier accept the proof the oracle's prover wrote (the bytes the library writes, by the test above), and reject v + 1"""
    name = "vesta_k3_c5_dead_verify"
    case = E.BY_NAME[name]
    assert [r[0] for r in case.recipes] == ["zero", "uniform", "uniform"] and case.recipes[2][1] == "zero" and case.dead
    cv = O.CURVE_BY_ID[case.cid]
    p = cv.scalar.p
    g, w, u = E.srs(case)
    polys, blinds, x3s, _ = E.operands(name)
    assert not any(polys[0]) and x3s[2] == 0
    ref = reference(name)
    hb = E.upload(gpu_ctx, case)
    try:
        for b in range(case.B):
            v, proof = ref[b]
            opening = proof[32:]       # after the primed point
            P = cv.add(cv.msm_naive(polys[b], g), cv.mul(blinds[b], w))
            for value, accept in ((v, True), ((v + 1) % p, False)):
                assert O.ipa_verify(cv, g, w, u, P, x3s[b], value, opening, K.primed_oracle(case.cid, b)) is accept
                trs = K.primed(case.cid, case.B)
                try:
                    assert gpu_ctx.ipa_verify(hb, P, x3s[b], value, opening, trs[b], [g[0], u, w]) is accept
                finally:
                    for t in trs:
                        t.close()
    finally:
        hb.free()
