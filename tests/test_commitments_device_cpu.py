"""The witness commitments on device-resident transcripts (bzh_commitments_plan, bzh_commitments_batch_device) without a device:
the header / exports agreement for the two names, the plan against the oracle's constraint system, the argument refusals that
need no device, the lane bodies (csrc/commitments_scalars.hpp) run lane by lane on the host against values computed here
(tests/helpers/commitments_scalars_check.hip, a stand-alone program under the host's address and undefined-behaviour sanitizers),
and the tests' integer model against the oracle on the two-column lookup case."""
import ctypes
import os
import random
import re
import shutil
import subprocess

import numpy as np
import pytest

import pasta as O
from helpers.real_parity import accelerated_oracle
from test_products_device_cpu import _blobs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("bzh_commitments_plan", "bzh_commitments_batch_device")
E_ARG = -1


def test_header_and_exports_name_the_entry_points():
    import bzh2
    from bzh2 import native as N
    header = open(os.path.join(ROOT, "include", "bzh2.h")).read()
    for name in NAMES:
        assert re.search(r"\bint %s\(" % name, header) and name in bzh2.EXPORTS
        getattr(bzh2.load(), name)
    assert header.index("int bzh_grand_products_batch_device(") < header.index("int bzh_commitments_plan(") < header.index("int bzh_commitments_batch_device(")
    assert "} bzh_commitments_out;" in header
    assert hasattr(bzh2.TranscriptBatch, "commitments") and callable(bzh2.commitments_plan)
    assert hasattr(N.NativeProvingKey, "commitments_plan")
    members = re.search(r"typedef struct \{([^}]*)\} bzh_commitments_out;", header).group(1)
    assert tuple(re.findall(r"\*(\w+)", members)) == bzh2.TranscriptBatch.COMMITMENTS_OUT   # the ctypes mirror is an array in this order


def test_plan_against_the_constraint_system():
    import bzh2
    from helpers import commitments_cases as K
    seen = set()
    for name, blob, cs in _blobs():
        want = K.plan(cs)
        assert bzh2.commitments_plan(bzh2.CURVE_VESTA, blob) == want, name
        seen.add(want[3:6])
    assert seen == {(3, 1, 0), (3, 1, 1), (11, 1, 1)}      # the sample circuit without and with its lookup; Shot and Board


def test_plan_refusals():
    import bzh2
    L = bzh2.load()
    L.bzh_commitments_plan.argtypes = [ctypes.c_int, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_void_p]
    blob = _blobs()[0][1]
    shape = np.full(8, 5, dtype=np.uint32)
    args = [0, blob, len(blob), ctypes.c_void_p(shape.ctypes.data)]
    for change in ((1, None), (3, None), (2, len(blob) // 2), (0, 7)):          # NULL pointers, a truncated blob, no such curve
        a = list(args)
        a[change[0]] = change[1]
        assert L.bzh_commitments_plan(*a) == E_ARG and (shape == 5).all(), change
    assert L.bzh_commitments_plan(*args) == 0 and shape[0] == 16
    with pytest.raises(bzh2.BzhError) as e:
        bzh2.commitments_plan(bzh2.CURVE_VESTA, blob[:len(blob) // 2])
    assert e.value.status == E_ARG


def test_argument_refusals_without_a_device():
    """every refusal that precedes the first use of ctx and needs no device, on made-up non-NULL handles that a refusal must not
    read through; a host-resident batch is left as it was and the output arrays are untouched"""
    import bzh2
    L = bzh2.load()
    vp, sz, ci = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
    L.bzh_commitments_batch_device.argtypes = [vp, vp, sz, vp, vp, sz, ci, ci, vp, sz, vp, vp, vp]
    B, n = 2, 4
    adv, inst = np.zeros((B, 1, n, 4), dtype=np.uint64), np.zeros((B, 1, 1, 4), dtype=np.uint64)
    raw = np.zeros(B * 64 * 16, dtype=np.uint8)
    outs = [np.full((B, 2 * n, 4), 7, dtype=np.uint64) for _ in range(12)]
    st = np.full(B, 7, dtype=np.uint8)
    fake = vp(0x1000)
    at = lambda a: vp(a.ctypes.data)   # noqa: E731
    names = bzh2.TranscriptBatch.COMMITMENTS_OUT

    def out_struct(drop=None):
        return (vp * 12)(*[None if nm == drop else at(o) for nm, o in zip(names, outs)])

    with bzh2.TranscriptBatch(bzh2.CURVE_VESTA, B, 256) as tb, bzh2.TranscriptBatch(bzh2.CURVE_VESTA, B, 256) as twin:   # host-resident
        full = out_struct()

        def call(**kw):
            a = dict(ctx=fake, pk=fake, batch=B, adv=at(adv), inst=at(inst), rows=1, form=bzh2.FORM_CANONICAL, mem=bzh2.MEM_HOST, rng=at(raw),
                     stride=64 * 16, trs=tb.h, out=ctypes.cast(full, vp), st=at(st))
            a.update(kw)
            return L.bzh_commitments_batch_device(*a.values())

        assert call() == E_ARG                                   # a host-resident batch: the made-up ctx and key are not read
        for kw in (dict(ctx=None), dict(pk=None), dict(trs=None), dict(rng=None), dict(out=None), dict(batch=0), dict(batch=65536), dict(form=2),
                   dict(form=-1), dict(mem=2), dict(mem=-1)):
            assert call(**kw) == E_ARG, kw
        for nm in ("theta", "beta", "gamma"):                    # the members every key needs
            assert call(out=ctypes.cast(out_struct(nm), vp)) == E_ARG, nm
        with pytest.raises(bzh2.BzhError) as e:                  # the Python mirror on a host-resident batch: refused the same way
            tb.commitments(fake, adv, inst, [bytes(64 * 16)] * B, shape=(n, 1, 2, 1, 1, 0, 4, 32))
        assert e.value.status == E_ARG
        assert all((o == 7).all() for o in outs) and (st == 7).all() and tb.proof_len() == 0
        assert (tb.squeeze() == twin.squeeze()).all()   # the batch is as it was


def _words(v):
    return [(v >> (32 * i)) & 0xffffffff for i in range(8)]


def test_lane_bodies_against_computed_values_standalone_under_host_sanitizers(tmp_path):
    """cm_const_lane and cm_status_lane, word for word, for Fp and Fq: theta in canonical and in Montgomery form, batches of 1 and
    3, a program that names theta (a row per proof) next to one that does not (one row), theta 0 and p - 1 among the values; the
    status over 0, 1 and 3 lookups with a failed pair in each place.  The expected words are computed here."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    rng = random.Random(91)
    lines, lanes, cases = [], 0, 0
    for fid, Fd in ((0, O.FP), (1, O.FQ)):
        p, R = Fd.p, Fd.R
        for batch in (1, 3):
            for canonical in (0, 1):
                thetas = [0, p - 1, rng.randrange(p)][:batch] if batch > 1 else [rng.randrange(p)]
                given = thetas if canonical else [t * R % p for t in thetas]
                # table 0: literal, theta, literal (per proof); table 1: two literals (one row); table 2: theta alone
                tables = [(3, 1, [None, "theta", None]), (2, 0, [None, None]), (1, 1, ["theta"])]
                lits = {(t, i): rng.randrange(p) for t, (_, _, ent) in enumerate(tables) for i, e in enumerate(ent) if e is None}
                descs = [(t, i) for t, (_, _, ent) in enumerate(tables) for i in range(len(ent))]
                rng.shuffle(descs)                                # a descriptor's place in the list does not matter
                out = ["consts %d %d %d %d" % (fid, batch, canonical, len(tables))]
                out += ["%d %d" % (nc, pp) for nc, pp, _ in tables]
                out.append(str(len(descs)))
                for t, i in descs:
                    sym = tables[t][2][i] == "theta"
                    out.append(" ".join(map(str, [t, int(sym), i] + _words(0 if sym else lits[(t, i)]))))
                out.append(" ".join(str(w) for g in given for w in _words(g)))
                for t, (nc, pp, ent) in enumerate(tables):
                    for b in range(batch if pp else 1):
                        for i, e in enumerate(ent):
                            out.append(" ".join(map(str, _words(thetas[b] * R % p if e == "theta" else lits[(t, i)]))))
                lines += out
                lanes += len(descs) * batch
                cases += 1
    for nl in (0, 1, 3):
        batch = 4
        words = [[0] * nl for _ in range(batch)]
        for b in range(1, batch):
            if nl:
                words[b][(b - 1) % nl] = 0xfffffffc                # BZH_E_RANGE as lookup_permute writes it
        lines.append("status %d %d" % (nl, batch))
        lines.append(" ".join(str(w) for row in words for w in row) or "")
        lines.append(" ".join(str(int(any(row))) for row in words))
        lanes += batch
        cases += 1
    path = tmp_path / "cases.txt"
    path.write_text("\n".join(lines) + "\n")
    csrc = os.path.join(ROOT, "battlezips-halo2_amd", "csrc")
    exe = str(tmp_path / "commitments_scalars_check")
    subprocess.check_call([hipcc, "-O1", "-g", "-std=c++17", "--offload-arch=gfx950", "-Wno-unused-function",
                           "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                           "-I", csrc, os.path.join(ROOT, "tests", "helpers", "commitments_scalars_check.hip"), "-o", exe])
    out = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=600)
    print(out.stdout[-3000:])
    assert out.returncode == 0 and out.stdout.strip().endswith("commitments_scalars_check: ok"), out.stdout[-3000:] + out.stderr[-3000:]
    assert re.search(r"(\d+) cases, (\d+) lanes", out.stdout).groups() == (str(cases), str(lanes))


@accelerated_oracle
def test_model_against_the_oracle_on_the_two_column_lookup(oracle_c):
    """the two-column lookup with a rotation: the oracle proves and verifies it (two_column_case asserts that), theta enters the
    compressed columns, and the model reproduces the oracle's columns, polynomials, blinds, challenges and bytes (model asserts
    that on the captured operands)"""
    from helpers import commitments_cases as K
    cs, keys, _, _, bounds, proofs, want = K.two_column_case()
    assert len(cs.lookups) == 1 and [len(s) for s in cs.lookups[0]] == [2, 2]
    for b, m in zip(bounds, want):
        a_c, s_c = m["lookup_compressed"][0]
        # Horner in theta: first expression times theta plus the second, row by row, the rotation wrapping into the blinding rows
        adv, th = m["advice"], m["theta"]
        assert a_c == [(3 * adv[0][r] * th + adv[1][(r + 1) % cs.n]) % K.P for r in range(cs.n)]
        assert s_c == [(keys.fixed[2][r] * th + keys.fixed[3][r]) % K.P for r in range(cs.n)]
        assert a_c[cs.usable_rows - 1] == adv[1][cs.usable_rows] != 0                   # the drawn value is looked up, and found
        assert sorted(m["lookup_permuted"][0][0][:cs.usable_rows]) == sorted(a_c[:cs.usable_rows])
        assert m["bytes"] == proofs[bounds.index(b)][:len(m["bytes"])]
