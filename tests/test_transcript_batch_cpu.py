"""bzh_transcript_batch_* without a device: a host-resident batch (ctx == NULL) runs csrc/transcript_batch.hpp's step code --
the code the kernels run -- in a loop over the transcripts.  Checked against oracle/pasta.py's Blake2bTranscript
(hashlib.blake2b) and against the host bzh_transcript objects fed the same items, over the schedules of
tests/helpers/transcript_cases.py: a last block that is exactly full, items that straddle a block edge at every kind of byte
position, and a schedule shaped like one proof; then statuses, refusals that must leave the state alone, crossing to host
objects and back in the middle of a schedule, Jacobian operands, every argument error, and the step code on its own under the
host's sanitizers."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from helpers import normalize_cases as K
from helpers import transcript_cases as T

VP = ctypes.c_void_p
FORMS = (0, 1)
BATCHES = (1, 3, 65)


@pytest.fixture(scope="module")
def bzh2_lib():
    import bzh2
    bzh2.load()
    return bzh2


@pytest.mark.parametrize("name", sorted(T.SCHEDULES))
@pytest.mark.parametrize("cid", [0, 1, 2])
def test_host_batch_matches_the_oracle_and_the_host_objects(bzh2_lib, cid, name):
    sched = T.SCHEDULES[name]()
    for batch in BATCHES:
        calls = T.operands(cid, name, batch)
        want_chal, want_proofs = T.expected(cid, name, batch)
        assert len(want_chal) == sum(op == "squeeze" for op, _ in sched) and len(want_proofs[0]) == T.proof_bytes(sched)
        assert T.run_host_objects(bzh2_lib, cid, sched, calls) == (want_chal, want_proofs)
        for form in FORMS:
            with bzh2_lib.TranscriptBatch(cid, batch, T.proof_bytes(sched)) as tb:
                got = T.run_batch(tb, cid, sched, calls, form)
                assert got == want_chal, (cid, name, batch, form)
                assert tb.proofs() == want_proofs, (cid, name, batch, form)
                assert tb.proof_len() == T.proof_bytes(sched)
                assert tb.status().tolist() == T.expected_status(cid, name, batch), (cid, name, batch, form)


def test_statuses_are_sticky_and_per_transcript(bzh2_lib):
    cid, batch = 0, 5
    p = K.curve_of(cid).p
    with bzh2_lib.TranscriptBatch(cid, batch, 64) as tb:
        assert tb.status().tolist() == [0] * batch
        pts = [[(3 + b, 5)] for b in range(batch)]
        pts[2] = [(0, 0)]
        tb.common_points(T.as_array(cid, "common_points", pts, 0))
        assert tb.status().tolist() == [0, 0, 1, 0, 0]
        pts = [[(1, 2), (p - 1, 0), (0, 1)] for b in range(batch)]           # a zero coordinate alone is no identity
        pts[4][2] = (0, 0)
        tb.write_points(T.as_array(cid, "write_points", pts, 1)[:, :2], form=1)
        assert tb.status().tolist() == [0, 0, 1, 0, 0]
        tb.common_points(T.as_array(cid, "common_points", pts, 1)[:, 2:], form=1)
        assert tb.status().tolist() == [0, 0, 1, 0, 1]                        # and it stays
        tb.common_scalars(np.zeros((batch, 1, 4), dtype=np.uint64))           # a zero scalar is an ordinary value
        assert tb.status().tolist() == [0, 0, 1, 0, 1]


@pytest.mark.parametrize("cid", [0, 1, 2])
def test_a_host_operand_not_below_its_modulus_is_refused_and_changes_nothing(bzh2_lib, cid):
    name, batch = "straddle", 3
    sched, calls = T.SCHEDULES[name](), T.operands(cid, name, batch)
    cv = K.curve_of(cid)
    cut = next(j for j, (op, _) in enumerate(sched) if op == "squeeze" and T.proof_bytes(sched[:j]) >= 96)
    assert T.proof_bytes(sched[:cut]) + 64 <= T.proof_bytes(sched)            # the refused writes would have had room
    status = [int(any((0, 0) in c[b] for (op, _), c in zip(sched[:cut], calls) if op.endswith("points"))) for b in range(batch)]
    want, want_proofs = T.oracle_run(cid, sched[:cut + 1], calls[:cut + 1])
    with bzh2_lib.TranscriptBatch(cid, batch, T.proof_bytes(sched)) as tb:
        got = T.run_batch(tb, cid, sched, calls, 0, last=cut)
        for op, mod, limbs in (("common_points", cv.p, 8), ("write_points", cv.p, 8), ("write_jacobian", cv.p, 12),
                               ("common_scalars", cv.scalar.p, 4), ("write_scalars", cv.scalar.p, 4)):
            for bad in (mod, (1 << 256) - 1):
                for b, i, limb in ((0, 0, 0), (batch - 1, 1, limbs // 4 - 1)):
                    arr = np.ones((batch, 2, limbs), dtype=np.uint64)
                    arr[b, i, 4 * limb:4 * limb + 4] = np.frombuffer(bad.to_bytes(32, "little"), dtype=np.uint64)
                    with pytest.raises(bzh2_lib.BzhError) as e:
                        getattr(tb, op)(arr, form=0)
                    assert e.value.status == bzh2_lib.E_RANGE, (op, bad, b, i)
        # the next challenge and the proof are the oracle's without any of those items
        got += T.run_batch(tb, cid, sched, calls, 0, first=cut, last=cut + 1)
        assert got == want and tb.proofs() == want_proofs and tb.status().tolist() == status


def test_a_write_past_proof_cap_is_refused_and_changes_nothing(bzh2_lib):
    cid, batch = 1, 3
    cv = K.curve_of(cid)
    calls = [[[(7 + b, 9), (11, 13 + b)] for b in range(batch)], [[5 + b] for b in range(batch)], None]
    sched = (("write_points", 2), ("write_scalars", 1), ("squeeze", 1))
    want, want_proofs = T.oracle_run(cid, sched, calls)
    with bzh2_lib.TranscriptBatch(cid, batch, 100) as tb:                      # room for three items, not for a fourth
        tb.write_points(T.as_array(cid, "write_points", calls[0], 0))
        tb.write_scalars(T.as_array(cid, "write_scalars", calls[1], 0))
        one_pt, two_sc = np.ones((batch, 1, 8), dtype=np.uint64), np.ones((batch, 2, 4), dtype=np.uint64)
        jac = np.ones((batch, 1, 12), dtype=np.uint64)
        for op, arr in (("write_points", one_pt), ("write_scalars", two_sc), ("write_jacobian", jac)):
            with pytest.raises(bzh2_lib.BzhError) as e:
                getattr(tb, op)(arr)
            assert e.value.status == bzh2_lib.E_RANGE, op
        assert tb.proof_len() == 96
        assert [T.challenge_ints(cid, tb.squeeze(), 0)] == want and tb.proofs() == want_proofs
        tb.common_points(one_pt)                                               # absorbing without writing needs no room
    with bzh2_lib.TranscriptBatch(cid, batch, 0) as tb:
        with pytest.raises(bzh2_lib.BzhError) as e:
            tb.write_scalars(two_sc)
        assert e.value.status == bzh2_lib.E_RANGE
        assert tb.proofs() == [b""] * batch


@pytest.mark.parametrize("cid,form", [(0, 1), (1, 0), (2, 1)])
def test_crossing_to_host_objects_and_back_in_the_middle_of_a_schedule(bzh2_lib, cid, form):
    name, batch = "proof", 3
    sched, calls = T.SCHEDULES[name](), T.operands(cid, name, batch)
    want, want_proofs = T.expected(cid, name, batch)
    cuts = (9, 30)                                                             # inside the commitments; inside the IPA rounds
    trs = [bzh2_lib.Transcript(bzh2_lib.CURVE_SCALAR_FIELD[cid]) for _ in range(batch)]
    try:
        with bzh2_lib.TranscriptBatch(cid, batch, T.proof_bytes(sched)) as tb, bzh2_lib.TranscriptBatch(cid, batch, T.proof_bytes(sched)) as tb2:
            got = T.run_batch(tb, cid, sched, calls, form, last=cuts[0])
            tb.to_host(trs)
            assert [t.proof() for t in trs] == tb.proofs()
            for (op, _), call in list(zip(sched, calls))[cuts[0]:cuts[1]]:     # the host objects carry on ...
                ch = T.host_objects_feed(bzh2_lib, trs, cid, op, call)
                if ch is not None:
                    got.append(ch)
            tb2.from_host(trs)                                                 # ... and a fresh batch takes over from them
            assert tb2.status().tolist() == [0] * batch
            got += T.run_batch(tb2, cid, sched, calls, form, first=cuts[1])
            assert got == want and tb2.proofs() == want_proofs
    finally:
        for t in trs:
            t.close()


def test_from_host_refusals(bzh2_lib):
    cid, batch = 0, 3
    fid = bzh2_lib.CURVE_SCALAR_FIELD[cid]
    mk = lambda f=fid: [bzh2_lib.Transcript(f) for _ in range(batch)]
    with bzh2_lib.TranscriptBatch(cid, batch, 64) as tb:
        tb.common_scalars(T.as_array(cid, "common_scalars", [[b] for b in range(batch)], 0))
        before = T.challenge_ints(cid, tb.squeeze(), 0)

        def refused(trs):
            with pytest.raises(bzh2_lib.BzhError) as e:
                tb.from_host(trs)
            assert e.value.status == bzh2_lib.E_ARG
        trs = mk()
        trs[1].common_scalar(5)                                                # unequal absorbed lengths
        refused(trs)
        trs = mk()
        trs[2].write_scalar(5)
        trs[0].common_scalar(5), trs[1].common_scalar(5)                       # equal absorbed lengths, unequal proof lengths
        refused(trs)
        trs = mk()
        for _ in range(3):                                                     # one is a whole block ahead: the same buffer fill
            trs[1].common_scalar(7)
        for _ in range(29):
            trs[1].squeeze_challenge()
        refused(trs)
        refused(mk(bzh2_lib.FIELD_FQ))                                         # not the curve's scalar field
        trs = mk()
        for t in trs:
            t.write_scalar(1), t.write_scalar(2), t.write_scalar(3)            # 96 proof bytes > proof_cap
        refused(trs)
        # none of it touched the batch: it continues where it was
        ref = [bzh2_lib.Transcript(fid) for _ in range(batch)]
        for b, t in enumerate(ref):
            t.common_scalar(b)
        assert [t.squeeze_challenge() for t in ref] == before
        assert T.challenge_ints(cid, tb.squeeze(), 0) == [t.squeeze_challenge() for t in ref]
        with pytest.raises(bzh2_lib.BzhError) as e:
            tb.to_host(mk(bzh2_lib.FIELD_FQ))
        assert e.value.status == bzh2_lib.E_ARG


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("cid", [0, 1, 2])
def test_write_jacobian_is_normalise_then_write(bzh2_lib, cid, form):
    batch, count, stride = 5, 3, 4
    cv = K.curve_of(cid)
    triples = K.batch(cid, batch * stride, seed=11, identities=[1, 6, 11])    # item 1 of transcript 0, item 2 of 1, the gap of 2
    exp = K.expected(cid, triples)
    jac = K.jac_array(cid, triples, form).reshape(batch, stride, 12)
    pts = [[(exp[b * stride + i][1], exp[b * stride + i][2]) for i in range(count)] for b in range(batch)]
    sched = (("common_scalars", 1), ("write_points", count), ("squeeze", 1))
    calls = [[[b + 1] for b in range(batch)], pts, None]
    want, want_proofs = T.oracle_run(cid, sched, calls)
    L = bzh2_lib._bind_transcript_batch()
    with bzh2_lib.TranscriptBatch(cid, batch, 32 * count) as tb:
        tb.common_scalars(T.as_array(cid, "common_scalars", calls[0], form), form=form)
        assert L.bzh_transcript_batch_write_jacobian(tb.h, VP(jac.ctypes.data), count, stride, form, bzh2_lib.MEM_HOST) == bzh2_lib.OK
        assert [T.challenge_ints(cid, tb.squeeze(form=form), form)] == want and tb.proofs() == want_proofs
        assert tb.status().tolist() == [int((0, 0) in row) for row in pts] and {0, 1} == set(tb.status().tolist())


def test_arguments(bzh2_lib):
    L = bzh2_lib._bind_transcript_batch()
    OK, E_ARG, H, D = bzh2_lib.OK, bzh2_lib.E_ARG, bzh2_lib.MEM_HOST, bzh2_lib.MEM_DEVICE
    h = VP()
    new = L.bzh_transcript_batch_new
    assert new(None, 0, 3, 64, None) == E_ARG                                  # no place for the handle
    for cid in (-1, 3):
        assert new(None, cid, 3, 64, ctypes.byref(h)) == E_ARG                 # unknown curve
    assert new(None, 0, 0, 64, ctypes.byref(h)) == E_ARG                       # an empty batch
    assert new(None, 0, 1 << 40, 64, ctypes.byref(h)) == E_ARG
    assert new(None, 0, 3, 1 << 40, ctypes.byref(h)) == E_ARG
    assert L.bzh_transcript_batch_free(None) == E_ARG
    assert new(None, 0, 3, 64, ctypes.byref(h)) == OK
    try:
        buf = np.ones((3, 2, 12), dtype=np.uint64)
        out = np.zeros((3, 4), dtype=np.uint64)
        p = lambda a: VP(a.ctypes.data)
        absorbers = [getattr(L, "bzh_transcript_batch_" + f) for f in ("common_points", "write_points", "write_jacobian", "common_scalars",
                                                                       "write_scalars")]
        for fn in absorbers:
            assert fn(None, p(buf), 1, 1, 0, H) == E_ARG                       # no batch
            assert fn(h, None, 1, 1, 0, H) == E_ARG                            # NULL operands with count > 0
            assert fn(h, p(buf), 2, 1, 0, H) == E_ARG                          # stride < count
            assert fn(h, p(buf), 1, 1 << 60, 0, H) == E_ARG                    # a stride whose offsets would not fit
            assert fn(h, p(buf), 1, 1, 2, H) == E_ARG                          # unknown form
            assert fn(h, p(buf), 1, 1, 0, 2) == E_ARG                          # unknown mem
            assert fn(h, p(buf), 1, 1, 0, D) == E_ARG                          # device memory on a host-resident batch
            assert fn(h, None, 0, 0, 0, H) == OK                               # count == 0
        sq = L.bzh_transcript_batch_squeeze
        for bad in ((None, 0, H, p(out)), (h, 2, H, p(out)), (h, 0, 2, p(out)), (h, 0, D, p(out)), (h, 0, H, None)):
            assert sq(*bad) == E_ARG
        ln = ctypes.c_size_t(99)
        pr = L.bzh_transcript_batch_proofs
        assert pr(None, H, None, 0, ctypes.byref(ln)) == E_ARG and pr(h, 2, None, 0, ctypes.byref(ln)) == E_ARG
        assert pr(h, H, None, 0, None) == E_ARG                                # nothing asked for
        assert pr(h, D, p(buf), 64, None) == E_ARG
        assert L.bzh_transcript_batch_status(None, p(out)) == E_ARG and L.bzh_transcript_batch_status(h, None) == E_ARG
        assert L.bzh_transcript_batch_from_host(h, None) == E_ARG and L.bzh_transcript_batch_to_host(h, None) == E_ARG
        assert L.bzh_transcript_batch_from_host(None, (VP * 3)()) == E_ARG
        assert L.bzh_transcript_batch_from_host(h, (VP * 3)()) == E_ARG        # NULL objects
        assert L.bzh_transcript_batch_to_host(h, (VP * 3)()) == E_ARG
        # none of the refusals changed the batch: it is still a fresh one
        assert pr(h, H, None, 0, ctypes.byref(ln)) == OK and ln.value == 0
        assert sq(h, 0, H, p(out)) == OK
        import pasta as O
        assert T.challenge_ints(0, out, 0) == [O.Blake2bTranscript(O.FP).squeeze_challenge()] * 3
        assert L.bzh_transcript_batch_write_scalars(h, p(buf), 2, 2, 0, H) == OK
        assert pr(h, H, p(buf), 63, None) == E_ARG                             # rows shorter than the proofs
        assert pr(h, H, p(buf), 64, ctypes.byref(ln)) == OK and ln.value == 64
    finally:
        assert L.bzh_transcript_batch_free(h) == OK


def test_step_code_standalone_under_host_sanitizers(tmp_path):
    """tests/helpers/transcript_batch_check.hip: the step code with its own main, built with ASan + UBSan for the host, on the CPU"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "transcript_batch_check")
    subprocess.check_call([hipcc, "-O1", "-g", "-std=c++17", "--offload-arch=gfx950", "-Wno-unused-function",
                           "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(root, "battlezips-halo2_amd", "csrc"),
                           os.path.join(root, "tests", "helpers", "transcript_batch_check.hip"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip().endswith("transcript_batch_check: ok"), out.stdout[-2000:] + out.stderr[-2000:]
