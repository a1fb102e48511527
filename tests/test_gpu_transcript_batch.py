"""csrc/transcript_batch.hip on the device: k_tb_absorb and k_tb_squeeze over the three curves, canonical and Montgomery,
through BZH_MEM_HOST and BZH_MEM_DEVICE operands -- byte for byte what the host path (ctx == NULL) gives, which
tests/test_transcript_batch_cpu.py pins to the oracle.  Batches of 1, 63, 64, 65 and 257 are the wave and block edges (257
puts a second block's first lane to work); the schedules are those of tests/helpers/transcript_cases.py.  Then: a device
operand that is not below its modulus, the seam bzh_msm -> write_jacobian -> squeeze without a read-back, and the enqueue-only
contract."""
import functools
import random

import numpy as np
import pytest

import coracle as C
from helpers import normalize_cases as K
from helpers import transcript_cases as T

pytestmark = pytest.mark.gpu
CAN, MONT = 0, 1
BATCHES = (1, 63, 64, 65, 257)


def _dev(arr):
    import torch
    return torch.from_numpy(np.ascontiguousarray(arr).view(np.int64).copy()).to("cuda")


@functools.lru_cache(maxsize=None)
def _host_path(cid, name, batch, form):
    """the host-resident batch's (squeeze outputs as bytes, proofs, statuses) -- computed once per shape"""
    import bzh2
    sched, calls = T.SCHEDULES[name](), T.operands(cid, name, batch)
    raw = []
    with bzh2.TranscriptBatch(cid, batch, T.proof_bytes(sched)) as tb:
        def squeeze():
            a = tb.squeeze(form=form)
            raw.append(a.tobytes())
            return a
        T.run_batch(tb, cid, sched, calls, form, squeeze=squeeze)
        return tuple(raw), tuple(tb.proofs()), tuple(tb.status().tolist())


def _run_device(gpu_ctx, cid, name, batch, form, device_operands, calls=None):
    """the schedule through a device batch: (squeeze outputs as bytes, proofs, statuses).  With device_operands every operand is
    uploaded first and checked afterwards to be unchanged, and every challenge and the proofs go to device buffers pre-filled
    with a pattern."""
    import torch
    import bzh2
    sched = T.SCHEDULES[name]()
    calls = calls or T.operands(cid, name, batch)
    cap = T.proof_bytes(sched)
    raw, keep = [], []
    with bzh2.TranscriptBatch(cid, batch, cap, ctx=gpu_ctx) as tb:
        if not device_operands:
            def squeeze():
                a = tb.squeeze(form=form)
                raw.append(a.tobytes())
                return a
            T.run_batch(tb, cid, sched, calls, form, squeeze=squeeze)
            return tuple(raw), tuple(tb.proofs()), tuple(tb.status().tolist())
        outs = []
        for (op, _), call in zip(sched, calls):
            if op == "squeeze":
                d_out = _dev(np.full((batch, 4), 0x5a5a, dtype=np.uint64))
                tb.squeeze(form=form, mem=bzh2.MEM_DEVICE, out=d_out.data_ptr())
                outs.append(d_out)
            else:
                arr = T.as_array(cid, op, call, form)
                d_in = _dev(arr)
                getattr(tb, op)(d_in.data_ptr(), form=form, mem=bzh2.MEM_DEVICE, n=arr.shape[1])
                keep.append((d_in, arr))
        d_pr = _dev(np.full((batch, cap + 32), 7, dtype=np.uint8))
        assert tb.proofs(mem=bzh2.MEM_DEVICE, out=d_pr.data_ptr(), out_stride=cap + 32) == cap
        status = tuple(tb.status().tolist())                  # waits for the stream
        for d_in, arr in keep:
            assert d_in.cpu().numpy().tobytes() == arr.tobytes()                 # the inputs are read only
        pr = d_pr.cpu().numpy().view(np.uint8).reshape(batch, cap + 32)
        assert (pr[:, cap:] == 7).all()                                          # nothing past a row's proof bytes
        return tuple(o.cpu().numpy().tobytes() for o in outs), tuple(pr[b, :cap].tobytes() for b in range(batch)), status


@pytest.mark.parametrize("name", sorted(T.SCHEDULES))
@pytest.mark.parametrize("cid,form", [(0, CAN), (0, MONT), (1, CAN), (1, MONT), (2, CAN), (2, MONT)])
def test_device_equals_host_path_at_wave_and_block_edges(gpu_ctx, cid, form, name):
    for batch in BATCHES:
        want = _host_path(cid, name, batch, form)
        assert want[2] == tuple(T.expected_status(cid, name, batch))
        assert _run_device(gpu_ctx, cid, name, batch, form, False) == want, (cid, form, name, batch, "host operands")
        assert _run_device(gpu_ctx, cid, name, batch, form, True) == want, (cid, form, name, batch, "device operands")


def test_host_path_reference_is_the_oracles(gpu_ctx):
    """the comparator of the test above against hashlib at one GPU-only shape (the CPU suite does batch 1, 3 and 65)"""
    cid, name, batch = 0, "straddle", 257
    raw, proofs, _ = _host_path(cid, name, batch, CAN)
    want, want_proofs = T.expected(cid, name, batch)
    got = [T.challenge_ints(cid, np.frombuffer(r, dtype=np.uint64).reshape(batch, 4), CAN) for r in raw]
    assert got == want and list(proofs) == want_proofs


@pytest.mark.parametrize("cid", [0, 2])
def test_a_device_operand_not_below_its_modulus_marks_its_lane_only(gpu_ctx, cid):
    import bzh2
    name, batch, lane = "straddle", 65, 17
    sched = T.SCHEDULES[name]()
    cv = K.curve_of(cid)
    clean = T.operands(cid, name, batch)
    # one bad coordinate in a point call, one bad scalar in a scalar call, both in `lane`
    jp = next(j for j, (op, _) in enumerate(sched) if op == "write_points")
    js = next(j for j, (op, _) in enumerate(sched) if op == "write_scalars")
    dirty = [None if c is None else [list(row) for row in c] for c in clean]
    dirty[jp][lane][0] = (clean[jp][lane][0][0], cv.p)                           # y = p
    dirty[js][lane][-1] = (1 << 256) - 1
    # ... which the transcript hashes as zeros: the oracle on the same data with zeros there
    zeroed = [None if c is None else [list(row) for row in c] for c in clean]
    zeroed[jp][lane][0] = (0, 0)
    zeroed[js][lane][-1] = 0
    want_lane, want_lane_proofs = T.oracle_run(cid, sched, [None if c is None else [c[lane]] for c in zeroed])
    want, want_proofs = T.expected(cid, name, batch)
    raw, proofs, status = _run_device(gpu_ctx, cid, name, batch, CAN, True, calls=dirty)
    got = [T.challenge_ints(cid, np.frombuffer(r, dtype=np.uint64).reshape(batch, 4), CAN) for r in raw]
    others = [b for b in range(batch) if b != lane]
    assert status[lane] == T.POINT_INVALID and [status[b] for b in others] == [T.expected_status(cid, name, batch)[b] for b in others]
    assert [[g[b] for b in others] for g in got] == [[w[b] for b in others] for w in want]      # the neighbours: the oracle's
    assert [proofs[b] for b in others] == [want_proofs[b] for b in others]
    assert [[g[lane]] for g in got] == want_lane and proofs[lane] == want_lane_proofs[0]
    # host operands are refused before the launch, and nothing is absorbed
    with bzh2.TranscriptBatch(cid, batch, 64, ctx=gpu_ctx) as tb:
        with pytest.raises(bzh2.BzhError) as e:
            tb.write_points(T.as_array(cid, "write_points", dirty[jp], CAN))
        assert e.value.status == bzh2.E_RANGE
        fresh = T.challenge_ints(cid, tb.squeeze(), CAN)
        assert fresh == [__import__("pasta").Blake2bTranscript(cv.scalar).squeeze_challenge()] * batch and tb.proof_len() == 0


def test_msm_to_challenge_without_leaving_the_device(gpu_ctx):
    """bzh_msm -> bzh_transcript_batch_write_jacobian -> bzh_transcript_batch_squeeze, every buffer in HBM, no read-back and no
    sync between the three calls: challenges and proof bytes are the oracle transcript's, fed the C oracle's MSM results"""
    import torch
    import bzh2
    import pasta as O
    cid, n, vecs = bzh2.CURVE_VESTA, 64, 4
    cv = K.curve_of(cid)
    rng = random.Random(0x7462)
    bases = C.point_walk(cid, C.points_to_array([cv.random_point(rng)])[0], n)
    sc = [[rng.randrange(O.FP.p) for _ in range(n)] for _ in range(vecs)]
    sc[2] = [0] * n                                            # this MSM's result is the identity
    sc_can = np.stack([C.ints_to_array(row) for row in sc])
    sc_m = np.frombuffer(K.limbs_bytes(K.to_form(s, O.FP.p, MONT) for row in sc for s in row), dtype=np.uint64).reshape(vecs, n, 4).copy()
    results = [C.array_to_point(C.msm(cid, sc_can[v], bases, 4)) for v in range(vecs)]
    assert results[2] is None and all(r is not None for r in results[:2] + results[3:])
    hb = gpu_ctx.upload_bases(cid, bases)
    try:
        d_s, d_jac = _dev(sc_m), torch.zeros((vecs, 12), dtype=torch.int64, device="cuda")
        for batch, count in ((4, 1), (2, 2)):                  # one point per transcript; two per transcript
            want_chal, want_proofs = [], []
            for b in range(batch):
                tr = O.Blake2bTranscript(cv.scalar)
                for pt in results[b * count:(b + 1) * count]:
                    tr.write_point(cv, pt)
                want_chal.append(tr.squeeze_challenge())
                want_proofs.append(bytes(tr.proof))
            d_ch = _dev(np.full((batch, 4), 0x5a5a, dtype=np.uint64))
            with bzh2.TranscriptBatch(cid, batch, 32 * count, ctx=gpu_ctx) as tb:
                gpu_ctx.msm_device(hb, d_s.data_ptr(), n, vecs, d_jac.data_ptr(), form=MONT)
                tb.write_jacobian(d_jac.data_ptr(), form=MONT, mem=bzh2.MEM_DEVICE, n=count)
                tb.squeeze(form=CAN, mem=bzh2.MEM_DEVICE, out=d_ch.data_ptr())
                gpu_ctx.sync()
                assert T.challenge_ints(cid, d_ch.cpu().numpy().view(np.uint64), CAN) == want_chal
                assert tb.proofs() == want_proofs
                assert tb.status().tolist() == [int(None in results[b * count:(b + 1) * count]) for b in range(batch)]
    finally:
        hb.free()


def test_enqueue_only_then_status_waits(gpu_ctx):
    """with BZH_MEM_DEVICE the calls only enqueue: nothing here synchronises but bzh_transcript_batch_status, after which every
    output is in place; the same schedule with a ctx.sync() after every call gives the same bytes"""
    import bzh2
    cid, name, batch, form = 1, "block_edge", 257, MONT
    sched, calls = T.SCHEDULES[name](), T.operands(cid, name, batch)
    want = _host_path(cid, name, batch, form)
    runs = []
    for sync_each in (False, True):
        outs, keep = [], []
        with bzh2.TranscriptBatch(cid, batch, T.proof_bytes(sched), ctx=gpu_ctx) as tb:
            for (op, _), call in zip(sched, calls):
                if op == "squeeze":
                    outs.append(_dev(np.full((batch, 4), 0x5a5a, dtype=np.uint64)))
                    tb.squeeze(form=form, mem=bzh2.MEM_DEVICE, out=outs[-1].data_ptr())
                else:
                    keep.append(_dev(T.as_array(cid, op, call, form)))
                    getattr(tb, op)(keep[-1].data_ptr(), form=form, mem=bzh2.MEM_DEVICE, n=len(call[0]))
                if sync_each:
                    gpu_ctx.sync()
            status = tuple(tb.status().tolist())              # the only wait of the first run
            runs.append((tuple(o.cpu().numpy().tobytes() for o in outs), tuple(tb.proofs()), status))
    assert runs[0] == runs[1] == want
