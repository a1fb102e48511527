"""bzh_transcript_batch_* against the host bzh_transcript objects: 64 transcripts through a schedule shaped like one Board
proof -- about 60 points, 60 scalars, the IPA's 14 rounds of two points and a challenge, and the challenges between (SCHEDULE;
tests/helpers/transcript_cases.py tests the same list).  Vesta, Montgomery operands.

Settings: `device` (a device batch, operands and challenges in BZH_MEM_DEVICE buffers: launches and one stream sync at the end;
needs torch for the buffers), `staged` (a device batch fed BZH_MEM_HOST operands: an upload per absorb, a read-back and a sync
per challenge) and `host` (64 bzh_transcript objects fed item by item through this binding, so its figure includes one ctypes
call per item).  One fresh process per setting, each under its own time limit: one warm-up call and five timed calls.  The
operands are uniform values below 2^253; the work does not depend on them.

    python tools/ubench_transcript.py > profiles/transcript_batch.json

It only prints: one JSON object per setting and a final summary.  A setting whose process ends abnormally stops the run.
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "battlezips-halo2_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

# (op, items per transcript): the vk digest and the instance, the advice, lookup, permutation and quotient commitments with
# their challenges, the evaluations, the multiopen commitments, then the IPA's S, its 14 rounds and its two closing scalars
SCHEDULE = ((("common_scalars", 1), ("common_points", 2), ("write_points", 11), ("squeeze", 1), ("write_points", 6), ("squeeze", 1),
             ("squeeze", 1), ("write_points", 9), ("squeeze", 1), ("write_points", 4), ("squeeze", 1), ("write_scalars", 58), ("squeeze", 1),
             ("squeeze", 1), ("write_points", 1), ("squeeze", 1), ("squeeze", 1), ("write_points", 1), ("squeeze", 1), ("squeeze", 1))
            + (("write_points", 2), ("squeeze", 1)) * 14 + (("write_scalars", 2),))
LIMBS = {"common_points": 8, "write_points": 8, "common_scalars": 4, "write_scalars": 4}


def measure(args):
    B = args.batch
    rng = np.random.default_rng(B)
    arrays = []
    for op, cnt in SCHEDULE:
        if op == "squeeze":
            arrays.append(None)
            continue
        a = np.frombuffer(rng.bytes(B * cnt * LIMBS[op] * 8), dtype=np.uint64).reshape(B, cnt, LIMBS[op]).copy()
        a[:, :, 3::4] &= (1 << 61) - 1                         # every element below 2^253
        arrays.append(a)
    cap = 32 * sum(c for op, c in SCHEDULE if op.startswith("write"))
    if args.where == "device":
        import torch
        torch.zeros(1, device="cuda")                          # torch's HIP runtime initialises before the library's
    import bzh2
    cid, form = bzh2.CURVE_VESTA, bzh2.FORM_MONTGOMERY
    if args.where == "host":
        ints = [None if a is None else [[[bzh2.limbs_to_int(a[b, i, 4 * k:4 * k + 4]) for k in range(a.shape[2] // 4)] for i in range(a.shape[1])]
                                        for b in range(B)] for a in arrays]

        def once():
            trs = [bzh2.Transcript(bzh2.FIELD_FP) for _ in range(B)]
            for (op, _), call in zip(SCHEDULE, ints):
                for b, t in enumerate(trs):
                    if op == "squeeze":
                        t.squeeze_challenge()
                        continue
                    for item in call[b]:
                        if op == "write_points":
                            t.write_point(cid, tuple(item))
                        elif op == "common_points":
                            t.common_point(tuple(item))
                        elif op == "write_scalars":
                            t.write_scalar(item[0])
                        else:
                            t.common_scalar(item[0])
            for t in trs:
                t.close()
        secs = timed(once)
    else:
        with bzh2.Context(0) as ctx:
            if args.where == "staged":
                def once():
                    with bzh2.TranscriptBatch(cid, B, cap, ctx=ctx) as tb:
                        for (op, _), a in zip(SCHEDULE, arrays):
                            if op == "squeeze":
                                tb.squeeze(form=form)
                            else:
                                getattr(tb, op)(a, form=form)
                        ctx.sync()
            else:
                d_in = [None if a is None else torch.from_numpy(a.view(np.int64)).to("cuda") for a in arrays]
                d_ch = torch.zeros((B, 4), dtype=torch.int64, device="cuda")

                def once():
                    with bzh2.TranscriptBatch(cid, B, cap, ctx=ctx) as tb:
                        for (op, cnt), d in zip(SCHEDULE, d_in):
                            if op == "squeeze":
                                tb.squeeze(form=form, mem=bzh2.MEM_DEVICE, out=d_ch.data_ptr())
                            else:
                                getattr(tb, op)(d.data_ptr(), form=form, mem=bzh2.MEM_DEVICE, n=cnt)
                        ctx.sync()
            secs = timed(once)
    print(json.dumps({"where": args.where, "batch": B, "calls_per_run": len(SCHEDULE), "call_seconds": [round(s, 6) for s in secs],
                      "mean_seconds": round(sum(secs) / 5, 6), "min_max_seconds": [round(min(secs), 6), round(max(secs), 6)]}), flush=True)


def timed(once):
    once()                                                     # warm-up: code objects, workspaces, the pinned ring
    secs = []
    for _ in range(5):
        t0 = time.perf_counter()
        once()
        secs.append(time.perf_counter() - t0)
    return secs


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--role", choices=["drive", "measure"], default="drive")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--where", choices=["device", "staged", "host"], default="host")
    ap.add_argument("--limit", type=int, default=90, help="seconds each child process may take")
    args = ap.parse_args()
    if args.role == "measure":
        return measure(args)
    rows = []
    for where in ("device", "staged", "host"):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--role", "measure", "--batch", str(args.batch), "--where", where],
                           check=True, timeout=args.limit, stdout=subprocess.PIPE, text=True)
        print(r.stdout.strip(), flush=True)
        rows.append(json.loads(r.stdout.strip().splitlines()[-1]))
    print(json.dumps({"summary": {"batch%d_%s" % (r["batch"], r["where"]): r["mean_seconds"] for r in rows}}))


if __name__ == "__main__":
    main()
