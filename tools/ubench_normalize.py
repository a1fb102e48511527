"""bzh_batch_normalize on the device against its host path (ctx == NULL), at 64 x 11 points -- the commitments of a batch of 64
proofs' advice columns -- and at 2^20 points: Vesta, Montgomery operands, affine points and encodings both asked for.

Settings: `host` (ctx == NULL), `staged` (BZH_MEM_HOST through the kernel: upload, launch, read-back) and `device`
(BZH_MEM_DEVICE buffers, launch and stream sync only; needs torch for the buffers).  One fresh process per setting, each under
its own time limit: one warm-up call and five timed calls.  The operands are uniform field elements with Z != 0 -- the call
does not check that a point is on the curve, and the work does not depend on it.

    python tools/ubench_normalize.py > profiles/normalize.json

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


def measure(args):
    n = args.n
    rng = np.random.default_rng(args.n)
    jac = np.frombuffer(rng.bytes(n * 96), dtype=np.uint64).reshape(n, 12).copy()
    jac[:, 3::4] &= (1 << 61) - 1                          # every coordinate below 2^253 < p
    jac[:, 8] |= 1                                         # Z != 0
    if args.where == "device":
        import torch
        torch.zeros(1, device="cuda")                      # torch's HIP runtime initialises before the library's
    import bzh2
    form = bzh2.FORM_MONTGOMERY
    lanes, chain = bzh2.batch_normalize_plan(n)
    if args.where == "host":
        once = lambda: bzh2.batch_normalize(bzh2.CURVE_VESTA, jac, form=form, want_bytes=True, want_status=True)
        secs = timed(once)
    else:
        with bzh2.Context(0) as ctx:
            if args.where == "staged":
                once = lambda: bzh2.batch_normalize(bzh2.CURVE_VESTA, jac, ctx=ctx, form=form, want_bytes=True, want_status=True)
            else:
                d_in = torch.from_numpy(jac.view(np.int64)).to("cuda")
                d_xy = torch.zeros((n, 8), dtype=torch.int64, device="cuda")
                d_enc, d_st = torch.zeros((n, 32), dtype=torch.uint8, device="cuda"), torch.zeros(n, dtype=torch.uint8, device="cuda")

                def once():
                    bzh2.batch_normalize(bzh2.CURVE_VESTA, d_in.data_ptr(), ctx=ctx, form=form, mem=bzh2.MEM_DEVICE, n=n,
                                         out_xy=d_xy.data_ptr(), out32=d_enc.data_ptr(), status=d_st.data_ptr())
                    ctx.sync()
            secs = timed(once)
    print(json.dumps({"where": args.where, "n": n, "lanes": lanes, "chain": chain, "call_seconds": [round(s, 6) for s in secs],
                      "mean_seconds": round(sum(secs) / 5, 6), "min_max_seconds": [round(min(secs), 6), round(max(secs), 6)]}), flush=True)


def timed(once):
    once()                                                 # warm-up: code objects, workspaces, the pinned ring
    secs = []
    for _ in range(5):
        t0 = time.perf_counter()
        once()
        secs.append(time.perf_counter() - t0)
    return secs


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--role", choices=["drive", "measure"], default="drive")
    ap.add_argument("--ns", default="%d,%d" % (64 * 11, 1 << 20))
    ap.add_argument("--n", type=int, default=64 * 11)
    ap.add_argument("--where", choices=["host", "staged", "device"], default="host")
    ap.add_argument("--limit", type=int, default=120, help="seconds each child process may take")
    args = ap.parse_args()
    if args.role == "measure":
        return measure(args)
    rows = []
    for n in [int(v) for v in args.ns.split(",")]:
        for where in ("host", "staged", "device"):
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--role", "measure", "--n", str(n), "--where", where],
                               check=True, timeout=args.limit, stdout=subprocess.PIPE, text=True)
            print(r.stdout.strip(), flush=True)
            rows.append(json.loads(r.stdout.strip().splitlines()[-1]))
    print(json.dumps({"summary": {"n%d_%s" % (r["n"], r["where"]): r["mean_seconds"] for r in rows}}))


if __name__ == "__main__":
    main()
