"""bzh_ipa_open_batch_device against bzh_ipa_open_batch: B = 1, 8 and 64 openings at k = 11 and 14 on the window-table SRS of
Params::new(k) (Vesta), Montgomery coefficients in device memory either way.

Settings: `host` (bzh_ipa_open_batch on B host bzh_transcript objects: k + 1 read-backs, host normalisation, BLAKE2b and
inversion, k + 1 uploads and stream waits) and `device` (bzh_ipa_open_batch_device on a device-resident bzh_transcript_batch
with every operand a BZH_MEM_DEVICE buffer: launches only, one stream sync at the end; needs torch for the buffers).  One fresh
process per (k, B, setting), each under its own time limit: one warm-up call and five timed calls, a fresh set of transcripts
for every call.  The `device` process then makes one more call under BZH_PROVE_TRACE=1, whose `[bzh_ipa_open_batch_device]`
line gives the event times of the steps: io:normalize_absorb_ms, io:squeeze_ms, io:round_scalars_ms and io:msm_ms (that call
waits for the stream once, at its end, to read the events).  The operands are uniform values; the work does not depend on them.

    python tools/ubench_ipa_open.py > profiles/ipa_open_device_calls.json

It only prints: one JSON object per setting and a final summary.  A setting whose process ends abnormally stops the run.
"""
import argparse
import ctypes
import json
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "battlezips-halo2_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def traced(fn):
    """run fn() with BZH_PROVE_TRACE=1 and hand back what the library wrote to stderr"""
    sys.stderr.flush()
    keep = os.dup(2)
    with tempfile.TemporaryFile() as f:
        os.environ["BZH_PROVE_TRACE"] = "1"
        os.dup2(f.fileno(), 2)
        try:
            fn()
        finally:
            os.dup2(keep, 2)
            os.close(keep)
            del os.environ["BZH_PROVE_TRACE"]
        f.seek(0)
        return f.read().decode(errors="replace")


def measure(args):
    import torch
    torch.zeros(1, device="cuda")                              # torch's HIP runtime initialises before the library's
    import bzh2
    from bzh2 import params as Pm
    B, k = args.batch, args.k
    n, nrand = 1 << k, (1 << k) + 1 + 2 * k
    rng = np.random.default_rng(100 * k + B)

    def elems(*shape):
        a = np.frombuffer(rng.bytes(int(np.prod(shape)) * 32), dtype=np.uint64).reshape(*shape, 4).copy()
        a[..., 3] &= (1 << 60) - 1                             # every element below 2^252
        return a

    polys, blinds, x3s = elems(B, n), elems(B), elems(B)
    raw = np.frombuffer(rng.bytes(B * nrand * 64), dtype=np.uint8).reshape(B, nrand * 64)
    cid, MONT = bzh2.CURVE_VESTA, bzh2.FORM_MONTGOMERY
    row = {"where": args.where, "k": k, "batch": B}
    with bzh2.Context(0) as ctx:
        prm = Pm.Params(ctx, k)
        d_polys = torch.from_numpy(polys.view(np.int64)).to("cuda")
        if args.where == "host":
            L = bzh2.load()
            vp, u64p = ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64)
            L.bzh_ipa_open_batch.argtypes = [vp, vp, vp, ctypes.c_int, ctypes.c_int, ctypes.c_size_t, u64p, u64p,
                                             ctypes.c_char_p, ctypes.c_size_t, ctypes.POINTER(vp), u64p]
            out = np.zeros((B, 4), dtype=np.uint64)
            stream = raw.tobytes()

            def once():
                trs = [bzh2.Transcript(bzh2.FIELD_FP) for _ in range(B)]
                hs = (vp * B)(*[t.h for t in trs])
                # blinds and x3s are canonical host limbs on this path
                rc = L.bzh_ipa_open_batch(ctx.handle, prm.bases.handle, vp(d_polys.data_ptr()), MONT, bzh2.MEM_DEVICE, B, bzh2._u64(blinds),
                                          bzh2._u64(x3s), stream, nrand * 64, hs, bzh2._u64(out))
                ctx._check(rc, "bzh_ipa_open_batch")
                ctx.sync()
                for t in trs:
                    t.close()
            secs = timed(once)
        else:
            d_bl, d_x3 = (torch.from_numpy(a.view(np.int64)).to("cuda") for a in (blinds, x3s))
            d_raw = torch.from_numpy(raw.copy()).to("cuda")
            d_v = torch.zeros((B, 4), dtype=torch.int64, device="cuda")
            d_st = torch.zeros((B,), dtype=torch.uint8, device="cuda")
            cap = 32 * (1 + 2 * k) + 64

            def once():
                with bzh2.TranscriptBatch(cid, B, cap, ctx=ctx) as tb:
                    tb.ipa_open(prm.bases, d_polys.data_ptr(), d_bl.data_ptr(), d_x3.data_ptr(), d_raw.data_ptr(), form=MONT,
                                mem=bzh2.MEM_DEVICE, out_v=d_v.data_ptr(), status=d_st.data_ptr(), rng_stride=nrand * 64)
                    ctx.sync()
            secs = timed(once)
            text = traced(once)
            m = re.search(r"\[bzh_ipa_open_batch_device\].*", text)
            row["trace"] = {name: float(val) for name, val in re.findall(r"(io:\w+)=([0-9.]+)", m.group(0))} if m else None
        prm.close()
    row.update({"call_seconds": [round(s, 6) for s in secs], "mean_seconds": round(sum(secs) / 5, 6),
                "min_max_seconds": [round(min(secs), 6), round(max(secs), 6)]})
    print(json.dumps(row), flush=True)


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
    ap.add_argument("--k", type=int, default=11)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--where", choices=["device", "host"], default="host")
    ap.add_argument("--limit", type=int, default=120, help="seconds each child process may take")
    args = ap.parse_args()
    if args.role == "measure":
        return measure(args)
    rows = []
    for k in (11, 14):
        for batch in (1, 8, 64):
            for where in ("host", "device"):
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--role", "measure", "--k", str(k), "--batch", str(batch),
                                    "--where", where], check=True, timeout=args.limit, stdout=subprocess.PIPE, text=True)
                print(r.stdout.strip(), flush=True)
                rows.append(json.loads(r.stdout.strip().splitlines()[-1]))
    print(json.dumps({"summary": {"k%d_batch%d_%s" % (r["k"], r["batch"], r["where"]): r["mean_seconds"] for r in rows}}))


if __name__ == "__main__":
    main()
