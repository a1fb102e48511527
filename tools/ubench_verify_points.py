#!/usr/bin/env python3
"""Where does bzh_verify_batch spend its time, and does decompressing the proofs' points on the device help?

Makes 64 real BoardCircuit proofs at k = 14 once (bzh_prove_batch_seeded), then times bzh_verify_batch -- 1 warm-up call and
5 timed calls -- with the points decompressed on the host (BZH_VERIFY_POINTS_HOST) and on the device
(BZH_VERIFY_POINTS_DEVICE), at BZH_HOST_THREADS = 2 and = 16.  Every setting runs in a process of its own under its own
time limit; one more call per setting runs with BZH_PROVE_TRACE=1 and its `[bzh_verify_batch]` lines are parsed for the split
of the host pass into point decompression and the rest (thread-summed wall time) and for k_decompress's own time.

    python tools/ubench_verify_points.py [--batch 64] [--k 14] > profiles/verify_points.json

Prints one JSON object per setting and a final summary object.  A setting whose process ends abnormally stops the run.
"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "battlezips-halo2_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

DECK = [(3, 3, True), (5, 4, False), (0, 1, False), (0, 5, True), (6, 1, False)]
FQ = 0x40000000000000000000000000000000224698fc0994a8dd8c46eb2100000001


def _key(ctx, k):
    import bzh2
    from bzh2 import circuits as Cm, native as N, params as Pm
    lay = Cm.CircuitLayout(Cm.BOARD, k)
    prm = Pm.Params(ctx, k)
    return lay, prm, N.NativeProvingKey(ctx, lay.blob(), bzh2.CURVE_VESTA, params=prm)


def make(args):
    import hashlib
    import numpy as np
    import bzh2
    from bzh2 import circuits as Cm
    with bzh2.Context(0) as ctx:
        lay, prm, pk = _key(ctx, args.k)
        ships, state = Cm.board_witness(DECK, None)
        circuits = [Cm.BoardCircuit(ships, state, (0x9e3779b97f4a7c15 * (i + 1) + (i << 130)) % FQ) for i in range(args.batch)]
        adv, insts = lay.synthesize(circuits)
        seeds = [hashlib.blake2b(b"ubench_verify_points %d" % i, digest_size=32).digest() for i in range(args.batch)]
        proofs = pk.prove_batch(adv, insts, None, seeds=seeds)
        assert all(pk.verify_batch(insts, proofs))
        np.savez(args.file, proofs=np.array([np.frombuffer(p, dtype=np.uint8) for p in proofs]),
                 insts=np.array([[[int(v).to_bytes(32, "little") for v in col] for col in cols] for cols in insts], dtype="S32"))
        pk.close(), prm.close(), lay.close()


def _traced_call(fn):
    """run fn() with BZH_PROVE_TRACE=1 and hand back what the library wrote to stderr"""
    sys.stderr.flush()
    with tempfile.TemporaryFile(mode="w+b") as tmp:
        saved = os.dup(2)
        os.environ["BZH_PROVE_TRACE"] = "1"
        os.dup2(tmp.fileno(), 2)
        try:
            fn()
        finally:
            os.dup2(saved, 2)
            os.close(saved)
            del os.environ["BZH_PROVE_TRACE"]
        tmp.seek(0)
        return tmp.read().decode(errors="replace")


def verify(args):
    import numpy as np
    import bzh2
    from bzh2 import native as N
    d = np.load(args.file)
    proofs = [bytes(r.tobytes()) for r in d["proofs"]]
    insts = [[[int.from_bytes(v, "little") for v in col] for col in cols] for cols in d["insts"].tolist()]
    os.environ["BZH_HOST_THREADS"] = str(args.threads)     # read by the library at every call
    with bzh2.Context(0) as ctx:
        lay, prm, pk = _key(ctx, args.k)
        pk.verify_select(N.VERIFY_POINTS_DEVICE if args.where == "device" else N.VERIFY_POINTS_HOST)
        assert all(pk.verify_batch(insts, proofs))          # warm-up (also computes the verifying key once)
        secs = []
        for _ in range(5):
            t0 = time.perf_counter()
            ok = pk.verify_batch(insts, proofs)
            secs.append(time.perf_counter() - t0)
            assert all(ok)
        trace = _traced_call(lambda: pk.verify_batch(insts, proofs))
        pk.close(), prm.close(), lay.close()
    split = {m.group(1).strip(): float(m.group(2)) for m in re.finditer(r"\[bzh_verify_batch\] (.{22}) +([0-9.]+) ms", trace)}
    points = re.search(r"\((\d+) points\)", trace)
    rates = [len(proofs) / s for s in secs]
    print(json.dumps({"points_where": args.where, "host_threads": args.threads, "batch": len(proofs), "k": args.k,
                      "call_seconds": [round(s, 6) for s in secs], "verifications_per_s": round(len(proofs) * 5 / sum(secs), 1),
                      "verifications_per_s_min_max": [round(min(rates), 1), round(max(rates), 1)],
                      "traced_call_ms": split, "points_on_device": int(points.group(1)) if points else 0}), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--role", choices=["drive", "make", "verify"], default="drive")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--k", type=int, default=14)
    ap.add_argument("--file")
    ap.add_argument("--where", choices=["host", "device"], default="host")
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--limit", type=int, default=240, help="seconds each child process may take")
    args = ap.parse_args()
    if args.role == "make":
        return make(args)
    if args.role == "verify":
        return verify(args)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "proofs.npz")
        base = [sys.executable, os.path.abspath(__file__), "--batch", str(args.batch), "--k", str(args.k), "--file", path]
        subprocess.run(base + ["--role", "make"], check=True, timeout=args.limit)
        rows = []
        for threads in (2, 16):
            for where in ("host", "device"):
                r = subprocess.run(base + ["--role", "verify", "--where", where, "--threads", str(threads)], check=True, timeout=args.limit,
                                   stdout=subprocess.PIPE, text=True)
                print(r.stdout.strip(), flush=True)
                rows.append(json.loads(r.stdout.strip().splitlines()[-1]))
    by = {(r["points_where"], r["host_threads"]): r for r in rows}
    h16, d16 = by[("host", 16)], by[("device", 16)]
    spread = h16["verifications_per_s_min_max"][1] - h16["verifications_per_s_min_max"][0]
    print(json.dumps({"summary": {"%s_%d" % k: v["verifications_per_s"] for k, v in by.items()},
                      "host_16_spread": round(spread, 1),
                      "device_no_slower_than_host_at_16_threads": d16["verifications_per_s"] >= h16["verifications_per_s"] - spread}))


if __name__ == "__main__":
    main()
