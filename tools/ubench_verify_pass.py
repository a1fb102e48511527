#!/usr/bin/env python3
"""Does running the verifier's per-proof pass on the device (BZH_VERIFY_PASS_DEVICE) help, and at which batch size?

Makes 64 real BoardCircuit proofs at k = 14 once (bzh_prove_batch_seeded) and verifies them as a batch of 64 and, repeated, as
a batch of 2 048: bzh_verify_batch -- 1 warm-up call and 5 timed calls -- with the per-proof pass on host threads
(BZH_VERIFY_PASS_HOST) and on the device (BZH_VERIFY_PASS_DEVICE), at BZH_HOST_THREADS = 2 and = 16.  Every setting runs in a
process of its own under its own time limit; one more call per setting runs with BZH_PROVE_TRACE=1 and its
`[bzh_verify_batch]` lines are kept (on the device path: vd:stage+decompress, vd:transcripts, vd:scalars -- HIP events around
k_vp_scalars, with the tape's length and inversion count --, vd:ipa check).

    python tools/ubench_verify_pass.py [--k 14] > profiles/verify_pass.json

It only prints: one JSON object per setting and a final summary object per batch size, whose last field says which way
DESIGN.md section 7's rule for the default fell.  A setting whose process ends abnormally stops the run.
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
        seeds = [hashlib.blake2b(b"ubench_verify_pass %d" % i, digest_size=32).digest() for i in range(args.batch)]
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
    reps = -(-args.verify_batch // len(proofs))              # the made proofs, repeated up to the batch size
    proofs, insts = (proofs * reps)[:args.verify_batch], (insts * reps)[:args.verify_batch]
    os.environ["BZH_HOST_THREADS"] = str(args.threads)     # read by the library at every call
    with bzh2.Context(0) as ctx:
        lay, prm, pk = _key(ctx, args.k)
        pk.verify_pass_select(N.VERIFY_PASS_DEVICE if args.where == "device" else N.VERIFY_PASS_HOST)
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
    tape = re.search(r"(\d+) ops, (\d+) inversions", trace)
    rates = [len(proofs) / s for s in secs]
    print(json.dumps({"pass_where": args.where, "host_threads": args.threads, "batch": len(proofs), "k": args.k,
                      "call_seconds": [round(s, 6) for s in secs], "verifications_per_s": round(len(proofs) * 5 / sum(secs), 1),
                      "verifications_per_s_min_max": [round(min(rates), 1), round(max(rates), 1)],
                      "traced_call_ms": split, "tape_ops": int(tape.group(1)) if tape else 0,
                      "tape_inversions": int(tape.group(2)) if tape else 0}), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--role", choices=["drive", "make", "verify"], default="drive")
    ap.add_argument("--batch", type=int, default=64, help="proofs to make")
    ap.add_argument("--verify-batch", type=int, default=64, help="proofs per bzh_verify_batch call (the made ones, repeated)")
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
        for vb in (64, 2048):
            rows = []
            for threads in (2, 16):
                for where in ("host", "device"):
                    r = subprocess.run(base + ["--role", "verify", "--where", where, "--threads", str(threads), "--verify-batch", str(vb)],
                                       check=True, timeout=args.limit, stdout=subprocess.PIPE, text=True)
                    print(r.stdout.strip(), flush=True)
                    rows.append(json.loads(r.stdout.strip().splitlines()[-1]))
            by = {(r["pass_where"], r["host_threads"]): r for r in rows}
            h16, d16 = by[("host", 16)], by[("device", 16)]
            spread = h16["verifications_per_s_min_max"][1] - h16["verifications_per_s_min_max"][0]
            print(json.dumps({"summary": {"%s_%d" % k: v["verifications_per_s"] for k, v in by.items()}, "batch": vb,
                              "host_16_spread": round(spread, 1),
                              "device_no_slower_than_host_at_16_threads": d16["verifications_per_s"] >= h16["verifications_per_s"] - spread}),
                  flush=True)

if __name__ == "__main__":
    main()
