#!/usr/bin/env python3
"""Does verifying records in one device-resident call (bzh_verify_records_device) help a few-core rank?

Makes 64 real ShotCircuit proofs at k = 11 and 64 real BoardCircuit proofs at k = 14 once (bzh_prove_batch_seeded), encodes them
as binary records (bzh_record_encode) and verifies each set two ways -- 1 warm-up call and 5 timed calls each:
    two_step   bzh_record_decode per record, then bzh_verify_batch_vk_with(.., BZH_VERIFY_PASS_DEVICE, ..) on the decoded batch
    one_call   bzh_verify_records_device on the record bytes
at BZH_HOST_THREADS = 2 and = 16.  Every setting runs in a process of its own under its own time limit.

    python tools/ubench_verify_records.py > profiles/verify_records.json

It only prints: one JSON object per setting and a summary object per circuit.  A setting whose process ends abnormally stops
the run.
"""
import argparse
import json
import os
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
CIRCUITS = {"shot": 11, "board": 14}


def _layout(kind, k):
    from bzh2 import circuits as Cm
    return Cm.CircuitLayout(Cm.SHOT if kind == "shot" else Cm.BOARD, k)


def _games(kind, count):
    from bzh2 import circuits as Cm
    from bzh2.game import BinaryValue
    ships, state = Cm.board_witness(DECK, None)
    trap = lambda i: (0x9e3779b97f4a7c15 * (i + 1) + (i << 130)) % FQ   # noqa: E731
    if kind == "board":
        return [Cm.BoardCircuit(ships, state, trap(i)) for i in range(count)]
    cells = {(x + (0 if z else j), y + (j if z else 0)) for (x, y, z), ln in zip(DECK, (5, 4, 3, 3, 2)) for j in range(ln)}
    out = []
    for i in range(count):
        x, y = i % 10, (i // 10) % 10
        out.append(Cm.ShotCircuit(state, trap(i), Cm.shot_serialize([x], [y]), BinaryValue.from_u8(1 if (x, y) in cells else 0)))
    return out


def make(args):
    import hashlib
    import numpy as np
    import bzh2
    from bzh2 import native as N, params as Pm, wire as W
    with bzh2.Context(0) as ctx:
        lay = _layout(args.kind, args.k)
        prm = Pm.Params(ctx, args.k)
        pk = N.NativeProvingKey(ctx, lay.blob(), bzh2.CURVE_VESTA, params=prm)
        adv, insts = lay.synthesize(_games(args.kind, args.batch))
        seeds = [hashlib.blake2b(b"ubench_verify_records %d" % i, digest_size=32).digest() for i in range(args.batch)]
        proofs = pk.prove_batch(adv, insts, None, seeds=seeds)
        assert all(pk.verify_batch(insts, proofs)), "a made proof does not verify (is the hit flag right for the deck?)"
        kind_tag = W.KIND_BOARD if args.kind == "board" else 1
        recs = [W.BattleZipsRecord([int(v) for v in i[0]], p, kind_tag, b).to_fixed(len(p)) for b, (i, p) in enumerate(zip(insts, proofs))]
        np.save(args.file, np.array([np.frombuffer(r, dtype=np.uint8) for r in recs]))
        pk.close(), prm.close(), lay.close()


def verify(args):
    import numpy as np
    import bzh2
    from bzh2 import native as N, params as Pm, wire as W
    recs = [bytes(r.tobytes()) for r in np.load(args.file)]
    n_inputs = 4 if args.kind == "shot" else 2
    os.environ["BZH_HOST_THREADS"] = str(args.threads)     # read by the library at every call
    with bzh2.Context(0) as ctx:
        lay = _layout(args.kind, args.k)
        prm = Pm.Params(ctx, args.k)
        vk = N.NativeVerifyingKey.create(ctx, prm, lay.blob())

        def two_step():
            dec = [W.BattleZipsRecord.from_fixed(r) for r in recs]
            return vk.verify_batch(ctx, prm, [[d.commitment] for d in dec], [d.proof for d in dec], pass_where=N.VERIFY_PASS_DEVICE)

        def one_call():
            return vk.verify_records(ctx, prm, recs, n_inputs)[0]

        fn = two_step if args.how == "two_step" else one_call
        assert all(fn())                                    # warm-up
        secs = []
        for _ in range(5):
            t0 = time.perf_counter()
            ok = fn()
            secs.append(time.perf_counter() - t0)
            assert all(ok)
        vk.close(), prm.close(), lay.close()
    rates = [len(recs) / s for s in secs]
    print(json.dumps({"circuit": args.kind, "k": args.k, "how": args.how, "host_threads": args.threads, "batch": len(recs),
                      "call_seconds": [round(s, 6) for s in secs], "verifications_per_s": round(len(recs) * 5 / sum(secs), 1),
                      "verifications_per_s_min_max": [round(min(rates), 1), round(max(rates), 1)]}), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--role", choices=["drive", "make", "verify"], default="drive")
    ap.add_argument("--kind", choices=sorted(CIRCUITS), default="shot")
    ap.add_argument("--k", type=int, default=0)
    ap.add_argument("--batch", type=int, default=64, help="records to make")
    ap.add_argument("--file")
    ap.add_argument("--how", choices=["two_step", "one_call"], default="one_call")
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--limit", type=int, default=240, help="seconds each child process may take")
    args = ap.parse_args()
    if args.role == "make":
        return make(args)
    if args.role == "verify":
        return verify(args)
    with tempfile.TemporaryDirectory() as tmp:
        for kind, k in CIRCUITS.items():
            path = os.path.join(tmp, kind + ".npy")
            base = [sys.executable, os.path.abspath(__file__), "--kind", kind, "--k", str(k), "--batch", str(args.batch), "--file", path]
            subprocess.run(base + ["--role", "make"], check=True, timeout=args.limit)
            rows = []
            for threads in (2, 16):
                for how in ("two_step", "one_call"):
                    r = subprocess.run(base + ["--role", "verify", "--how", how, "--threads", str(threads)], check=True, timeout=args.limit,
                                       stdout=subprocess.PIPE, text=True)
                    print(r.stdout.strip(), flush=True)
                    rows.append(json.loads(r.stdout.strip().splitlines()[-1]))
            print(json.dumps({"summary": {"%s_%d" % (r["how"], r["host_threads"]): r["verifications_per_s"] for r in rows}, "circuit": kind,
                              "k": k}), flush=True)


if __name__ == "__main__":
    main()
