#!/usr/bin/env python3
"""Is one accumulated opening check per batch (bzh_verify_records_accumulated) faster than one check per record
(bzh_verify_records_device)?

Per shape -- 64 and 1024 Board records at k = 14, 128 and 1024 Shot records at k = 11 -- a process of its own makes up to 64 real
proofs (bzh_prove_batch_seeded), encodes them as binary records, tiles them to the batch size and verifies the batch with both
calls in ONE process, alternating, 1 warm-up call and 5 timed calls each, on one key and one ctx.  Then one failing batch (the
last record's opening scalar f with its low bit flipped): the accumulated call falls back to the per-record check (path = 1), so
its time shows what a failing batch costs.

    python tools/ubench_verify_accumulated.py > profiles/verify_accumulated.json

It only prints: one JSON object per shape.  A shape whose process ends abnormally stops the run.
"""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "battlezips-halo2_amd"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

SHAPES = [("board", 14, 64), ("board", 14, 1024), ("shot", 11, 128), ("shot", 11, 1024)]


def shape(args):
    import bzh2
    from bzh2 import native as N, params as Pm, wire as W
    from ubench_verify_records import _games, _layout
    made = min(args.batch, 64)
    n_inputs = 4 if args.kind == "shot" else 2
    with bzh2.Context(0) as ctx:
        lay = _layout(args.kind, args.k)
        prm = Pm.Params(ctx, args.k)
        pk = N.NativeProvingKey(ctx, lay.blob(), bzh2.CURVE_VESTA, params=prm)
        adv, insts = lay.synthesize(_games(args.kind, made))
        seeds = [hashlib.blake2b(b"ubench_verify_accumulated %d" % i, digest_size=32).digest() for i in range(made)]
        proofs = pk.prove_batch(adv, insts, None, seeds=seeds)
        vk = N.NativeVerifyingKey.from_pk(pk)
        pk.close()
        tag = W.KIND_BOARD if args.kind == "board" else 1
        base = [W.BattleZipsRecord([int(v) for v in i[0]], p, tag, b).to_fixed(len(p)) for b, (i, p) in enumerate(zip(insts, proofs))]
        recs = [base[b % made] for b in range(args.batch)]
        bad_proof = proofs[(args.batch - 1) % made]
        at = len(bad_proof) - 32
        bad_proof = bad_proof[:at] + bytes([bad_proof[at] ^ 1]) + bad_proof[at + 1:]
        failing = recs[:-1] + [W.BattleZipsRecord([int(v) for v in insts[(args.batch - 1) % made][0]], bad_proof, tag, 0).to_fixed(len(bad_proof))]

        def per_record(rr):
            return vk.verify_records(ctx, prm, rr, n_inputs)[0], None

        def accumulated(rr):
            res, _, path = vk.verify_records_accumulated(ctx, prm, rr, n_inputs, seed=os.urandom(32))
            return res, path

        def timed(rr, want, want_path):
            secs = {"per_record": [], "accumulated": []}
            for it in range(6):                                             # call 0 of each is the warm-up
                for name, fn in (("per_record", per_record), ("accumulated", accumulated)):
                    t0 = time.perf_counter()
                    res, path = fn(rr)
                    dt = time.perf_counter() - t0
                    assert res == want and path in (None, want_path), (name, path)
                    if it:
                        secs[name].append(dt)
            return secs

        ok = timed(recs, [True] * args.batch, 0)
        fail = timed(failing, [True] * (args.batch - 1) + [False], 1)
        vk.close(), prm.close(), lay.close()

    def row(s):
        return {"call_seconds": [round(x, 6) for x in s], "verifications_per_s": round(args.batch * len(s) / sum(s), 1)}
    print(json.dumps({"circuit": args.kind, "k": args.k, "batch": args.batch, "distinct_proofs": made,
                      "valid_batch": {n: row(s) for n, s in ok.items()},
                      "failing_batch_path_1": {n: row(s) for n, s in fail.items()}}), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--role", choices=["drive", "shape"], default="drive")
    ap.add_argument("--kind", choices=["shot", "board"], default="shot")
    ap.add_argument("--k", type=int, default=11)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--limit", type=int, default=400, help="seconds each shape's process may take")
    args = ap.parse_args()
    if args.role == "shape":
        return shape(args)
    for kind, k, batch in SHAPES:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--role", "shape", "--kind", kind, "--k", str(k), "--batch", str(batch)],
                           check=True, timeout=args.limit, stdout=subprocess.PIPE, text=True)
        print(r.stdout.strip(), flush=True)


if __name__ == "__main__":
    main()
