"""Game inputs to proofs, three ways, on the same commit, key, inputs and seeds: Board at k = 14 for 64 proofs and Shot at k = 11
for 128 proofs (Params::new SRS, the key's default quotient flavour).

Paths, one fresh process for every (circuit, path) setting:
  `one_call`    bzh_prove_shots_device / bzh_prove_boards_device: the synthesis kernels fill the key's own advice tensor, the
                instance rows are made on the device, one read-back at the end;
  `two_calls`   bzh_synthesize_*_with(BZH_SYNTH_DEVICE) into a device tensor of the caller's (one stream wait, the status words
                and the commitments come back, the instances are rebuilt on the host), then bzh_prove_batch_device_seeded on that
                tensor and those instances (uploaded and converted again);
  `host_synth`  bzh_synthesize_* on the host into host memory, then bzh_prove_batch_seeded with the advice uploaded by the call.
One warm-up call and five timed calls of the whole path, inputs marshalled inside; the median is the figure.  Every setting's proofs
are verified, and the three paths' first proofs are compared byte for byte by the driver.

    python tools/ubench_prove_game.py > profiles/prove_game_calls.json

It only prints: one JSON object per setting and a final summary.  A setting whose process ends abnormally stops the run.
"""
import argparse
import hashlib
import json
import os
import random
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "battlezips-halo2_amd"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

from ubench_ipa_open import timed  # noqa: E402

FQ = 0x40000000000000000000000000000000224698fc0994a8dd8c46eb2100000001
SHIPS = [(3, 3, True), (5, 4, False), (0, 1, False), (0, 5, True), (6, 1, False)]
CIRCUITS = {"board": (14, 64), "shot": (11, 128)}
PATHS = ("one_call", "two_calls", "host_synth")


def measure(args):
    import torch
    torch.zeros(1, device="cuda")                              # torch's HIP runtime initialises before the library's
    import bzh2
    from bzh2 import circuits as Cm, native as N, params as Pm
    from bzh2.game import BinaryValue
    shot = args.circuit == "shot"
    k, B = CIRCUITS[args.circuit]
    rng = random.Random(1000 * k + B)
    ships, state = Cm.board_witness(SHIPS, None)
    if shot:
        cells = [rng.randrange(100) for _ in range(B)]
        circuits = [Cm.ShotCircuit(state, rng.randrange(FQ), BinaryValue(1 << c), BinaryValue(state.value >> c & 1)) for c in cells]
    else:
        circuits = [Cm.BoardCircuit(ships, state, rng.randrange(FQ)) for _ in range(B)]
    seeds = [rng.randbytes(32) for _ in range(B)]
    ctx = bzh2.Context(0)
    lay = Cm.CircuitLayout(Cm.SHOT if shot else Cm.BOARD, k)
    prm = Pm.Params(ctx, k)
    pk = N.NativeProvingKey(ctx, lay.blob(), bzh2.CURVE_VESTA, params=prm)
    dev = torch.empty((B, lay.num_advice, lay.n, 4), dtype=torch.int64, device="cuda") if args.path == "two_calls" else None
    out = {}

    def once():
        if args.path == "one_call":
            fn = pk.prove_shots_device if shot else pk.prove_boards_device
            out["insts"], out["proofs"], st = fn(lay, circuits, seeds)
            assert not st.any()
        elif args.path == "two_calls":
            _, out["insts"] = lay.synthesize(circuits, ctx=ctx, device_ptr=dev.data_ptr(), where="device")
            out["proofs"], st = pk.prove_batch_device(None, out["insts"], seeds=seeds, device_ptr=dev.data_ptr())
            assert not st.any()
        else:
            adv, out["insts"] = lay.synthesize(circuits)
            out["proofs"] = pk.prove_batch(adv, out["insts"], None, seeds=seeds)

    secs = timed(once)
    verified = int(sum(pk.verify_batch(out["insts"], out["proofs"])))
    assert verified == B
    row = {"circuit": args.circuit, "k": k, "batch": B, "path": args.path, "proof_bytes": len(out["proofs"][0]), "verified": verified,
           "proofs_sha256": hashlib.sha256(b"".join(out["proofs"])).hexdigest(), "call_seconds": [round(s, 6) for s in secs],
           "median_seconds": round(statistics.median(secs), 6), "min_max_seconds": [round(min(secs), 6), round(max(secs), 6)]}
    print(json.dumps(row), flush=True)
    pk.close()
    prm.close()
    lay.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--role", choices=["drive", "measure"], default="drive")
    ap.add_argument("--circuit", choices=sorted(CIRCUITS), default="board")
    ap.add_argument("--path", choices=PATHS, default="one_call")
    ap.add_argument("--limit", type=int, default=240, help="seconds each child process may take")
    args = ap.parse_args()
    if args.role == "measure":
        return measure(args)
    rows = []
    for circuit in ("board", "shot"):
        for path in PATHS:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--role", "measure", "--circuit", circuit, "--path", path], check=True,
                               timeout=args.limit, stdout=subprocess.PIPE, text=True)
            print(r.stdout.strip(), flush=True)
            rows.append(json.loads(r.stdout.strip().splitlines()[-1]))
        same = len({r["proofs_sha256"] for r in rows[-3:]}) == 1
        assert same, "the three paths' proofs differ for " + circuit
    print(json.dumps({"summary": {"%s_k%d_b%d" % (r["circuit"], r["k"], r["batch"]) + ":" + r["path"]: r["median_seconds"] for r in rows}}))


if __name__ == "__main__":
    main()
