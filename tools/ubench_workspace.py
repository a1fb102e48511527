"""BZH_WORKSPACE_EXTENDED against BZH_WORKSPACE_COSETWISE (bzh_pk_workspace_select): bzh_prove_batch_seeded on the Board circuit,
bench.py's proof workload and key, the synthesized witness in device memory.

Settings, one fresh process each: `extended` and `cosetwise` at k = 14 for 64 proofs -- one warm-up call and five timed calls,
the median is the figure, and the two settings' proofs must be the same bytes (each row carries their SHA-256) and verify --
and `cosetwise_k17`, ONE call at k = 17 for 32 proofs (a batch the extended layout's cosets, 17 GiB by bzh_workspace_plan, keep
the bench from running), timed as it is, warm-up and all.  Every row carries the plan's figures for its setting and the device
bytes the key holds after its calls (bzh_pk_device_bytes: key + arena).

    python tools/ubench_workspace.py > profiles/workspace_modes.json

It only prints: one JSON object per setting and a final summary.  A setting whose process ends abnormally stops the run.
Each child has a time limit (LIMITS below); the k = 17 child's covers creating the 2^17 Params and key, which nobody has timed
in a fresh process: a child that is killed at its limit needed longer, raise --limit-k17.
"""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "battlezips-halo2_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

SETTINGS = {"extended": (14, 64, 0, 5), "cosetwise": (14, 64, 1, 5), "cosetwise_k17": (17, 32, 1, 0)}   # k, batch, mode, timed calls
# seconds a setting's child process may take.  The k = 17 child also creates the 2^17 Params (generators, g_lagrange, window
# tables) and the key before its one call; how long that takes in a fresh process has not been measured, so its limit is a
# generous guess: a child killed at it needed longer, it did not hang -- raise --limit-k17.
LIMITS = {"extended": 420, "cosetwise": 420, "cosetwise_k17": 1500}


def measure(args):
    import torch
    torch.zeros(1, device="cuda")                              # torch's HIP runtime initialises before the library's
    import bzh2
    from bzh2 import native as N
    k, B, mode, calls = SETTINGS[args.setting]
    os.chdir(ROOT)
    argv, sys.argv = sys.argv, ["bench.py", "--no-cpu-baseline", "--concurrency", "1"]
    import bench
    sys.argv = argv
    ctx = bzh2.Context(0)
    wl = bench.Workload("proof_k%d" % k, ctx, torch.device("cuda:0"), 1, concurrency=1, batch=B)
    r = wl.runner
    pk, wctx = r.pk, r.ctxs[0]
    # The advice tensor is this tool's own, B proofs of it: the bench caps the runner's batch -- and with it the runner's tensor --
    # at 8 for k = 17, and bzh_synthesize_* / bzh_prove_batch take a bare pointer whose capacity nothing checks.
    adv = torch.zeros((B, r.layout.num_advice, r.layout.n, 4), dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    assert adv.shape[0] == B and adv.numel() * 8 == B * r.layout.num_advice * (1 << k) * 32, (tuple(adv.shape), B, k)
    _, insts = r.layout.synthesize(r._circuits(0, B), ctx=wctx, device_ptr=adv.data_ptr(), threads=4)
    assert len(insts) == B
    seeds = [bytes((17 * b + i) & 0xff for i in range(32)) for b in range(B)]
    pk.workspace_select(mode)
    assert pk.workspace_selected() == mode
    got, secs = [], []
    for _ in range(1 + calls):
        wctx.sync()
        t0 = time.perf_counter()
        got[:] = pk.prove_batch(None, insts, None, device_ptr=adv.data_ptr(), seeds=seeds, ctx=wctx)
        secs.append(time.perf_counter() - t0)
    timed_secs = secs[1:] or secs
    row = {"setting": args.setting, "k": k, "batch": B, "mode": ["EXTENDED", "COSETWISE"][mode], "quotient_flavour": pk.quotient_selected()[0],
           "first_call_seconds": round(secs[0], 6), "call_seconds": [round(s, 6) for s in timed_secs],
           "median_seconds": round(statistics.median(timed_secs), 6), "proof_bytes": len(got[0]),
           "proofs_sha256": hashlib.sha256(b"".join(got)).hexdigest(), "verified": int(sum(pk.verify_batch(insts, got, ctx=wctx))),
           "plan": N.workspace_plan_items(bzh2.CURVE_VESTA, pk.blob, B, mode)}
    if hasattr(pk, "device_bytes"):
        row["key_device_bytes"] = pk.device_bytes()
    assert row["verified"] == B, row
    print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--role", choices=["drive", "measure"], default="drive")
    ap.add_argument("--setting", choices=sorted(SETTINGS), default="cosetwise")
    ap.add_argument("--limit", type=int, default=None, help="seconds each k = 14 child process may take (default %d)" % LIMITS["extended"])
    ap.add_argument("--limit-k17", type=int, default=None, help="seconds the k = 17 child may take, key creation included (default %d)" % LIMITS["cosetwise_k17"])
    args = ap.parse_args()
    if args.role == "measure":
        return measure(args)
    rows = []
    for setting in ("extended", "cosetwise", "cosetwise_k17"):
        limit = (args.limit_k17 if setting == "cosetwise_k17" else args.limit) or LIMITS[setting]
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--role", "measure", "--setting", setting], check=True,
                           timeout=limit, stdout=subprocess.PIPE, text=True)
        print(r.stdout.strip(), flush=True)
        rows.append(json.loads(r.stdout.strip().splitlines()[-1]))
    same = rows[0]["proofs_sha256"] == rows[1]["proofs_sha256"]
    print(json.dumps({"summary": {r["setting"]: r["median_seconds"] for r in rows}, "k14_proofs_identical": same}))
    assert same, "the two modes' proofs differ"


if __name__ == "__main__":
    main()
