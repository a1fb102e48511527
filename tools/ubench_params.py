"""Cold Params::new (cache_dir="") with the generators made on the host or on the device: bzh_params_create_with under
BZH_GENERATORS_HOST and BZH_GENERATORS_DEVICE, with BZH_HOST_THREADS = 2 (a rank's share of a 16-core box under an 8-rank
launcher) and 16, at k = 14 and k = 17.

One fresh process per setting (a launcher sets BZH_HOST_THREADS once per process), each under its own time limit: one warm-up
call and five timed calls, then one more call with BZH_PROVE_TRACE=1 whose `[bzh_params_create]` lines give the split between
generators, group FFT and table upload plus precompute, and the HIP-event times of k_hash_to_field and k_map_to_curve.

    python tools/ubench_params.py [--ks 14,17] > profiles/params_generators.json

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


def measure(args):
    import bzh2
    from bzh2 import params as Pm
    os.environ["BZH_HOST_THREADS"] = str(args.threads)     # read by the library at every call
    with bzh2.Context(0) as ctx:
        def once():
            Pm.Params(ctx, args.k, cache_dir="", generators=args.where).close()
        once()                                             # warm-up: code objects, workspaces, the pinned ring
        secs = []
        for _ in range(5):
            t0 = time.perf_counter()
            once()
            secs.append(time.perf_counter() - t0)
        trace = _traced_call(once)
    split = {m.group(1).strip(): float(m.group(2)) for m in re.finditer(r"\[bzh_params_create\] (.{22}) +([0-9.]+) ms", trace)}
    print(json.dumps({"generators": args.where, "host_threads": args.threads, "k": args.k, "call_seconds": [round(s, 4) for s in secs],
                      "mean_seconds": round(sum(secs) / 5, 4), "min_max_seconds": [round(min(secs), 4), round(max(secs), 4)],
                      "traced_call_ms": split}), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--role", choices=["drive", "measure"], default="drive")
    ap.add_argument("--ks", default="14,17")
    ap.add_argument("--k", type=int, default=14)
    ap.add_argument("--where", choices=["host", "device"], default="host")
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--limit", type=int, default=300, help="seconds each child process may take")
    args = ap.parse_args()
    if args.role == "measure":
        return measure(args)
    rows = []
    for k in [int(v) for v in args.ks.split(",")]:
        for threads in (2, 16):
            for where in ("host", "device"):
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--role", "measure", "--k", str(k), "--where", where,
                                    "--threads", str(threads)], check=True, timeout=args.limit, stdout=subprocess.PIPE, text=True)
                print(r.stdout.strip(), flush=True)
                rows.append(json.loads(r.stdout.strip().splitlines()[-1]))
    by = {(r["k"], r["generators"], r["host_threads"]): r for r in rows}
    verdict = {}
    for k in sorted({r["k"] for r in rows}):
        h16, d16 = by[(k, "host", 16)], by[(k, "device", 16)]
        spread = h16["min_max_seconds"][1] - h16["min_max_seconds"][0]
        verdict["k%d" % k] = {"host_16_spread_s": round(spread, 4),
                              "device_no_slower_than_host_at_16_threads": d16["mean_seconds"] <= h16["mean_seconds"] + spread}
    print(json.dumps({"summary": {"k%d_%s_%d" % key: v["mean_seconds"] for key, v in by.items()}, "rule": verdict}))


if __name__ == "__main__":
    main()
