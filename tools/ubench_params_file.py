"""Reading a params file against making the SRS: Params.from_bytes at each check level ("points", "lagrange", "full") against a cold
Params::new (cache_dir="") and a hit of the BZSRS1 cache file, at k = 14 and k = 17.

One fresh process per setting, each under its own time limit: one warm-up call and five timed calls.  The file read back is the
one Params(ctx, k).to_bytes() gives; to_bytes is timed the same way.

    python tools/ubench_params_file.py [--ks 14,17]

It only prints: one JSON object per setting.  A setting whose process ends abnormally stops the run.  Nothing here is a recorded
measurement until the output is kept under profiles/.
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

SETTINGS = ["from_bytes:points", "from_bytes:lagrange", "from_bytes:full", "to_bytes", "cold", "cache_hit"]


def measure(args):
    import bzh2
    from bzh2 import params as Pm
    with bzh2.Context(0) as ctx, tempfile.TemporaryDirectory() as cache:
        base = Pm.Params(ctx, args.k, cache_dir=cache)       # also leaves the cache file for the cache_hit setting
        data = base.to_bytes()
        if args.setting.startswith("from_bytes:"):
            level = args.setting.split(":")[1]

            def once():
                Pm.Params.from_bytes(ctx, data, check=level).close()
        elif args.setting == "to_bytes":
            once = base.to_bytes
        elif args.setting == "cold":
            def once():
                Pm.Params(ctx, args.k, cache_dir="").close()
        else:
            def once():
                p = Pm.Params(ctx, args.k, cache_dir=cache)
                assert p.points(want_g=False, want_lagrange=False)[4], "the cache file was not used"
                p.close()
        once()                                               # warm-up: code objects, workspaces, the pinned buffers
        secs = []
        for _ in range(5):
            t0 = time.perf_counter()
            once()
            secs.append(time.perf_counter() - t0)
        base.close()
    print(json.dumps({"setting": args.setting, "k": args.k, "file_bytes": len(data), "call_seconds": [round(s, 4) for s in secs],
                      "mean_seconds": round(sum(secs) / 5, 4), "min_max_seconds": [round(min(secs), 4), round(max(secs), 4)]}), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--role", choices=["drive", "measure"], default="drive")
    ap.add_argument("--ks", default="14,17")
    ap.add_argument("--k", type=int, default=14)
    ap.add_argument("--setting", choices=SETTINGS, default=SETTINGS[0])
    ap.add_argument("--limit", type=int, default=300, help="seconds each child process may take")
    args = ap.parse_args()
    if args.role == "measure":
        return measure(args)
    for k in [int(v) for v in args.ks.split(",")]:
        for setting in SETTINGS:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--role", "measure", "--k", str(k), "--setting", setting], check=True,
                               timeout=args.limit, stdout=subprocess.PIPE, text=True)
            print(r.stdout.strip(), flush=True)


if __name__ == "__main__":
    main()
