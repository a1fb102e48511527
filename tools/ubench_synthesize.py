#!/usr/bin/env python3
"""Witness synthesis, host threads against the device kernels (bzh_synthesize_*_with): 64 Board witnesses at k = 14 and 128 Shot
witnesses at k = 11 into a device tensor.  Settings: `host2` / `host16` (BZH_SYNTH_HOST with BZH_HOST_THREADS = 2 / 16: host
threads, pinned compact block, expansion kernel) and `device` (BZH_SYNTH_DEVICE).  One fresh process per (circuit, setting), each
under its own time limit: one warm-up call and five timed calls, each followed by a stream synchronisation; the device setting
makes one more call under BZH_PROVE_TRACE=1, whose `[bzh_synthesize]` line gives the event times of the zero fill and the three
kernels.  Prints one JSON line per (circuit, setting) and writes them to --out.

    python tools/ubench_synthesize.py --out profiles/synth_device_ubench.json
"""
import argparse
import json
import os
import random
import re
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "battlezips-halo2_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)
FQ = 0x40000000000000000000000000000000224698fc0994a8dd8c46eb2100000001
CASES = {"board": (14, 64), "shot": (11, 128)}
SETTINGS = {"host2": ("host", 2), "host16": ("host", 16), "device": ("device", 0)}


def child(circuit, setting):
    where, threads = SETTINGS[setting]
    if threads:
        os.environ["BZH_HOST_THREADS"] = str(threads)
    import torch
    torch.zeros(1, device="cuda")
    import bzh2
    from bzh2 import circuits as Cm
    from bzh2.game import BinaryValue
    k, batch = CASES[circuit]
    rng = random.Random(5)
    ships, state = Cm.board_witness([(3, 3, True), (5, 4, False), (0, 1, False), (0, 5, True), (6, 1, False)], None)
    if circuit == "board":
        lay = Cm.CircuitLayout(Cm.BOARD, k)
        circuits = [Cm.BoardCircuit(ships, state, rng.randrange(FQ)) for _ in range(batch)]
    else:
        lay = Cm.CircuitLayout(Cm.SHOT, k)
        circuits = [Cm.ShotCircuit(state, rng.randrange(FQ), Cm.shot_serialize([rng.randrange(10)], [rng.randrange(10)]), BinaryValue(0)) for _ in range(batch)]
    dev = torch.empty((batch, lay.num_advice, lay.n, 4), dtype=torch.int64, device="cuda")
    times = []
    with bzh2.Context(0) as ctx:
        def call():
            t0 = time.perf_counter()
            lay.synthesize(circuits, ctx=ctx, device_ptr=dev.data_ptr(), threads=threads, where=where)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3
        call()
        times = [call() for _ in range(5)]
        trace = None
        if where == "device":
            r, w = os.pipe()
            saved = os.dup(2)
            os.dup2(w, 2)
            os.environ["BZH_PROVE_TRACE"] = "1"
            try:
                call()
            finally:
                del os.environ["BZH_PROVE_TRACE"]
                os.dup2(saved, 2)
                os.close(w)
            text = os.read(r, 1 << 16).decode(errors="replace")
            m = re.search(r"\[bzh_synthesize\] device (.*)", text)
            if m:
                trace = {kv.split("=")[0]: float(kv.split("=")[1]) for kv in m.group(1).split()}
    lay.close()
    print(json.dumps({"circuit": circuit, "k": k, "batch": batch, "setting": setting, "calls_ms": [round(t, 3) for t in times],
                      "median_ms": round(statistics.median(times), 3), "spread_ms": round(max(times) - min(times), 3), "trace": trace}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", nargs=2)
    ap.add_argument("--out", default=None)
    ap.add_argument("--timeout", type=int, default=240)
    a = ap.parse_args()
    if a.child:
        return child(*a.child)
    lines = []
    for circuit in CASES:
        for setting in SETTINGS:
            res = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", circuit, setting], capture_output=True, text=True, timeout=a.timeout)
            if res.returncode != 0:       # a fault or an abort: start nothing more on the device
                sys.stderr.write(res.stdout[-2000:] + res.stderr[-2000:])
                sys.exit("ubench_synthesize: %s / %s ended with status %d" % (circuit, setting, res.returncode))
            line = [ln for ln in res.stdout.splitlines() if ln.startswith("{")][-1]
            print(line, flush=True)
            lines.append(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
