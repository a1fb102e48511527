"""bzh_commitments_batch_device next to the instance, advice and lookup phases of bzh_prove_batch: the Board circuit at k = 14
for 64 proofs (Vesta's scalar field), the advice a synthesized witness in a BZH_MEM_DEVICE buffer in Montgomery form, the
instance and the draws in device memory, every output a device buffer.

One process and one proving key.  For the key as the workload builds it (with g_lagrange when its parameters carry the table)
and then for the same key without g_lagrange: one warm-up call and five timed calls of bzh_commitments_batch_device, a fresh
device-resident transcript batch that has absorbed vk_repr for every call and one stream wait at its end.  Then one
bzh_prove_batch of the same shape on the same key (bench.py's proof_k14 workload) under BZH_PROVE_TRACE=1, whose `instance`,
`advice` and `lookup` marks are the host-transcript path's times for the same work on the same commit; `lookup` there also
covers extend_witness (the witness on the extended coset), which is the vanishing leaf's work here.  The trace waits for the
device at every mark, the call only at its end.

    python tools/ubench_commitments.py > profiles/commitments_device_calls.json

It only prints: one JSON object.
"""
import argparse
import json
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "battlezips-halo2_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

from ubench_ipa_open import timed, traced  # noqa: E402
from ubench_products import board_blob  # noqa: E402

SHAPE = ("n", "usable", "blinding_factors", "num_advice", "num_instance", "lookups", "draws_per_proof", "proof_bytes")
SAME_WORK = ("instance", "advice", "lookup")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--k", type=int, default=14)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--plan-only", action="store_true", help="print the call's shape and stop (needs no GPU)")
    args = ap.parse_args()
    if not args.plan_only:
        import torch
        torch.zeros(1, device="cuda")                          # torch's HIP runtime initialises before the library's
    import bzh2
    B, k = args.batch, args.k
    shape = bzh2.commitments_plan(bzh2.CURVE_VESTA, board_blob(k))
    n, _, _, na, ni, nl, nd, grow = shape
    row = {"k": k, "batch": B, **dict(zip(SHAPE, shape))}
    if args.plan_only:
        print(json.dumps(row), flush=True)
        return
    # the key and the ctx of bench.py's workload, so that the traced prove below runs on the key the calls ran on
    os.chdir(ROOT)
    argv, sys.argv = sys.argv, ["bench.py", "--no-cpu-baseline", "--concurrency", "1"]
    import bench
    sys.argv = argv
    ctx = bzh2.Context(0)
    wl = bench.Workload("proof_k%d" % k, ctx, torch.device("cuda:0"), 1, concurrency=1, batch=B)
    r = wl.runner
    pk, wctx = r.pk, r.ctxs[0]
    assert pk.commitments_plan() == shape
    rng = np.random.default_rng(100 * k + B)
    cid, MONT = bzh2.CURVE_VESTA, bzh2.FORM_MONTGOMERY
    p_mod = pk.p
    R = (1 << 256) % p_mod

    # a witness the lookups hold for: the workload's own synthesis, advice on the device in Montgomery form
    _, insts = r.layout.synthesize(r._circuits(0, B), ctx=wctx, device_ptr=r.adv[0].data_ptr(), threads=4)
    rows = max([len(col) for cols in insts for col in cols] + [0])
    inst = np.zeros((B, max(ni, 1), max(rows, 1), 4), dtype=np.uint64)
    for b, cols in enumerate(insts):
        for i, col in enumerate(cols):
            for j, v in enumerate(col):
                inst[b, i, j] = bzh2.int_to_limbs(int(v) * R % p_mod)
    d_inst = torch.from_numpy(inst.view(np.int64)).to("cuda")
    d_rng = torch.from_numpy(np.frombuffer(rng.bytes(B * nd * 64), dtype=np.uint8).copy()).to("cuda")
    sizes = {"advice": B * na * n, "instance": B * ni * n, "lookup_compressed": B * nl * 2 * n, "lookup_permuted": B * nl * 2 * n,
             "advice_polys": B * na * n, "instance_polys": B * ni * n, "lookup_polys": B * nl * 2 * n, "advice_blinds": B * na,
             "lookup_blinds": B * nl * 2, "theta": B, "beta": B, "gamma": B}
    d_out = {nm: torch.zeros(max(sz, 1) * 4, dtype=torch.int64, device="cuda") for nm, sz in sizes.items()}
    out = {nm: t.data_ptr() for nm, t in d_out.items() if sizes[nm]}
    d_st = torch.zeros(B, dtype=torch.uint8, device="cuda")
    vk = np.stack([bzh2.int_to_limbs(pk.vk_repr()[0])] * B).reshape(B, 1, 4)

    def once():
        with bzh2.TranscriptBatch(cid, B, grow, ctx=wctx) as tb:
            tb.common_scalars(vk)
            tb.commitments(pk, r.adv[0].data_ptr(), d_inst.data_ptr(), d_rng.data_ptr(), form=MONT, mem=bzh2.MEM_DEVICE, out=out,
                           status=d_st.data_ptr(), instance_rows=rows, rng_stride=64 * nd)
            wctx.sync()

    lagrange = getattr(getattr(pk, "_params", None), "bases_lagrange", None)
    settings = [("g_lagrange", lagrange)] if lagrange is not None else []
    settings.append(("coefficients", None))
    for name, table in settings:
        pk.set_lagrange(table)
        secs = timed(once)
        row[name] = {"call_seconds": [round(s, 6) for s in secs], "mean_seconds": round(sum(secs) / 5, 6),
                     "min_max_seconds": [round(min(secs), 6), round(max(secs), 6)], "flagged_proofs": int(d_st.cpu().numpy().astype(bool).sum())}
    pk.set_lagrange(lagrange)
    del d_out

    # the host-transcript path: one traced prove of the same shape on the same key (a warm-up prove first)
    def prove():
        _, ins = r.layout.synthesize(r._circuits(0, B), ctx=wctx, device_ptr=r.adv[0].data_ptr(), threads=4)
        blob = r.np_rng[0].bytes(r.rng_bytes * B)
        r.pks[0].prove_batch(None, ins, [blob[i * r.rng_bytes:(i + 1) * r.rng_bytes] for i in range(B)], device_ptr=r.adv[0].data_ptr())
    prove()
    marks = {}
    for name, ms in re.findall(r"\[bzh_prove_batch\]\s+(\S+)\s+([0-9.]+) ms", traced(prove)):
        marks[name] = marks.get(name, 0.0) + float(ms)
    row["prove_trace_ms"] = {name: round(v, 3) for name, v in marks.items() if name.startswith("lk:") or name in SAME_WORK}
    if all(name in marks for name in SAME_WORK):
        row["prove_trace_same_work_seconds"] = round(sum(marks[name] for name in SAME_WORK) / 1e3, 6)
    print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
