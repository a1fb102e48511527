"""bzh_grand_products_batch_device next to the grand-product phase of bzh_prove_batch: the Board circuit's own shape (its advice and
instance columns, its permutation sets and lookups) at k = 14 for 64 proofs (Vesta's scalar field), every operand a
BZH_MEM_DEVICE buffer in Montgomery form, beta and gamma in device memory.  The operands are uniform values, not a witness; the
work does not depend on them (no product closes, so every proof is flagged).

One process and one proving key: one warm-up call and five timed calls of bzh_grand_products_batch_device, a fresh device-resident
transcript batch for every call and one stream wait at its end; then one bzh_prove_batch of the same shape on the same key
(bench.py's proof_k14 workload) under BZH_PROVE_TRACE=1, whose ` gp:*` and `fp:*` marks are the host-transcript path's times on the
same commit.  Of those marks perm_set, lookup_product, the fp: marks and commit are the work the call does; extend_z (the products
on the extended coset) is the vanishing leaf's.  The trace waits for the device at every mark, the call only at its end.

    python tools/ubench_products.py > profiles/products_device_calls.json

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

SHAPE = ("n", "usable", "blinding_factors", "nsets", "lookups", "nz", "chunk_len", "draws_per_proof")
SAME_WORK = ("gp:perm_set", "gp:lookup_product", "fp:exprs", "fp:invert", "fp:mul+scan", "gp:commit")


def board_blob(k):
    from bzh2 import circuits as Cm
    lay = Cm.CircuitLayout(Cm.BOARD, k)
    blob = lay.blob()
    lay.close()
    return blob


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
    blob = board_blob(k)
    shape = bzh2.grand_products_plan(bzh2.CURVE_VESTA, blob)
    n, _, _, _, nl, nz, _, nd = shape
    na, ni = bzh2.vanishing_plan(bzh2.CURVE_VESTA, blob)[0][2:4]
    row = {"k": k, "batch": B, **dict(zip(SHAPE, shape)), "num_advice": na, "num_instance": ni, "commitments_per_proof": nz}
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
    assert pk.grand_products_plan() == shape
    rng = np.random.default_rng(100 * k + B)

    def elems(*dims):
        a = np.frombuffer(rng.bytes(int(np.prod(dims)) * 32), dtype=np.uint64).reshape(*dims, 4).copy()
        a[..., 3] &= (1 << 60) - 1                             # every element below 2^252
        return torch.from_numpy(a.view(np.int64)).to("cuda")

    cid, MONT = bzh2.CURVE_VESTA, bzh2.FORM_MONTGOMERY
    d_ops = [elems(B, max(na, 1), n), elems(B, max(ni, 1), n), elems(B, max(nl, 1), 2, n), elems(B, max(nl, 1), 2, n)]
    d_ch = [elems(B) for _ in range(2)]
    d_rng = torch.from_numpy(np.frombuffer(rng.bytes(B * nd * 64), dtype=np.uint8).copy()).to("cuda")
    d_z, d_zp, d_zb = (torch.zeros(B * nz * m * 4, dtype=torch.int64, device="cuda") for m in (n, n, 1))
    d_st = torch.zeros(B, dtype=torch.uint8, device="cuda")
    ptr = lambda t, count=1: t.data_ptr() if count else 0     # noqa: E731

    def once():
        with bzh2.TranscriptBatch(cid, B, 32 * nz, ctx=wctx) as tb:
            tb.grand_products(pk, ptr(d_ops[0], na), ptr(d_ops[1], ni), ptr(d_ops[2], nl), ptr(d_ops[3], nl), ptr(d_ch[0]), ptr(d_ch[1]),
                              ptr(d_rng), form=MONT, mem=bzh2.MEM_DEVICE, out_z=ptr(d_z), out_z_polys=ptr(d_zp), out_z_blinds=ptr(d_zb),
                              status=ptr(d_st), rng_stride=64 * nd)
            wctx.sync()
    secs = timed(once)
    row["flagged_proofs"] = int(d_st.cpu().numpy().astype(bool).sum())
    del d_ops, d_z, d_zp
    row.update({"call_seconds": [round(s, 6) for s in secs], "mean_seconds": round(sum(secs) / 5, 6),
                "min_max_seconds": [round(min(secs), 6), round(max(secs), 6)]})

    # the host-transcript path: one traced prove of the same shape on the same key (a warm-up prove first)
    def prove():
        _, insts = r.layout.synthesize(r._circuits(0, B), ctx=wctx, device_ptr=r.adv[0].data_ptr(), threads=4)
        blob = r.np_rng[0].bytes(r.rng_bytes * B)
        r.pks[0].prove_batch(None, insts, [blob[i * r.rng_bytes:(i + 1) * r.rng_bytes] for i in range(B)], device_ptr=r.adv[0].data_ptr())
    prove()
    marks = {}
    for name, ms in re.findall(r"\[bzh_prove_batch\]\s+(\S+)\s+([0-9.]+) ms", traced(prove)):
        marks[name] = marks.get(name, 0.0) + float(ms)
    row["prove_trace_ms"] = {name: round(v, 3) for name, v in marks.items() if name.startswith(("gp:", "fp:")) or name == "grand_products"}
    if all(name in marks for name in SAME_WORK if name != "gp:lookup_product" or nl):
        row["prove_trace_same_work_seconds"] = round(sum(marks.get(name, 0.0) for name in SAME_WORK) / 1e3, 6)
    print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
