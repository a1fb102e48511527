"""The whole device-resident chain against bzh_prove_batch: the Board circuit at k = 14 for 64 proofs (Vesta's scalar field), the
same key (bench.py's proof_k14 workload), the same synthesized witness in device memory in Montgomery form, the same draws.

Settings, one fresh process each: `prove_batch` (bzh_prove_batch with the advice's device pointer: host transcripts, the proofs
in host memory when it returns; the draws, 2.1 MB a proof, come from host memory inside the call), `prove_batch_seeded`
(bzh_prove_batch_seeded: the same work with the draws expanded on the device from a seed per proof -- other draws, and no draw
crosses to the device, which is also the chain's position: its draws lie in device memory before the call) and `chain` (a new device transcript batch, common_scalars(vk_repr), then
bzh_commitments_batch_device, bzh_grand_products_batch_device, bzh_vanishing_batch_device, bzh_evaluations_batch_device and
bzh_multiopen_batch_device with the opening, every operand a BZH_MEM_DEVICE buffer in Montgomery form, one 64-byte draw stream
per proof cut at the leaves' draw counts, and bzh_transcript_batch_proofs into host memory at the end), `prove_batch_device`
(bzh_prove_batch_device: the same chain inside the library in one call, the key's own fixed and permutation polynomials, no
arrangement copies; the advice and the draws in device memory, the chain's position) and `prove_batch_device_seeded`
(bzh_prove_batch_device_seeded, the seeds of `prove_batch_seeded`).  The two one-call settings use the key's real polynomials, so
their proofs must verify: the tool checks verified == batch for them.  One warm-up call and
five timed calls; the median is the figure.  The `chain` process then makes one more call with a stream wait after every leaf,
whose wall times per leaf are `leaf_ms` (their sum is above the timed call's, which waits only where it must).

What the chain does here that a caller inside a prover would not: between the leaves the polynomial table and the blind table
of the evaluations and the multiopen are arranged from the leaves' outputs by device-to-device copies on another stream (torch),
with a wait on either side (`arrange_ms`); and the key's fixed and permutation polynomials, which the library does not hand
out, are uniform values in those two leaves' `shared` operand.  Their work does not depend on the values, but the chain's proofs
then do not verify: byte parity with bzh_prove_batch and the oracle is tests/test_gpu_commitments_device.py's business, this
tool only times.

    python tools/ubench_device_chain.py > profiles/prove_device_calls.json

It only prints: one JSON object per setting and a final summary.  A setting whose process ends abnormally stops the run.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "battlezips-halo2_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

from ubench_ipa_open import timed  # noqa: E402
from ubench_products import board_blob  # noqa: E402

OUT = ("advice", "instance", "lookup_compressed", "lookup_permuted", "advice_polys", "instance_polys", "lookup_polys", "advice_blinds",
       "lookup_blinds", "theta", "beta", "gamma")


def chain_plan(blob):
    """the chain's shapes and query lists from a circuit blob (host only): the polynomial table of the evaluations and the
    multiopen is instance, advice, random, grand products, lookups (a, s per lookup), h; then the key's fixed and permutation
    polynomials as `shared`.  ev: (poly, rotation) in upstream's write order; mo: (poly, point number) in upstream's query order"""
    import bzh2
    import blob as Bm
    import halo2_oracle as H
    cid = bzh2.CURVE_VESTA
    c = Bm.decode(blob)
    cs = H.ConstraintSystem(c.k, c.num_advice, c.num_fixed, c.num_instance, c.gates, c.perm_columns, c.lookups, degree=c.min_degree,
                            queries=c.queries)
    cshape, gshape, (vshape, _) = bzh2.commitments_plan(cid, blob), bzh2.grand_products_plan(cid, blob), bzh2.vanishing_plan(cid, blob)
    n, _, bf, na, ni, nl, nd_c, _ = cshape
    nsets, nz, nd_g = gshape[3], gshape[5], gshape[7]
    en, npieces, nd_v = vshape[1], vshape[6], vshape[7]
    nf, m, k = cs.num_fixed, len(cs.perm_columns), cs.k
    z0, l0 = ni + na + 1, ni + na + 1 + nz
    nown = l0 + 2 * nl + 1
    hid, last_rot = nown - 1, -(bf + 1)
    ev = [(c_, r) for c_, r in cs.instance_queries] + [(ni + c_, r) for c_, r in cs.advice_queries] + [(nown + c_, r) for c_, r in cs.fixed_queries]
    ev += [(ni + na, 0)] + [(nown + nf + j, 0) for j in range(m)]
    for i in range(nsets):
        ev += [(z0 + i, 0), (z0 + i, 1)] + ([(z0 + i, last_rot)] if i != nsets - 1 else [])
    for li in range(nl):
        ev += [(z0 + nsets + li, 0), (z0 + nsets + li, 1), (l0 + 2 * li, 0), (l0 + 2 * li, -1), (l0 + 2 * li + 1, 0)]
    rotations = bzh2.evaluations_plan(ev, nown + nf + m)[0]
    pt = rotations.index
    mo = [(c_, pt(r)) for c_, r in cs.instance_queries] + [(ni + c_, pt(r)) for c_, r in cs.advice_queries]
    for i in range(nsets):
        mo += [(z0 + i, pt(0)), (z0 + i, pt(1))] + ([(z0 + i, pt(last_rot))] if i != nsets - 1 else [])
    for li in range(nl):
        lz, la, ls = z0 + nsets + li, l0 + 2 * li, l0 + 2 * li + 1
        mo += [(lz, pt(0)), (la, pt(0)), (ls, pt(0)), (la, pt(-1)), (lz, pt(1))]
    mo += [(nown + c_, pt(r)) for c_, r in cs.fixed_queries] + [(nown + nf + j, pt(0)) for j in range(m)] + [(hid, pt(0)), (ni + na, pt(0))]
    nd_m = n + 2 + 2 * k
    return dict(k=k, n=n, en=en, na=na, ni=ni, nl=nl, nz=nz, nf=nf, m=m, npieces=npieces, nown=nown, hid=hid, ev=ev, mo=mo, nrot=len(rotations),
                draws=(nd_c, nd_g, nd_v, nd_m))


def measure(args):
    import torch
    torch.zeros(1, device="cuda")                              # torch's HIP runtime initialises before the library's
    import bzh2
    B, k = args.batch, args.k
    blob = board_blob(k)
    P = chain_plan(blob)
    os.chdir(ROOT)
    argv, sys.argv = sys.argv, ["bench.py", "--no-cpu-baseline", "--concurrency", "1"]
    import bench
    sys.argv = argv
    ctx = bzh2.Context(0)
    wl = bench.Workload("proof_k%d" % k, ctx, torch.device("cuda:0"), 1, concurrency=1, batch=B)
    r = wl.runner
    pk, wctx = r.pk, r.ctxs[0]
    n, en, na, ni, nl, nz, nf, m, npieces, nown, hid, nrot = (P[x] for x in ("n", "en", "na", "ni", "nl", "nz", "nf", "m", "npieces", "nown", "hid", "nrot"))
    nd_c, nd_g, nd_v, nd_m = P["draws"]
    total = nd_c + nd_g + nd_v + nd_m
    assert 64 * total == pk.rng_bytes
    cap = pk.max_proof_bytes
    rng = np.random.default_rng(100 * k + B)                   # the same witness and the same draws in both settings
    _, insts = r.layout.synthesize(r._circuits(0, B), ctx=wctx, device_ptr=r.adv[0].data_ptr(), threads=4)
    streams = rng.bytes(B * 64 * total)
    row = {"k": k, "batch": B, "setting": args.setting, "draws_per_proof": total, "leaf_draws": [nd_c, nd_g, nd_v, nd_m],
           "queries": [len(P["ev"]), len(P["mo"])], "table_polynomials": nown, "shared_polynomials": nf + m}

    if args.setting in ("prove_batch", "prove_batch_seeded", "prove_batch_device", "prove_batch_device_seeded"):
        seeded = args.setting.endswith("_seeded")
        one_call = "_device" in args.setting
        rng_list = None if seeded else [streams[b * 64 * total:(b + 1) * 64 * total] for b in range(B)]
        seeds = [streams[32 * b:32 * (b + 1)] for b in range(B)] if seeded else None
        d_rng = torch.from_numpy(np.frombuffer(streams, dtype=np.uint8).copy()).to("cuda") if one_call and not seeded else None
        got, flagged = [], []

        def once():
            if not one_call:
                got[:] = pk.prove_batch(None, insts, rng_list, device_ptr=r.adv[0].data_ptr(), seeds=seeds, ctx=wctx)
            elif seeded:
                got[:], flagged[:] = pk.prove_batch_device(None, insts, seeds=seeds, device_ptr=r.adv[0].data_ptr(), ctx=wctx)
            else:
                got[:], flagged[:] = pk.prove_batch_device(None, insts, device_ptr=r.adv[0].data_ptr(), rng_device_ptr=d_rng.data_ptr(),
                                                           rng_stride=64 * total, ctx=wctx)
        secs = timed(once)
        row["proof_bytes"] = len(got[0])
        row["verified"] = int(sum(pk.verify_batch(insts, got, ctx=wctx)))
        if one_call:
            row["flagged"] = int(sum(bool(x) for x in flagged))
            assert row["verified"] == B and not row["flagged"], row
    else:
        cid, MO, DEV = bzh2.CURVE_VESTA, bzh2.FORM_MONTGOMERY, bzh2.MEM_DEVICE
        p_mod = pk.p
        R = (1 << 256) % p_mod
        rows = max([len(col) for cols in insts for col in cols] + [0])
        inst = np.zeros((B, max(ni, 1), max(rows, 1), 4), dtype=np.uint64)
        for b, cols in enumerate(insts):
            for i, col in enumerate(cols):
                for j, v in enumerate(col):
                    inst[b, i, j] = bzh2.int_to_limbs(int(v) * R % p_mod)
        d_inst = torch.from_numpy(inst.view(np.int64)).to("cuda")
        d_rng = torch.from_numpy(np.frombuffer(streams, dtype=np.uint8).copy()).to("cuda")
        at = lambda draws: d_rng.data_ptr() + 64 * draws   # noqa: E731
        z64 = lambda *shape: torch.zeros(shape + (4,), dtype=torch.int64, device="cuda")   # noqa: E731

        def elems(*dims):
            a = np.frombuffer(rng.bytes(int(np.prod(dims)) * 32), dtype=np.uint64).reshape(*dims, 4).copy()
            a[..., 3] &= (1 << 60) - 1                         # every element below 2^252
            return torch.from_numpy(a.view(np.int64)).to("cuda")

        sizes = {"advice": (B, na, n), "instance": (B, ni, n), "lookup_compressed": (B, 2 * nl, n), "lookup_permuted": (B, 2 * nl, n),
                 "advice_polys": (B, na, n), "instance_polys": (B, ni, n), "lookup_polys": (B, 2 * nl, n), "advice_blinds": (B, na),
                 "lookup_blinds": (B, 2 * nl), "theta": (B,), "beta": (B,), "gamma": (B,)}
        c_out = {nm: z64(*sizes[nm]) for nm in OUT}
        zp, zb = z64(B, nz, n), z64(B, nz)
        rp, rb, h, hb = z64(B, 1, n), z64(B, 1), z64(B, en), z64(B, npieces)
        table, blinds = z64(B, nown, n), z64(B, nown)
        pts, d_h, d_hbl = z64(B, nrot), z64(B, n), z64(B)
        one = torch.from_numpy(np.asarray(bzh2.int_to_limbs(R), dtype=np.uint64).view(np.int64).copy()).to("cuda")
        shared, shared_blinds = elems(nf + m, n), elems(nf + m)
        d_st = torch.zeros(4 * B, dtype=torch.uint8, device="cuda")
        vk = np.stack([bzh2.int_to_limbs(pk.vk_repr()[0])] * B).reshape(B, 1, 4)
        p = lambda t: t.data_ptr() if t.numel() else 0   # noqa: E731
        stride = 64 * total
        got, laps = [], {}

        def once(split=False):
            t = [time.perf_counter()]

            def lap(name, wait):
                if wait:
                    wctx.sync()
                t.append(time.perf_counter())
                laps[name] = laps.get(name, 0.0) + (t[-1] - t[-2]) * 1e3

            with bzh2.TranscriptBatch(cid, B, cap, ctx=wctx) as tb:
                tb.common_scalars(vk)
                tb.commitments(pk, r.adv[0].data_ptr(), p(d_inst), at(0), form=MO, mem=DEV, out={nm: p(c_out[nm]) for nm in OUT},
                               status=p(d_st), instance_rows=rows, rng_stride=stride)
                lap("commitments", split)
                tb.grand_products(pk, p(c_out["advice"]), p(c_out["instance"]), p(c_out["lookup_compressed"]), p(c_out["lookup_permuted"]),
                                  p(c_out["beta"]), p(c_out["gamma"]), at(nd_c), form=MO, mem=DEV, out_z=None, out_z_polys=p(zp),
                                  out_z_blinds=p(zb), status=p(d_st) + B, rng_stride=stride)
                lap("grand_products", split)
                tb.vanishing(pk, p(c_out["advice_polys"]), p(c_out["instance_polys"]), p(c_out["lookup_polys"]), p(zp), p(c_out["theta"]),
                             p(c_out["beta"]), p(c_out["gamma"]), at(nd_c + nd_g), form=MO, mem=DEV, out_random=p(rp), out_random_blind=p(rb),
                             out_h=p(h), out_h_blinds=p(hb), status=p(d_st) + 2 * B, rng_stride=stride)
                lap("vanishing", True)                         # (the copies below run on another stream)
                table[:, :hid] = torch.cat([c_out["instance_polys"], c_out["advice_polys"], rp, zp, c_out["lookup_polys"]], dim=1)
                blinds[:, :hid] = torch.cat([one.view(1, 1, 4).expand(B, ni, 4), c_out["advice_blinds"], rb, zb, c_out["lookup_blinds"]], dim=1)
                torch.cuda.synchronize()
                lap("arrange", False)
                tb.evaluations(k, p(table), P["ev"], shared=p(shared), h_pieces=p(h), h_blinds=p(hb), npieces=npieces, h_stride=en, form=MO,
                               mem=DEV, out_points=p(pts), out_h=p(d_h), out_h_blind=p(d_hbl), npolys_own=nown, npolys_shared=nf + m)
                lap("evaluations", True)
                table[:, hid] = d_h
                blinds[:, hid] = d_hbl
                torch.cuda.synchronize()
                lap("arrange", False)
                tb.multiopen(pk.bases, k, p(table), p(blinds), p(pts), P["mo"], at(nd_c + nd_g + nd_v), shared=p(shared),
                             shared_blinds=p(shared_blinds), form=MO, mem=DEV, status=p(d_st) + 3 * B, rng_stride=stride, npolys_own=nown,
                             npolys_shared=nf + m, npoints=nrot)
                lap("multiopen", split)
                got[:] = tb.proofs()
                lap("proofs", False)

        secs = timed(once)
        laps.clear()
        once(split=True)
        row["leaf_ms"] = {name: round(v, 3) for name, v in laps.items()}
        row["proof_bytes"] = len(got[0])
        row["flagged"] = [int(x) for x in d_st.cpu().numpy().reshape(4, B).astype(bool).sum(axis=1)]
    row.update({"call_seconds": [round(s, 6) for s in secs], "median_seconds": round(statistics.median(secs), 6),
                "min_max_seconds": [round(min(secs), 6), round(max(secs), 6)]})
    print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--role", choices=["drive", "measure"], default="drive")
    ap.add_argument("--setting", choices=["prove_batch", "prove_batch_seeded", "chain", "prove_batch_device", "prove_batch_device_seeded"],
                    default="chain")
    ap.add_argument("--k", type=int, default=14)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--limit", type=int, default=240, help="seconds each child process may take")
    ap.add_argument("--plan-only", action="store_true", help="print the chain's shape and stop (needs no GPU)")
    args = ap.parse_args()
    if args.plan_only:
        P = chain_plan(board_blob(args.k))
        print(json.dumps({x: P[x] for x in P if x not in ("ev", "mo")} | {"queries": [len(P["ev"]), len(P["mo"])]}), flush=True)
        return
    if args.role == "measure":
        return measure(args)
    rows = []
    for setting in ("prove_batch", "prove_batch_seeded", "chain", "prove_batch_device", "prove_batch_device_seeded"):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--role", "measure", "--setting", setting, "--k", str(args.k), "--batch",
                            str(args.batch)], check=True, timeout=args.limit, stdout=subprocess.PIPE, text=True)
        print(r.stdout.strip(), flush=True)
        rows.append(json.loads(r.stdout.strip().splitlines()[-1]))
    print(json.dumps({"summary": {r["setting"]: r["median_seconds"] for r in rows}}))


if __name__ == "__main__":
    main()
