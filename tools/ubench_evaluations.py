"""bzh_evaluations_batch_device next to the evaluations and h_poly phases of bzh_prove_batch: the Board circuit's own
(polynomial, rotation) list (its instance, advice, permutation, lookup and random polynomials per proof; its fixed and sigma
polynomials shared) and its quotient pieces at k = 14 for 64 proofs (Vesta's scalar field), every operand a BZH_MEM_DEVICE buffer
in Montgomery form, the pieces in rows of the extended domain's size as the prover keeps them.  The operands are uniform values;
the work does not depend on them.

One process: one warm-up call and five timed calls of bzh_evaluations_batch_device, a fresh device-resident transcript batch for
every call and one stream wait at its end; then one bzh_prove_batch of the same shape (bench.py's proof_k14 workload) under
BZH_PROVE_TRACE=1, whose `evaluations` and `h_poly` marks are the host-transcript path's times for the same work on the same
commit.

    python tools/ubench_evaluations.py > profiles/evaluations_device_calls.json

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


def board_queries(k):
    """the (polynomial, rotation) list of the evaluations phase for the Board circuit, in the order csrc/prover.hpp's evaluations()
    writes them: own ids first, then the shared ones; returns (queries, npolys_own, npolys_shared, npieces)"""
    import blob as Bm
    import halo2_oracle as H
    from bzh2 import circuits as Cm
    lay = Cm.CircuitLayout(Cm.BOARD, k)
    circ = Bm.decode(lay.blob())
    lay.close()
    cs = H.ConstraintSystem(circ.k, circ.num_advice, circ.num_fixed, circ.num_instance, circ.gates, circ.perm_columns, circ.lookups,
                            degree=circ.min_degree, queries=circ.queries)
    nz = (len(cs.perm_columns) + cs.chunk_len - 1) // cs.chunk_len if cs.perm_columns else 0
    last_rot = -(cs.blinding_factors + 1)
    own, shared, q = {}, {}, []

    def add(table, name, rot):
        q.append((table, table.setdefault(name, len(table)), rot))

    for c, r in cs.instance_queries:
        add(own, ("inst", c), r)
    for c, r in cs.advice_queries:
        add(own, ("adv", c), r)
    for c, r in cs.fixed_queries:
        add(shared, ("fix", c), r)
    add(own, ("rand", 0), 0)
    for j in range(len(cs.perm_columns)):
        add(shared, ("sig", j), 0)
    for i in range(nz):
        add(own, ("pz", i), 0), add(own, ("pz", i), 1)
        if i != nz - 1:
            add(own, ("pz", i), last_rot)
    for i in range(len(cs.lookups)):
        add(own, ("lz", i), 0), add(own, ("lz", i), 1), add(own, ("la", i), 0), add(own, ("la", i), -1), add(own, ("ls", i), 0)
    return [(i if t is own else len(own) + i, rot) for t, i, rot in q], len(own), len(shared), cs.degree - 1


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--k", type=int, default=14)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--plan-only", action="store_true", help="print the query list's shape and stop (needs no GPU)")
    args = ap.parse_args()
    if not args.plan_only:
        import torch
        torch.zeros(1, device="cuda")                          # torch's HIP runtime initialises before the library's
    import bzh2
    B, k = args.batch, args.k
    n = 1 << k
    queries, nown, nshared, npieces = board_queries(k)
    rotations, _, order, count = bzh2.evaluations_plan(queries, nown + nshared)
    row = {"k": k, "batch": B, "npolys_own": nown, "npolys_shared": nshared, "nqueries": len(queries), "nrotations": len(rotations),
           "npolys_queried": len(order), "polys_by_rotation_count": {str(c): count.count(c) for c in sorted(set(count)) if c},
           "npieces": npieces}
    if args.plan_only:
        print(json.dumps(row), flush=True)
        return
    rng = np.random.default_rng(100 * k + B)

    def elems(*shape):
        a = np.frombuffer(rng.bytes(int(np.prod(shape)) * 32), dtype=np.uint64).reshape(*shape, 4).copy()
        a[..., 3] &= (1 << 60) - 1                             # every element below 2^252
        return torch.from_numpy(a.view(np.int64)).to("cuda")

    en = n
    while en < npieces * n:
        en *= 2                                                # a row of the prover's quotient buffer: the extended domain
    cid, MONT = bzh2.CURVE_VESTA, bzh2.FORM_MONTGOMERY
    with bzh2.Context(0) as ctx:
        d_polys, d_shared, d_h, d_hb = elems(B, nown, n), elems(nshared, n), elems(B, en), elems(B, npieces)
        d_pts, d_ev, d_oh, d_ohb = (torch.zeros(B * m * 4, dtype=torch.int64, device="cuda") for m in (len(rotations), len(queries), n, 1))
        cap = 32 * len(queries)

        def once():
            with bzh2.TranscriptBatch(cid, B, cap, ctx=ctx) as tb:
                tb.evaluations(k, d_polys.data_ptr(), queries, shared=d_shared.data_ptr(), h_pieces=d_h.data_ptr(), h_blinds=d_hb.data_ptr(),
                               npieces=npieces, h_stride=en, form=MONT, mem=bzh2.MEM_DEVICE, out_points=d_pts.data_ptr(),
                               out_evals=d_ev.data_ptr(), out_h=d_oh.data_ptr(), out_h_blind=d_ohb.data_ptr(), npolys_own=nown,
                               npolys_shared=nshared)
                ctx.sync()
        secs = timed(once)
        del d_polys, d_shared, d_h
    row.update({"call_seconds": [round(s, 6) for s in secs], "mean_seconds": round(sum(secs) / 5, 6),
                "min_max_seconds": [round(min(secs), 6), round(max(secs), 6)]})
    # the host-transcript path: one traced prove of the same shape (a warm-up prove first)
    os.chdir(ROOT)
    argv, sys.argv = sys.argv, ["bench.py", "--no-cpu-baseline", "--concurrency", "1"]
    import bench
    sys.argv = argv
    ctx = bzh2.Context(0)
    wl = bench.Workload("proof_k%d" % k, ctx, torch.device("cuda:0"), 1, concurrency=1, batch=B)
    r = wl.runner

    def prove():
        _, insts = r.layout.synthesize(r._circuits(0, B), ctx=r.ctxs[0], device_ptr=r.adv[0].data_ptr(), threads=4)
        blob = r.np_rng[0].bytes(r.rng_bytes * B)
        r.pks[0].prove_batch(None, insts, [blob[i * r.rng_bytes:(i + 1) * r.rng_bytes] for i in range(B)], device_ptr=r.adv[0].data_ptr())
    prove()
    marks = {}
    for name, ms in re.findall(r"\[bzh_prove_batch\] (\w+)\s+([0-9.]+) ms", traced(prove)):
        marks[name] = marks.get(name, 0.0) + float(ms)
    row["prove_trace_ms"] = {name: marks.get(name) for name in ("evaluations", "h_poly")}
    if all(v is not None for v in row["prove_trace_ms"].values()):
        row["prove_trace_sum_seconds"] = round(sum(row["prove_trace_ms"].values()) / 1e3, 6)
    print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
