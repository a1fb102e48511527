"""The grand products on device-resident transcripts (bzh_grand_products_plan, bzh_grand_products_batch_device) without a device:
the header / exports agreement for the two names, the plan against the oracle's constraint system, the argument refusals that
need no device, and the lane bodies (csrc/products_scalars.hpp) run lane by lane on the host against fe_mul
(tests/helpers/products_scalars_check.hip, a stand-alone program under the host's address and undefined-behaviour sanitizers)."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import halo2_oracle as H
import pasta as O
import sample_circuit as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("bzh_grand_products_plan", "bzh_grand_products_batch_device")
E_ARG = -1
F = O.FP


def test_header_and_exports_name_the_entry_points():
    import bzh2
    from bzh2 import native as N
    header = open(os.path.join(ROOT, "include", "bzh2.h")).read()
    for name in NAMES:
        assert re.search(r"\bint %s\(" % name, header) and name in bzh2.EXPORTS
        getattr(bzh2.load(), name)
    assert header.index("int bzh_vanishing_batch_device(") < header.index("int bzh_grand_products_plan(") < header.index("int bzh_grand_products_batch_device(")
    assert hasattr(bzh2.TranscriptBatch, "grand_products") and callable(bzh2.grand_products_plan)
    assert hasattr(N.NativeProvingKey, "grand_products_plan")


def _blobs():
    """(name, blob, the oracle's ConstraintSystem): the sample circuit at k = 4, 5, 6 with and without its lookup at degree 3 / 4
    and at degree 9, and the reference's two circuits"""
    import blob as Bm
    from bzh2 import circuit_data as P, circuits as Cm
    out = []
    for k in (4, 5, 6):
        for with_lookup in (False, True):
            for degree in (None, 9):
                cs, fixed, copies, _, _ = S.build(k=k, seed=3, with_lookup=with_lookup, degree=degree)
                circ = P.Circuit(cs.k, cs.num_advice, cs.num_fixed, cs.num_instance, cs.gates, cs.perm_columns, cs.lookups, fixed, copies,
                                 degree=degree)
                out.append(("sample k=%d lookup=%d degree=%s" % (k, with_lookup, degree), P.serialize_circuit(circ, F.p, 0x1234), cs))
    for name, kind, k in (("shot", Cm.SHOT, 11), ("board", Cm.BOARD, 12)):
        lay = Cm.CircuitLayout(kind, k)
        blob = lay.blob()
        lay.close()
        c = Bm.decode(blob)
        cs = H.ConstraintSystem(c.k, c.num_advice, c.num_fixed, c.num_instance, c.gates, c.perm_columns, c.lookups, degree=c.min_degree,
                                queries=c.queries)
        out.append((name, blob, cs))
    return out


def test_plan_against_the_constraint_system():
    import bzh2
    seen = set()
    for name, blob, cs in _blobs():
        nsets = (len(cs.perm_columns) + cs.chunk_len - 1) // cs.chunk_len if cs.perm_columns else 0
        nl, bf = len(cs.lookups), cs.blinding_factors
        assert bzh2.grand_products_plan(bzh2.CURVE_VESTA, blob) == (cs.n, cs.usable_rows, bf, nsets, nl, nsets + nl, cs.chunk_len,
                                                                    (nsets + nl) * (bf + 1)), name
        seen.add((cs.chunk_len, nsets))
    # degree 3: one column per set, the longest chain; degree 9: one set with a short chunk
    assert (1, 4) in seen and (7, 1) in seen and len({c for c, _ in seen}) >= 3


def test_plan_refusals():
    import bzh2
    L = bzh2.load()
    L.bzh_grand_products_plan.argtypes = [ctypes.c_int, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_void_p]
    blob = _blobs()[0][1]
    shape = np.full(8, 5, dtype=np.uint32)
    args = [0, blob, len(blob), ctypes.c_void_p(shape.ctypes.data)]
    for change in ((1, None), (3, None), (2, len(blob) // 2), (0, 7)):          # NULL pointers, a truncated blob, no such curve
        a = list(args)
        a[change[0]] = change[1]
        assert L.bzh_grand_products_plan(*a) == E_ARG and (shape == 5).all(), change
    assert L.bzh_grand_products_plan(*args) == 0 and shape[0] == 16
    with pytest.raises(bzh2.BzhError) as e:
        bzh2.grand_products_plan(bzh2.CURVE_VESTA, blob[:len(blob) // 2])
    assert e.value.status == E_ARG


def test_argument_refusals_without_a_device():
    """every refusal that needs no device, on made-up non-NULL handles that a refusal must not read through; a host-resident batch is
    left as it was and the output arrays are untouched"""
    import bzh2
    L = bzh2.load()
    vp, sz, ci = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
    L.bzh_grand_products_batch_device.argtypes = [vp, vp, sz, vp, vp, vp, vp, vp, vp, ci, ci, vp, sz, vp, vp, vp, vp, vp]
    B, n = 2, 4
    ops = [np.zeros((B, 1, n, 4), dtype=np.uint64) for _ in range(2)] + [np.zeros((B, 1, 2, n, 4), dtype=np.uint64) for _ in range(2)]
    chs = [np.zeros((B, 4), dtype=np.uint64) for _ in range(2)]
    raw = np.zeros(B * 64 * 16, dtype=np.uint8)
    outs = [np.full((B, m, 4), 7, dtype=np.uint64) for m in (n, n, 1)]
    st = np.full(B, 7, dtype=np.uint8)
    fake = vp(0x1000)
    at = lambda a: vp(a.ctypes.data)   # noqa: E731
    with bzh2.TranscriptBatch(bzh2.CURVE_VESTA, B, 256) as tb, bzh2.TranscriptBatch(bzh2.CURVE_VESTA, B, 256) as twin:   # host-resident

        def call(**kw):
            a = dict(ctx=fake, pk=fake, batch=B, adv=at(ops[0]), inst=at(ops[1]), lc=at(ops[2]), lp=at(ops[3]), beta=at(chs[0]), gamma=at(chs[1]),
                     form=bzh2.FORM_CANONICAL, mem=bzh2.MEM_HOST, rng=at(raw), stride=64 * 16, trs=tb.h, z=at(outs[0]), zp=at(outs[1]),
                     zb=at(outs[2]), st=at(st))
            a.update(kw)
            return L.bzh_grand_products_batch_device(*a.values())

        assert call() == E_ARG                                   # a host-resident batch: the made-up ctx and key are not read
        for kw in (dict(ctx=None), dict(pk=None), dict(trs=None), dict(rng=None), dict(beta=None), dict(gamma=None), dict(zp=None), dict(zb=None),
                   dict(adv=None), dict(inst=None), dict(lc=None), dict(lp=None), dict(batch=0), dict(batch=65536), dict(form=2), dict(form=-1),
                   dict(mem=2), dict(mem=-1)):
            assert call(**kw) == E_ARG, kw
        with pytest.raises(bzh2.BzhError) as e:                  # the Python mirror on a host-resident batch: refused the same way
            tb.grand_products(fake, ops[0], ops[1], ops[2], ops[3], chs[0], chs[1], [bytes(64 * 16)] * B, shape=(n, 1, 1, 1, 0, 1, 1, 2))
        assert e.value.status == E_ARG
        assert all((o == 7).all() for o in outs) and (st == 7).all() and tb.proof_len() == 0
        assert (tb.squeeze() == twin.squeeze()).all()   # the batch is as it was


def test_lane_bodies_against_the_host_arithmetic_standalone_under_host_sanitizers(tmp_path):
    """gp_carry_lane and gp_status_lane against fe_mul, word for word, for Fp and Fq: nsets 0, 1, 2 and 5 with 0 and 2 lookups;
    per buffer a proof that closes, one that does not close in its sets, one that does not close in a lookup, one whose first
    set hands a zero on"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    csrc = os.path.join(ROOT, "battlezips-halo2_amd", "csrc")
    exe = str(tmp_path / "products_scalars_check")
    subprocess.check_call([hipcc, "-O1", "-g", "-std=c++17", "--offload-arch=gfx950", "-Wno-unused-function",
                           "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                           "-I", csrc, os.path.join(ROOT, "tests", "helpers", "products_scalars_check.hip"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(out.stdout[-3000:])
    assert out.returncode == 0 and out.stdout.strip().endswith("products_scalars_check: ok"), out.stdout[-3000:] + out.stderr[-3000:]
    # per buffer 4 proofs x (nz carries + 1 status); nz = 0, 2, 1, 3, 2, 4, 5, 7; 2 fields
    assert int(re.search(r"(\d+) lanes", out.stdout).group(1)) == 4 * 32 * 2
