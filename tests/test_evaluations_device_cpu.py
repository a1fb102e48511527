"""The evaluation phase on device-resident transcripts (bzh_evaluations_plan, bzh_evaluations_batch_device) without a device: the
header / exports agreement for the two names, the plan against a few lines of Python, the argument refusals that need no device,
and the lane bodies (csrc/evaluations_scalars.hpp) run lane by lane on the host against fe_mul / fe_sqr / fe_add
(tests/helpers/evaluations_scalars_check.hip, a stand-alone program under the host's address and undefined-behaviour
sanitizers)."""
import ctypes
import os
import random
import re
import shutil
import subprocess

import numpy as np
import pytest

from helpers import evaluations_cases as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("bzh_evaluations_plan", "bzh_evaluations_batch_device")
E_ARG = -1


def test_header_and_exports_name_the_entry_points():
    import bzh2
    header = open(os.path.join(ROOT, "include", "bzh2.h")).read()
    for name in NAMES:
        assert re.search(r"\bint %s\(" % name, header) and name in bzh2.EXPORTS
        getattr(bzh2.load(), name)
    assert header.index("int bzh_multiopen_batch_device(") < header.index("int bzh_evaluations_plan(") < header.index("int bzh_evaluations_batch_device(")
    assert re.search(r"#define BZH_EVAL_MAX_ROTATIONS 8\b", header)
    assert re.search(r"typedef struct \{\s*uint32_t poly;\s*int32_t rotation;\s*\} bzh_eval_query;", header)
    assert hasattr(bzh2.TranscriptBatch, "evaluations") and callable(bzh2.evaluations_plan)


def test_plan_on_the_pattern():
    import bzh2
    got = bzh2.evaluations_plan(V.QUERIES, V.NOWN + V.NSHARED)
    assert got == V.plan(V.QUERIES, V.NOWN + V.NSHARED)
    rotations, point, order, count = got
    assert rotations == V.ROTATIONS and count == V.ROT_COUNT and order == V.POLY_ORDER
    assert [rotations[j] for j in point] == [r for _, r in V.QUERIES]


def test_plan_on_seeded_random_lists():
    import bzh2
    rng = random.Random(20261)
    for _ in range(200):
        npolys = rng.randrange(1, 25)
        rots = [rng.choice([0, 1, -1, 2, -7, 2 ** 31 - 1, -2 ** 31]) for _ in range(rng.randrange(1, 8))]
        queries = [(rng.randrange(npolys), rng.choice(rots)) for _ in range(rng.randrange(1, 61))]
        assert bzh2.evaluations_plan(queries, npolys) == V.plan(queries, npolys)


def test_plan_refusals():
    import bzh2
    L = bzh2.load()
    vp, sz = ctypes.c_void_p, ctypes.c_size_t
    L.bzh_evaluations_plan.argtypes = [vp, sz, sz, vp, ctypes.POINTER(sz), vp, vp, vp]
    for queries, npolys in (([(2, 0)], 2), ([], 2), ([(0, j) for j in range(9)], 1)):
        with pytest.raises(bzh2.BzhError) as e:                       # an id out of range, no queries, 9 rotations on one polynomial
            bzh2.evaluations_plan(queries, npolys)
        assert e.value.status == E_ARG
    assert bzh2.evaluations_plan([(0, j) for j in range(8)] + [(1, 8)], 2)[3] == [8, 1]   # 8 rotations are taken, 9 in all
    q = np.array([(0, 0)], dtype=[("poly", np.uint32), ("rotation", np.int32)])
    rots, point, order, count = np.full(1, 5, dtype=np.int32), *(np.full(1, 5, dtype=np.uint32) for _ in range(3))
    nrot = sz(5)
    args = [vp(q.ctypes.data), 1, 1, vp(rots.ctypes.data), ctypes.byref(nrot)] + [vp(a.ctypes.data) for a in (point, order, count)]
    for i in (0, 3, 4, 5, 6, 7):                                         # each pointer in turn NULL: refused, nothing written
        a = list(args)
        a[i] = None
        assert L.bzh_evaluations_plan(*a) == E_ARG
        assert nrot.value == 5 and rots[0] == 5 and point[0] == 5 and order[0] == 5 and count[0] == 5
    assert L.bzh_evaluations_plan(*args) == 0 and nrot.value == 1 and (rots[0], point[0], order[0], count[0]) == (0, 0, 0, 1)


def test_argument_refusals_without_a_device():
    """every refusal that needs no device, on made-up non-NULL handles that a refusal must not read through; a host-resident batch is
    left as it was and the output arrays are untouched"""
    import bzh2
    L = bzh2.load()
    vp, sz, ci = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
    L.bzh_evaluations_batch_device.argtypes = [vp, sz, ctypes.c_uint, vp, sz, vp, sz, vp, sz, vp, sz, sz, vp, ci, ci, vp, vp, vp, vp, vp]
    B, k, n = 2, 2, 4
    polys = np.zeros((B, 1, n, 4), dtype=np.uint64)
    shared = np.zeros((1, n, 4), dtype=np.uint64)
    pieces = np.zeros((B, 2 * n, 4), dtype=np.uint64)
    hblinds = np.zeros((B, 2, 4), dtype=np.uint64)
    q = np.array([(0, 0), (1, 1)], dtype=[("poly", np.uint32), ("rotation", np.int32)])
    outs = [np.full((B, m, 4), 7, dtype=np.uint64) for m in (2, 2, n, 1)]
    fake = vp(0x1000)
    with bzh2.TranscriptBatch(bzh2.CURVE_VESTA, B, 64) as tb, bzh2.TranscriptBatch(bzh2.CURVE_VESTA, B, 64) as twin:   # host-resident

        def call(**kw):
            a = dict(ctx=fake, batch=B, k=k, polys=vp(polys.ctypes.data), nown=1, shared=vp(shared.ctypes.data), nshared=1,
                     queries=vp(q.ctypes.data), nq=2, pieces=vp(pieces.ctypes.data), npieces=2, stride=2 * n, hblinds=vp(hblinds.ctypes.data),
                     form=bzh2.FORM_CANONICAL, mem=bzh2.MEM_HOST, trs=tb.h, o0=vp(outs[0].ctypes.data), o1=vp(outs[1].ctypes.data),
                     o2=vp(outs[2].ctypes.data), o3=vp(outs[3].ctypes.data))
            a.update(kw)
            return L.bzh_evaluations_batch_device(*a.values())

        assert call() == E_ARG                                   # a host-resident batch: the made-up ctx is not read
        for kw in (dict(ctx=None), dict(trs=None), dict(polys=None), dict(queries=None), dict(o0=None),    # NULL ctx, transcripts, pointers
                   dict(shared=None), dict(pieces=None), dict(hblinds=None), dict(o2=None), dict(o3=None),
                   dict(batch=0), dict(batch=65536), dict(k=33), dict(nq=0), dict(nown=0, nshared=2),
                   dict(nshared=0),                                # poly id 1 out of range
                   dict(stride=2 * n - 1), dict(form=2), dict(mem=2)):
            assert call(**kw) == E_ARG, kw
        q9 = np.array([(0, j) for j in range(9)], dtype=q.dtype)
        assert call(queries=vp(q9.ctypes.data), nq=9) == E_ARG     # what the plan refuses
        # the Python mirror on a host-resident batch: refused the same way
        with pytest.raises(bzh2.BzhError) as e:
            tb.evaluations(k, polys, [(0, 0)])
        assert e.value.status == E_ARG
        assert all((o == 7).all() for o in outs) and tb.proof_len() == 0
        assert (tb.squeeze() == twin.squeeze()).all()   # the batch is as it was


def test_lane_bodies_against_the_host_arithmetic_standalone_under_host_sanitizers(tmp_path):
    """ev_points_lane, ev_xn_lane, ev_hblind_lane and ev_export_lane against fe_mul / fe_sqr / fe_add / h_pow_u64, word for word, for
    Fp and Fq and both operand forms; x random, 0, 1 and p - 1; k = 0, 1 and 17"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    csrc = os.path.join(ROOT, "battlezips-halo2_amd", "csrc")
    exe = str(tmp_path / "evaluations_scalars_check")
    subprocess.check_call([hipcc, "-O1", "-g", "-std=c++17", "--offload-arch=gfx950", "-Wno-unused-function",
                           "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                           "-I", csrc, os.path.join(ROOT, "tests", "helpers", "evaluations_scalars_check.hip"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(out.stdout[-3000:])
    assert out.returncode == 0 and out.stdout.strip().endswith("evaluations_scalars_check: ok"), out.stdout[-3000:] + out.stderr[-3000:]
    # per run: 4 point lanes, 4 x^n, 4 blinds, 12 exports; 3 shapes x 2 forms x 2 fields
    assert int(re.search(r"(\d+) lanes", out.stdout).group(1)) == 12 * 24
