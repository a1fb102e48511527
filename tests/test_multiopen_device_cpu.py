"""The multiopen argument on device-resident transcripts (bzh_multiopen_plan, bzh_multiopen_batch_device) without a device: the
header / exports agreement for the two names, the grouping against oracle/halo2_oracle.py: query_sets, the argument refusals
that need no device, and the lane bodies (csrc/multiopen_scalars.hpp) run lane by lane on the host against h_interpolate /
h_batch_invert / fe_mul / fe_add (tests/helpers/multiopen_scalars_check.hip, a stand-alone program under the host's address and
undefined-behaviour sanitizers)."""
import ctypes
import os
import random
import re
import shutil
import subprocess

import numpy as np
import pytest

from helpers import multiopen_cases as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("bzh_multiopen_plan", "bzh_multiopen_batch_device")
E_ARG = -1


def test_header_and_exports_name_the_entry_points():
    import bzh2
    header = open(os.path.join(ROOT, "include", "bzh2.h")).read()
    for name in NAMES:
        assert re.search(r"\bint %s\(" % name, header) and name in bzh2.EXPORTS
        getattr(bzh2.load(), name)
    assert header.index("int bzh_ipa_open_batch_device(") < header.index("int bzh_multiopen_batch_device(")
    assert re.search(r"#define BZH_MULTIOPEN_MAX_POINTS 8\b", header) and "bzh_open_query" in header
    assert hasattr(bzh2.TranscriptBatch, "multiopen") and callable(bzh2.multiopen_plan)


def _same_grouping(queries, npolys, npoints):
    import bzh2
    point_sets, groups, set_of = bzh2.multiopen_plan(queries, npolys, npoints)
    want_sets, want_groups = M.oracle_sets(queries)
    assert groups == want_groups                                        # set order, membership and group order
    assert [set(s) for s in point_sets] == [set(s) for s in want_sets]  # each set's points, as a set
    assert all(len(s) == len(set(s)) for s in point_sets)
    for pid in range(npolys):
        where = [s for s, g in enumerate(want_groups) if pid in g]
        assert set_of[pid] == (where[0] if where else None)


def test_plan_groups_the_provers_pattern_as_query_sets_does():
    import bzh2
    _same_grouping(M.QUERIES, M.NOWN + M.NSHARED, M.NPOINTS)
    point_sets, groups, set_of = bzh2.multiopen_plan(M.QUERIES, M.NOWN + M.NSHARED, M.NPOINTS)
    assert groups == [[0, 6, 7], [1, 3], [2], [4]] and [sorted(s) for s in point_sets] == [[0], [0, 1], [0, 1, 2], [0, 3]]
    assert set_of[5] is None and len(groups) == M.NSETS


def test_plan_groups_seeded_random_lists_as_query_sets_does():
    rng = random.Random(20260)
    for _ in range(200):
        npolys, npoints = rng.randrange(1, 25), rng.randrange(1, 6)
        queries = [(rng.randrange(npolys), rng.randrange(npoints)) for _ in range(rng.randrange(1, 61))]
        _same_grouping(queries, npolys, npoints)


def test_plan_refusals():
    import bzh2
    L = bzh2.load()
    vp, sz = ctypes.c_void_p, ctypes.c_size_t
    L.bzh_multiopen_plan.argtypes = [vp, sz, sz, sz, vp, vp, vp, vp, ctypes.POINTER(sz)]
    for queries, npolys, npoints in (([(2, 0)], 2, 1), ([(0, 3)], 2, 3), ([], 2, 2), ([(0, j) for j in range(9)], 1, 9)):
        with pytest.raises(bzh2.BzhError) as e:                       # an id out of range (twice), no queries, a 9-point set
            bzh2.multiopen_plan(queries, npolys, npoints)
        assert e.value.status == E_ARG
    assert bzh2.multiopen_plan([(0, j) for j in range(8)], 1, 9)[0] == [list(range(8))]   # 8 points are taken
    q = np.array([[0, 0]], dtype=np.uint32)
    bufs = [np.zeros(8, dtype=np.uint32) for _ in range(4)]
    nsets = sz(0)
    args = [vp(q.ctypes.data), 1, 1, 1] + [vp(b.ctypes.data) for b in bufs] + [ctypes.byref(nsets)]
    assert L.bzh_multiopen_plan(*args) == 0 and nsets.value == 1
    for i in (0, 4, 5, 6, 7, 8):                                         # each pointer in turn NULL
        a = list(args)
        a[i] = None
        assert L.bzh_multiopen_plan(*a) == E_ARG


def test_argument_refusals_without_a_device():
    """NULL ctx / bases / transcripts, and a host-resident batch: BZH_E_ARG before anything is touched.  The handles that are not
    the one under test are made-up non-NULL addresses: a refusal must not read through them."""
    import bzh2
    L = bzh2.load()
    vp, sz, ci = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
    L.bzh_multiopen_batch_device.argtypes = [vp, vp, sz, ctypes.c_uint, vp, sz, vp, sz, vp, vp, vp, sz, vp, sz, ci, ci, vp, sz, vp, vp]
    B, k, n = 2, 2, 4
    polys = np.zeros((B, 1, n, 4), dtype=np.uint64)
    blinds, points = (np.zeros((B, 1, 4), dtype=np.uint64) for _ in range(2))
    q = np.array([[0, 0]], dtype=np.uint32)
    rng = np.zeros(B * 64 * (n + 2 + 2 * k), dtype=np.uint8)
    status = np.full(B, 7, dtype=np.uint8)
    cap = M.proof_growth(k, 1)
    with bzh2.TranscriptBatch(bzh2.CURVE_VESTA, B, cap) as tb:   # host-resident: ctx None

        def call(ctx, bases, trs):
            return L.bzh_multiopen_batch_device(ctx, bases, B, k, vp(polys.ctypes.data), 1, None, 0, vp(blinds.ctypes.data), None,
                                                vp(points.ctypes.data), 1, vp(q.ctypes.data), 1, bzh2.FORM_CANONICAL, bzh2.MEM_HOST,
                                                vp(rng.ctypes.data), rng.size // B, trs, vp(status.ctypes.data))

        twin = bzh2.TranscriptBatch(bzh2.CURVE_VESTA, B, cap)
        assert call(None, None, None) == E_ARG
        assert call(None, None, tb.h) == E_ARG          # NULL ctx and bases
        assert call(None, vp(0x1000), tb.h) == E_ARG    # NULL ctx
        assert call(vp(0x1000), None, tb.h) == E_ARG    # NULL bases
        assert call(vp(0x1000), vp(0x1000), None) == E_ARG   # NULL transcripts
        assert call(vp(0x1000), vp(0x1000), tb.h) == E_ARG   # a host-resident batch: neither made-up handle is read
        # the Python mirror on a host-resident batch: refused the same way
        with pytest.raises(bzh2.BzhError) as e:
            tb.multiopen(None, k, polys, blinds, points, [(0, 0)], [rng[:rng.size // B].tobytes()] * B)
        assert e.value.status == E_ARG
        assert (status == 7).all() and tb.proof_len() == 0
        assert (tb.squeeze() == twin.squeeze()).all()   # the batch is as it was
        twin.close()


def test_lane_bodies_against_the_host_arithmetic_standalone_under_host_sanitizers(tmp_path):
    """mo_point_lane, mo_blind_lane, mo_interpolate_lane, mo_final_blind_lane and mo_status_lane against h_interpolate /
    h_batch_invert / fe_mul / fe_add, word for word, for Fp and Fq and both operand forms; sets of 1, 2, 3 and 8 points; points
    random, 0, 1 and p - 1 -- the lane with two equal points must come out flagged, with finite output and without a fault."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    csrc = os.path.join(ROOT, "battlezips-halo2_amd", "csrc")
    exe = str(tmp_path / "multiopen_scalars_check")
    subprocess.check_call([hipcc, "-O1", "-g", "-std=c++17", "--offload-arch=gfx950", "-Wno-unused-function",
                           "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                           "-I", csrc, os.path.join(ROOT, "tests", "helpers", "multiopen_scalars_check.hip"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(out.stdout[-3000:])
    assert out.returncode == 0 and out.stdout.strip().endswith("multiopen_scalars_check: ok"), out.stdout[-3000:] + out.stderr[-3000:]
    # per run: 14 x 5 point lanes, 4 x 5 interpolations, 4 x 5 blinds, 5 final blinds, 5 status bytes; 16 runs
    assert int(re.search(r"(\d+) lanes", out.stdout).group(1)) == 16 * (70 + 20 + 20 + 5 + 5)
