"""The opening on device-resident transcripts (bzh_ipa_open_batch_device) without a device: the header / exports agreement for the
new name, the argument refusals that need no device, and the scalar kernels' lane bodies (csrc/ipa_scalars.hpp) run lane by lane
on the host against the arithmetic the host-transcript opening does between its rounds (tests/helpers/ipa_scalars_check.hip, a
stand-alone program under the host's address and undefined-behaviour sanitizers)."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "bzh_ipa_open_batch_device"
E_ARG = -1


def test_header_and_exports_name_the_entry_point():
    import bzh2
    header = open(os.path.join(ROOT, "include", "bzh2.h")).read()
    assert re.search(r"\bint %s\(" % NAME, header) and NAME in bzh2.EXPORTS
    getattr(bzh2.load(), NAME)
    assert hasattr(bzh2.TranscriptBatch, "ipa_open")


def test_argument_refusals_without_a_device():
    """NULL ctx / bases / transcripts, and a host-resident batch: BZH_E_ARG before anything is touched.  The handles that are not
    the one under test are made-up non-NULL addresses: a refusal must not read through them."""
    import bzh2
    L = bzh2.load()
    vp, sz, ci = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
    L.bzh_ipa_open_batch_device.argtypes = [vp, vp, vp, ci, ci, sz, vp, vp, vp, sz, vp, vp, vp]
    B, n, k = 2, 4, 2
    polys = np.zeros((B, n, 4), dtype=np.uint64)
    blinds, x3s, out_v = (np.zeros((B, 4), dtype=np.uint64) for _ in range(3))
    rng = np.zeros(B * 64 * (n + 1 + 2 * k), dtype=np.uint8)
    status = np.full(B, 7, dtype=np.uint8)
    with bzh2.TranscriptBatch(bzh2.CURVE_VESTA, B, 32 * (1 + 2 * k) + 64) as tb:   # host-resident: ctx None

        def call(ctx, bases, trs):
            return L.bzh_ipa_open_batch_device(ctx, bases, vp(polys.ctypes.data), bzh2.FORM_CANONICAL, bzh2.MEM_HOST, B, vp(blinds.ctypes.data),
                                               vp(x3s.ctypes.data), vp(rng.ctypes.data), rng.size // B, trs, vp(out_v.ctypes.data),
                                               vp(status.ctypes.data))

        twin = bzh2.TranscriptBatch(bzh2.CURVE_VESTA, B, 32 * (1 + 2 * k) + 64)
        assert call(None, None, None) == E_ARG
        assert call(None, None, tb.h) == E_ARG          # NULL ctx and bases
        assert call(None, vp(0x1000), tb.h) == E_ARG    # NULL ctx
        assert call(vp(0x1000), None, tb.h) == E_ARG    # NULL bases
        assert call(vp(0x1000), vp(0x1000), None) == E_ARG   # NULL transcripts
        # the Python mirror on a host-resident batch: refused the same way
        with pytest.raises(bzh2.BzhError) as e:
            tb.ipa_open(None, polys, blinds, x3s, [rng[:rng.size // B].tobytes()] * B)
        assert e.value.status == E_ARG
        assert (status == 7).all() and not out_v.any() and tb.proof_len() == 0
        assert (tb.squeeze() == twin.squeeze()).all()   # the batch is as it was
        twin.close()


def test_lane_bodies_against_the_host_arithmetic_standalone_under_host_sanitizers(tmp_path):
    """ipa_x3_lane, ipa_head_lane, ipa_round_lane and ipa_tail_lane against fe_mul / fe_add / h_batch_invert, word for word, for
    Fp and Fq and both operand forms; round challenges 1, 2, p - 1, random and 0 -- the zero lane must come out flagged, with
    u^-1 = 0 and f unchanged, and without a fault."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    csrc = os.path.join(ROOT, "battlezips-halo2_amd", "csrc")
    exe = str(tmp_path / "ipa_scalars_check")
    subprocess.check_call([hipcc, "-O1", "-g", "-std=c++17", "--offload-arch=gfx950", "-Wno-unused-function",
                           "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                           "-I", csrc, os.path.join(ROOT, "tests", "helpers", "ipa_scalars_check.hip"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(out.stdout[-3000:])
    assert out.returncode == 0 and out.stdout.strip().endswith("ipa_scalars_check: ok"), out.stdout[-3000:] + out.stderr[-3000:]
    assert int(re.search(r"(\d+) lanes", out.stdout).group(1)) == 16 * 5 * 6
