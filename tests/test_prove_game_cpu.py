"""The game-input prover (bzh_prove_shots_device, bzh_prove_boards_device) without a device: the header / exports agreement for
the two names, the argument refusals that come before any device use, and the two lane bodies (csrc/prove_game_scalars.hpp) run
lane by lane on the host against the arithmetic of the host's synthesize_device (tests/helpers/prove_game_scalars_check.hip, a
stand-alone program built plain and under the host's address and undefined-behaviour sanitizers)."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("bzh_prove_shots_device", "bzh_prove_boards_device")
E_ARG = -1


def test_header_and_exports_name_the_entry_points():
    import bzh2
    from bzh2 import native as N
    header = open(os.path.join(ROOT, "include", "bzh2.h")).read()
    for name in NAMES:
        assert re.search(r"\bint %s\(" % name, header) and name in bzh2.EXPORTS
        getattr(bzh2.load(), name)
    assert header.index("typedef struct bzh_circuit bzh_circuit;") < header.index("int bzh_prove_shots_device(")
    assert hasattr(N.NativeProvingKey, "prove_shots_device") and hasattr(N.NativeProvingKey, "prove_boards_device")


def test_argument_refusals_without_a_device():
    """a NULL ctx, pk, circuit, input array, seeds, proofs or proof_lens, batch == 0, and a circuit of the other kind: BZH_E_ARG on
    made-up non-NULL ctx and key handles that a refusal must not read through; the outputs are untouched"""
    from bzh2 import circuits as Cm, native as N
    L = N._bind()
    vp = ctypes.c_void_p
    shot, board = Cm.CircuitLayout(Cm.SHOT, 11), Cm.CircuitLayout(Cm.BOARD, 12)
    try:
        B = 2
        words = np.zeros((B, 10, 4), dtype=np.uint64)
        seeds = bytes(32 * B)
        inst = np.full((B, 4, 4), 7, dtype=np.uint64)
        proofs, lens, st = np.full((B, 64), 7, dtype=np.uint8), (ctypes.c_size_t * B)(9, 9), np.full(B, 7, dtype=np.uint8)
        fake = vp(0x1000)
        at = lambda a: vp(a.ctypes.data)   # noqa: E731

        def call(which, **kw):
            a = dict(ctx=fake, pk=fake, circuit=(shot if which == "shots" else board).handle, batch=B, a=at(words), b=at(words), c=at(words))
            if which == "shots":
                a["d"] = at(words)
            a.update(seeds=seeds, inst=at(inst), proofs=at(proofs), pstride=64, lens=lens, st=at(st))
            a.update(kw)
            return getattr(L, "bzh_prove_%s_device" % which)(*a.values())

        for which in ("shots", "boards"):
            for kw in (dict(ctx=None), dict(pk=None), dict(circuit=None), dict(seeds=None), dict(batch=0), dict(a=None), dict(b=None),
                       dict(c=None), dict(proofs=None), dict(lens=None), dict(batch=65537)):
                assert call(which, **kw) == E_ARG, (which, kw)
        assert call("shots", d=None) == E_ARG
        assert call("boards", circuit=shot.handle) == E_ARG                     # a Shot circuit given to the boards call
        assert call("shots", circuit=board.handle) == E_ARG
        assert (proofs == 7).all() and list(lens) == [9, 9] and (st == 7).all() and (inst == 7).all()
    finally:
        shot.close()
        board.close()


def test_lane_bodies_against_the_hosts_arithmetic_standalone_plain_and_under_host_sanitizers(tmp_path):
    """pg_instance_lane for Shot and Board with the commitment coordinates 0, 1, p - 1 and seeded values and shot / hit words
    with bits above bit 127; pd_status_lane followed by pg_status_lane over all 8 x 16 combinations of synthesis and leaf bits"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    csrc = os.path.join(ROOT, "battlezips-halo2_amd", "csrc")
    src = os.path.join(ROOT, "tests", "helpers", "prove_game_scalars_check.hip")
    base = [hipcc, "-O1", "-g", "-std=c++17", "--offload-arch=gfx950", "-Wno-unused-function"]
    sanitizers = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"]
    for tag, extra in (("plain", []), ("sanitized", sanitizers)):
        exe = str(tmp_path / ("prove_game_scalars_check_" + tag))
        subprocess.check_call(base + extra + ["-I", csrc, src, "-o", exe])
        out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
        print(out.stdout[-3000:])
        assert out.returncode == 0 and out.stdout.strip().endswith("prove_game_scalars_check: ok"), out.stdout[-3000:] + out.stderr[-3000:]
        cases, lanes = map(int, re.search(r"(\d+) cases, (\d+) lanes", out.stdout).groups())
        assert cases == 2 * 3 * 4 * 2 + 3 * 2 and lanes == 2 * 4 * 2 * (1 + 3 + 70) + 6 * 128
