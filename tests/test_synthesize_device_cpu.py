"""Device witness synthesis without a device: the kernels' lane bodies (csrc/synthesize_device.hpp) run lane by lane on the host
against the Layouter path for both circuits (tests/helpers/synth_device_check.hip, a stand-alone program under the host's
address and undefined-behaviour sanitizers), the argument refusals of the two new entry points, and the header / exports
agreement for their names."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_NAMES = ("bzh_synthesize_shot_with", "bzh_synthesize_board_with")
E_ARG = -1


def test_lane_bodies_against_the_layouter_standalone_under_host_sanitizers(tmp_path):
    """Every word of the advice tensor, the instances and the status of each operand, Shot at k = 11 and Board at k = 12; the
    program prints how many lanes it ran.  It also calls syn_incomplete_exceptional directly on hand-made operands (P and P,
    P and -P, an identity on either side).  Through the entry points no scalar reaches that flag: the running sum before window w
    is [sum_{j<w} (k_j + 2) 8^j] B, a multiple below 2 * 8^w, and the window's point is [(k_w + 2) 8^w] B, a multiple of at least
    2 * 8^w and below q for every w <= 83, so the two never share an x-coordinate and neither is the identity."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    csrc = os.path.join(ROOT, "battlezips-halo2_amd", "csrc")
    exe = str(tmp_path / "synth_device_check")
    subprocess.check_call([hipcc, "-O1", "-g", "-std=c++17", "--offload-arch=gfx950", "-Wno-unused-function",
                           "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                           "-I", csrc, os.path.join(ROOT, "tests", "helpers", "synth_device_check.hip"), os.path.join(csrc, "circuits.hip"),
                           os.path.join(csrc, "synthesize_device.hip"), "-o", exe])
    env = dict(os.environ, BZH_CACHE_DIR=os.path.join(ROOT, "battlezips-halo2_amd", ".bzh2_cache"))
    out = subprocess.run([exe], capture_output=True, text=True, timeout=900, env=env)
    print(out.stdout[-3000:])
    assert out.returncode == 0 and out.stdout.strip().endswith("synth_device_check: ok"), out.stdout[-3000:] + out.stderr[-3000:]
    lanes = int(re.search(r"(\d+) lanes", out.stdout).group(1))
    assert lanes > 20000


def test_argument_refusals_without_a_device():
    import bzh2
    from bzh2 import circuits as Cm
    L = Cm._bind()
    VP = ctypes.c_void_p
    lay = Cm.CircuitLayout(Cm.SHOT, 11)
    blay = Cm.CircuitLayout(Cm.BOARD, 12)
    try:
        _, state = Cm.board_witness([(3, 3, True), (5, 4, False), (0, 1, False), (0, 5, True), (6, 1, False)], None)
        words = [np.ascontiguousarray(bzh2.int_to_limbs(v)) for v in (state.value, 0x5eed, 1 << 35, 1)]
        ptrs = [VP(w.ctypes.data) for w in words]
        adv = np.zeros((1, lay.num_advice, lay.n, 4), dtype=np.uint64)
        inst = np.zeros((4, 4), dtype=np.uint64)

        def call(form, mem, where, handle=None):
            return L.bzh_synthesize_shot_with(None, handle or lay.handle, 1, *ptrs, VP(adv.ctypes.data), form, mem, VP(inst.ctypes.data), 1, where)

        # BZH_SYNTH_DEVICE needs a ctx, device memory and Montgomery form; `where` is one of the two
        for form in (bzh2.FORM_CANONICAL, bzh2.FORM_MONTGOMERY):
            for mem in (bzh2.MEM_HOST, bzh2.MEM_DEVICE):
                assert call(form, mem, Cm.SYNTH_DEVICE) == E_ARG
        assert call(bzh2.FORM_MONTGOMERY, bzh2.MEM_HOST, 2) == E_ARG and call(bzh2.FORM_MONTGOMERY, bzh2.MEM_HOST, -1) == E_ARG
        assert call(bzh2.FORM_MONTGOMERY, bzh2.MEM_HOST, Cm.SYNTH_HOST, blay.handle) == E_ARG          # a Board circuit
        assert L.bzh_synthesize_board_with(None, lay.handle, 1, *ptrs[:3], VP(adv.ctypes.data), bzh2.FORM_MONTGOMERY, bzh2.MEM_HOST,
                                           VP(inst.ctypes.data), 1, Cm.SYNTH_HOST) == E_ARG               # a Shot circuit
        with pytest.raises(ValueError):
            lay.synthesize([], where="gpu")
        # BZH_SYNTH_HOST through the new entry point is bzh_synthesize_shot
        assert call(bzh2.FORM_MONTGOMERY, bzh2.MEM_HOST, Cm.SYNTH_HOST) == 0
        want, winst = np.zeros_like(adv), np.zeros_like(inst)
        assert L.bzh_synthesize_shot(None, lay.handle, 1, *ptrs, VP(want.ctypes.data), bzh2.FORM_MONTGOMERY, bzh2.MEM_HOST,
                                     VP(winst.ctypes.data), 1) == 0
        assert (adv == want).all() and (inst == winst).all() and adv.any()
    finally:
        lay.close()
        blay.close()


def test_header_and_exports_name_the_new_entry_points():
    import bzh2
    header = open(os.path.join(ROOT, "include", "bzh2.h")).read()
    for name in NEW_NAMES:
        assert re.search(r"\bint %s\(" % name, header) and name in bzh2.EXPORTS
        getattr(bzh2.load(), name)
    assert re.search(r"#define BZH_SYNTH_HOST\s+0", header) and re.search(r"#define BZH_SYNTH_DEVICE\s+1", header)
