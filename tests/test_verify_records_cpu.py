"""bzh_verify_records_device without a device: the header / exports agreement for the name, the argument refusals that come
before any device use -- on a real verifying key read from bytes and made-up table handles a refusal must not read through --,
and the lane bodies (csrc/verify_records.hpp) run lane by lane on the host against bzh_record_decode on adversarial record
bytes (tests/helpers/verify_records_check.hip, a stand-alone program built plain and under the host's address and
undefined-behaviour sanitizers)."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from helpers import verify_pass_cases as VP
from helpers import vk_cases as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "bzh_verify_records_device"


def test_header_and_exports_name_the_entry_point():
    import bzh2
    from bzh2 import native as N
    header = open(os.path.join(ROOT, "include", "bzh2.h")).read()
    assert re.search(r"\bint %s\(" % NAME, header) and NAME in bzh2.EXPORTS
    getattr(bzh2.load(), NAME)
    assert header.index("#define BZH_RECORD_MAX_INPUTS") < header.index("int %s(" % NAME)
    assert hasattr(N.NativeVerifyingKey, "verify_records")
    assert re.search(r"largest batch a call takes is 4096", header)


def _vk(num_instance):
    from bzh2 import native as N
    fc, sc = V.oracle_commitments(V.K, 70, num_instance)
    return N.NativeVerifyingKey.from_bytes(V.bzv1(V.circuit(V.K, 70, num_instance)[5], fc, sc))


def test_argument_refusals_without_a_device():
    """a NULL ctx, vk, srs, g_lagrange, records or results; n_inputs of 0 and 5; a batch above the limit; a key with 0 and with 2
    instance columns; a stride one byte short of the key's proof length: BZH_E_ARG, and the outputs are untouched"""
    from bzh2 import native as N
    L = N._bind()
    vp = ctypes.c_void_p
    fake = vp(0x1000)
    keys = {ni: _vk(ni) for ni in (0, 1, 2)}
    try:
        B = 2
        plen = len(VP.oracle_proof(1, 0)[1])                                 # the key's proof length: what its prover writes
        stride = 144 + plen
        recs = np.zeros(B * stride, dtype=np.uint8)
        res = (ctypes.c_int * B)(7, 7)
        st = np.full(B, 7, dtype=np.uint8)

        def call(**kw):
            a = dict(ctx=fake, vk=keys[1].handle, srs=fake, lag=fake, batch=B, n_inputs=2, records=vp(recs.ctypes.data), stride=stride, g0=None,
                     res=res, st=vp(st.ctypes.data))
            a.update(kw)
            return L.bzh_verify_records_device(*a.values())

        for kw in (dict(ctx=None), dict(vk=None), dict(srs=None), dict(lag=None), dict(records=None), dict(res=None), dict(n_inputs=0),
                   dict(n_inputs=5), dict(batch=4097), dict(vk=keys[0].handle), dict(vk=keys[2].handle), dict(stride=stride - 1),
                   dict(stride=143), dict(stride=0)):
            assert call(**kw) == V.E_ARG, kw
        assert list(res) == [7, 7] and (st == 7).all()
    finally:
        for k in keys.values():
            k.close()


def test_lane_bodies_against_record_decode_standalone_plain_and_under_host_sanitizers(tmp_path):
    """vr_parse_lane on records with every header field at its bounds and the inputs p - 1, p, p + 1, 2^255, 2^256 - 1 and 0 in every
    position, against bzh_record_decode; vr_add_w_lane on the identity; vr_result_lane on rescaled, different and identity sums"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    csrc = os.path.join(ROOT, "battlezips-halo2_amd", "csrc")
    src = os.path.join(ROOT, "tests", "helpers", "verify_records_check.hip")
    base = [hipcc, "-O1", "-g", "-std=c++17", "--offload-arch=gfx950", "-Wno-unused-function"]
    sanitizers = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"]
    for tag, extra in (("plain", []), ("sanitized", sanitizers)):
        exe = str(tmp_path / ("verify_records_check_" + tag))
        subprocess.check_call(base + extra + ["-I", csrc, src, os.path.join(csrc, "record.hip"), "-o", exe])
        out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
        print(out.stdout[-3000:])
        assert out.returncode == 0 and out.stdout.strip().endswith("verify_records_check: ok"), out.stdout[-3000:] + out.stderr[-3000:]
        records, lanes = map(int, re.search(r"(\d+) records, (\d+) lanes", out.stdout).groups())
        assert records == 2 * 70 and lanes == 70 * 2 + 70 * 4 + 4 * 6 + 3 + 2
