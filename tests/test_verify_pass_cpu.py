"""The verifier's device pass without a device: the key's scalar program (csrc/verify_program.hpp) through its host interpreter,
with host transcripts walking the key's schedule, against verify_host -- word for word on every proof verify_host accepts for
the device pass, a reject on every proof it refuses (tests/helpers/verify_pass_check.hip, a stand-alone program under the
host's address and undefined-behaviour sanitizers).  Keys and proofs come from the ORACLE.  Also the selector entry points'
statuses that need no device, and the header / exports agreement for the new names."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

from helpers import verify_pass_cases as VP
from helpers import vk_cases as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_NAMES = ("bzh_pk_verify_pass_select", "bzh_pk_verify_pass_selected", "bzh_verify_batch_vk_with")


def _circuit_block(num_instance):
    fc, sc = V.oracle_commitments(V.K, 70, num_instance)
    kb = V.bzv1(V.circuit(V.K, 70, num_instance)[5], fc, sc)
    inst, proof = VP.oracle_proof(num_instance, 0)
    ic = VP.instance_commitments(num_instance, inst)
    proofs = [(1, ic, proof)]
    other = None
    if num_instance == 1:
        inst1, proof1 = VP.oracle_proof(1, 1)
        ic1 = VP.instance_commitments(1, inst1)
        proofs += [(1, ic1, proof1), (1, ic1, proof), (1, ic, proof1)]      # two valid ones, and their instances swapped: both still parse
        other = VP.oracle_proof(1, 0, k=6)[1]
    proofs += [(expect, ic, pr) for _, pr, expect in VP.damaged(num_instance, proof, other)]
    proofs.append((0, ic, b""))
    return kb, max(num_instance, 1), proofs


def test_tape_against_verify_host_standalone_under_host_sanitizers(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    csrc = os.path.join(ROOT, "battlezips-halo2_amd", "csrc")
    exe = str(tmp_path / "verify_pass_check")
    subprocess.check_call([hipcc, "-O1", "-g", "-std=c++17", "--offload-arch=gfx950", "-Wno-unused-function",
                           "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                           "-I", csrc, os.path.join(ROOT, "tests", "helpers", "verify_pass_check.hip"), os.path.join(csrc, "transcript.hip"),
                           "-o", exe])
    circuits = [_circuit_block(ni) for ni in (0, 1, 2)]
    assert VP.oracle_accepts(1, *VP.oracle_proof(1, 0))                     # the oracle's own verifier takes what its prover made
    total = sum(len(c[2]) for c in circuits)
    path = tmp_path / "verify_pass_cases.bin"
    path.write_bytes(VP.check_file(circuits))
    out = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=600)
    print(out.stdout[-3000:])
    assert out.returncode == 0 and out.stdout.strip().endswith("verify_pass_check: ok"), out.stdout[-3000:] + out.stderr[-3000:]
    assert ("%d proofs" % total) in out.stdout


def test_selector_statuses_without_a_key():
    from bzh2 import native as N
    L = N._bind()
    w = ctypes.c_int(7)
    assert L.bzh_pk_verify_pass_select(None, N.VERIFY_PASS_HOST) == V.E_ARG
    assert L.bzh_pk_verify_pass_select(None, N.VERIFY_PASS_DEVICE) == V.E_ARG
    assert L.bzh_pk_verify_pass_selected(None, ctypes.byref(w)) == V.E_ARG and w.value == 7
    assert (N.VERIFY_PASS_HOST, N.VERIFY_PASS_DEVICE) == (0, 1)
    # an unknown pass_where is refused before anything else is looked at
    assert L.bzh_verify_batch_vk_with(None, None, None, None, 2, 1, None, 0, None, 0, None, None, None) == V.E_ARG
    assert L.bzh_verify_batch_vk_with(None, None, None, None, N.VERIFY_PASS_DEVICE, 1, None, 0, None, 0, None, None, None) == V.E_ARG


def test_header_and_exports_name_the_new_entries():
    import bzh2
    header = open(os.path.join(ROOT, "include", "bzh2.h")).read()
    L = bzh2.load()
    for name in NEW_NAMES:
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in bzh2.EXPORTS and getattr(L, name)
    assert re.search(r"BZH_VERIFY_PASS_HOST = 0, BZH_VERIFY_PASS_DEVICE = 1 \} bzh_verify_pass_where;", header)
    assert not re.search(r"BZH_VERIFY_POINTS_\w+ = 2", header)            # no third value on the points selector
