"""The device-resident batch prover in one call (bzh_prove_device_plan, bzh_prove_batch_device, bzh_prove_batch_device_seeded)
without a device: the header / exports agreement for the three names, the plan against the four drawing leaves' plans and the
oracle's constraint systems, the plan's refusals, the argument refusals that need no device, and the two lane bodies
(csrc/prove_device_scalars.hpp) run lane by lane on the host against a plain loop (tests/helpers/prove_device_scalars_check.hip,
a stand-alone program built plain and under the host's address and undefined-behaviour sanitizers)."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import pasta as O
from helpers.real_parity import accelerated_oracle
from test_products_device_cpu import _blobs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("bzh_prove_device_plan", "bzh_prove_batch_device", "bzh_prove_batch_device_seeded")
E_ARG = -1
F = O.FP


def test_header_and_exports_name_the_entry_points():
    import bzh2
    from bzh2 import native as N
    header = open(os.path.join(ROOT, "include", "bzh2.h")).read()
    for name in NAMES:
        assert re.search(r"\bint %s\(" % name, header) and name in bzh2.EXPORTS
        getattr(bzh2.load(), name)
    assert header.index("int bzh_prove_batch_seeded(") < header.index("int bzh_prove_device_plan(") < header.index("int bzh_prove_batch_device(")
    assert callable(bzh2.prove_device_plan) and hasattr(N.NativeProvingKey, "prove_device_plan") and hasattr(N.NativeProvingKey, "prove_batch_device")


def _check_plan(name, blob, cs, proof_len=None):
    import bzh2
    cid = bzh2.CURVE_VESTA
    got = bzh2.prove_device_plan(cid, blob)
    cshape, gshape = bzh2.commitments_plan(cid, blob), bzh2.grand_products_plan(cid, blob)
    n, na, ni, nl = cshape[0], cshape[3], cshape[4], cshape[5]
    nz, npieces = gshape[5], cs.chunk_len + 1                            # degree - 1 pieces
    try:
        vshape = bzh2.vanishing_plan(cid, blob)[0]
        assert (vshape[6], vshape[7]) == (npieces, n + 1 + npieces), name
    except bzh2.BzhError as e:                                           # a circuit without a VM v2 program has no vanishing plan; the draws
        assert e.status == -4, name                                      # are the random polynomial, its blind and a blind per piece
    draws = (cshape[6], gshape[7], n + 1 + npieces, n + 2 + 2 * cs.k)    # the four leaf plans' draws, in chain order
    assert got[:4] == draws, name
    assert got[4] == sum(draws), name
    # (64 * got[4] is the key-independent rng_bytes those four plans imply; the GPU tests hold it against bzh_pk_info's)
    assert (na, ni, nl) == (cs.num_advice, cs.num_instance, len(cs.lookups)), name
    assert got[6] == ni + na + 1 + nz + 2 * nl + 1, name
    assert got[7] == 65535 // max(na, ni, 2 * nl, nz, npieces), name
    if proof_len is not None:
        assert got[5] == proof_len, name
    return got


def test_plan_for_the_sample_circuits_and_the_reference_circuits():
    seen = set()
    for name, blob, cs in _blobs():
        got = _check_plan(name, blob, cs)
        seen.add(got[7])
    assert len(seen) >= 3                                                 # several widest kinds among the circuits


@accelerated_oracle
def test_plan_against_the_oracles_proofs(oracle_c):
    """k = 5 with the lookup, k = 4 without instance column and lookup, the two-column lookup: the plan's proof bytes are the
    oracle proof's length"""
    from bzh2 import circuit_data as Pd
    from helpers import commitments_cases as K
    for name, case in (("k5 lookup", K.case(5, True, None, 3)), ("k4 no instance", K.no_instance_case()), ("two-column", K.two_column_case())):
        cs, circ, proofs = case[0], case[2], case[5]
        assert len({len(p) for p in proofs}) == 1
        _check_plan(name, Pd.serialize_circuit(circ, F.p, 0x1234), cs, len(proofs[0]))


def test_plan_refusals():
    import bzh2
    L = bzh2.load()
    L.bzh_prove_device_plan.argtypes = [ctypes.c_int, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_void_p]
    blob = _blobs()[0][1]
    shape = np.full(8, 5, dtype=np.uint32)
    args = [0, blob, len(blob), ctypes.c_void_p(shape.ctypes.data)]
    for change in ((1, None), (3, None), (2, len(blob) // 2), (0, 7)):          # NULL pointers, a truncated blob, no such curve
        a = list(args)
        a[change[0]] = change[1]
        assert L.bzh_prove_device_plan(*a) == E_ARG and (shape == 5).all(), change
    assert L.bzh_prove_device_plan(*args) == 0 and shape[4] == shape[:4].sum()
    with pytest.raises(bzh2.BzhError) as e:
        bzh2.prove_device_plan(bzh2.CURVE_VESTA, blob[:len(blob) // 2])
    assert e.value.status == E_ARG


def test_argument_refusals_without_a_device():
    """every refusal that reads neither the key nor the device, on made-up non-NULL handles that a refusal must not read through;
    the outputs are untouched"""
    import bzh2
    from bzh2 import native as N
    L = N._bind()
    vp = ctypes.c_void_p
    B, n = 2, 4
    adv, inst = np.zeros((B, 1, n, 4), dtype=np.uint64), np.zeros((B, 1, 1, 4), dtype=np.uint64)
    raw = np.zeros(B * 64 * 16, dtype=np.uint8)
    proofs, lens, st = np.full((B, 64), 7, dtype=np.uint8), (ctypes.c_size_t * B)(9, 9), np.full(B, 7, dtype=np.uint8)
    fake = vp(0x1000)
    at = lambda a: vp(a.ctypes.data)   # noqa: E731

    def call(seeded=False, **kw):
        a = dict(ctx=fake, pk=fake, batch=B, adv=at(adv), form=bzh2.FORM_CANONICAL, mem=bzh2.MEM_HOST, inst=at(inst), rows=1, rng=at(raw),
                 stride=64 * 16, proofs=at(proofs), pstride=64, lens=lens, st=at(st))
        a.update(kw)
        if seeded:
            a["rng"] = None if a["rng"] is None else raw.tobytes()[:32 * B]
            del a["stride"]
            return L.bzh_prove_batch_device_seeded(*a.values())
        return L.bzh_prove_batch_device(*a.values())

    for seeded in (False, True):
        for kw in (dict(ctx=None), dict(pk=None), dict(adv=None), dict(rng=None), dict(proofs=None), dict(lens=None), dict(batch=0), dict(form=2),
                   dict(form=-1), dict(mem=2), dict(mem=-1), dict(mem=bzh2.MEM_DEVICE),                       # a device call in canonical form
                   dict(mem=bzh2.MEM_DEVICE, form=bzh2.FORM_MONTGOMERY, adv=vp(adv.ctypes.data + 8))):       # a misaligned device pointer
            assert call(seeded, **kw) == E_ARG, (seeded, kw)
    assert call(stride=0) == E_ARG                                           # the unseeded call without a stride
    assert (proofs == 7).all() and list(lens) == [9, 9] and (st == 7).all()


def test_lane_bodies_against_a_plain_loop_standalone_plain_and_under_host_sanitizers(tmp_path):
    """pd_blind_lane and pd_status_lane for Fp and Fq: the blind table with counts of 0 (ni = 0, nl = 0), strides of 0 and batches
    past a wave; the status fold over all 16 combinations of leaf bytes, with the bytes 1, 0x80, 0xf0 and 0xff"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    csrc = os.path.join(ROOT, "battlezips-halo2_amd", "csrc")
    src = os.path.join(ROOT, "tests", "helpers", "prove_device_scalars_check.hip")
    base = [hipcc, "-O1", "-g", "-std=c++17", "--offload-arch=gfx950", "-Wno-unused-function"]
    sanitizers = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"]
    for tag, extra in (("plain", []), ("sanitized", sanitizers)):
        exe = str(tmp_path / ("prove_device_scalars_check_" + tag))
        subprocess.check_call(base + extra + ["-I", csrc, src, "-o", exe])
        out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
        print(out.stdout[-3000:])
        assert out.returncode == 0 and out.stdout.strip().endswith("prove_device_scalars_check: ok"), out.stdout[-3000:] + out.stderr[-3000:]
        cases, lanes = map(int, re.search(r"(\d+) cases, (\d+) lanes", out.stdout).groups())
        assert cases == 5 * 3 * 3 + 4 * 2 and lanes > 10000
