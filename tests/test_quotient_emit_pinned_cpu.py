"""What the quotient compiler and the two source emitters (csrc/quotient_compiler.hpp, csrc/quotient_emit.hpp) produce, pinned
byte for byte.  The builtin kernels are text printed on the host (bzh_quotient_source_for_circuit; csrc/gen_quotient.cpp prints
the same text into quotient_builtin.hip at build time) from a program that bzh_quotient_program_for_circuit hands out: when
text, program and hash are what they were, the device code and the kernels the program hash finds are what they were.  The
reference evaluates the same h(X) in halo2_proofs 0.2.0 `plonk::prover::create_proof` (UPSTREAM); nothing here is compared
with it: the pins are this library's own output, recorded in tests/golden/quotient_emit_pins.json (its header says from which
commit).  Host only.

A change that alters the emitted program on purpose regenerates the file -- python tests/test_quotient_emit_pinned_cpu.py
prints it -- and says why."""
import ctypes
import hashlib
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PINS = os.path.join(ROOT, "tests", "golden", "quotient_emit_pins.json")
CIRCUITS = {"ShotCircuit": 11, "BoardCircuit": 12}
KNOBS = ("BZH_VM2_LEAF", "BZH_VM2_CSE", "BZH_VM2_GLOBAL")
SETTINGS = [{}, {"BZH_VM2_LEAF": "0"}, {"BZH_VM2_LEAF": "8"}, {"BZH_VM2_CSE": "2"}, {"BZH_VM2_GLOBAL": "0"}]


def setting_id(setting):
    return ",".join("%s=%s" % kv for kv in sorted(setting.items())) or "default"


_blobs = {}


def measure(bzh2, name, setting):
    """the pinned figures of one circuit's quotient program under one setting of the compiler's knobs"""
    from bzh2 import circuits as Cm
    if name not in _blobs:
        lay = Cm.CircuitLayout(Cm.SHOT if name == "ShotCircuit" else Cm.BOARD, CIRCUITS[name])
        _blobs[name] = lay.blob()
        lay.close()
    blob = _blobs[name]
    L = bzh2.load()
    VP, SZ = ctypes.c_void_p, ctypes.c_size_t
    L.bzh_quotient_program_for_circuit.argtypes = [ctypes.c_int, ctypes.c_char_p, SZ, VP, SZ, ctypes.POINTER(SZ), VP, SZ, ctypes.POINTER(SZ),
                                                   ctypes.POINTER(ctypes.c_uint32)]
    L.bzh_quotient_source_for_circuit.argtypes = [ctypes.c_int, ctypes.c_char_p, SZ, ctypes.c_char_p, SZ, ctypes.POINTER(SZ),
                                                  ctypes.POINTER(ctypes.c_uint64)]
    old = {k: os.environ.pop(k, None) for k in KNOBS}
    try:
        os.environ.update(setting)
        nops, nconsts, stats = SZ(), SZ(), (ctypes.c_uint32 * 8)()
        assert L.bzh_quotient_program_for_circuit(0, blob, len(blob), None, 0, ctypes.byref(nops), None, 0, ctypes.byref(nconsts), stats) == 0
        ops, consts = ctypes.create_string_buffer(16 * nops.value), ctypes.create_string_buffer(40 * nconsts.value)
        assert L.bzh_quotient_program_for_circuit(0, blob, len(blob), ops, len(ops), ctypes.byref(nops), consts, len(consts),
                                                  ctypes.byref(nconsts), stats) == 0
        ln, h = SZ(), ctypes.c_uint64()
        assert L.bzh_quotient_source_for_circuit(0, blob, len(blob), None, 0, ctypes.byref(ln), ctypes.byref(h)) == 0
        buf = ctypes.create_string_buffer(ln.value + 1)
        assert L.bzh_quotient_source_for_circuit(0, blob, len(blob), buf, ln.value + 1, ctypes.byref(ln), ctypes.byref(h)) == 0
    finally:
        for k in KNOBS:
            os.environ.pop(k, None)
            if old[k] is not None:
                os.environ[k] = old[k]
    text = buf.raw[:ln.value]
    assert b"\0" not in text
    return {"source_sha256": hashlib.sha256(text).hexdigest(), "source_len": ln.value,
            "ops_sha256": hashlib.sha256(ops.raw).hexdigest(), "consts_sha256": hashlib.sha256(consts.raw).hexdigest(),
            "stats": [int(x) for x in stats], "program_hash": int(h.value)}


@pytest.fixture(scope="module")
def bzh2_lib():
    import __graft_entry__ as g
    import bzh2
    if not os.path.exists(bzh2.lib_path()):
        g.build()
    return bzh2


@pytest.fixture(scope="module")
def pins():
    with open(PINS) as f:
        return json.load(f)["pins"]


@pytest.mark.parametrize("setting", SETTINGS, ids=setting_id)
@pytest.mark.parametrize("name", sorted(CIRCUITS))
def test_emitted_program_and_source_are_the_pinned_ones(bzh2_lib, pins, name, setting):
    want = pins[name][setting_id(setting)]
    got = measure(bzh2_lib, name, setting)
    for k in ("stats", "program_hash", "ops_sha256", "consts_sha256", "source_len", "source_sha256"):   # the coarse figures first
        assert got[k] == want[k], k


if __name__ == "__main__":   # the golden file of the library that `import bzh2` finds, on stdout; argv[1]: what that library is
    sys.path.append(os.path.join(ROOT, "battlezips-halo2_amd"))
    import bzh2 as _bzh2
    print(json.dumps({"header": "sha256 / lengths / integers of the quotient programs and kernel sources emitted by " + sys.argv[1] +
                                " (tests/test_quotient_emit_pinned_cpu.py prints this file)",
                      "pins": {n: {setting_id(s): measure(_bzh2, n, s) for s in SETTINGS} for n in sorted(CIRCUITS)}}, indent=1))
