"""TEST HELPER (no GPU): inputs and programs shared by the expression-VM tests (tests/test_gpu_vm2.py, tests/test_gpu_exprvm.py,
tests/test_vm_model_cpu.py): operand columns built from the adversarial set of tests/helpers/field_edges.py plus uniform values
(tests/randutil.py), a generator of random valid VM v2 programs, and the real quotient programs of the reference's two circuits."""
from __future__ import annotations

import ctypes
import os
import random

import numpy as np

import randutil
from . import field_edges as E
from . import vm_model as M

ROTATIONS = [0, 0, 8, -8, 1, -1, 24, -300, 32767, -32768]
CONST_DTYPE = np.dtype([("sym", "<i4"), ("pad", "<u4"), ("val", "<u4", (8,))])   # bzh_quotient_program_for_circuit's constants


def uniform_ints(p: int, n: int, seed: int) -> list:
    return E.array_to_ints(randutil.uniform_below(np.random.default_rng(seed), n, p))


def operand_columns(p: int, ncols: int, n: int, seed: int = 0) -> list:
    """ncols columns of n values below p.  Column 0 cycles through edge_values(p) (0, 1, p - 1, R, R^2, limb patterns, ...); column
    c > 0 is, by row mod 4: p - column c-1 (the sum is p), column c-1 itself (the difference is 0), another edge value, a
    uniform value.  So neighbouring columns meet every corner of add / sub / rsub, and every column holds edge and uniform values."""
    edges = E.edge_values(p)
    uni = uniform_ints(p, ncols * n, seed + 1)
    cols = [[edges[i % len(edges)] for i in range(n)]]
    for c in range(1, ncols):
        prev = cols[-1]
        cols.append([(p - prev[i]) % p if i % 4 == 0 else prev[i] if i % 4 == 1 else
                     edges[(i * (2 * c + 1) + 17 * c) % len(edges)] if i % 4 == 2 else uni[c * n + i] for i in range(n)])
    return cols


def operand_consts(p: int, n: int, seed: int = 0) -> list:
    """n constants: edge values (0, 1, p - 1, R mod p, R^2 mod p first) and uniform ones, alternating"""
    edges, uni = E.edge_values(p), uniform_ints(p, n, seed + 2)
    pick = [0, 1, 3, 7, 8] + list(range(9, len(edges)))
    return [edges[pick[i // 2]] if i % 2 == 0 else uni[i] for i in range(n)]


def random_vm2_program(rng: random.Random, n: int, ncols: int, nconsts: int, nlds: int) -> list:
    """about n instructions over all 52 words and every leaf kind; a slot of the slot file is read only after a STORE to it.  The
    tail folds r3, r2, r1 and every written slot into r0, so that no value is dead."""
    written = []

    def leaf():
        kind = rng.choice([M.COLUMN, M.COLUMN, M.CONST, M.LDS])
        if kind == M.LDS and written:
            return (M.LDS, rng.choice(written), 0)
        if kind == M.CONST:
            return (M.CONST, rng.randrange(nconsts), 0)
        return (M.COLUMN, rng.randrange(ncols), rng.choice(ROTATIONS))

    ops = [(M.UN, M.LOAD, k, leaf(), M.NO_LEAF) for k in range(4)]
    words = list(M.VM2_WORDS)
    rng.shuffle(words)
    words += [rng.choice(M.VM2_WORDS) for _ in range(max(n - len(words), 0))]
    for form, op, pos in words:
        if form == M.UN and op == M.STORE:
            s = rng.randrange(nlds)
            ops.append((form, op, pos, (M.LDS, s, 0), M.NO_LEAF))
            if s not in written:
                written.append(s)
            continue
        ra, rb = M.vm2_reads(form, op)
        ops.append((form, op, pos, leaf() if ra else M.NO_LEAF, leaf() if rb else M.NO_LEAF))
    ops += [(M.SS, M.ADD, 2, M.NO_LEAF, M.NO_LEAF), (M.SS, M.SUB, 1, M.NO_LEAF, M.NO_LEAF), (M.SS, M.ADD, 0, M.NO_LEAF, M.NO_LEAF)]
    ops += [(M.SL, M.ADD if i % 2 else M.RSUB, 0, M.NO_LEAF, (M.LDS, s, 0)) for i, s in enumerate(sorted(written))]
    return ops


class QuotientProgram:
    """the VM v2 program bzh_prove_batch runs for a circuit's quotient, as bzh_quotient_program_for_circuit hands it out"""

    def __init__(self, ops, consts, stats):
        self.ops, self.consts = ops, consts                  # VM2_OP_DTYPE / CONST_DTYPE records
        self.nlds = int(stats[2])
        dec = M.decode_vm2(ops)
        cols = [x[1] for form, op, _, a, b in dec for used, x in zip(M.vm2_reads(form, op), (a, b)) if used and x[0] == M.COLUMN]
        self.ncols = 1 + max(cols)
        self.decoded = dec

    def bind(self, p: int, rng: random.Random) -> list:
        """one vector's constants (raw Montgomery-form bits): the literals as they are, one fresh value per symbol"""
        syms = {}
        return [sum(int(w) << (32 * i) for i, w in enumerate(c["val"])) if c["sym"] < 0 else syms.setdefault(int(c["sym"]), rng.randrange(p))
                for c in self.consts]


_programs = {}


def quotient_program(bzh2, name: str) -> QuotientProgram:
    """ShotCircuit at k = 11 or BoardCircuit at k = 12, compiled once per session (host only)"""
    if name not in _programs:
        from bzh2 import circuits as Cm
        lay = Cm.CircuitLayout(Cm.SHOT if name == "ShotCircuit" else Cm.BOARD, 11 if name == "ShotCircuit" else 12)
        blob = lay.blob()
        lay.close()
        L = bzh2.load()
        VP, SZ = ctypes.c_void_p, ctypes.c_size_t
        L.bzh_quotient_program_for_circuit.argtypes = [ctypes.c_int, ctypes.c_char_p, SZ, VP, SZ, ctypes.POINTER(SZ), VP, SZ,
                                                       ctypes.POINTER(SZ), ctypes.POINTER(ctypes.c_uint32)]
        old = os.environ.pop("BZH_VM2_LEAF", None)           # the default program, whatever the caller's environment says
        try:
            nops, nconsts, stats = SZ(), SZ(), (ctypes.c_uint32 * 8)()
            assert L.bzh_quotient_program_for_circuit(0, blob, len(blob), None, 0, ctypes.byref(nops), None, 0, ctypes.byref(nconsts), stats) == 0
            ops, consts = np.zeros(nops.value, M.VM2_OP_DTYPE), np.zeros(nconsts.value, CONST_DTYPE)
            assert L.bzh_quotient_program_for_circuit(0, blob, len(blob), ops.ctypes.data, ops.nbytes, ctypes.byref(nops), consts.ctypes.data,
                                                      consts.nbytes, ctypes.byref(nconsts), stats) == 0
        finally:
            if old is not None:
                os.environ["BZH_VM2_LEAF"] = old
        _programs[name] = QuotientProgram(ops, consts, list(stats))
    return _programs[name]


def word_histogram(decoded) -> dict:
    """{(form, op, pos): count}"""
    hist = {}
    for form, op, pos, _, _ in decoded:
        hist[(form, op, pos)] = hist.get((form, op, pos), 0) + 1
    return hist
