"""TEST HELPER (pure Python, no GPU, no library): integer models of the two expression instruction sets of csrc/exprvm.hip,
written from their specifications -- VM v1 from include/bzh2.h (bzh_expr_op), VM v2 from the header comment of csrc/vm2_isa.hpp --
and not from the kernels.  A program is executed row by row on Python integers.

  memory     column c of vector v is cols[c][v * strides[c] + row] (stride 0: one vector shared by all), constant i of vector v
             is consts[v * const_stride + i] (stride 0: shared); the result is a flat list, vector v at [v * size, (v + 1) * size)
  rotation   a column leaf reads row (row + rot) mod size
  state      registers (VM v2), slots (VM v1) and the slot file (VM v2) start at zero for every row.  The kernels clear only what
             they keep in registers (r0..r3; the four slots of k_expr_eval_regs4): a program meant for the device reads a slot
             only after writing it, which `unwritten_reads_vm2` / `unwritten_reads_vm1` check
  VM v2      SS r[p] = r[p] op r[p+1];  SL r[p] = r[p] op leaf b;  LL r[p] = leaf a op leaf b;  UN: NEG r[p] = -r[p],
             LOAD r[p] = leaf a, STORE slot a = r[p];  op in ADD, SUB, MUL, RSUB (b - a);  the result is r0
  VM v1      dst = a op b for ADD, SUB, MUL;  dst = -a (NEG), dst = a (COPY);  the result is slot `result_slot`
  product    a * b mod p, or with montgomery=True what the device computes on raw Montgomery-form bits, a * b * 2^-256 mod p

A word outside the instruction set raises ValueError: the model has no silent case."""
from __future__ import annotations

import numpy as np

# operand kinds (include/bzh2.h BZH_EXPR_SLOT / COLUMN / CONST; csrc/vm2_isa.hpp BZH_EXPR_LDS)
SLOT, COLUMN, CONST, LDS = 0, 1, 2, 3
# VM v1 operations
ADD, SUB, MUL, NEG, COPY = 0, 1, 2, 3, 4
V1_MAX_SLOTS = 24
# VM v2 forms, operations, and the operations of form UN
SS, SL, LL, UN = 0, 1, 2, 3
RSUB = 3
V2_NEG, LOAD, STORE = 0, 1, 2
FORM_NAME = {SS: "SS", SL: "SL", LL: "LL", UN: "UN"}
OP_NAME = {ADD: "ADD", SUB: "SUB", MUL: "MUL", RSUB: "RSUB"}
UN_NAME = {V2_NEG: "NEG", LOAD: "LOAD", STORE: "STORE"}
NO_LEAF = (0, 0, 0)

# the instruction set: every (form, operation, result register) that is a word -- 12 SS + 16 SL + 12 LL + 12 UN = 52
VM2_WORDS = ([(SS, op, pos) for pos in range(3) for op in (ADD, SUB, MUL, RSUB)] +
             [(SL, op, pos) for pos in range(4) for op in (ADD, SUB, MUL, RSUB)] +
             [(LL, op, pos) for pos in range(4) for op in (ADD, SUB, MUL)] +
             [(UN, op, pos) for pos in range(4) for op in (V2_NEG, LOAD, STORE)])
assert len(VM2_WORDS) == len(set(VM2_WORDS)) == 52

VM2_OP_DTYPE = np.dtype([("code", "u1"), ("a_kind", "u1"), ("b_kind", "u1"), ("pad", "u1"), ("a_idx", "<i4"), ("b_idx", "<i4"),
                         ("a_rot", "<i2"), ("b_rot", "<i2")])
assert VM2_OP_DTYPE.itemsize == 16


def word_name(form: int, op: int, pos: int) -> str:
    return "%s-%s-r%d" % (FORM_NAME[form], (UN_NAME if form == UN else OP_NAME).get(op, "op%d" % op), pos)


def encode_vm2(ops) -> np.ndarray:
    """[(form, op, pos, (kind, idx, rot), (kind, idx, rot))] -> the 16-byte instruction words: code = form << 4 | op << 2 | pos"""
    arr = np.zeros(len(ops), VM2_OP_DTYPE)
    for i, (form, op, pos, a, b) in enumerate(ops):
        arr[i] = ((form << 4) | (op << 2) | pos, a[0], b[0], 0, a[1], b[1], a[2], b[2])
    return arr


def decode_vm2(arr) -> list:
    return [(int(o["code"]) >> 4, (int(o["code"]) >> 2) & 3, int(o["code"]) & 3, (int(o["a_kind"]), int(o["a_idx"]), int(o["a_rot"])),
             (int(o["b_kind"]), int(o["b_idx"]), int(o["b_rot"]))) for o in arr]


def vm2_reads(form: int, op: int):
    """(reads leaf a, reads leaf b)"""
    return form == LL or (form == UN and op == LOAD), form in (SL, LL)


def _arith(op, a, b, p, mul):
    if op == ADD:
        return (a + b) % p
    if op == SUB:
        return (a - b) % p
    if op == MUL:
        return mul(a, b)
    if op == RSUB:
        return (b - a) % p
    raise ValueError("operation %d" % op)


def _product(p, montgomery):
    if not montgomery:
        return lambda a, b: a * b % p
    rinv = pow(1 << 256, -1, p)
    return lambda a, b: a * b * rinv % p


def run_vm2(ops, cols, strides, consts, const_stride, size, batch, nlds, p, montgomery=False) -> list:
    ops = decode_vm2(ops) if isinstance(ops, np.ndarray) else list(ops)
    for form, op, pos, _, _ in ops:
        if (form, op, pos) not in VM2_WORDS:
            raise ValueError("not an instruction word: form %d operation %d register %d" % (form, op, pos))
    mul = _product(p, montgomery)
    out = []
    for v in range(batch):
        cbase = v * const_stride
        for row in range(size):
            r = [0, 0, 0, 0]
            lds = [0] * nlds

            def leaf(x):
                kind, idx, rot = x
                if kind == COLUMN:
                    return cols[idx][v * strides[idx] + (row + rot) % size]
                if kind == CONST:
                    return consts[cbase + idx]
                if kind == LDS:
                    return lds[idx]
                raise ValueError("operand kind %d" % kind)

            for form, op, pos, a, b in ops:
                if form == SS:
                    r[pos] = _arith(op, r[pos], r[pos + 1], p, mul)
                elif form == SL:
                    r[pos] = _arith(op, r[pos], leaf(b), p, mul)
                elif form == LL:
                    r[pos] = _arith(op, leaf(a), leaf(b), p, mul)
                elif op == V2_NEG:
                    r[pos] = -r[pos] % p
                elif op == LOAD:
                    r[pos] = leaf(a)
                else:
                    lds[a[1]] = r[pos]
            out.append(r[0])
    return out


def run_vm1(ops, cols, strides, consts, const_stride, size, batch, result_slot, p, montgomery=False) -> list:
    """ops: [(op, dst, (kind, idx, rot), (kind, idx, rot))], as tests/helpers/expr.py's Program.ops"""
    mul = _product(p, montgomery)
    for op, dst, _, _ in ops:
        if not (0 <= op <= COPY and 0 <= dst < V1_MAX_SLOTS):
            raise ValueError("not an instruction: operation %d dst %d" % (op, dst))
    out = []
    for v in range(batch):
        cbase = v * const_stride
        for row in range(size):
            slots = [0] * V1_MAX_SLOTS

            def operand(x):
                kind, idx, rot = x
                if kind == SLOT:
                    return slots[idx]
                if kind == COLUMN:
                    return cols[idx][v * strides[idx] + (row + rot) % size]
                if kind == CONST:
                    return consts[cbase + idx]
                raise ValueError("operand kind %d" % kind)

            for op, dst, a, b in ops:
                if op == NEG:
                    slots[dst] = -operand(a) % p
                elif op == COPY:
                    slots[dst] = operand(a)
                else:
                    slots[dst] = _arith(op, operand(a), operand(b), p, mul)
            out.append(slots[result_slot])
    return out


def unwritten_reads_vm2(ops) -> list:
    """indices of the instructions that read a slot of the slot file before any STORE to it"""
    ops = decode_vm2(ops) if isinstance(ops, np.ndarray) else ops
    written, bad = set(), []
    for i, (form, op, pos, a, b) in enumerate(ops):
        ra, rb = vm2_reads(form, op)
        if (ra and a[0] == LDS and a[1] not in written) or (rb and b[0] == LDS and b[1] not in written):
            bad.append(i)
        if form == UN and op == STORE:
            written.add(a[1])
    return bad


def unwritten_reads_vm1(ops, result_slot) -> list:
    """indices of the instructions that read a slot before it was written (len(ops) stands for the result)"""
    written, bad = set(), []
    for i, (op, dst, a, b) in enumerate(ops):
        used = (a,) if op in (NEG, COPY) else (a, b)
        if any(x[0] == SLOT and x[1] not in written for x in used):
            bad.append(i)
        written.add(dst)
    if result_slot not in written:
        bad.append(len(ops))
    return bad


def vm1_slots_touched(ops, result_slot) -> int:
    """1 + the highest slot a program names: bzh_expr_eval_batch runs k_expr_eval_regs4 when this is at most 4, k_expr_eval above"""
    n = result_slot + 1
    for op, dst, a, b in ops:
        n = max(n, dst + 1)
        for x in ((a,) if op in (NEG, COPY) else (a, b)):
            if x[0] == SLOT:
                n = max(n, x[1] + 1)
    return n
