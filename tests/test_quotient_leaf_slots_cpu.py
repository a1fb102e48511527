"""Column leaves in cross-group slots (csrc/quotient_compiler.hpp, Compiler2::select_leaves; BZH_VM2_LEAF).  The quotient
program re-loaded the same (column, rotation) leaf in nearly every gate group; hot leaves are now loaded once into a slot
(V2_UN/V2_LOAD + V2_STORE when their residence begins) and read from it (slot operands) until it ends.  Host only: the
programs come from bzh_quotient_program_for_circuit, and are evaluated here by a small integer evaluator that mirrors
csrc/exprvm.hip's instruction forms.  The reference computes the same h(X) in halo2_proofs 0.2.0
`plonk::prover::create_proof` with one column query per use (UPSTREAM); SURVEY section 8 a6.

  load counts    multiplications per row unchanged, column loads per row strictly lower, Board at most 450
  value equality the leaf-slot program and the BZH_VM2_LEAF=0 program give the same value on random columns (64 rows, every
                 rotation wrapping), for 0, 1, the default and the maximum number of leaf slots
  live ranges    walking the op list: without the slot fills the program is the BZH_VM2_LEAF=0 program operation by operation,
                 and every read of a leaf slot finds in it exactly the (column, rotation) the other program loads there"""
import ctypes
import os
import random

import numpy as np
import pytest

P_FP = 0x40000000000000000000000000000000224698fc094cf91b992d30ed00000001
COLUMN, CONST, LDS = 1, 2, 3            # operand kinds (include/bzh2.h BZH_EXPR_COLUMN / BZH_EXPR_CONST; csrc/vm2_isa.hpp BZH_EXPR_LDS)
SS, SL, LL, UN = 0, 1, 2, 3             # instruction forms
ADD, SUB, MUL, RSUB = 0, 1, 2, 3
NEG, LOAD, STORE = 0, 1, 2
LEAF_MAX = 8                            # kV2LdsLeafMax
ROWS = 64

OP_DTYPE = np.dtype([("code", "u1"), ("a_kind", "u1"), ("b_kind", "u1"), ("pad", "u1"), ("a_idx", "<i4"), ("b_idx", "<i4"),
                     ("a_rot", "<i2"), ("b_rot", "<i2")])
CONST_DTYPE = np.dtype([("sym", "<i4"), ("pad", "<u4"), ("val", "<u4", (8,))])

# measured on the programs of this commit: (multiplications, column loads per row without leaf slots,
# with the default number, leaf slots the default program uses)
KNOWN = {"BoardCircuit": (475, 564, 340, 3), "ShotCircuit": (356, 421, 258, 3)}


@pytest.fixture(scope="module")
def bzh2_lib():
    import __graft_entry__ as g
    import bzh2
    if not os.path.exists(bzh2.lib_path()):
        g.build()
    return bzh2


class Prog:
    def __init__(self, ops, consts, stats, source29):
        self.ops, self.consts = ops, consts
        self.n_ops, self.muls, self.nlds, self.loads, self.leaf_slots, self.leaf_base = (int(x) for x in stats[:6])
        self.dot2 = source29.count(" = dot2x(")


_blobs = {}


def program(bzh2_lib, kind_name, leaf):
    """the quotient program of the circuit as Compiler2 emits it under BZH_VM2_LEAF=leaf (None: the default)"""
    from bzh2 import circuits as Cm
    if kind_name not in _blobs:
        lay = Cm.CircuitLayout(Cm.SHOT if kind_name == "ShotCircuit" else Cm.BOARD, 11 if kind_name == "ShotCircuit" else 12)
        _blobs[kind_name] = lay.blob()
        lay.close()
    blob = _blobs[kind_name]
    L = bzh2_lib.load()
    VP, SZ = ctypes.c_void_p, ctypes.c_size_t
    L.bzh_quotient_program_for_circuit.argtypes = [ctypes.c_int, ctypes.c_char_p, SZ, VP, SZ, ctypes.POINTER(SZ), VP, SZ, ctypes.POINTER(SZ),
                                                   ctypes.POINTER(ctypes.c_uint32)]
    L.bzh_quotient_source_for_circuit.argtypes = [ctypes.c_int, ctypes.c_char_p, SZ, ctypes.c_char_p, SZ, ctypes.POINTER(SZ),
                                                  ctypes.POINTER(ctypes.c_uint64)]
    old = os.environ.pop("BZH_VM2_LEAF", None)
    try:
        if leaf is not None:
            os.environ["BZH_VM2_LEAF"] = str(leaf)
        nops, nconsts, stats = SZ(), SZ(), (ctypes.c_uint32 * 8)()
        assert L.bzh_quotient_program_for_circuit(0, blob, len(blob), None, 0, ctypes.byref(nops), None, 0, ctypes.byref(nconsts), stats) == 0
        ops, consts = np.zeros(nops.value, OP_DTYPE), np.zeros(nconsts.value, CONST_DTYPE)
        assert L.bzh_quotient_program_for_circuit(0, blob, len(blob), ops.ctypes.data, ops.nbytes, ctypes.byref(nops), consts.ctypes.data,
                                                  consts.nbytes, ctypes.byref(nconsts), stats) == 0
        ln, h = SZ(), ctypes.c_uint64()
        assert L.bzh_quotient_source_for_circuit(0, blob, len(blob), None, 0, ctypes.byref(ln), ctypes.byref(h)) == 0
        buf = ctypes.create_string_buffer(ln.value + 1)
        assert L.bzh_quotient_source_for_circuit(0, blob, len(blob), buf, ln.value + 1, ctypes.byref(ln), ctypes.byref(h)) == 0
        text = buf.value.decode()
    finally:
        os.environ.pop("BZH_VM2_LEAF", None)
        if old is not None:
            os.environ["BZH_VM2_LEAF"] = old
    return Prog(ops, consts, list(stats), text[text.index("namespace bzh_q29_"):])


def decode(ops):
    return [(int(o["code"]) >> 4, (int(o["code"]) >> 2) & 3, int(o["code"]) & 3, (int(o["a_kind"]), int(o["a_idx"]), int(o["a_rot"])),
             (int(o["b_kind"]), int(o["b_idx"]), int(o["b_rot"]))) for o in ops]


def operands(form, op):
    """which of the two operand fields an instruction reads or writes: (a, b)"""
    return (form == LL or (form == UN and op != NEG), form in (SL, LL))


def count_loads(ops):
    n = 0
    for form, op, _, a, b in decode(ops):
        ua, ub = operands(form, op)
        n += (ua and a[0] == COLUMN) + (ub and b[0] == COLUMN)
    return n


def count_muls(ops):
    return sum(1 for form, op, _, _, _ in decode(ops) if form != UN and op == MUL)


def evaluate(prog, columns, const_of):
    """r0 of every row: the program over integers mod p.  columns[c][row]; const_of(entry) -> value"""
    p = P_FP
    cv = [const_of(c) for c in prog.consts]
    dec = decode(prog.ops)
    out = []
    for row in range(ROWS):
        r = [0, 0, 0, 0, 0]
        slots = {}

        def leaf(x):
            kind, idx, rot = x
            if kind == COLUMN:
                return columns[idx][(row + rot) % ROWS]
            if kind == CONST:
                return cv[idx]
            assert kind == LDS
            return slots[idx]                       # KeyError: a slot read before anything was stored to it

        def arith(op, a, b):
            return (a + b) % p if op == ADD else (a - b) % p if op == SUB else a * b % p if op == MUL else (b - a) % p
        for form, op, pos, a, b in dec:
            if form == SS:
                r[pos] = arith(op, r[pos], r[pos + 1])
            elif form == SL:
                r[pos] = arith(op, r[pos], leaf(b))
            elif form == LL:
                r[pos] = arith(op, leaf(a), leaf(b))
            elif op == NEG:
                r[pos] = -r[pos] % p
            elif op == LOAD:
                r[pos] = leaf(a)
            else:
                assert op == STORE and a[0] == LDS
                slots[a[1]] = r[pos]
        out.append(r[0])
    return out


def inputs(progs, seed):
    rng = random.Random(seed)
    ncols = 1 + max(max((int(o["a_idx"]) for o in pg.ops if o["a_kind"] == COLUMN), default=0) for pg in progs)
    ncols = max(ncols, 1 + max(max((int(o["b_idx"]) for o in pg.ops if o["b_kind"] == COLUMN), default=0) for pg in progs))
    columns = [[rng.randrange(P_FP) for _ in range(ROWS)] for _ in range(ncols)]
    syms = {}

    def const_of(c):   # literals are what they are; a challenge symbol (y, a power of y, theta, ...) is one random value
        if c["sym"] < 0:
            return sum(int(w) << (32 * i) for i, w in enumerate(c["val"])) % P_FP
        return syms.setdefault(int(c["sym"]), rng.randrange(P_FP))
    return columns, const_of


@pytest.fixture(scope="module")
def programs(bzh2_lib):
    """every program the tests look at, compiled once: {circuit: {setting: Prog}}"""
    return {name: {leaf: program(bzh2_lib, name, leaf) for leaf in (0, 1, None, LEAF_MAX)} for name in ("BoardCircuit", "ShotCircuit")}


@pytest.mark.parametrize("kind_name", ["BoardCircuit", "ShotCircuit"])
def test_leaf_slots_cut_the_loads_and_leave_the_products(programs, kind_name):
    base, dflt = programs[kind_name][0], programs[kind_name][None]
    for pg in (base, dflt):   # what the library reports is what the op list says
        assert pg.n_ops == len(pg.ops) and pg.loads == count_loads(pg.ops) and pg.muls == count_muls(pg.ops)
    print("%s: loads per row %d -> %d, products %d -> %d, leaf slots %d, dot2 pairs %d -> %d, slots %d -> %d" % (
        kind_name, base.loads, dflt.loads, base.muls, dflt.muls, dflt.leaf_slots, base.dot2, dflt.dot2, base.nlds, dflt.nlds))
    assert base.leaf_slots == 0
    assert dflt.muls == base.muls == KNOWN[kind_name][0]
    assert dflt.loads < base.loads
    if kind_name == "BoardCircuit":
        assert dflt.loads <= 450
    assert (base.loads, dflt.loads, dflt.leaf_slots) == KNOWN[kind_name][1:]
    assert dflt.dot2 >= base.dot2                      # the pairing pass still finds its pairs
    # more slots never cost loads; one slot already saves some
    one, most = programs[kind_name][1], programs[kind_name][LEAF_MAX]
    assert base.loads > one.loads >= dflt.loads >= most.loads and one.leaf_slots == 1 and most.leaf_slots <= LEAF_MAX
    assert one.muls == most.muls == base.muls


@pytest.mark.parametrize("kind_name", ["BoardCircuit", "ShotCircuit"])
def test_leaf_slot_programs_evaluate_to_the_same_values(programs, kind_name):
    progs = programs[kind_name]
    columns, const_of = inputs(list(progs.values()), 2024)
    want = evaluate(progs[0], columns, const_of)
    assert len(set(want)) == ROWS
    for leaf in (1, None, LEAF_MAX):
        assert evaluate(progs[leaf], columns, const_of) == want, leaf


@pytest.mark.parametrize("kind_name", ["BoardCircuit", "ShotCircuit"])
@pytest.mark.parametrize("leaf", [1, None, LEAF_MAX])
def test_leaf_slot_live_ranges(programs, kind_name, leaf):
    base, pg = decode(programs[kind_name][0].ops), decode(programs[kind_name][leaf].ops)
    lo, hi = programs[kind_name][leaf].leaf_base, programs[kind_name][leaf].leaf_base + programs[kind_name][leaf].leaf_slots
    assert hi == programs[kind_name][leaf].nlds        # the leaf slots are the last ones
    holds = {}                                         # leaf slot -> the (column, rotation) it holds now
    fills = reads = 0
    i = j = 0
    while j < len(pg):
        form, op, pos, a, b = pg[j]
        nxt = pg[j + 1] if j + 1 < len(pg) else None
        if form == UN and op == LOAD and a[0] == COLUMN and nxt and nxt[0] == UN and nxt[1] == STORE and lo <= nxt[3][1] < hi:
            assert nxt[2] == pos
            holds[nxt[3][1]] = (a[1], a[2])            # a fill: column leaf -> register -> leaf slot
            fills += 1
            j += 2
            continue
        bform, bop, bpos, ba, bb = base[i]
        assert (form, op, pos) == (bform, bop, bpos), (i, j)
        ua, ub = operands(form, op)
        for used, x, bx in ((ua, a, ba), (ub, b, bb)):
            if not used:
                continue
            if x[0] == LDS and lo <= x[1] < hi:
                assert not (form == UN and op == STORE), "only a fill writes a leaf slot"
                assert bx[0] == COLUMN and holds.get(x[1]) == (bx[1], bx[2]), (i, j, x, bx, holds.get(x[1]))
                reads += 1
            else:
                assert x == bx, (i, j)
        i += 1
        j += 1
    assert i == len(base)
    assert fills >= programs[kind_name][leaf].leaf_slots and reads > fills
    assert len(base) + 2 * fills == len(pg) and programs[kind_name][0].loads - reads + fills == programs[kind_name][leaf].loads
