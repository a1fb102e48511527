"""The integer model of the two expression instruction sets (tests/helpers/vm_model.py), which the GPU tests of csrc/exprvm.hip
(tests/test_gpu_vm2.py, tests/test_gpu_exprvm.py) compare the kernels with, bit for bit.  No GPU here.

  hand-computed  a dozen small programs over the field of 101 elements, four rows, results written out by hand
  compiler       VM v1: the model on what tests/helpers/expr.compile_expression emits against evaluate_tree, the definition
  real programs  VM v2: the model on the ShotCircuit / BoardCircuit quotient programs against the evaluator of
                 tests/test_quotient_leaf_slots_cpu.py's kind (same values), and which of the 52 instruction words those programs
                 contain -- how much of the interpreter's switch the proof-byte tests reach
  generator      the random programs the GPU tests run are valid: words of the set only, no slot read before it is stored to"""
import os
import random

import pytest

from helpers import vm_cases as VC
from helpers import vm_model as M
from helpers.vm_model import ADD, COLUMN, CONST, COPY, LDS, LL, LOAD, MUL, NEG, NO_LEAF, RSUB, SL, SLOT, SS, STORE, SUB, UN, V2_NEG

P = 101
COL0, COL1 = [1, 2, 3, 4], [10, 20, 30, 40]
CONSTS = [5, 100]
C0, C1 = (COLUMN, 0, 0), (COLUMN, 1, 0)


def vm2(ops, cols=(COL0, COL1), strides=(0, 0), consts=CONSTS, const_stride=0, batch=1, nlds=2, **kw):
    return M.run_vm2(ops, list(cols), list(strides), consts, const_stride, 4, batch, nlds, P, **kw)


def vm1(ops, result_slot, cols=(COL0, COL1), strides=(0, 0), consts=CONSTS, const_stride=0, batch=1, **kw):
    return M.run_vm1(ops, list(cols), list(strides), consts, const_stride, 4, batch, result_slot, P, **kw)


def load(pos, leaf):
    return (UN, LOAD, pos, leaf, NO_LEAF)


def test_vm2_load_and_rotation():
    assert vm2([load(0, C0)]) == [1, 2, 3, 4]
    assert vm2([load(0, (COLUMN, 0, 1))]) == [2, 3, 4, 1]
    assert vm2([load(0, (COLUMN, 0, -1))]) == [4, 1, 2, 3]
    assert vm2([load(0, (COLUMN, 0, 5))]) == [2, 3, 4, 1]           # (row + 5) mod 4
    assert vm2([load(0, (COLUMN, 0, -3))]) == [2, 3, 4, 1]          # (row - 3) mod 4
    assert vm2([load(0, (COLUMN, 0, 32767))]) == [4, 1, 2, 3]       # 32767 = 3 mod 4
    assert vm2([load(0, (CONST, 1, 0))]) == [100] * 4


def test_vm2_result_is_r0_and_registers_start_at_zero():
    assert vm2([load(1, C0)]) == [0] * 4
    assert vm2([load(3, C0), (SS, ADD, 0, NO_LEAF, NO_LEAF)]) == [0] * 4      # r0 + r1, both still zero
    assert vm2([(UN, V2_NEG, 0, NO_LEAF, NO_LEAF)]) == [0] * 4                   # -0 is 0, not 101


def test_vm2_ll_operand_order():
    assert vm2([(LL, SUB, 0, C1, C0)]) == [9, 18, 27, 36]
    assert vm2([(LL, SUB, 0, C0, C1)]) == [92, 83, 74, 65]
    assert vm2([(LL, ADD, 0, C1, (CONST, 1, 0))]) == [9, 19, 29, 39]         # + 100 = - 1
    assert vm2([(LL, MUL, 0, C1, C1)]) == [100, 97, 92, 85]                  # 100, 400, 900, 1600 mod 101


def test_vm2_sl_and_rsub():
    assert vm2([load(0, C0), (SL, SUB, 0, NO_LEAF, (CONST, 0, 0))]) == [97, 98, 99, 100]   # r0 - 5
    assert vm2([load(0, C0), (SL, RSUB, 0, NO_LEAF, (CONST, 0, 0))]) == [4, 3, 2, 1]       # 5 - r0
    assert vm2([load(0, C0), (SL, MUL, 0, (CONST, 1, 0), C1)]) == [10, 40, 90, 59]         # leaf a is not read


def test_vm2_ss_uses_the_register_above():
    pre = [load(0, C0), load(1, C1)]
    assert vm2(pre + [(SS, SUB, 0, NO_LEAF, NO_LEAF)]) == [92, 83, 74, 65]                 # r0 - r1
    assert vm2(pre + [(SS, RSUB, 0, NO_LEAF, NO_LEAF)]) == [9, 18, 27, 36]                 # r1 - r0
    # r1 = r1 * r2 leaves r0 alone; then r0 = r0 + r1
    pre3 = pre + [load(2, (CONST, 0, 0)), (SS, MUL, 1, NO_LEAF, NO_LEAF)]
    assert vm2(pre3) == [1, 2, 3, 4]
    assert vm2(pre3 + [(SS, ADD, 0, NO_LEAF, NO_LEAF)]) == [51, 1, 52, 2]                  # 1+50, 2+100, 3+49, 4+99 mod 101
    # r2 = r2 - r3, folded down: r0 = r0 + (r1 + (r2 - r3))
    prog = [load(0, C0), load(1, C0), load(2, C1), load(3, C0), (SS, SUB, 2, NO_LEAF, NO_LEAF), (SS, ADD, 1, NO_LEAF, NO_LEAF),
            (SS, ADD, 0, NO_LEAF, NO_LEAF)]
    assert vm2(prog) == [11, 22, 33, 44]


def test_vm2_neg_store_load():
    assert vm2([load(0, (CONST, 1, 0)), (UN, V2_NEG, 0, NO_LEAF, NO_LEAF)]) == [1] * 4
    prog = [load(3, C1), (UN, STORE, 3, (LDS, 1, 0), NO_LEAF), load(0, (LDS, 1, 0))]
    assert vm2(prog) == [10, 20, 30, 40]
    assert vm2(prog[:2] + [load(0, (LDS, 0, 0))]) == [0] * 4                  # the other slot: the model's slot file starts at zero
    assert M.unwritten_reads_vm2(prog) == [] and M.unwritten_reads_vm2(prog[:2] + [load(0, (LDS, 0, 0))]) == [2]
    # a STORE leaves its register as it was, and a slot is per row
    assert vm2([load(0, C0), (UN, STORE, 0, (LDS, 0, 0), NO_LEAF), (SL, ADD, 0, NO_LEAF, (LDS, 0, 0))]) == [2, 4, 6, 8]


def test_vm2_batch_strides():
    col = [1, 2, 3, 4, 0, 0, 5, 6, 7, 8]                                       # two vectors, 6 apart
    consts = [5, 100, 0, 7, 9]                                                 # two vectors, 3 apart
    prog = [(LL, ADD, 0, (COLUMN, 0, 1), (CONST, 0, 0)), (SL, ADD, 0, NO_LEAF, C1)]
    assert vm2(prog, cols=(col, COL1), strides=(6, 0), consts=consts, const_stride=3, batch=2) == [17, 28, 39, 46, 23, 34, 45, 52]
    assert vm2(prog, cols=(col, COL1), strides=(0, 0), consts=consts, const_stride=0, batch=2) == [17, 28, 39, 46] * 2


def test_vm2_montgomery_product():
    r = (1 << 256) % P
    assert vm2([(LL, MUL, 0, C0, (CONST, 0, 0))], consts=[r], montgomery=True) == COL0     # R mod p is the one of that form
    assert vm2([(LL, MUL, 0, C0, (CONST, 0, 0))], consts=[r * r % P], montgomery=True) == [x * r % P for x in COL0]
    assert vm2([(LL, ADD, 0, C0, (CONST, 0, 0))], consts=[r], montgomery=True) == [(x + r) % P for x in COL0]


def test_vm2_words_outside_the_set_are_errors():
    for bad in [(SS, ADD, 3), (SS, RSUB, 3), (LL, RSUB, 0), (LL, RSUB, 3), (UN, 3, 0), (4, 0, 0)]:
        assert bad not in M.VM2_WORDS
        with pytest.raises(ValueError):
            vm2([(bad[0], bad[1], bad[2], C0, C1)])
    with pytest.raises(ValueError):
        vm2([load(0, (SLOT, 0, 0))])
    names = [M.word_name(*w) for w in M.VM2_WORDS]
    assert len(set(names)) == 52 and "SS-RSUB-r2" in names and "UN-STORE-r3" in names and "LL-MUL-r0" in names
    arr = M.encode_vm2([(SL, RSUB, 2, NO_LEAF, (COLUMN, 7, -300))])
    assert arr.tobytes() == bytes([0x1E, 0, 1, 0]) + (0).to_bytes(4, "little") + (7).to_bytes(4, "little") + bytes(2) + (-300).to_bytes(2, "little", signed=True)
    assert M.decode_vm2(arr) == [(SL, RSUB, 2, NO_LEAF, (COLUMN, 7, -300))]


def test_vm1_operations_and_operand_order():
    s1 = (SLOT, 1, 0)
    assert vm1([(SUB, 0, C1, C0)], 0) == [9, 18, 27, 36]
    assert vm1([(SUB, 0, C0, C1)], 0) == [92, 83, 74, 65]
    assert vm1([(SUB, 2, (CONST, 0, 0), (COLUMN, 0, -1))], 2) == [1, 4, 3, 2]                # 5 - [4, 1, 2, 3]
    assert vm1([(COPY, 1, C0, NO_LEAF), (SUB, 0, s1, s1)], 0) == [0] * 4
    assert vm1([(COPY, 1, C0, NO_LEAF), (SUB, 0, (CONST, 0, 0), s1)], 0) == [4, 3, 2, 1]
    assert vm1([(ADD, 0, C0, (CONST, 1, 0))], 0) == [0, 1, 2, 3]
    assert vm1([(MUL, 23, C1, C1)], 23) == [100, 97, 92, 85]
    assert vm1([(NEG, 0, C0, C1)], 0) == [100, 99, 98, 97]                                   # operand b is not read
    assert vm1([(NEG, 0, (SLOT, 5, 0), NO_LEAF)], 0) == [0] * 4                              # a fresh slot is zero, and -0 is 0
    assert vm1([(COPY, 3, (COLUMN, 1, 2), NO_LEAF)], 3) == [30, 40, 10, 20]
    assert vm1([(COPY, 3, C0, NO_LEAF)], 2) == [0] * 4                                       # the result is result_slot


def test_vm1_batch_strides_and_helpers():
    col = [1, 2, 3, 4, 0, 0, 5, 6, 7, 8]
    consts = [5, 100, 0, 7, 9]
    prog = [(ADD, 4, (COLUMN, 0, 1), (CONST, 0, 0)), (ADD, 0, (SLOT, 4, 0), C1)]
    assert vm1(prog, 0, cols=(col, COL1), strides=(6, 0), consts=consts, const_stride=3, batch=2) == [17, 28, 39, 46, 23, 34, 45, 52]
    assert M.vm1_slots_touched(prog, 0) == 5 and M.vm1_slots_touched(prog[:1], 3) == 5 and M.vm1_slots_touched([(NEG, 1, C0, (SLOT, 9, 0))], 0) == 2
    assert M.unwritten_reads_vm1(prog, 0) == [] and M.unwritten_reads_vm1(prog[1:], 0) == [0] and M.unwritten_reads_vm1(prog, 1) == [2]
    with pytest.raises(ValueError):
        vm1([(5, 0, C0, C1)], 0)
    with pytest.raises(ValueError):
        vm1([(ADD, 24, C0, C1)], 0)
    with pytest.raises(ValueError):
        vm1([(ADD, 0, (LDS, 0, 0), C1)], 0)


@pytest.mark.parametrize("seed", range(6))
def test_vm1_model_against_the_tree_definition(seed):
    """what compile_expression emits, run by the model, is the tree's value (helpers/expr.evaluate_tree) at every row"""
    from helpers import expr
    from test_gpu_exprvm import rand_tree
    p = (1 << 61) - 1
    rng = random.Random(seed)
    size, ncols = 32, 6
    cols = [[rng.randrange(p) for _ in range(size)] for _ in range(ncols)]
    tree = rand_tree(rng, ncols, 6, p)
    prog = expr.compile_expression(tree, p)
    assert M.unwritten_reads_vm1(prog.ops, prog.result_slot) == []
    got = M.run_vm1(prog.ops, cols, [0] * ncols, prog.consts, 0, size, 1, prog.result_slot, p)
    assert got == [expr.evaluate_tree(tree, cols, r, size, p) for r in range(size)]


@pytest.mark.parametrize("seed", range(16))
def test_random_vm2_programs_are_valid(seed):
    rng = random.Random(seed)
    nlds = [1, 4, 16, 17, 32][seed % 5]
    ops = VC.random_vm2_program(rng, 300, 7, 5, nlds)
    assert 300 <= len(ops) <= 300 + 4 + 3 + nlds
    assert {(f, o, q) for f, o, q, _, _ in ops} == set(M.VM2_WORDS)
    assert M.unwritten_reads_vm2(ops) == []
    kinds = {x[0] for f, o, _, a, b in ops for used, x in zip(M.vm2_reads(f, o), (a, b)) if used}
    assert kinds == {COLUMN, CONST, LDS}
    assert all(x[1] < nlds for f, o, _, a, b in ops for x in (a, b) if x[0] == LDS)
    p = VC.E.MODULI[0]
    cols = VC.operand_columns(p, 7, 16, seed)
    out = M.run_vm2(M.encode_vm2(ops), cols, [0] * 7, VC.operand_consts(p, 5), 0, 16, 1, nlds, p)
    assert len(set(out)) > 8                                                   # the result depends on the row: not degenerate


def test_operand_columns_meet_the_corners():
    p = VC.E.MODULI[1]
    cols = VC.operand_columns(p, 4, 256)
    assert all(0 <= x < p for c in cols for x in c) and len(set(map(tuple, cols))) == 4
    assert {0, 1, p - 1, VC.E.R % p, VC.E.R * VC.E.R % p} <= set(cols[0])
    for a, b in zip(cols, cols[1:]):
        assert sum(1 for x, y in zip(a, b) if x and x + y == p) >= 60 and sum(1 for x, y in zip(a, b) if x == y) >= 64
    consts = VC.operand_consts(p, 8)
    assert consts[0] == 0 and consts[2] == 1 and consts[4] == p - 1 and consts[6] == VC.E.R % p


@pytest.fixture(scope="module")
def bzh2_lib():
    import __graft_entry__ as g
    import bzh2
    if not os.path.exists(bzh2.lib_path()):
        g.build()
    return bzh2


@pytest.mark.parametrize("name", ["ShotCircuit", "BoardCircuit"])
def test_real_quotient_programs_use_words_of_the_set_only(bzh2_lib, name):
    """Which instruction words the quotient compiler emits for the reference's circuits -- all that the proof-byte tests reach of
    the interpreter.  Only membership in the set is asserted; the table is printed (pytest -s)."""
    pg = VC.quotient_program(bzh2_lib, name)
    hist = VC.word_histogram(pg.decoded)
    assert set(hist) <= set(M.VM2_WORDS), sorted(set(hist) - set(M.VM2_WORDS))
    assert M.unwritten_reads_vm2(pg.decoded) == []                            # the slot file needs no clearing
    print("%s: %d instructions, %d of the 52 words, %d slots, %d columns" % (name, len(pg.decoded), len(hist), pg.nlds, pg.ncols))
    for w in M.VM2_WORDS:
        print("  %-12s %5d" % (M.word_name(*w), hist.get(w, 0)))
    assert pg.nlds > 16                                                       # a program of the 64-row kernel


def test_model_runs_the_real_program_like_the_leaf_slot_evaluator(bzh2_lib):
    """two independently written evaluators of the same ISA agree on a 700-instruction program"""
    import test_quotient_leaf_slots_cpu as T
    pg = VC.quotient_program(bzh2_lib, "ShotCircuit")
    other = T.Prog(pg.ops, pg.consts, [len(pg.ops), 0, pg.nlds, 0, 0, 0, 0, 0], "")
    columns, const_of = T.inputs([other], 7)
    want = T.evaluate(other, columns, const_of)
    consts = [const_of(c) for c in pg.consts]
    assert M.run_vm2(pg.ops, columns, [0] * len(columns), consts, 0, T.ROWS, 1, pg.nlds, T.P_FP) == want
