"""The device field arithmetic of csrc/field.cuh -- fe_add, fe_sub, fe_cond_sub_p, fe_neg and the generated Montgomery product
(field_mul_fips.inc), inline-assembly carry chains in a sparse (Pasta) and a dense (BN254) flavour -- bit for bit against Python
integers on the adversarial operand set of tests/helpers/field_edges.py: all 256 x 256 ordered pairs per field and operation.

Every call uses FORM_MONTGOMERY, so the chosen bits reach the registers unchanged (a canonical-form call would first multiply
them by R^2).  The programs are written by hand, one op each, and run in both instantiations of the evaluator
(k_expr_eval_regs4 for programs of at most four slots, k_expr_eval for wider ones).  No row is skipped or filtered; the
expected values come from `reference()` alone."""
import ctypes
import random

import numpy as np
import pytest

import pasta as O
from helpers import field_edges as E
from helpers.expr import ADD, COLUMN, CONST, COPY, MUL, NEG, SLOT, SUB, Program

pytestmark = pytest.mark.gpu

FIELDS = [0, 1, 2, 3]
OPNAME = {ADD: "add", SUB: "sub", MUL: "mul", NEG: "neg"}
COL_A, COL_B, NONE = (COLUMN, 0, 0), (COLUMN, 1, 0), (SLOT, 0, 0)
_cache = {}


def pair_table(fid):
    """(edge values, column A ints, column B ints, A array, B array) of the 65 536-row all-pairs table"""
    if fid not in _cache:
        vals = E.edge_values(E.MODULI[fid])
        a, b = E.all_pairs(vals)
        _cache[fid] = (vals, a, b, E.ints_to_array(a), E.ints_to_array(b))
    return _cache[fid]


def program(ops, result_slot, wide, consts=()):
    """hand-written bzh_expr_op program; `wide` prepends COPYs into slots 4..6 so that the program touches more than four
    slots and the library runs it in k_expr_eval instead of k_expr_eval_regs4"""
    prog = Program()
    for c in consts:
        prog.consts.append(c)
    if wide:
        prog.ops += [(COPY, 4, COL_A, NONE), (COPY, 5, COL_A, NONE), (COPY, 6, COL_A, NONE)]
    prog.ops += list(ops)
    prog.result_slot = result_slot
    return prog


def run(ctx, fid, prog, cols):
    import bzh2
    return E.array_to_ints(ctx.expr_eval(fid, prog, cols, form=bzh2.FORM_MONTGOMERY))


def check(got, want, a, b, fid, what):
    msg = E.first_mismatch(got, want, a, b, "field %d (%s) %s" % (fid, O.FIELD_BY_ID[fid].name, what))
    assert msg is None, msg


@pytest.mark.parametrize("wide", [False, True], ids=["regs4", "slotfile"])
@pytest.mark.parametrize("op", [ADD, SUB, MUL, NEG], ids=["add", "sub", "mul", "neg"])
@pytest.mark.parametrize("fid", FIELDS)
def test_one_op_all_pairs(gpu_ctx, fid, op, wide):
    p = E.MODULI[fid]
    _, a, b, A, B = pair_table(fid)
    prog = program([(op, 0, COL_A, NONE if op == NEG else COL_B)], 0, wide)
    got = run(gpu_ctx, fid, prog, [A, B])
    want = [E.reference(OPNAME[op], x, y, p) for x, y in zip(a, b)]
    check(got, want, a, b, fid, "%s(colA, colB)" % OPNAME[op])


@pytest.mark.parametrize("wide", [False, True], ids=["regs4", "slotfile"])
@pytest.mark.parametrize("fid", FIELDS)
def test_aliased_operands(gpu_ctx, fid, wide):
    """both operands in the same registers: op(colA, colA), and op(slot0, slot0) after a COPY; a - a is 0, never p"""
    p = E.MODULI[fid]
    _, a, b, A, B = pair_table(fid)
    for op in (ADD, SUB, MUL):
        want = [E.reference(OPNAME[op], x, x, p) for x in a]
        if op == SUB:
            assert not any(want)
        got = run(gpu_ctx, fid, program([(op, 0, COL_A, COL_A)], 0, wide), [A, B])
        check(got, want, a, a, fid, "%s(colA, colA)" % OPNAME[op])
        got = run(gpu_ctx, fid, program([(COPY, 0, COL_A, NONE), (op, 0, (SLOT, 0, 0), (SLOT, 0, 0))], 0, wide), [A, B])
        check(got, want, a, a, fid, "%s(slot0, slot0)" % OPNAME[op])
        got = run(gpu_ctx, fid, program([(COPY, 2, COL_A, NONE), (op, 1, (SLOT, 2, 0), (SLOT, 2, 0))], 1, wide), [A, B])
        check(got, want, a, a, fid, "slot1 = %s(slot2, slot2)" % OPNAME[op])


@pytest.mark.parametrize("wide", [False, True], ids=["regs4", "slotfile"])
@pytest.mark.parametrize("fid", FIELDS)
def test_constant_operands(gpu_ctx, fid, wide):
    """an operand from the constants table (every 16th edge value), on either side, against the column of all 256 edge values"""
    p = E.MODULI[fid]
    vals = pair_table(fid)[0]
    consts = vals[::16]
    V = E.ints_to_array(vals)
    for k, c in enumerate(consts):
        for op in (ADD, SUB, MUL):
            got = run(gpu_ctx, fid, program([(op, 0, COL_A, (CONST, k, 0))], 0, wide, consts), [V])
            check(got, [E.reference(OPNAME[op], x, c, p) for x in vals], vals, [c] * 256, fid, "%s(colA, const)" % OPNAME[op])
            got = run(gpu_ctx, fid, program([(op, 0, (CONST, k, 0), COL_A)], 0, wide, consts), [V])
            check(got, [E.reference(OPNAME[op], c, x, p) for x in vals], [c] * 256, vals, fid, "%s(const, colA)" % OPNAME[op])
        got = run(gpu_ctx, fid, program([(NEG, 0, (CONST, k, 0), NONE)], 0, wide, consts), [V])
        check(got, [E.reference("neg", c, 0, p)] * 256, [c] * 256, None, fid, "neg(const)")


@pytest.mark.parametrize("wide", [False, True], ids=["regs4", "slotfile"])
@pytest.mark.parametrize("fid", FIELDS)
def test_chains_on_results(gpu_ctx, fid, wide):
    """operands that are themselves results: ((a + b) - a) * b, (a - b) + b == a, -(-a) == a"""
    p = E.MODULI[fid]
    _, a, b, A, B = pair_table(fid)
    s0, s1 = (SLOT, 0, 0), (SLOT, 1, 0)
    got = run(gpu_ctx, fid, program([(ADD, 0, COL_A, COL_B), (SUB, 0, s0, COL_A), (MUL, 0, s0, COL_B)], 0, wide), [A, B])
    check(got, [E.reference("mul", y, y, p) for y in b], a, b, fid, "((a + b) - a) * b")
    got = run(gpu_ctx, fid, program([(SUB, 1, COL_A, COL_B), (ADD, 0, s1, COL_B)], 0, wide), [A, B])
    check(got, a, a, b, fid, "(a - b) + b")
    got = run(gpu_ctx, fid, program([(NEG, 1, COL_A, NONE), (NEG, 0, s1, NONE)], 0, wide), [A, B])
    check(got, a, a, None, fid, "-(-a)")


@pytest.mark.parametrize("fid", FIELDS)
def test_vec_mul_all_pairs_and_targeted_products(gpu_ctx, fid):
    """k_vec_mul (csrc/polyops.hip), another instantiation of the product: all pairs, and pairs whose Montgomery product is
    exactly a structured target t, so the accumulator before the final conditional subtraction is t or t + p"""
    import bzh2
    p = E.MODULI[fid]
    _, a, b, A, B = pair_table(fid)
    got = E.array_to_ints(gpu_ctx.vec_mul(fid, A, B, form=bzh2.FORM_MONTGOMERY))
    check(got, [E.reference("mul", x, y, p) for x, y in zip(a, b)], a, b, fid, "vec_mul")
    trip = E.targeted_products(p, random.Random(5 + fid))
    xs, ys, ts = [t[0] for t in trip], [t[1] for t in trip], [t[2] for t in trip]
    assert ts == [E.reference("mul", x, y, p) for x, y in zip(xs, ys)]
    got = E.array_to_ints(gpu_ctx.vec_mul(fid, E.ints_to_array(xs), E.ints_to_array(ys), form=bzh2.FORM_MONTGOMERY))
    check(got, ts, xs, ys, fid, "vec_mul, targeted products")
    prog = program([(MUL, 0, COL_A, COL_B)], 0, False)
    pad = (1 << (len(xs) - 1).bit_length()) - len(xs)           # the evaluator wants a power-of-two row count
    got = run(gpu_ctx, fid, prog, [E.ints_to_array(xs + [0] * pad), E.ints_to_array(ys + [0] * pad)])
    check(got, ts + [0] * pad, xs + [0] * pad, ys + [0] * pad, fid, "mul(colA, colB), targeted products")


@pytest.mark.parametrize("fid", FIELDS)
def test_field_convert_both_directions(gpu_ctx, fid):
    """bzh_field_convert: to Montgomery x -> x R, from Montgomery x -> x R^-1, on the raw edge bits"""
    import bzh2
    p = E.MODULI[fid]
    vals = pair_table(fid)[0]
    L = bzh2.load()
    L.bzh_field_convert.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_int]
    rinv = pow(E.R, -1, p)
    for to_mont, want in ((1, [x * E.R % p for x in vals]), (0, [x * rinv % p for x in vals])):
        buf = E.ints_to_array(vals)
        rc = L.bzh_field_convert(gpu_ctx.handle, fid, ctypes.c_void_p(buf.ctypes.data), len(vals), to_mont, bzh2.MEM_HOST)
        assert rc == 0
        check(E.array_to_ints(buf), want, vals, None, fid, "field_convert(to_montgomery=%d)" % to_mont)


@pytest.mark.parametrize("n", [256, 257])
@pytest.mark.parametrize("fid", FIELDS)
def test_vector_primitives_on_edge_vectors(gpu_ctx, fid, n):
    """batch_invert, prefix_product, inner_product, fold, eval_polynomial on vectors of raw edge bits in FORM_MONTGOMERY: the
    big-int definitions of oracle/pasta.py conjugated by R (input x stands for x R^-1, the output is the result times R)"""
    import bzh2
    F = O.FIELD_BY_ID[fid]
    p = F.p
    assert p == E.MODULI[fid]
    rinv = pow(E.R, -1, p)
    vals = pair_table(fid)[0]
    M = bzh2.FORM_MONTGOMERY
    v = (vals + [vals[3]])[:n]                                   # 257: one more element, p - 1 again
    w = (vals[::-1] + [vals[4]])[:n]                             # a second vector: the set reversed
    canon = lambda xs: [x * rinv % p for x in xs]
    mont = lambda xs: [x * E.R % p for x in xs]
    V, W = E.ints_to_array(v), E.ints_to_array(w)
    assert 0 in v
    got = E.array_to_ints(gpu_ctx.batch_invert(fid, V, form=M))
    want = mont(O.batch_invert(canon(v), F))
    assert [g for g, x in zip(got, v) if x == 0] == [0] * v.count(0)
    check(got, want, v, None, fid, "batch_invert n=%d" % n)
    nz = [x for x in v if x] + [v[1]] * v.count(0)               # a zero factor would blank everything after it
    got = E.array_to_ints(gpu_ctx.prefix_product(fid, E.ints_to_array(nz), form=M))
    check(got, mont(O.prefix_product(canon(nz), F)), nz, None, fid, "prefix_product n=%d" % n)
    got = E.array_to_ints(gpu_ctx.prefix_product(fid, V, form=M))
    check(got, mont(O.prefix_product(canon(v), F)), v, None, fid, "prefix_product with the zero, n=%d" % n)
    got = E.array_to_ints(gpu_ctx.inner_product(fid, V, W, form=M))
    check(got, mont([O.inner_product(canon(v), canon(w), F)]), v[:1], w[:1], fid, "inner_product n=%d" % n)
    for u in (vals[3], vals[7], vals[200]):                      # p - 1, R mod p, a uniform value
        got = E.array_to_ints(gpu_ctx.fold(fid, V, E.ints_to_array([u]), form=M)[0])
        check(got, mont(O.fold_scalars(canon(v), u * rinv % p, F)), v, [u] * n, fid, "fold n=%d" % n)
    xs = [vals[0], vals[1], vals[3], vals[7], vals[200]]          # 0, 1, p - 1, R mod p (the field's one), uniform
    polys = np.stack([V, W, V, W, V])
    got = E.array_to_ints(gpu_ctx.eval_polynomial(fid, polys, E.ints_to_array(xs), form=M))
    want = mont([O.eval_polynomial(canon(c), x * rinv % p, F) for c, x in zip([v, w, v, w, v], xs)])
    check(got, want, xs, None, fid, "eval_polynomial n=%d" % n)
