"""GPU parity of the gate-expression evaluator: compiled straight-line
programs on the GPU against direct recursive evaluation of the expression tree with Python integers.
Reference seam: poly::Evaluator under vanishing::Argument::construct (create_proof step 6,
benches/shot.rs:68); gate shapes as built by the reference's create_gate calls
(src/chips/bitify.rs:63-88, src/chips/transpose.rs:60-88)."""
import random

import numpy as np
import pytest

import coracle as C
import pasta as O

pytestmark = pytest.mark.gpu


def rand_tree(rng, ncols, depth, p):
    from helpers.expr import Constant, Negated, Product, Query, Scaled, Sum
    if depth == 0 or rng.random() < 0.15:
        if rng.random() < 0.75:
            return Query(rng.randrange(ncols), rng.choice([0, 0, 8, -8, 16, -24]))
        return Constant(rng.randrange(p))
    k = rng.randrange(6)
    if k == 0:
        return Negated(rand_tree(rng, ncols, depth - 1, p))
    if k == 1:
        return Scaled(rand_tree(rng, ncols, depth - 1, p), rng.randrange(p))
    if k in (2, 3):
        return Sum(rand_tree(rng, ncols, depth - 1, p), rand_tree(rng, ncols, depth - 1, p))
    return Product(rand_tree(rng, ncols, depth - 1, p), rand_tree(rng, ncols, depth - 1, p))


@pytest.mark.parametrize("seed", range(8))
def test_random_expression_trees(gpu_ctx, seed):
    from helpers import expr
    F = O.FP
    rng = random.Random(seed)
    size, ncols = 256, 6
    cols = [[rng.randrange(F.p) for _ in range(size)] for _ in range(ncols)]
    tree = rand_tree(rng, ncols, 6, F.p)
    prog = expr.compile_expression(tree, F.p)
    got = C.array_to_ints(gpu_ctx.expr_eval(0, prog, [C.ints_to_array(c) for c in cols]))
    want = [expr.evaluate_tree(tree, cols, r, size, F.p) for r in range(size)]
    assert got == want


def test_num2bits_and_permutation_shaped_gates_folded_with_y(gpu_ctx):
    """Gate shapes of the reference folded Horner-style with a challenge y, as vanishing::construct does:
    bitify (src/chips/bitify.rs:63-88): bit*(1-bit), e2' - 2*e2, lc1' - lc1 - bit*e2;
    plus a permutation-product shaped term z(wX)*(a+beta*s+gamma) - z(X)*(a+beta*id+gamma)."""
    from helpers.expr import Constant, Product, Query, Sum, compile_expression, evaluate_tree
    F = O.FQ
    rng = random.Random(42)
    size, ext = 1 << 10, 8
    cols = [[rng.randrange(F.p) for _ in range(size)] for _ in range(7)]
    bit, lc1, e2, z, a, sig, idc = (Query(i) for i in range(7))
    nxt = lambda q: Query(q.column, ext)                       # Rotation::next() on the extended domain
    beta, gamma, y = (Constant(rng.randrange(F.p)) for _ in range(3))
    one = Constant(1)
    gates = [
        bit * (one - bit),
        nxt(e2) - e2 * 2,
        nxt(lc1) - lc1 - bit * e2,
        nxt(z) * (a + beta * sig + gamma) - z * (a + beta * idc + gamma),
    ]
    folded = gates[0]
    for g in gates[1:]:
        folded = folded * y + g
    prog = compile_expression(folded, F.p)
    got = C.array_to_ints(gpu_ctx.expr_eval(1, prog, [C.ints_to_array(c) for c in cols]))
    assert got == [evaluate_tree(folded, cols, r, size, F.p) for r in range(size)]


def test_program_validation(gpu_ctx):
    import bzh2
    from helpers import expr
    prog = expr.compile_expression(expr.Query(0) * expr.Query(3), O.P)   # column 3 does not exist below
    with pytest.raises(bzh2.BzhError):
        gpu_ctx.expr_eval(0, prog, [np.zeros((8, 4), dtype=np.uint64)])


# ---- hand-written programs against the integer model of tests/helpers/vm_model.py ------------------------------------------
# The compiler above never emits SUB, always runs one vector of 256 or 1024 rows, and which of the two kernels a tree reaches is
# up to the tree.  Below, every program is written by hand so that the dispatch of expr_eval_t (csrc/exprvm.hip) is known:
# k_expr_eval_regs4 when the program names slots 0..3 only, k_expr_eval when it names slot 4 or slot 23.  Operands are the
# adversarial columns of tests/helpers/vm_cases.operand_columns; every comparison is equality of all limbs.
KERNELS = {"regs4": 3, "generic-slot4": 4, "generic-slot23": 23}      # name -> the highest slot the program names
V1_FIELDS = [0, 1, 2]


def v1_data(fid, n, ncols=4, seed=0):
    from helpers import field_edges as E, vm_cases as VC
    p = E.MODULI[fid]
    return VC.operand_columns(p, ncols, n, seed=seed + fid), VC.operand_consts(p, 4, seed=seed + fid)


def v1_device(ctx, fid, ops, result_slot, cols, consts, log_size, batch=1, strides=None, const_stride=0, nconsts=None, mont=True,
              device=False):
    """bzh_expr_eval_batch on host arrays, or (device=True) on torch tensors holding the same bits"""
    import ctypes
    import bzh2
    from helpers import expr, field_edges as E
    L = bzh2.load()
    VP, SZ = ctypes.c_void_p, ctypes.c_size_t
    L.bzh_expr_eval_batch.argtypes = [VP, ctypes.c_int, ctypes.POINTER(expr.ExprOp), SZ, ctypes.POINTER(VP), ctypes.POINTER(SZ), SZ, VP, SZ, SZ,
                                      ctypes.c_uint, ctypes.c_int, SZ, ctypes.c_int, ctypes.c_int, VP]
    prog = expr.Program()
    prog.ops = list(ops)
    size = 1 << log_size
    arrays = [E.ints_to_array(c) for c in cols]
    carr = E.ints_to_array(consts)
    nconsts = nconsts if nconsts is not None else (const_stride or len(consts))
    form = bzh2.FORM_MONTGOMERY if mont else bzh2.FORM_CANONICAL
    strides_arr = (SZ * max(len(cols), 1))(*(strides or [0] * len(cols)))
    if device:
        import torch
        tensors = [torch.from_numpy(a.view(np.int64)).cuda() for a in arrays]
        out = torch.zeros((batch * size, 4), dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        ptrs = (VP * max(len(cols), 1))(*[t.data_ptr() for t in tensors])
        rc = L.bzh_expr_eval_batch(ctx.handle, fid, prog.as_array(), len(ops), ptrs, strides_arr, len(cols), carr.ctypes.data, nconsts,
                                   const_stride, log_size, result_slot, batch, form, bzh2.MEM_DEVICE, out.data_ptr())
        ctx._check(rc, "bzh_expr_eval_batch")
        ctx.sync()
        return E.array_to_ints(out.cpu().numpy().view(np.uint64))
    out = np.zeros((batch * size, 4), dtype=np.uint64)
    ptrs = (VP * max(len(cols), 1))(*[a.ctypes.data for a in arrays])
    rc = L.bzh_expr_eval_batch(ctx.handle, fid, prog.as_array(), len(ops), ptrs, strides_arr, len(cols), carr.ctypes.data, nconsts,
                               const_stride, log_size, result_slot, batch, form, bzh2.MEM_HOST, out.ctypes.data)
    ctx._check(rc, "bzh_expr_eval_batch")
    return E.array_to_ints(out)


def v1_check(ctx, fid, ops, result_slot, cols, consts, log_size, kernel, what, batch=1, strides=None, const_stride=0, nconsts=None,
             mont=True, device=False):
    from helpers import field_edges as E, vm_model as M
    touched = M.vm1_slots_touched(ops, result_slot)
    assert touched == KERNELS[kernel] + 1 and (touched <= 4) == (kernel == "regs4"), "the program does not reach the kernel it names"
    assert M.unwritten_reads_vm1(ops, result_slot) == [], "k_expr_eval does not clear its slots"
    got = v1_device(ctx, fid, ops, result_slot, cols, consts, log_size, batch, strides, const_stride, nconsts, mont, device)
    want = M.run_vm1(ops, cols, strides or [0] * len(cols), consts, const_stride, 1 << log_size, batch, result_slot, E.MODULI[fid],
                     montgomery=mont)
    bad = [i for i in range(len(want)) if got[i] != want[i]]
    assert len(got) == len(want) and not bad, "%s, %s, field %d: %d of %d rows differ; first at row %d: got=%#066x want=%#066x" % (
        what, kernel, fid, len(bad), len(want), bad[0], got[bad[0]], want[bad[0]])
    return want


def v1_slot_layouts(kernel):
    """(slot of operand a, slot of operand b, dst) twice: the kernel's highest slot once as an operand, once as the destination"""
    hi = KERNELS[kernel]
    return [(hi, 1, 0), (1, 2, hi)]


@pytest.mark.parametrize("fid", V1_FIELDS)
@pytest.mark.parametrize("kernel", list(KERNELS))
def test_v1_every_opcode_with_every_pair_of_operand_kinds(gpu_ctx, kernel, fid):
    """SUB first (no compiled program holds one), ADD, MUL with all nine pairs of operand kinds, NEG and COPY with all three"""
    from helpers.expr import ADD, COLUMN, CONST, COPY, MUL, NEG, SLOT, SUB
    cols, consts = v1_data(fid, 256)
    none = (SLOT, 0, 0)
    for sa, sb, d in v1_slot_layouts(kernel):
        pre = [(COPY, sa, (COLUMN, 2, 8), none), (COPY, sb, (COLUMN, 3, -8), none)]
        as_a = {"slot": (SLOT, sa, 0), "column": (COLUMN, 0, -1), "const": (CONST, 0, 0)}
        as_b = {"slot": (SLOT, sb, 0), "column": (COLUMN, 1, 1), "const": (CONST, 3, 0)}
        for op, name in ((SUB, "SUB"), (ADD, "ADD"), (MUL, "MUL")):
            for ka, a in as_a.items():
                for kb, b in as_b.items():
                    v1_check(gpu_ctx, fid, pre + [(op, d, a, b)], d, cols, consts, 8, kernel, "slot%d = %s(%s, %s)" % (d, name, ka, kb))
        for op, name in ((NEG, "NEG"), (COPY, "COPY")):
            for ka, a in as_a.items():
                v1_check(gpu_ctx, fid, pre + [(op, d, a, as_b["slot"])], d, cols, consts, 8, kernel, "slot%d = %s(%s)" % (d, name, ka))
        # the operands of SUB the other way round, and a - a
        want = v1_check(gpu_ctx, fid, pre + [(SUB, d, as_b["column"], as_a["column"])], d, cols, consts, 8, kernel, "SUB(b, a)")
        assert want != v1_check(gpu_ctx, fid, pre + [(SUB, d, as_a["column"], as_b["column"])], d, cols, consts, 8, kernel, "SUB(a, b)")
        assert not any(v1_check(gpu_ctx, fid, pre + [(SUB, d, as_a["slot"], as_a["slot"])], d, cols, consts, 8, kernel, "SUB(slot, slot)"))


def v1_program(kernel):
    """((c0[r+1] - c1[r-1]) * k0 + c2[r+8]) - (-c3) over two slots, the kernel's highest among them"""
    from helpers.expr import ADD, COLUMN, CONST, MUL, NEG, SLOT, SUB
    hi = KERNELS[kernel]
    return [(SUB, hi, (COLUMN, 0, 1), (COLUMN, 1, -1)), (MUL, hi, (SLOT, hi, 0), (CONST, 0, 0)), (ADD, 1, (SLOT, hi, 0), (COLUMN, 2, 8)),
            (NEG, hi, (COLUMN, 3, 0), (SLOT, 0, 0)), (SUB, 0, (SLOT, 1, 0), (SLOT, hi, 0)), (ADD, 0, (SLOT, 0, 0), (CONST, 2, 0))], 0


@pytest.mark.parametrize("log_size", [0, 1, 6, 7, 8, 10])
@pytest.mark.parametrize("kernel", list(KERNELS))
def test_v1_sizes_below_and_above_one_block(gpu_ctx, kernel, log_size):
    """1, 2, 64 and 128 rows leave most of the one 256-thread block idle; every rotation wraps (at one row onto the row itself)"""
    ops, result = v1_program(kernel)
    for fid in V1_FIELDS:
        cols, consts = v1_data(fid, 1 << log_size, seed=3)
        v1_check(gpu_ctx, fid, ops, result, cols, consts, log_size, kernel, "2^%d rows" % log_size)


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("kernel", list(KERNELS))
def test_v1_batch_strides(gpu_ctx, kernel, device):
    """batch = blockIdx.y: three vectors; columns shared (stride 0), per vector back to back, per vector with a stride above the
    size; constants shared and per vector.  Device-resident columns and output are not repacked: the kernel sees those strides."""
    from helpers import field_edges as E, vm_cases as VC
    ops, result = v1_program(kernel)
    size, batch, big = 256, 3, 256 + 40
    for fid in V1_FIELDS:
        p = E.MODULI[fid]
        base = VC.operand_columns(p, 4, big * batch, seed=30 + fid)
        cols = [base[0][:size], base[1][:size * batch], base[2][:big * (batch - 1) + size], base[3][:size]]
        strides = [0, size, big, 0]
        consts = VC.operand_consts(p, 5 * (batch - 1) + 3, seed=40 + fid)
        per = v1_check(gpu_ctx, fid, ops, result, cols, consts, 8, kernel, "per-vector constants", batch, strides, 5, 3, True, device)
        shared = v1_check(gpu_ctx, fid, ops, result, cols, consts[:3], 8, kernel, "shared constants", batch, strides, 0, 3, True, device)
        assert per[:size] == shared[:size] and per[size:] != shared[size:]
        assert len({tuple(per[v * size:(v + 1) * size]) for v in range(batch)}) == batch


@pytest.mark.parametrize("kernel", list(KERNELS))
def test_v1_canonical_against_montgomery_form(gpu_ctx, kernel):
    """the same values handed over in canonical form and as x R mod p: the results are the same values in the two forms"""
    from helpers import field_edges as E
    ops, result = v1_program(kernel)
    for fid in V1_FIELDS:
        p = E.MODULI[fid]
        cols, consts = v1_data(fid, 256, seed=5)
        canon = v1_check(gpu_ctx, fid, ops, result, cols, consts, 8, kernel, "canonical", mont=False)
        mcols, mconsts = [[x * E.R % p for x in c] for c in cols], [x * E.R % p for x in consts]
        mont = v1_check(gpu_ctx, fid, ops, result, mcols, mconsts, 8, kernel, "Montgomery", mont=True)
        assert mont == [x * E.R % p for x in canon]
        assert mont == v1_check(gpu_ctx, fid, ops, result, mcols, mconsts, 8, kernel, "Montgomery, device-resident", mont=True, device=True)


def test_v1_slot_24_is_refused(gpu_ctx):
    import bzh2
    from helpers.expr import ADD, COLUMN, COPY, NEG, SLOT
    cols, consts = v1_data(0, 256)
    c0 = (COLUMN, 0, 0)
    for what, ops, result in (("dst", [(ADD, 24, c0, c0)], 0), ("operand a", [(COPY, 0, c0, c0), (NEG, 1, (SLOT, 24, 0), c0)], 0),
                              ("operand b", [(COPY, 0, c0, c0), (ADD, 1, (SLOT, 0, 0), (SLOT, 24, 0))], 1),
                              ("result slot", [(COPY, 0, c0, c0)], 24)):
        with pytest.raises(bzh2.BzhError) as e:
            v1_device(gpu_ctx, 0, ops, result, cols, consts, 8)
        assert e.value.status == bzh2.E_ARG, what
    v1_check(gpu_ctx, 0, [(COPY, 23, c0, c0), (NEG, 0, (SLOT, 23, 0), c0)], 0, cols, consts, 8, "generic-slot23", "slot 23 is the last")
