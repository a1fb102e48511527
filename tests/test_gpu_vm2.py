"""VM v2 (csrc/exprvm.hip: k_expr_vm2<P, 128> and k_expr_vm2<P, 64>, the quotient interpreter of bzh_prove_batch) instruction by
instruction through bzh_vm2_eval, bit for bit against the integer model of tests/helpers/vm_model.py.  Every comparison is
equality of all limbs.  The reference computes the same values in halo2_proofs 0.2.0 `poly::Evaluator` (UPSTREAM, un-vendored);
the instruction set itself is this project's (csrc/vm2_isa.hpp).

Operand columns come from tests/helpers/vm_cases.operand_columns: the adversarial values of tests/helpers/field_edges.py (0, 1,
p - 1, R, R^2, limb patterns), neighbouring columns summing to p or equal on half of the rows, and uniform values.  Most calls
use FORM_MONTGOMERY, so those bits reach the registers unchanged.  Size 256 unless a test says otherwise: two workgroups of the
128-row kernel, four of the 64-row kernel (programs of more than 16 slots)."""
import ctypes
import random

import numpy as np
import pytest

from helpers import field_edges as E
from helpers import vm_cases as VC
from helpers import vm_model as M
from helpers.vm_model import ADD, COLUMN, CONST, LDS, LL, LOAD, MUL, NO_LEAF, RSUB, SL, SS, STORE, SUB, UN, V2_NEG

pytestmark = pytest.mark.gpu

SIZE = 256
FIELDS = [0, 1]
_data = {}


def data(fid, ncols=8, n=SIZE):
    """(columns as int lists, constants as ints) of one field, built once"""
    key = (fid, ncols, n)
    if key not in _data:
        p = E.MODULI[fid]
        _data[key] = (VC.operand_columns(p, ncols, n, seed=fid), VC.operand_consts(p, 8, seed=fid))
    return _data[key]


def device_run(ctx, fid, ops, cols, consts, size=SIZE, batch=1, nlds=1, strides=None, const_stride=0, nconsts=None, mont=True):
    import bzh2
    arr = ops if isinstance(ops, np.ndarray) else M.encode_vm2(ops)
    out = ctx.vm2_eval(fid, arr, [E.ints_to_array(c) for c in cols], E.ints_to_array(consts), size, batch, nlds, strides, const_stride,
                       form=bzh2.FORM_MONTGOMERY if mont else bzh2.FORM_CANONICAL, nconsts=nconsts)
    return E.array_to_ints(out)


def model_run(fid, ops, cols, consts, size=SIZE, batch=1, nlds=1, strides=None, const_stride=0, nconsts=None, mont=True):
    assert M.unwritten_reads_vm2(ops) == [], "the kernel does not clear the slot file"
    return M.run_vm2(ops, cols, strides or [0] * len(cols), consts, const_stride, size, batch, nlds, E.MODULI[fid], montgomery=mont)


def check(ctx, fid, ops, cols, consts, what, **kw):
    got, want = device_run(ctx, fid, ops, cols, consts, **kw), model_run(fid, ops, cols, consts, **kw)
    assert len(got) == len(want)
    bad = [i for i in range(len(want)) if got[i] != want[i]]
    assert not bad, "%s, field %d: %d of %d rows differ; first at row %d: got=%#066x want=%#066x" % (
        what, fid, len(bad), len(want), bad[0], got[bad[0]], want[bad[0]])
    return want


def load(pos, leaf):
    return (UN, LOAD, pos, leaf, NO_LEAF)


def store(pos, slot):
    return (UN, STORE, pos, (LDS, slot, 0), NO_LEAF)


@pytest.mark.parametrize("fid", FIELDS)
@pytest.mark.parametrize("word", M.VM2_WORDS, ids=[M.word_name(*w) for w in M.VM2_WORDS])
def test_every_instruction_word(gpu_ctx, word, fid):
    """r0..r3 preloaded from four distinct columns, the one instruction (leaf a = column 4, leaf b = column 5, a STORE's target =
    slot 5), then each register read back in a run of its own (STORE to a slot, LOAD into r0): a wrong destination, a wrong source
    register, swapped operands of SUB / RSUB and a clobbered bystander all change one of the four results."""
    form, op, pos = word
    cols, consts = data(fid)
    a, b = ((LDS, 5, 0) if (form, op) == (UN, STORE) else (COLUMN, 4, 0)), (COLUMN, 5, 0)
    body = [load(k, (COLUMN, k, 0)) for k in range(4)] + [(form, op, pos, a, b)]
    for k in range(4):
        want = check(gpu_ctx, fid, body + [store(k, k), load(0, (LDS, k, 0))], cols, consts, "%s, register r%d" % (M.word_name(*word), k),
                     nlds=6)
        if k != pos or (form, op) == (UN, STORE):
            assert want == cols[k]                 # the model: a bystander (and a STORE's source) keeps its value
        else:
            assert want != cols[k]
    if (form, op) == (UN, STORE):
        assert check(gpu_ctx, fid, body + [load(0, (LDS, 5, 0))], cols, consts, "%s, the slot" % M.word_name(*word), nlds=6) == cols[pos]


def leaf_cases():
    out = [("column-rot%+d" % rot, (COLUMN, 4, rot), 4) for rot in (0, 8, -8, -300, 32767)]
    out.append(("constant", (CONST, 3, 0), 4))
    for nlds in (16, 32):                          # the last count of the 128-row kernel, the last of the 64-row kernel
        out += [("slot0-of-%d" % nlds, (LDS, 0, 0), nlds), ("slot%d-of-%d" % (nlds - 1, nlds), (LDS, nlds - 1, 0), nlds)]
    return out


@pytest.mark.parametrize("fid", FIELDS)
@pytest.mark.parametrize("name,leaf,nlds", leaf_cases(), ids=[c[0] for c in leaf_cases()])
def test_every_leaf_kind_in_both_positions(gpu_ctx, name, leaf, nlds, fid):
    """the leaf as operand a and as operand b of LL (SUB: the positions are not interchangeable), as operand b of SL, and as a
    LOAD's operand; the slots hold columns 5 and 6, stored first"""
    cols, consts = data(fid)
    pre = [load(1, (COLUMN, 5, 0)), store(1, 0), load(1, (COLUMN, 6, 0)), store(1, nlds - 1), load(0, (COLUMN, 0, 0))]
    other = (COLUMN, 1, 0)
    for what, ins in (("LL a", (LL, SUB, 0, leaf, other)), ("LL b", (LL, SUB, 0, other, leaf)), ("LL both", (LL, MUL, 0, leaf, leaf)),
                      ("SL b", (SL, SUB, 0, other, leaf)), ("SL RSUB b", (SL, RSUB, 0, other, leaf)), ("LOAD a", load(0, leaf))):
        want = check(gpu_ctx, fid, pre + [ins], cols, consts, "%s as %s" % (name, what), nlds=nlds)
        if what == "LOAD a" and leaf[0] == COLUMN:  # the model: rotation is (row + rot) mod size, past either end of the vector
            assert want == [cols[4][(r + leaf[2]) % SIZE] for r in range(SIZE)]
        if what == "LOAD a" and leaf[0] == LDS:
            assert want == cols[5 if leaf[1] == 0 else 6]


def fill_all_slots(nlds, ncols, nconsts):
    """a distinct value into every slot, then all of them folded into r0"""
    ops = []
    for s in range(nlds):
        ops += [(LL, ADD, 1, (COLUMN, s % ncols, s), (CONST, s % nconsts, 0)), store(1, s)]
    ops.append(load(0, (LDS, 0, 0)))
    for s in range(1, nlds):
        ops.append((SL, (ADD, RSUB, MUL, SUB)[s % 4], 0, NO_LEAF, (LDS, s, 0)))
    return ops


@pytest.mark.parametrize("fid", FIELDS)
def test_slot_file_sizes(gpu_ctx, fid):
    """nlds 1 and 16 run in the 128-row kernel, 17 and 32 in the 64-row kernel: one program, equal results; then every slot of
    each file written and read; 33 slots do not fit 64 KB of LDS"""
    import bzh2
    cols, consts = data(fid)
    prog = [load(0, (COLUMN, 0, 0)), (SL, MUL, 0, NO_LEAF, (COLUMN, 1, -8)), store(0, 0), load(0, (COLUMN, 2, 8)),
            (SL, RSUB, 0, NO_LEAF, (LDS, 0, 0)), store(0, 0), (LL, MUL, 0, (LDS, 0, 0), (LDS, 0, 0))]
    results = [check(gpu_ctx, fid, prog, cols, consts, "one slot of %d" % nlds, nlds=nlds) for nlds in (1, 16, 17, 32)]
    assert results[0] == results[1] == results[2] == results[3] and len(set(results[0])) > SIZE // 2
    for nlds in (1, 16, 17, 32):
        check(gpu_ctx, fid, fill_all_slots(nlds, len(cols), len(consts)), cols, consts, "all %d slots" % nlds, nlds=nlds)
    with pytest.raises(bzh2.BzhError) as e:
        device_run(gpu_ctx, fid, prog, cols, consts, nlds=33)
    assert e.value.status == bzh2.E_RANGE


def geometry_case(fid, size, batch=3):
    """one column shared by the vectors, one per vector back to back, one per vector with a stride above the size; constants for
    `batch` vectors, const_stride apart"""
    p = E.MODULI[fid]
    big = size + 40
    base = VC.operand_columns(p, 3, big * batch, seed=10 + fid)
    cols = [base[0][:size], base[1][:size * batch], base[2][:big * (batch - 1) + size]]
    strides = [0, size, big]
    nconsts, const_stride = 4, 5
    consts = VC.operand_consts(p, const_stride * (batch - 1) + nconsts, seed=20 + fid)
    prog = [(LL, MUL, 0, (COLUMN, 0, 8), (COLUMN, 1, -8)), (LL, SUB, 1, (COLUMN, 2, size - 1), (CONST, 3, 0)), (SS, ADD, 0, NO_LEAF, NO_LEAF),
            (SL, MUL, 0, NO_LEAF, (CONST, 0, 0)), store(0, 1), load(2, (COLUMN, 2, 0)), (SL, RSUB, 2, NO_LEAF, (COLUMN, 1, 0)), store(2, 0),
            (LL, ADD, 0, (LDS, 0, 0), (LDS, 1, 0)), (SL, ADD, 0, NO_LEAF, (CONST, 1, 0))]
    return cols, strides, consts, nconsts, const_stride, prog


@pytest.mark.parametrize("size", [128, 256, 1024])
@pytest.mark.parametrize("fid", FIELDS)
def test_batch_strides_and_sizes(gpu_ctx, fid, size):
    """batch = blockIdx.y: per-vector column strides (0, size, above size), shared and per-vector constants, in both forms"""
    cols, strides, consts, nconsts, const_stride, prog = geometry_case(fid, size)
    for mont in (True, False):
        per = check(gpu_ctx, fid, prog, cols, consts, "per-vector constants", size=size, batch=3, nlds=2, strides=strides,
                    const_stride=const_stride, nconsts=nconsts, mont=mont)
        shared = check(gpu_ctx, fid, prog, cols, consts[:nconsts], "shared constants", size=size, batch=3, nlds=2, strides=strides, mont=mont)
        assert per[:size] == shared[:size] and per[size:] != shared[size:]         # the model: only vector 0 has the same constants
        assert len({tuple(per[v * size:(v + 1) * size]) for v in range(3)}) == 3
    check(gpu_ctx, fid, prog, cols, consts, "batch 1", size=size, batch=1, nlds=17, strides=strides)
    check(gpu_ctx, fid, prog, cols, consts, "64-row kernel", size=size, batch=3, nlds=17, strides=strides, const_stride=const_stride, nconsts=nconsts)


@pytest.mark.parametrize("fid", FIELDS)
def test_device_resident_columns_keep_their_strides(gpu_ctx, fid):
    """BZH_MEM_DEVICE: nothing is repacked, so the kernel itself sees the stride above the size and the stride 0"""
    import bzh2
    import torch
    size, batch = 256, 3
    cols, strides, consts, nconsts, const_stride, prog = geometry_case(fid, size)
    dev = [torch.from_numpy(E.ints_to_array(c).view(np.int64)).cuda() for c in cols]
    for nlds in (2, 17):
        out = torch.zeros((batch * size, 4), dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        gpu_ctx.vm2_eval(fid, M.encode_vm2(prog), [t.data_ptr() for t in dev], E.ints_to_array(consts), size, batch, nlds, strides, const_stride,
                         form=bzh2.FORM_MONTGOMERY, mem=bzh2.MEM_DEVICE, out=out.data_ptr(), nconsts=nconsts)
        gpu_ctx.sync()
        got = E.array_to_ints(out.cpu().numpy().view(np.uint64))
        assert got == model_run(fid, prog, cols, consts, size=size, batch=batch, nlds=nlds, strides=strides, const_stride=const_stride)
    with pytest.raises(bzh2.BzhError) as e:        # device operands are Montgomery form only, as for bzh_expr_eval_batch
        gpu_ctx.vm2_eval(fid, M.encode_vm2(prog), [t.data_ptr() for t in dev], E.ints_to_array(consts), size, batch, 2, strides, const_stride,
                         form=bzh2.FORM_CANONICAL, mem=bzh2.MEM_DEVICE, out=out.data_ptr(), nconsts=nconsts)
    assert e.value.status == bzh2.E_ARG


@pytest.mark.parametrize("fid", FIELDS)
def test_single_instruction_programs(gpu_ctx, fid):
    """nops = 1: the interpreter fetches prog[i + 1] while instruction i executes"""
    cols, consts = data(fid)
    for nlds in (1, 17):
        check(gpu_ctx, fid, [(LL, SUB, 0, (COLUMN, 0, 0), (COLUMN, 1, 0))], cols, consts, "one LL", nlds=nlds)
        check(gpu_ctx, fid, [load(0, (COLUMN, 3, -1))], cols, consts, "one LOAD", nlds=nlds)
        assert check(gpu_ctx, fid, [(UN, V2_NEG, 0, NO_LEAF, NO_LEAF)], cols, consts, "one NEG of the zero register", nlds=nlds) == [0] * SIZE
        assert check(gpu_ctx, fid, [load(1, (COLUMN, 3, 0))], cols, consts, "r0 never written", nlds=nlds) == [0] * SIZE


@pytest.mark.parametrize("seed", range(16))
def test_random_programs(gpu_ctx, seed):
    """about 300 valid instructions over all 52 words and every leaf kind (tests/helpers/vm_cases.random_vm2_program), two
    vectors; the slot counts put half of the seeds in each kernel"""
    fid, nlds, mont = seed % 2, [3, 17, 16, 32][(seed // 2) % 4], seed % 8 < 6
    p = E.MODULI[fid]
    rng = random.Random(1000 + seed)
    ncols, nconsts, batch = 7, 6, 2
    ops = VC.random_vm2_program(rng, 300, ncols, nconsts, nlds)
    cols = VC.operand_columns(p, ncols, SIZE * batch, seed=seed)
    strides = [0 if c % 3 == 0 else SIZE for c in range(ncols)]
    cols = [c[:SIZE] if s == 0 else c for c, s in zip(cols, strides)]
    consts = VC.operand_consts(p, nconsts * batch, seed=seed)
    want = check(gpu_ctx, fid, ops, cols, consts, "seed %d" % seed, batch=batch, nlds=nlds, strides=strides, const_stride=nconsts,
                 nconsts=nconsts, mont=mont)
    assert len(set(want)) > SIZE                  # the model: the result is not degenerate


@pytest.mark.parametrize("name", ["ShotCircuit", "BoardCircuit"])
def test_real_quotient_programs_on_adversarial_columns(gpu_ctx, name):
    """the programs bzh_prove_batch runs for the reference's circuits (k = 11 / 12; 950 / 1 340 instructions, 19 slots: the 64-row
    kernel with leaf slots) over edge-value columns, two vectors, each with its own values for the challenge constants"""
    import bzh2
    pg = VC.quotient_program(bzh2, name)
    assert pg.nlds > 16 and len(pg.ops) > 900
    fid, batch = 0, 2
    p = E.MODULI[fid]
    cols = VC.operand_columns(p, pg.ncols, SIZE * batch, seed=5)
    strides = [0 if c % 4 == 0 else SIZE for c in range(pg.ncols)]
    cols = [c[:SIZE] if s == 0 else c for c, s in zip(cols, strides)]
    rng = random.Random(77)
    consts = pg.bind(p, rng) + pg.bind(p, rng)
    want = check(gpu_ctx, fid, pg.ops, cols, consts, name, batch=batch, nlds=pg.nlds, strides=strides, const_stride=len(pg.consts),
                 nconsts=len(pg.consts))
    assert len(set(want)) > SIZE


def test_refusals_leave_the_output_alone(gpu_ctx):
    """everything bzh_vm2_eval checks before it launches: BZH_E_ARG, or BZH_E_RANGE for the slot count, and `out` as it was"""
    import bzh2
    fid = 0
    cols, consts = data(fid, ncols=2)
    consts = consts[:2]
    c0, c1, k0 = (COLUMN, 0, 0), (COLUMN, 1, 0), (CONST, 0, 0)
    good = [load(0, c0), (SL, ADD, 0, NO_LEAF, k0), store(0, 1), (LL, MUL, 0, (LDS, 1, 0), c1)]
    ok = dict(fid=fid, ops=good, size=SIZE, batch=1, nlds=2)
    bad_ops = {
        "SS at register 3": (SS, ADD, 3, NO_LEAF, NO_LEAF),
        "SS RSUB at register 3": (SS, RSUB, 3, NO_LEAF, NO_LEAF),
        "LL with RSUB": (LL, RSUB, 0, c0, c1),
        "LL with RSUB at register 3": (LL, RSUB, 3, c0, c1),
        "UN with operation 3": (UN, 3, 0, c0, NO_LEAF),
        "UN with operation 3 at register 2": (UN, 3, 2, c0, NO_LEAF),
        "a code above 63": (4, 0, 0, c0, c1),
        "the code 255": (15, 3, 3, c0, c1),
        "LL operand a of kind 0": (LL, ADD, 0, (0, 0, 0), c1),
        "LL operand a of kind 4": (LL, ADD, 0, (4, 0, 0), c1),
        "LL operand b of kind 0": (LL, ADD, 0, c0, (0, 0, 0)),
        "SL operand b of kind 4": (SL, ADD, 0, NO_LEAF, (4, 0, 0)),
        "SL operand b of kind 255": (SL, ADD, 0, NO_LEAF, (255, 0, 0)),
        "LOAD operand of kind 0": load(0, (0, 0, 0)),
        "column index = ncols": load(0, (COLUMN, 2, 0)),
        "column index -1": (LL, ADD, 0, c0, (COLUMN, -1, 0)),
        "constant index = nconsts": (SL, MUL, 0, NO_LEAF, (CONST, 2, 0)),
        "constant index -1": load(0, (CONST, -1, 0)),
        "slot index = nlds": (SL, ADD, 0, NO_LEAF, (LDS, 2, 0)),
        "slot index -1": load(0, (LDS, -1, 0)),
        "STORE target = nlds": store(0, 2),
        "STORE target -1": store(0, -1),
        "STORE target far away": store(3, 1 << 30),
    }
    cases = [(what, dict(ok, ops=good[:3] + [ins] + good[3:]), bzh2.E_ARG) for what, ins in bad_ops.items()]
    cases += [("a bad word as the only instruction", dict(ok, ops=[(SS, MUL, 3, NO_LEAF, NO_LEAF)]), bzh2.E_ARG),
              ("a bad word last", dict(ok, ops=good + [(LL, RSUB, 1, c0, c1)]), bzh2.E_ARG),
              ("size 64", dict(ok, size=64), bzh2.E_ARG), ("size 1", dict(ok, size=1), bzh2.E_ARG),
              ("batch 0", dict(ok, batch=0), bzh2.E_ARG), ("batch 65536", dict(ok, batch=65536), bzh2.E_ARG),
              ("field 2 (BN254 Fr)", dict(ok, fid=2), bzh2.E_ARG), ("field 3 (BN254 Fq)", dict(ok, fid=3), bzh2.E_ARG),
              ("field -1", dict(ok, fid=-1), bzh2.E_ARG), ("a negative slot count", dict(ok, nlds=-1), bzh2.E_ARG),
              ("no slots for a program with a STORE", dict(ok, nlds=0), bzh2.E_ARG),
              ("33 slots", dict(ok, nlds=33), bzh2.E_RANGE), ("1000 slots", dict(ok, nlds=1000), bzh2.E_RANGE)]
    col_arrays, const_array = [E.ints_to_array(c) for c in cols], E.ints_to_array(consts)
    for what, kw, status in cases:
        out = np.full((SIZE, 4), 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
        with pytest.raises(bzh2.BzhError) as e:
            gpu_ctx.vm2_eval(kw["fid"], M.encode_vm2(kw["ops"]), col_arrays, const_array, kw["size"], kw["batch"], kw["nlds"],
                             form=bzh2.FORM_MONTGOMERY, out=out)
        assert e.value.status == status, what
        assert (out == np.uint64(0xA5A5A5A5A5A5A5A5)).all(), what
    L = bzh2.load()                                # an empty program, and no program at all
    ptrs = (ctypes.c_void_p * 2)(*[c.ctypes.data for c in col_arrays])
    out = np.zeros((SIZE, 4), dtype=np.uint64)
    arr = M.encode_vm2(good)
    for ops_ptr, nops in ((arr.ctypes.data, 0), (None, len(arr))):
        assert L.bzh_vm2_eval(gpu_ctx.handle, fid, ops_ptr, nops, ptrs, None, 2, const_array.ctypes.data, 2, 0, 8, 1, 2, bzh2.FORM_MONTGOMERY,
                              bzh2.MEM_HOST, out.ctypes.data) == bzh2.E_ARG
    assert not out.any()
    # operands an instruction does not read may hold anything, and the same context still runs a good program afterwards
    junk = (9, -5, 0)
    check(gpu_ctx, fid, good + [(SS, ADD, 0, junk, junk), (UN, V2_NEG, 1, junk, junk), (SL, SUB, 0, junk, c0), (UN, LOAD, 2, c1, junk),
                                (UN, STORE, 2, (7, 0, 0), junk)], cols, consts, "junk in unread operands", nlds=2)
