"""bzh_vm2_eval_cosets (k_expr_vm2_cosets: the VM v2 interpreter run coset by coset, csrc/exprvm.hip) against bzh_vm2_eval over
the whole 8 n domain on the same data.  Every comparison is equality of all limbs.

n = 2^log_n rows per coset, log_n = 3, 5, 11: at 3 and 5 a workgroup is partial (8 and 32 lanes of 128) and every rotation
wraps; 11 is the Shot circuit's own size, 16 workgroups per coset.  The n-sized columns are the 8 n columns sliced [j::8] on the
host.  bzh_vm2_eval takes whole 128-row workgroups only, so the 64-row reference of log_n = 3 is computed on the data laid out
twice (128 rows): a rotation modulo 128 over data of period 64 reads what the rotation modulo 64 reads, and its first 64 rows
are the 64-row evaluation."""
import numpy as np
import pytest

from helpers import field_edges as E
from helpers import vm_cases as VC
from helpers import vm_model as M
from helpers.vm_model import ADD, COLUMN, CONST, LDS, LL, LOAD, MUL, NO_LEAF, RSUB, SL, SS, STORE, SUB, UN

pytestmark = pytest.mark.gpu

FIELDS = [0, 1]
LOG_NS = [3, 5, 11]
BATCH = 3
# columns 0, 1: the key's (8 n, shared) | 2: n-sized, shared | 3, 4: n-sized, per vector | 5: 8 n, per vector
EXTENDED = [True, True, False, False, False, True]
PER_VECTOR = [False, False, False, True, True, True]


def load(pos, leaf):
    return (UN, LOAD, pos, leaf, NO_LEAF)


def store(pos, slot):
    return (UN, STORE, pos, (LDS, slot, 0), NO_LEAF)


def program(n):
    """rotations 0, +-8, +-8 (n - 1) and -8 n + 8 on both kinds of column; an 8 n column and an n-sized one in one instruction; a
    shared column beside per-vector ones; constants and slots"""
    far = 8 * (n - 1)
    return [
        (LL, MUL, 0, (COLUMN, 0, 0), (COLUMN, 3, 8)),          # key-style 8 n column x n-sized per-vector column
        (SL, ADD, 0, NO_LEAF, (COLUMN, 2, -8)),                # n-sized shared column, one step back over the wrap at row 0
        store(0, 0),
        (LL, SUB, 1, (COLUMN, 4, far), (COLUMN, 1, -far)),     # the wrap crossed forwards and backwards
        (SL, MUL, 1, NO_LEAF, (CONST, 1, 0)),
        store(1, 1),
        (LL, ADD, 2, (COLUMN, 3, -8 * n + 8), (COLUMN, 5, -8 * n + 8)),
        (SL, RSUB, 2, NO_LEAF, (COLUMN, 5, far)),
        (LL, MUL, 3, (COLUMN, 4, -far), (COLUMN, 0, 8)),
        (SS, ADD, 2, NO_LEAF, NO_LEAF),                        # r2 += r3
        (SL, MUL, 2, NO_LEAF, (LDS, 0, 0)),
        (SL, SUB, 2, NO_LEAF, (LDS, 1, 0)),
        (SL, ADD, 2, NO_LEAF, (CONST, 0, 0)),
        store(2, 0),
        load(0, (LDS, 0, 0)),
        (SL, ADD, 0, NO_LEAF, (COLUMN, 1, -8)),
    ]


_data = {}


def data(fid, log_n):
    """per column BATCH (or 1) vectors of 8 n ints, and the constants: built once per (field, size)"""
    key = (fid, log_n)
    if key not in _data:
        p, en = E.MODULI[fid], 8 << log_n
        flat = VC.operand_columns(p, sum(BATCH if pv else 1 for pv in PER_VECTOR), en, seed=fid + 2 * log_n)
        cols, at = [], 0
        for pv in PER_VECTOR:
            cols.append(flat[at:at + (BATCH if pv else 1)])
            at += BATCH if pv else 1
        _data[key] = (cols, VC.operand_consts(p, 4, seed=fid))
    return _data[key]


def full_domain(ctx, fid, ops, cols, consts, en):
    """the reference: bzh_vm2_eval over batch vectors of en rows (en = 64: see the module's head)"""
    import bzh2
    rep = 2 if en < 128 else 1
    arrs = [E.ints_to_array([x for vec in c for x in vec * rep]) for c in cols]
    strides = [en * rep if len(c) > 1 else 0 for c in cols]
    out = ctx.vm2_eval(fid, M.encode_vm2(ops), arrs, E.ints_to_array(consts), en * rep, BATCH, 2, strides, form=bzh2.FORM_MONTGOMERY)
    return np.ascontiguousarray(out.reshape(BATCH, en * rep, 4)[:, :en]).reshape(BATCH * en, 4)


def coset_arrays(cols, extended, n):
    """extended columns as they are; n-sized ones as (8, vectors, n): block j = rows j, j + 8, ..."""
    arrs, strides = [], []
    for c, ext in zip(cols, extended):
        if ext:
            arrs.append(E.ints_to_array([x for vec in c for x in vec]))
            strides.append(8 * n if len(c) > 1 else 0)
        else:
            arrs.append(E.ints_to_array([x for j in range(8) for vec in c for x in vec[j::8]]))
            strides.append(n if len(c) > 1 else 0)
    return arrs, strides


def cosets(ctx, fid, ops, cols, consts, log_n, extended=EXTENDED, **kw):
    import bzh2
    arrs, strides = coset_arrays(cols, extended, 1 << log_n)
    return ctx.vm2_eval_cosets(fid, M.encode_vm2(ops), arrs, extended, E.ints_to_array(consts), log_n, BATCH, 2, strides,
                               form=bzh2.FORM_MONTGOMERY, **kw)


@pytest.mark.parametrize("fid", FIELDS)
@pytest.mark.parametrize("log_n", LOG_NS)
def test_coset_by_coset_equals_the_full_domain(gpu_ctx, log_n, fid):
    n = 1 << log_n
    cols, consts = data(fid, log_n)
    ops = program(n)
    want = full_domain(gpu_ctx, fid, ops, cols, consts, 8 * n)
    got = cosets(gpu_ctx, fid, ops, cols, consts, log_n)
    assert got.shape == want.shape
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, "log_n %d, field %d: %d of %d rows differ; first at vector %d, row %d (coset %d)" % (
        log_n, fid, bad.size, len(want), bad[0] // (8 * n), bad[0] % (8 * n), bad[0] % 8)
    # the program does not collapse: a quarter of every column's rows are uniform values (vm_cases.operand_columns), the rest
    # repeat edge values, so the results take well over 8 n / 8 distinct values unless they degenerate
    assert len({tuple(r) for r in want[:8 * n].tolist()}) > n
    assert (want[:8 * n] != want[8 * n:16 * n]).any()                      # ... and the vectors differ


@pytest.mark.parametrize("fid", FIELDS)
def test_every_column_kind_alone_at_every_rotation(gpu_ctx, fid):
    """LOAD of one column at one rotation, for both kinds of column, shared and per vector: the result IS the rotated column"""
    log_n = 3
    n, en = 8, 64
    cols, consts = data(fid, log_n)
    for c in (0, 2, 3, 5):
        for rot in (0, 8, -8, 8 * (n - 1), -8 * (n - 1), -8 * n + 8):
            got = E.array_to_ints(cosets(gpu_ctx, fid, [load(0, (COLUMN, c, rot))], cols, consts, log_n))
            want = [cols[c][v if len(cols[c]) > 1 else 0][(r + rot) % en] for v in range(BATCH) for r in range(en)]
            assert got == want, "column %d at rotation %d" % (c, rot)


@pytest.mark.parametrize("fid", FIELDS)
def test_operands_at_the_fields_edges(gpu_ctx, fid):
    """0, 1 and p - 1 (and their Montgomery forms' neighbours, tests/helpers/field_edges.py) in every column, multiplied, added
    and subtracted across the two kinds of column, against the full domain"""
    log_n = 5
    n, en, p = 32, 256, E.MODULI[fid]
    edge = [0, 1, p - 1] + list(E.edge_values(p))[:13]
    cols = [[[edge[(3 * c + 5 * v + r + (r >> 3)) % len(edge)] for r in range(en)] for v in range(BATCH if pv else 1)]
            for c, pv in enumerate(PER_VECTOR)]
    consts = [0, 1, p - 1, 2]
    ops = [(LL, MUL, 0, (COLUMN, 0, 0), (COLUMN, 3, 8)), (SL, ADD, 0, NO_LEAF, (COLUMN, 2, -8)), (SL, SUB, 0, NO_LEAF, (COLUMN, 5, 8 * (n - 1))),
           (SL, MUL, 0, NO_LEAF, (CONST, 2, 0)), (SL, RSUB, 0, NO_LEAF, (COLUMN, 4, 0)), (SL, ADD, 0, NO_LEAF, (CONST, 1, 0))]
    want = full_domain(gpu_ctx, fid, ops, cols, consts, en)
    assert (cosets(gpu_ctx, fid, ops, cols, consts, log_n) == want).all()


def test_refusals(gpu_ctx):
    """a rotation that is not a multiple of 8, an output size that is not 8 * 2^log_n, a misaligned pointer: BZH_E_ARG, `out`
    untouched; the same call without the fault runs"""
    import bzh2
    log_n, fid = 3, 0
    cols, consts = data(fid, log_n)
    good = [load(0, (COLUMN, 3, 8)), (SL, ADD, 0, NO_LEAF, (COLUMN, 0, -8))]
    out = np.full((BATCH * 64, 4), 0x5a5a5a5a5a5a5a5a, dtype=np.uint64)
    for rot in (1, 4, -7, 12):
        for ops in ([load(0, (COLUMN, 3, rot))], [load(0, (COLUMN, 0, 0)), (SL, MUL, 0, NO_LEAF, (COLUMN, 0, rot))]):
            with pytest.raises(bzh2.BzhError) as e:
                cosets(gpu_ctx, fid, ops, cols, consts, log_n, out=out)
            assert e.value.status == bzh2.E_ARG
    for size in (63, 8, 128, 0):
        with pytest.raises(bzh2.BzhError) as e:
            cosets(gpu_ctx, fid, good, cols, consts, log_n, out=out, out_size=size)
        assert e.value.status == bzh2.E_ARG
    raw = np.zeros(BATCH * 64 * 4 + 1, dtype=np.uint64)
    crooked = raw.view(np.uint8)[4:4 + BATCH * 64 * 32].view(np.uint64).reshape(BATCH * 64, 4)      # 4 bytes off an 8-byte boundary
    assert crooked.ctypes.data % 8 == 4
    with pytest.raises(bzh2.BzhError) as e:
        cosets(gpu_ctx, fid, good, cols, consts, log_n, out=crooked)
    assert e.value.status == bzh2.E_ARG and not raw.any()
    assert (out == 0x5a5a5a5a5a5a5a5a).all()
    got = cosets(gpu_ctx, fid, good, cols, consts, log_n, out=out)
    assert got is out and (out == full_domain(gpu_ctx, fid, good, cols, consts, 64)).all()


def test_misaligned_column_and_device_pointers(gpu_ctx):
    """host memory wants 8-byte limbs, device memory whole 32-byte elements: a host column 4 bytes off, and a device column and a
    device `out` 16 bytes off, are BZH_E_ARG with the output untouched; the device call with aligned pointers equals the full domain"""
    import bzh2
    import torch
    log_n, fid, en = 3, 0, 64
    cols, consts = data(fid, log_n)
    good = [load(0, (COLUMN, 3, 8)), (SL, ADD, 0, NO_LEAF, (COLUMN, 0, -8))]
    want = full_domain(gpu_ctx, fid, good, cols, consts, en)
    arrs, strides = coset_arrays(cols, EXTENDED, 8)
    ops, cv = M.encode_vm2(good), E.ints_to_array(consts)
    # host: column 3 moved 4 bytes off an 8-byte boundary
    raw = np.zeros(arrs[3].size + 1, dtype=np.uint64)
    crooked = raw.view(np.uint8)[4:4 + arrs[3].nbytes].view(np.uint64).reshape(arrs[3].shape)
    crooked[...] = arrs[3]
    assert crooked.ctypes.data % 8 == 4 and crooked.flags["C_CONTIGUOUS"]
    out = np.full((BATCH * en, 4), 0x5a5a5a5a5a5a5a5a, dtype=np.uint64)
    with pytest.raises(bzh2.BzhError) as e:
        gpu_ctx.vm2_eval_cosets(fid, ops, arrs[:3] + [crooked] + arrs[4:], EXTENDED, cv, log_n, BATCH, 2, strides, form=bzh2.FORM_MONTGOMERY,
                                out=out)
    assert e.value.status == bzh2.E_ARG and (out == 0x5a5a5a5a5a5a5a5a).all()
    # device: every column with 32 spare bytes in front, so that a pointer 16 bytes on still has its whole column behind it
    dev = [torch.from_numpy(np.concatenate([np.zeros((1, 4), dtype=np.uint64), a.reshape(-1, 4), np.zeros((1, 4), dtype=np.uint64)])
                            .view(np.int64)).to("cuda") for a in arrs]
    ptrs = [d.data_ptr() + 32 for d in dev]
    d_out = torch.full((BATCH * en + 1, 4), 0x5a5a5a5a5a5a5a5a, dtype=torch.int64, device="cuda")
    assert all(p % 32 == 0 for p in ptrs) and d_out.data_ptr() % 32 == 0
    run = lambda pp, o: gpu_ctx.vm2_eval_cosets(fid, ops, pp, EXTENDED, cv, log_n, BATCH, 2, strides, form=bzh2.FORM_MONTGOMERY,   # noqa: E731
                                                mem=bzh2.MEM_DEVICE, out=o)
    for pp, o in ((ptrs[:3] + [ptrs[3] + 16] + ptrs[4:], d_out.data_ptr()), ([ptrs[0] + 16] + ptrs[1:], d_out.data_ptr()),
                  (ptrs, d_out.data_ptr() + 16)):
        with pytest.raises(bzh2.BzhError) as e:
            run(pp, o)
        assert e.value.status == bzh2.E_ARG
    gpu_ctx.sync()
    assert (d_out.cpu().numpy().view(np.uint64) == 0x5a5a5a5a5a5a5a5a).all()
    run(ptrs, d_out.data_ptr())
    gpu_ctx.sync()
    assert (d_out.cpu().numpy().view(np.uint64)[:BATCH * en] == want).all()
