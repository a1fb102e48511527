"""The vector primitives of csrc/polyops.hip at batch-scale launch geometry, bit for bit against the big-int definitions of
oracle/pasta.py (cases and expectations: tests/helpers/polyops_cases.py).

tests/test_gpu_polyops.py checks the shapes of one small proof and tests/test_gpu_field_edges.py the arithmetic operands; this
file walks the launch shapes: the batch-inversion launch at and past its 65 536-thread cap and at its thread-count steps, the
grand-product scan over more vectors than one block of its totals kernel and than one chunk of its driver loop, every
(threads, L, S) regime of kate_division (bzh_kate_division_plan; tests/test_polyops_cases_cpu.py asserts that KATE_CASES
reaches each of them), and inner product, fold and evaluation with many vectors per launch."""
import numpy as np
import pytest

import pasta as O
from helpers import polyops_cases as K

pytestmark = pytest.mark.gpu

# batch inversion: past the thread cap, chains of 19 and 20 elements
CAPPED_COUNT = (1 << 20) + 3 * 65536 + 17
# ... and the counts on either side of a step of the thread count: 64 -> 65 threads, below the cap -> capped
STEP_COUNTS = [1024, 1025, 1040, 1 << 20, (1 << 20) + 1]
ALL_ZERO_COUNTS = [1040, 70000]
SCAN_CASES = [(2049, 65), (2049, 130), (4096, 65)]
SCAN_SECOND_CHUNK = (3, 70000)
# (n, batch) of kate_division on field 0, and the subset run on fields 1 and 2
KATE_CASES = [(2, 1), (3, 300), (258, 3), (513, 3), (514, 3), (1025, 1), (1026, 1), (2050, 256), (4097, 64), (4098, 64), (8193, 40),
              (32769, 2), (32770, 2)]
KATE_CASES_OTHER_FIELDS = [(1026, 1), (2050, 256), (8193, 40)]


def prime(fid):
    return O.FIELD_BY_ID[fid].p


def assert_same(got, want, what, nthreads=None, per_vector=None):
    d = K.first_difference(got, want)
    if d is None:
        return
    i, bad = d
    where = "element %d" % i
    if nthreads:
        where += " (chain %d of %d, place %d in it)" % (i % nthreads, nthreads, i // nthreads)
    if per_vector:
        where += " (vector %d, index %d)" % (i // per_vector, i % per_vector)
    pytest.fail("%s: %d of %d elements differ; first at %s: got=%s want=%s"
                % (what, bad, want.size // 4, where, K.hex_of(got, i), K.hex_of(want, i)))


def check_batch_invert(ctx, fid, count, montgomery=False):
    import bzh2
    nthreads = bzh2.batch_invert_plan(count)
    v, want, info = K.tiled_inverse_case(prime(fid), count, nthreads, montgomery)
    assert not v[info["zero_chain"]::nthreads].any() and v.any()
    got = ctx.batch_invert(fid, v, form=bzh2.FORM_MONTGOMERY if montgomery else bzh2.FORM_CANONICAL)
    assert_same(got, want, "batch_invert field %d count %d%s" % (fid, count, " (Montgomery form)" if montgomery else ""), nthreads=nthreads)


@pytest.mark.parametrize("fid", [0, 1, 2])
def test_batch_invert_capped_launch(gpu_ctx, fid):
    """count > 2^20: the driver's `nthreads > 65536` cap, so chains grow past 16 elements (19 and 20 here), with three zeros
    in a row inside a chain and one chain that is all zeros"""
    check_batch_invert(gpu_ctx, fid, CAPPED_COUNT)
    if fid == 0:
        check_batch_invert(gpu_ctx, fid, CAPPED_COUNT, montgomery=True)


def test_batch_invert_thread_count_steps(gpu_ctx):
    """either side of 64 -> 65 threads and of the cap; an input of zeros alone comes back as zeros"""
    import bzh2
    for count in STEP_COUNTS:
        check_batch_invert(gpu_ctx, 0, count)
    for count in ALL_ZERO_COUNTS:
        got = gpu_ctx.batch_invert(0, np.zeros((count, 4), dtype=np.uint64))
        assert_same(got, np.zeros((count, 4), dtype=np.uint64), "batch_invert of %d zeros" % count, nthreads=bzh2.batch_invert_plan(count))


@pytest.mark.parametrize("fid,n,batch", [(f, n, b) for f in (0, 1, 2) for n, b in SCAN_CASES] + [(0,) + SCAN_SECOND_CHUNK])
def test_prefix_product_many_vectors(gpu_ctx, fid, n, batch):
    """more than 64 vectors of more than one tile: k_scan_totals runs a second (and third) block, and the vectors on either
    side of the block boundary lose everything behind a zero in the last element of tile 0 / the first of tile 1.  More than
    65 535 vectors: the second pass of prefix_scan_t's chunk loop (the grid's y extent)."""
    v, want, _ = K.scan_case(prime(fid), n, batch)
    got = gpu_ctx.prefix_product(fid, v)
    what = "prefix_product field %d n %d batch %d" % (fid, n, batch)
    if batch > 65535:
        for vec in (65534, 65535, 65536, batch - 1):
            assert_same(got[vec], want[vec], "%s, vector %d" % (what, vec))
    assert_same(got, want, what, per_vector=n)


@pytest.mark.parametrize("fid,n,batch", [(0, n, b) for n, b in KATE_CASES] + [(f, n, b) for f in (1, 2) for n, b in KATE_CASES_OTHER_FIELDS])
def test_kate_division_every_plan(gpu_ctx, fid, n, batch):
    coeffs, xs, want = K.kate_case(prime(fid), n, batch)
    got = gpu_ctx.kate_division_batch(fid, coeffs, xs)
    assert_same(got, want, "kate_division field %d n %d batch %d" % (fid, n, batch), per_vector=n - 1)


@pytest.mark.parametrize("fid", [0, 1, 2])
def test_inner_product_fold_eval_batched(gpu_ctx, fid):
    """many vectors per launch: vector boundaries inside a workgroup (fold), vectors shorter than a workgroup, a u or an x
    per vector and one shared by all"""
    p = prime(fid)
    for n in (1, 255, 257, 1000):
        a, b, want = K.inner_product_case(p, n, 300)
        assert_same(gpu_ctx.inner_product(fid, a, b), want, "inner_product field %d n %d batch 300" % (fid, n))
    for half in (1, 255, 257, 1000):
        for nu in (1, 37):
            v, u, want = K.fold_case(p, half, 37, nu)
            assert_same(gpu_ctx.fold(fid, v, u), want, "fold field %d half %d batch 37 nu %d" % (fid, half, nu), per_vector=half)
    for n in (1, 255, 256, 257, 513):
        for nx in (1, 300):
            c, x, want = K.eval_case(p, n, 300, nx)
            assert_same(gpu_ctx.eval_polynomial(fid, c, x), want, "eval_polynomial field %d n %d batch 300 nx %d" % (fid, n, nx))
