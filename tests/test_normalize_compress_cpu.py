"""bzh_batch_normalize, bzh_affine_compress_batch and bzh_batch_normalize_plan without a device: the host path (ctx == NULL)
runs csrc/normalize.hpp's chain code -- the code the kernels run -- with the launch's own shape, so the running products sit in
the output buffers here too.  Checked against Python integers (tests/helpers/normalize_cases.py), against the separate host
code behind bzh_jacobian_to_affine / bzh_affine_compress, through bzh_affine_decompress and back, with identities at every
position of a chain, and on every argument error."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from helpers import normalize_cases as K

VP = ctypes.c_void_p
FORMS = (0, 1)


@pytest.fixture(scope="module")
def bzh2_lib():
    import bzh2
    bzh2.load()
    return bzh2


def _plan(bzh2_lib):
    return bzh2_lib.batch_normalize_plan


def _check_against(bzh2_lib, cid, form, triples):
    exp = K.expected(cid, triples)
    xy, enc, st = bzh2_lib.batch_normalize(cid, K.jac_array(cid, triples, form), form=form, want_bytes=True, want_status=True)
    assert st.tolist() == K.want_status(exp), (cid, form, len(triples))
    assert xy.tobytes() == K.want_xy_bytes(cid, exp, form), (cid, form, len(triples))
    assert enc.tobytes() == K.want_enc_bytes(exp), (cid, form, len(triples))
    return xy, enc, st


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("cid", [0, 1, 2])
def test_host_path_matches_python_integers(bzh2_lib, cid, form):
    cv = K.curve_of(cid)
    es = K.edge_set(cid)
    exp = K.expected(cid, es)
    pts = K.affine_points(cid)
    assert (exp[0][1], exp[0][2]) == (exp[2][1], exp[2][2]) and (exp[0][1], exp[0][2]) in pts   # the division gives back the construction
    assert {e[0] for e in exp} == {K.POINT_OK, K.POINT_IDENTITY} and {e[2] & 1 for e in exp if e[0] == 0} == {0, 1}
    assert exp[8][1] == exp[9][1] and exp[8][2] == cv.p - exp[9][2]                                # a point next to its negation
    for n in K.CPU_SIZES:
        _check_against(bzh2_lib, cid, form, K.batch(cid, n, seed=n))


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("cid", [0, 1, 2])
def test_host_path_matches_the_existing_entry_points_and_round_trips(bzh2_lib, cid, form):
    triples = K.batch(cid, 257, seed=3)
    jac = K.jac_array(cid, triples, form)
    xy, enc, st = bzh2_lib.batch_normalize(cid, jac, form=form, want_bytes=True, want_status=True)
    old_xy = bzh2_lib.jacobian_to_affine(cid, jac, form)
    assert xy.tobytes() == old_xy.tobytes()
    old_enc = b"".join(bzh2_lib.affine_compress(cid, old_xy, form))
    assert enc.tobytes() == old_enc
    assert bzh2_lib.affine_compress_batch(cid, old_xy, form=form).tobytes() == old_enc
    assert bzh2_lib.affine_compress_batch(cid, np.zeros((0, 8), dtype=np.uint64), form=form).shape == (0, 32)
    # only one of the two outputs: the running products then wait in that output alone
    only_xy = bzh2_lib.batch_normalize(cid, jac, form=form)
    assert only_xy[0].tobytes() == xy.tobytes() and only_xy[1] is None and only_xy[2] is None
    only_enc = bzh2_lib.batch_normalize(cid, jac, form=form, want_xy=False, want_bytes=True)
    assert only_enc[0] is None and only_enc[1].tobytes() == enc.tobytes()
    # from_bytes of the encodings gives the points and the statuses back
    back, back_st = bzh2_lib.affine_decompress(cid, [bytes(r) for r in enc], form)
    assert back.tobytes() == xy.tobytes() and back_st.tolist() == st.tolist()


def _host(bzh2_lib, cid, form, triples):
    xy, enc, st = bzh2_lib.batch_normalize(cid, K.jac_array(cid, triples, form), form=form, want_bytes=True, want_status=True)
    return xy, enc, st


@pytest.mark.parametrize("cid,form", [(0, 1), (1, 0), (2, 1)])
def test_identities_do_not_poison_their_chain(bzh2_lib, cid, form):
    plan = _plan(bzh2_lib)
    n = K.smallest_n_with_chain(plan, 3) + 5
    lanes, chain = plan(n)
    assert chain == 3
    own = lambda t: K.chain_indices(n, lanes, t)
    assert len(own(0)) == 3 and len(own(lanes - 1)) == 2                      # the last chains are one point shorter
    places = [own(1)[0], own(2)[1], own(3)[2], own(lanes - 1)[-1]] + own(5) + own(lanes - 2)   # first, interior, last; whole chains
    clean = K.batch(cid, n, seed=7)
    marked = K.batch(cid, n, seed=7, identities=places)
    keep = np.array([t[2] != 0 for t in clean]) & ~np.isin(np.arange(n), places)
    a, b = _host(bzh2_lib, cid, form, clean), _host(bzh2_lib, cid, form, marked)
    for x, y in zip(a, b):
        assert (x[keep] == y[keep]).all()
    assert not b[0][places].any() and not b[1][places].any() and (b[2][places] == K.POINT_IDENTITY).all()
    assert (b[2][keep] == K.POINT_OK).all() and b[0][keep].any(axis=1).all()
    assert b[0].tobytes() == bzh2_lib.jacobian_to_affine(cid, K.jac_array(cid, marked, form), form).tobytes()
    # a sample of the long batch against Python integers, the marked places and their chain neighbours among them
    sample = sorted(set(places[:4] + own(1) + own(2) + own(3) + list(range(0, n, 997))))
    exp = K.expected(cid, [marked[i] for i in sample])
    assert b[0][sample].tobytes() == K.want_xy_bytes(cid, exp, form) and b[1][sample].tobytes() == K.want_enc_bytes(exp)
    # every point the identity
    zeros = K.batch(cid, 300, seed=1, identities=range(300))
    xy, enc, st = _host(bzh2_lib, cid, form, zeros)
    assert not xy.any() and not enc.any() and (st == K.POINT_IDENTITY).all()
    # ... which is not an error without a status buffer either
    assert not bzh2_lib.batch_normalize(cid, K.jac_array(cid, zeros, form), form=form)[0].any()


def test_arguments(bzh2_lib):
    L = bzh2_lib._bind_normalize()
    OK, E_ARG, E_RANGE, H, D = bzh2_lib.OK, bzh2_lib.E_ARG, bzh2_lib.E_RANGE, bzh2_lib.MEM_HOST, bzh2_lib.MEM_DEVICE
    triples = K.batch(0, 7)
    jac = K.jac_array(0, triples, 0)
    xy, enc, st = np.full((7, 8), 0x5a, dtype=np.uint64), np.full((7, 32), 0x5a, dtype=np.uint8), np.full(7, 0x5a, dtype=np.uint8)
    p = lambda a: VP(a.ctypes.data)
    call = L.bzh_batch_normalize
    assert call(None, 0, p(jac), 7, 0, H, p(xy), p(enc), p(st)) == OK
    for cid in (-1, 3):
        assert call(None, cid, p(jac), 7, 0, H, p(xy), p(enc), p(st)) == E_ARG                 # unknown curve
    assert call(None, 0, p(jac), 7, 2, H, p(xy), p(enc), p(st)) == E_ARG                       # unknown form
    assert call(None, 0, p(jac), 7, 0, 2, p(xy), p(enc), p(st)) == E_ARG                       # unknown mem
    assert call(None, 0, p(jac), 7, 0, H, None, None, p(st)) == E_ARG                          # both outputs NULL
    assert call(None, 0, None, 7, 0, H, p(xy), p(enc), p(st)) == E_ARG                         # NULL input with n > 0
    assert call(None, 0, p(jac), 7, 0, D, p(xy), p(enc), p(st)) == E_ARG                       # device memory without a ctx
    assert call(None, 0, None, 0, 0, H, None, None, None) == OK                                # n == 0
    assert call(None, 0, p(jac), 0, 1, H, p(xy), None, None) == OK
    comp = L.bzh_affine_compress_batch
    axy = np.zeros((7, 8), dtype=np.uint64)
    assert comp(None, 0, p(axy), 7, 0, H, p(enc)) == OK
    for bad in ((None, 3, p(axy), 7, 0, H, p(enc)), (None, 0, p(axy), 7, 2, H, p(enc)), (None, 0, p(axy), 7, 0, 2, p(enc)),
                (None, 0, None, 7, 0, H, p(enc)), (None, 0, p(axy), 7, 0, H, None), (None, 0, p(axy), 7, 0, D, p(enc))):
        assert comp(*bad) == E_ARG
    assert comp(None, 0, None, 0, 0, H, None) == OK
    lanes, chain = ctypes.c_size_t(), ctypes.c_size_t()
    assert L.bzh_batch_normalize_plan(5, None, ctypes.byref(chain)) == E_ARG
    assert L.bzh_batch_normalize_plan(5, ctypes.byref(lanes), None) == E_ARG


@pytest.mark.parametrize("cid", [0, 1, 2])
def test_a_canonical_coordinate_not_below_p_is_refused_before_anything_is_written(bzh2_lib, cid):
    L = bzh2_lib._bind_normalize()
    prime = K.curve_of(cid).p
    triples = K.batch(cid, 7)
    for bad in (prime, (1 << 256) - 1):
        for pos, coord in ((0, 0), (3, 1), (6, 2)):
            t = [list(x) for x in triples]
            t[pos][coord] = bad
            jac = np.frombuffer(K.limbs_bytes(c for x in t for c in x), dtype=np.uint64).reshape(-1, 12).copy()
            for with_status in (True, False):
                xy, enc, st = np.full((7, 8), 0x5a5a, dtype=np.uint64), np.full((7, 32), 0x5a, dtype=np.uint8), np.full(7, 0x5a, dtype=np.uint8)
                rc = L.bzh_batch_normalize(None, cid, VP(jac.ctypes.data), 7, bzh2_lib.FORM_CANONICAL, bzh2_lib.MEM_HOST, VP(xy.ctypes.data),
                                           VP(enc.ctypes.data), VP(st.ctypes.data) if with_status else None)
                assert rc == bzh2_lib.E_RANGE, (bad, pos, coord)
                assert (xy == 0x5a5a).all() and (enc == 0x5a).all() and (st == 0x5a).all()
            with pytest.raises(bzh2_lib.BzhError) as e:
                bzh2_lib.batch_normalize(cid, jac, want_status=True)
            assert e.value.status == bzh2_lib.E_RANGE


def test_plan(bzh2_lib):
    plan = _plan(bzh2_lib)
    assert plan(1) == (1, 1)
    ns = sorted(set(list(range(1, 300)) + [2 ** k + d for k in range(8, 27) for d in (-1, 0, 1)] + list(range(1, 1 << 21, 4099))))
    prev, longest = 1, 1
    for n in ns:
        lanes, chain = plan(n)
        assert lanes * chain >= n and lanes >= 1 and chain >= prev, n
        assert (chain - 1) * lanes < n, n                    # no lane is empty and every lane's chain is `chain` or one shorter
        prev, longest = chain, max(longest, chain)
    assert longest >= 2
    n2, n3 = K.smallest_n_with_chain(plan, 2), K.smallest_n_with_chain(plan, 3)
    assert plan(n2 - 1)[1] == 1 and plan(n2)[1] == 2 and plan(n3 - 1)[1] == 2 and plan(n3)[1] == 3


def test_chain_code_standalone_under_host_sanitizers(tmp_path):
    """tests/helpers/normalize_check.hip: the chain code with its own main, built with ASan + UBSan for the host, on the CPU"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "normalize_check")
    subprocess.check_call([hipcc, "-O1", "-g", "-std=c++17", "--offload-arch=gfx950", "-Wno-unused-function",
                           "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(root, "battlezips-halo2_amd", "csrc"),
                           os.path.join(root, "tests", "helpers", "normalize_check.hip"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip().endswith("normalize_check: ok"), out.stdout[-2000:] + out.stderr[-2000:]
