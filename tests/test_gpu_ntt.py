"""GPU parity: bzh_ntt (HIP, through the C ABI) vs the CPU oracle, bit-exact.
Reference seam: halo2_proofs best_fft / EvaluationDomain::{ifft, coeff_to_extended,
extended_to_coeff} as reached from create_proof (benches/shot.rs:68)."""
import numpy as np
import pytest

import coracle as C
import pasta as O
from randutil import FIELD_MODULUS, uniform_below

pytestmark = pytest.mark.gpu


def rand_elems(rng, n, fid=0):
    """uniform below the modulus of field `fid` (tests/randutil.py)"""
    return uniform_below(rng, n, FIELD_MODULUS[fid])


@pytest.mark.parametrize("fid", [0, 1, 2])
@pytest.mark.parametrize("k", [0, 1, 2, 5, 8, 11, 12, 13, 14, 17])
def test_ntt_matches_oracle(gpu_ctx, oracle_c, fid, k):
    F = O.FIELD_BY_ID[fid]
    rng = np.random.default_rng(100 * fid + k)
    a = rand_elems(rng, 1 << k, fid)
    w = F.omega(k)
    got = gpu_ctx.ntt(fid, a, omega=w)
    assert (got == C.ntt(fid, a, w, threads=8)).all()


@pytest.mark.parametrize("k", [3, 11, 14, 17])
def test_intt_and_coset_match_oracle(gpu_ctx, oracle_c, k):
    F = O.FP
    rng = np.random.default_rng(k)
    a = rand_elems(rng, 1 << k)
    w, zeta = F.omega(k), F.g
    assert (gpu_ctx.ntt(0, a, omega=w, inverse=True) == C.ntt(0, a, w, inverse=True, threads=8)).all()
    assert (gpu_ctx.ntt(0, a, omega=w, coset_shift=zeta) == C.ntt(0, a, w, coset_shift=zeta, threads=8)).all()
    back = gpu_ctx.ntt(0, gpu_ctx.ntt(0, a, omega=w, coset_shift=zeta), omega=w, inverse=True, coset_shift=zeta)
    assert (back == a).all()


def test_ntt_domain_tables_follow_their_context(gpu_ctx, oracle_c):
    """The domain tables are cached per ctx and go with it: forward and inverse transforms at 2^4 (one pass) and 2^12 (two passes,
    the smallest size with a direct twiddle table) through a context, which is then closed; the next contexts -- often at the
    address the closed one had -- build their own tables and give the first one's outputs bit for bit, which are the oracle's."""
    import bzh2
    F = O.FP
    jobs = []
    for k in (4, 12):
        a = rand_elems(np.random.default_rng(900 + k), 1 << k)
        for inverse in (False, True):
            jobs.append((a, F.omega(k), inverse, C.ntt(0, a, F.omega(k), inverse=inverse, threads=8)))
    first = None
    for it in range(3):
        with bzh2.Context(0) as ctx:
            got = [ctx.ntt(0, a, omega=w, inverse=inverse) for a, w, inverse, _ in jobs]
            again = [ctx.ntt(0, a, omega=w, inverse=inverse) for a, w, inverse, _ in jobs]     # ... and from the cached tables
        if first is None:
            first = got
        for j, (_, _, _, want) in enumerate(jobs):
            assert (got[j] == first[j]).all() and (again[j] == first[j]).all() and (got[j] == want).all(), (it, j)


def test_ntt_batched_and_montgomery(gpu_ctx, oracle_c):
    import bzh2
    F = O.FP
    k, batch = 11, 19
    rng = np.random.default_rng(7)
    a = rand_elems(rng, batch << k).reshape(batch, 1 << k, 4)
    w = F.omega(k)
    got = gpu_ctx.ntt(0, a, omega=w)
    for b in range(batch):
        assert (got[b] == C.ntt(0, a[b], w)).all()
    # Montgomery in / out: same transform on x*R
    R, p = F.R, F.p
    am = C.ints_to_array([x * R % p for x in C.array_to_ints(a[0])])
    gm = gpu_ctx.ntt(0, am, omega=w * R % p, form=bzh2.FORM_MONTGOMERY)
    assert C.array_to_ints(gm) == [x * R % p for x in C.array_to_ints(got[0])]


def test_ntt_default_omega_is_domain_generator(gpu_ctx, oracle_c):
    F = O.FQ
    rng = np.random.default_rng(8)
    a = rand_elems(rng, 1 << 9, 1)
    assert (gpu_ctx.ntt(1, a) == C.ntt(1, a, F.omega(9))).all()


def test_ntt_errors(gpu_ctx):
    import bzh2
    with pytest.raises(bzh2.BzhError):
        gpu_ctx.ntt(0, np.zeros((3, 4), dtype=np.uint64))       # not a power of two
    with pytest.raises(bzh2.BzhError):
        gpu_ctx.ntt(3, np.zeros((4, 4), dtype=np.uint64), omega=1)  # BN254 Fq has 2-adicity 1


def test_ntt_2_22_roundtrip_and_spot_values(gpu_ctx, oracle_c):
    """Config 5 size: round trip + linearity-free spot check of 3 outputs by the definition
    restricted to a sparse input (oracle finishes in seconds)."""
    F = O.FP
    k = 22
    n = 1 << k
    rng = np.random.default_rng(22)
    a = rand_elems(rng, n)
    w = F.omega(k)
    fwd = gpu_ctx.ntt(0, a, omega=w)
    assert (gpu_ctx.ntt(0, fwd, omega=w, inverse=True) == a).all()
    sparse = np.zeros((n, 4), dtype=np.uint64)
    idx = [0, 1, 2049, n // 2 + 3, n - 1]
    sparse[idx] = a[idx]
    out = gpu_ctx.ntt(0, sparse, omega=w)
    vals = [C.limbs_to_int(a[i]) for i in idx]
    for i in (0, 5, 123457, n - 1):
        want = sum(v * pow(w, i * j, F.p) for j, v in zip(idx, vals)) % F.p
        assert C.limbs_to_int(out[i]) == want


@pytest.mark.parametrize("k", [2, 3, 11, 14, 17])
def test_coset_zeta_fast_path(gpu_ctx, oracle_c, k):
    """halo2's extended coset generator is ZETA (a primitive cube root of unity): the library takes a
    3-constant fast path for shift^3 == 1; results must equal the general-shift oracle."""
    F = O.FP
    zeta = pow(F.g, (F.p - 1) // 3, F.p)
    assert pow(zeta, 3, F.p) == 1 and zeta != 1
    rng = np.random.default_rng(300 + k)
    a = rand_elems(rng, 1 << k)
    w = F.omega(k)
    fwd = gpu_ctx.ntt(0, a, omega=w, coset_shift=zeta)
    assert (fwd == C.ntt(0, a, w, coset_shift=zeta, threads=8)).all()
    inv = gpu_ctx.ntt(0, a, omega=w, inverse=True, coset_shift=zeta)
    assert (inv == C.ntt(0, a, w, inverse=True, coset_shift=zeta, threads=8)).all()
    assert (gpu_ctx.ntt(0, fwd, omega=w, inverse=True, coset_shift=zeta) == a).all()


@pytest.mark.parametrize("k", [1, 11, 12, 19])
def test_plain_inverse_all_pass_counts(gpu_ctx, oracle_c, k):
    """n^-1 is a constant post-multiply for one pass and folded into the first inter-pass twiddle for
    two (k=12) and three (k=19) passes."""
    F = O.FQ
    rng = np.random.default_rng(400 + k)
    a = rand_elems(rng, 1 << k, 1)
    w = F.omega(k)
    assert (gpu_ctx.ntt(1, a, omega=w, inverse=True) == C.ntt(1, a, w, inverse=True, threads=8)).all()


@pytest.mark.parametrize("k,ext", [(3, 3), (5, 2), (8, 3), (9, 3), (11, 3), (11, 2), (12, 1), (14, 3), (10, 4), (6, 0), (12, 0), (4, 8), (3, 10)])
@pytest.mark.parametrize("shift", ["zeta", "generator", None])
def test_coeff_to_extended_matches_padded_oracle_ntt(gpu_ctx, oracle_c, k, ext, shift):
    """bzh_coeff_to_extended reads only the 2^k coefficients; the result is the coset NTT of the zero-padded vector
    (EvaluationDomain::coeff_to_extended).  ZETA is the shift create_proof uses (a cube root of unity: three-valued
    scaling path); the multiplicative generator exercises the general power table; None the plain transform."""
    F = O.FP
    batch = 3
    rng = np.random.default_rng(1000 * k + ext)
    a = rand_elems(rng, batch << k).reshape(batch, 1 << k, 4)
    ek = k + ext
    w = F.omega(ek)
    s = {"zeta": pow(F.g, (F.p - 1) // 3, F.p), "generator": F.g, None: None}[shift]
    got = gpu_ctx.coeff_to_extended(0, a, ek, omega_ext=w, coset_shift=s)
    assert got.shape == (batch, 1 << ek, 4)
    for b in range(batch):
        padded = np.zeros((1 << ek, 4), dtype=np.uint64)
        padded[: 1 << k] = a[b]
        assert (got[b] == C.ntt(0, padded, w, coset_shift=s, threads=8)).all()


def test_coeff_to_extended_montgomery_device_path_leaves_source_intact(gpu_ctx, oracle_c):
    import ctypes
    import torch
    import bzh2
    F = O.FP
    k, ek, batch = 11, 14, 5
    rng = np.random.default_rng(99)
    a = rand_elems(rng, batch << k).reshape(batch, 1 << k, 4)
    R, p = F.R, F.p
    am = C.ints_to_array([x * R % p for x in C.array_to_ints(a.reshape(-1, 4))]).reshape(batch, 1 << k, 4)
    src = torch.from_numpy(am.view(np.int64)).cuda()
    dst = torch.empty((batch, 1 << ek, 4), dtype=torch.int64, device="cuda")
    zeta = pow(F.g, (F.p - 1) // 3, F.p)
    L = bzh2.load()
    L.bzh_coeff_to_extended.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_uint, ctypes.c_void_p, ctypes.c_uint,
                                        ctypes.c_size_t, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64),
                                        ctypes.c_int, ctypes.c_int]
    wm = bzh2.int_to_limbs(F.omega(ek) * R % p)
    zm = bzh2.int_to_limbs(zeta * R % p)
    torch.cuda.synchronize()
    rc = L.bzh_coeff_to_extended(gpu_ctx.handle, 0, ctypes.c_void_p(src.data_ptr()), k, ctypes.c_void_p(dst.data_ptr()), ek, batch,
                                 wm.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), zm.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)),
                                 bzh2.FORM_MONTGOMERY, bzh2.MEM_DEVICE)
    assert rc == 0
    gpu_ctx.sync()
    assert (src.cpu().numpy().view(np.uint64) == am).all()
    got = dst.cpu().numpy().view(np.uint64)
    for b in range(batch):
        padded = np.zeros((1 << ek, 4), dtype=np.uint64)
        padded[: 1 << k] = a[b]
        want = C.array_to_ints(C.ntt(0, padded, F.omega(ek), coset_shift=zeta, threads=8))
        assert C.array_to_ints(got[b]) == [x * R % p for x in want]


# ---- closed-form inputs: expected values from Python integers by iterated products, no second NTT involved -------------------
def _batch_inverse(ds, p):
    """inverses of the non-zero ds (Montgomery's trick: one modular inversion)"""
    pre, acc = [], 1
    for d in ds:
        pre.append(acc)
        acc = acc * d % p
    inv = pow(acc, -1, p)
    out = [0] * len(ds)
    for i in range(len(ds) - 1, -1, -1):
        out[i] = inv * pre[i] % p
        inv = inv * ds[i] % p
    return out


def _geometric_unit(q, n, w, shift, p):
    """forward transform of a[j] = q^j on the coset `shift`: out[i] = sum_j (q shift w^i)^j -- n where the ratio is 1,
    otherwise ((q shift)^n - 1) / (q shift w^i - 1), which is EXACTLY zero when (q shift)^n == 1"""
    base = q * shift % p
    num = (pow(base, n, p) - 1) % p
    ratios, r = [], base
    for _ in range(n):
        ratios.append(r)
        r = r * w % p
    if num == 0:
        return [n if r == 1 else 0 for r in ratios]
    assert 1 not in ratios
    return [num * d % p for d in _batch_inverse([r - 1 for r in ratios], p)]


def _impulse_transform(v, j, n, w, shift, p):
    """forward transform of v at index j: out[i] = v shift^j (w^j)^i"""
    step, x, out = pow(w, j, p), v * pow(shift, j, p) % p, []
    if step == 1:
        return [x] * n
    if step == p - 1:
        return [x, p - x if x else 0] * (n // 2)
    for _ in range(n):
        out.append(x)
        x = x * step % p
    return out


def _closed_form_cases(fid, k, mode):
    """[(name, input array, expected ints)] for one field, size and mode ('forward', 'inverse', 'coset')"""
    from helpers import field_edges as E
    F = O.FIELD_BY_ID[fid]
    p, n = F.p, 1 << k
    vals = E.edge_values(p)
    w = F.omega(k)
    assert (p - 1) % 3 == 0
    zeta = pow(F.g, (p - 1) // 3, p)
    shift = zeta if mode == "coset" else 1
    w_eff = pow(w, -1, p) if mode == "inverse" else w
    ninv = pow(n, -1, p)
    post = (lambda out: [x * ninv % p for x in out]) if mode == "inverse" else (lambda out: out)
    cases = []
    # impulses: values p - 1, R mod p, 2^224 - 1 and a low part of p, one at each of the four positions
    for j, v in zip(sorted({0, 1, n // 2, n - 1}), (vals[3], vals[7], (1 << 224) - 1, p % (1 << 96))):
        assert v in vals
        a = np.zeros((n, 4), dtype=np.uint64)
        a[j] = C.int_to_limbs(v)
        cases.append(("impulse %#x at %d" % (v, j), a, post(_impulse_transform(v, j, n, w_eff, shift, p))))
    unit = {}
    for name, c, q in (("constant R^2 mod p", vals[8], 1), ("all p - 1", p - 1, 1), ("alternating (x, p - x)", vals[5], p - 1)):
        a = np.tile(C.ints_to_array([c, c if q == 1 else p - c]), (max(n // 2, 1), 1))[:n]
        if q not in unit:
            unit[q] = _geometric_unit(q, n, w_eff, shift, p)
        want = post([c * u % p if u else 0 for u in unit[q]])
        if mode != "coset":                       # n c (forward) or c (inverse) at one index, exactly zero elsewhere
            at = 0 if q == 1 else n // 2
            assert want == [(c if mode == "inverse" else n * c % p) if i == at else 0 for i in range(n)]
        cases.append((name, a, want))
    return w, (zeta if mode == "coset" else None), cases


@pytest.mark.parametrize("mode", ["forward", "inverse", "coset"])
@pytest.mark.parametrize("k", [1, 6, 11, 12, 17, 19])
@pytest.mark.parametrize("fid", [0, 1, 2])
def test_ntt_closed_form_inputs(gpu_ctx, fid, k, mode):
    """Impulses, constant vectors, all p - 1 and alternating (x, p - x) through one, two and three passes: inputs whose
    transform has a closed form (a geometric sequence, or n c at one index and exactly zero elsewhere), with edge values of
    tests/helpers/field_edges.py as the non-zero entries.  Butterflies then meet a + b == p, a - a and operands 0 and p - 1
    at every stage, which uniform inputs never produce."""
    w, shift, cases = _closed_form_cases(fid, k, mode)
    a = np.stack([c[1] for c in cases])
    got = gpu_ctx.ntt(fid, a, omega=w, inverse=(mode == "inverse"), coset_shift=shift)
    for b, (name, _, want) in enumerate(cases):
        bad = (got[b] != C.ints_to_array(want)).any(axis=1)
        assert not bad.any(), "field %d k=%d %s, %s: %d outputs differ, first at index %d: got %#x want %#x" % (
            fid, k, mode, name, int(bad.sum()), int(np.argmax(bad)), C.limbs_to_int(got[b][int(np.argmax(bad))]),
            want[int(np.argmax(bad))])


@pytest.mark.parametrize("mode", ["forward", "inverse", "coset"])
@pytest.mark.parametrize("k", [1, 6, 11, 12, 14])
@pytest.mark.parametrize("fid", [0, 1, 2])
def test_ntt_of_the_edge_values_in_montgomery_form(gpu_ctx, oracle_c, fid, k, mode):
    """a vector cycling through the 256 edge values as raw Montgomery-form bits (no conversion touches them before the first
    butterfly) against the oracle's transform of the same values times R^-1"""
    import bzh2
    from helpers import field_edges as E
    F = O.FIELD_BY_ID[fid]
    p, n = F.p, 1 << k
    vals = E.edge_values(p)
    raw = [vals[i % 256] for i in range(n)]
    rinv = pow(E.R, -1, p)
    w = F.omega(k)
    zeta = pow(F.g, (p - 1) // 3, p) if mode == "coset" else None
    want = C.array_to_ints(C.ntt(fid, C.ints_to_array([x * rinv % p for x in raw]), w, inverse=(mode == "inverse"),
                                 coset_shift=zeta, threads=8))
    got = gpu_ctx.ntt(fid, C.ints_to_array(raw), omega=w * E.R % p, inverse=(mode == "inverse"),
                      coset_shift=None if zeta is None else zeta * E.R % p, form=bzh2.FORM_MONTGOMERY)
    assert C.array_to_ints(got) == [x * E.R % p for x in want], (fid, k, mode)
