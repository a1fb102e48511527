"""bzh2 -- ctypes host binding over the C ABI of include/bzh2.h (libbzh2.so).

The product path: every call below lands in hand-written HIP kernels for
gfx950.  There is NO CPU fallback: if libbzh2.so is missing or there is no GPU,
calls raise.  This module never imports anything from oracle/.

Host-side mirror of the interface the reference reaches for the create_proof hot
path (halo2_proofs 0.2.0, un-vendored):
    best_multiexp(coeffs, bases)            -> Context.msm(bases, scalars)
    Params::commit / commit_lagrange        -> Context.upload_bases + Context.msm
    best_fft(a, omega, log_n)               -> Context.ntt(...)
    EvaluationDomain::ifft / coeff_to_extended / extended_to_coeff
                                            -> Context.ntt(inverse=, coset_shift=)
Names, argument meaning and error behaviour follow the upstream functions: a
length mismatch between scalars and bases is an error (upstream asserts), field
elements are 4 x u64 little-endian limbs.
"""
from __future__ import annotations

import ctypes
import os

import numpy as np

_PKG = os.path.dirname(os.path.abspath(__file__))
_LIB_PATH = os.path.join(os.path.dirname(_PKG), "libbzh2.so")

OK, E_ARG, E_OOM, E_HIP, E_RANGE, E_NOGPU = 0, -1, -2, -3, -4, -5
CURVE_VESTA, CURVE_PALLAS, CURVE_BN254 = 0, 1, 2
FIELD_FP, FIELD_FQ, FIELD_BN254_FR, FIELD_BN254_FQ = 0, 1, 2, 3
FORM_CANONICAL, FORM_MONTGOMERY = 0, 1
MEM_HOST, MEM_DEVICE = 0, 1
T_MSM_DIGITS, T_MSM_ACCUMULATE, T_MSM_REDUCE, T_MSM_FINALIZE, T_NTT, T_COUNT = 0, 1, 2, 3, 4, 8
TIMER_NAMES = {0: "msm_digits", 1: "msm_accumulate", 2: "msm_reduce", 3: "msm_finalize", 4: "ntt"}

# scalar field of each curve (Vesta scalars are Fp, Pallas scalars are Fq)
CURVE_SCALAR_FIELD = {CURVE_VESTA: FIELD_FP, CURVE_PALLAS: FIELD_FQ, CURVE_BN254: FIELD_BN254_FR}

# every symbol include/bzh2.h declares
EXPORTS = [
    "bzh_version", "bzh_strerror", "bzh_device_count", "bzh_ctx_create", "bzh_ctx_create_on_stream",
    "bzh_ctx_destroy", "bzh_ctx_sync", "bzh_last_error", "bzh_ctx_profile", "bzh_ctx_timings", "bzh_ctx_work", "bzh_ctx_msm_additions",
    "bzh_bases_upload", "bzh_bases_precompute", "bzh_bases_free", "bzh_bases_len", "bzh_bases_walk", "bzh_bases_points", "bzh_msm", "bzh_ntt", "bzh_coeff_to_extended",
    "bzh_jacobian_to_affine", "bzh_jacobian_sum", "bzh_affine_compress", "bzh_field_omega",
]


class BzhError(RuntimeError):
    def __init__(self, status: int, where: str, detail: str = ""):
        self.status = status
        super().__init__("%s failed: %s (%d)%s" % (where, _strerror(status), status, (": " + detail) if detail else ""))


_lib = None


def lib_path() -> str:
    return _LIB_PATH


def load():
    """Load libbzh2.so or raise -- the product path has no fallback."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(_LIB_PATH):
        raise ImportError("libbzh2.so not built at %s: run `python -c 'import __graft_entry__ as g; g.build()'`" % _LIB_PATH)
    L = ctypes.CDLL(_LIB_PATH)
    u64p = ctypes.POINTER(ctypes.c_uint64)
    vp = ctypes.c_void_p
    L.bzh_version.restype = ctypes.c_char_p
    L.bzh_strerror.restype = ctypes.c_char_p
    L.bzh_strerror.argtypes = [ctypes.c_int]
    L.bzh_device_count.restype = ctypes.c_int
    L.bzh_ctx_create.argtypes = [ctypes.c_int, ctypes.POINTER(vp)]
    L.bzh_ctx_create_on_stream.argtypes = [ctypes.c_int, vp, ctypes.POINTER(vp)]
    L.bzh_ctx_destroy.argtypes = [vp]
    L.bzh_ctx_sync.argtypes = [vp]
    L.bzh_last_error.argtypes = [vp]
    L.bzh_last_error.restype = ctypes.c_char_p
    L.bzh_ctx_profile.argtypes = [vp, ctypes.c_int]
    L.bzh_ctx_timings.argtypes = [vp, ctypes.POINTER(ctypes.c_double), u64p]
    L.bzh_bases_upload.argtypes = [vp, ctypes.c_int, vp, ctypes.c_size_t, ctypes.c_int, ctypes.c_int, ctypes.POINTER(vp)]
    L.bzh_bases_precompute.argtypes = [vp, vp, ctypes.c_int]
    L.bzh_bases_free.argtypes = [vp, vp]
    L.bzh_bases_len.argtypes = [vp]
    L.bzh_bases_len.restype = ctypes.c_size_t
    L.bzh_msm.argtypes = [vp, vp, vp, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_int, ctypes.c_int, vp]
    L.bzh_ntt.argtypes = [vp, ctypes.c_int, vp, ctypes.c_uint, ctypes.c_size_t, u64p, u64p, ctypes.c_int, ctypes.c_int,
                          ctypes.c_int]
    L.bzh_jacobian_to_affine.argtypes = [ctypes.c_int, u64p, ctypes.c_size_t, ctypes.c_int, u64p]
    L.bzh_affine_compress.argtypes = [ctypes.c_int, u64p, ctypes.c_size_t, ctypes.c_int, ctypes.POINTER(ctypes.c_uint8)]
    L.bzh_field_omega.argtypes = [ctypes.c_int, ctypes.c_uint, ctypes.c_int, u64p]
    _lib = L
    return L


def _strerror(status: int) -> str:
    try:
        return load().bzh_strerror(status).decode()
    except Exception:  # pragma: no cover
        return "status %d" % status


def device_count() -> int:
    return load().bzh_device_count()


def _u64(a: np.ndarray):
    assert a.dtype == np.uint64 and a.flags["C_CONTIGUOUS"], "need contiguous uint64"
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))


def int_to_limbs(x: int) -> np.ndarray:
    return np.frombuffer(int(x).to_bytes(32, "little"), dtype=np.uint64).copy()


def limbs_to_int(a) -> int:
    return int.from_bytes(np.ascontiguousarray(a, dtype=np.uint64).tobytes(), "little")


class Bases:
    """Device-resident commitment bases (halo2 Params.g / g_lagrange)."""

    def __init__(self, ctx: "Context", handle, curve: int, n: int):
        self.ctx, self.handle, self.curve, self.n = ctx, handle, curve, n

    def precompute(self, window_bits: int = 0):
        """Expand into the fixed-base window table (bzh_bases_precompute)."""
        self.ctx._check(load().bzh_bases_precompute(self.ctx.handle, self.handle, window_bits), "bzh_bases_precompute")
        return self

    def free(self):
        if self.handle is not None:
            load().bzh_bases_free(self.ctx.handle, self.handle)
            self.handle = None

    def __len__(self):
        return self.n


class Context:
    """One device + one HIP stream (bzh_ctx)."""

    def __init__(self, device: int = 0, stream: int | None = None):
        L = load()
        h = ctypes.c_void_p()
        if stream is None:
            rc = L.bzh_ctx_create(device, ctypes.byref(h))
        else:
            rc = L.bzh_ctx_create_on_stream(device, ctypes.c_void_p(stream), ctypes.byref(h))
        if rc != OK:
            raise BzhError(rc, "bzh_ctx_create")
        self.handle = h
        self.device = device

    def _check(self, rc: int, where: str):
        if rc != OK:
            raise BzhError(rc, where, load().bzh_last_error(self.handle).decode())

    def close(self):
        if self.handle is not None:
            load().bzh_ctx_destroy(self.handle)
            self.handle = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def sync(self):
        self._check(load().bzh_ctx_sync(self.handle), "bzh_ctx_sync")

    def profile(self, enable: bool = True):
        self._check(load().bzh_ctx_profile(self.handle, int(enable)), "bzh_ctx_profile")

    def timings(self) -> dict:
        ms = (ctypes.c_double * T_COUNT)()
        n = (ctypes.c_uint64 * T_COUNT)()
        self._check(load().bzh_ctx_timings(self.handle, ms, n), "bzh_ctx_timings")
        wb = (ctypes.c_double * T_COUNT)()
        load().bzh_ctx_work.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_double)]
        self._check(load().bzh_ctx_work(self.handle, wb), "bzh_ctx_work")
        return {TIMER_NAMES[i]: {"ms": ms[i], "launches": int(n[i]), "algorithmic_bytes": wb[i]} for i in TIMER_NAMES}

    def msm_additions(self) -> int:
        """bucket additions made by the MSM accumulation since profile(True)"""
        v = ctypes.c_uint64()
        L = load()
        L.bzh_ctx_msm_additions.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64)]
        self._check(L.bzh_ctx_msm_additions(self.handle, ctypes.byref(v)), "bzh_ctx_msm_additions")
        return int(v.value)

    # ---- bases ----
    def upload_bases(self, curve: int, xy, n: int | None = None, form: int = FORM_CANONICAL, device_ptr: bool = False) -> Bases:
        h = ctypes.c_void_p()
        if device_ptr:
            ptr, mem = ctypes.c_void_p(int(xy)), MEM_DEVICE
            assert n is not None
        else:
            xy = np.ascontiguousarray(xy, dtype=np.uint64)
            n = xy.size // 8 if n is None else n
            ptr, mem = ctypes.c_void_p(xy.ctypes.data), MEM_HOST
        self._check(load().bzh_bases_upload(self.handle, curve, ptr, n, form, mem, ctypes.byref(h)), "bzh_bases_upload")
        return Bases(self, h, curve, n)

    def bases_walk(self, curve: int, g_xy, n: int, form: int = FORM_CANONICAL) -> Bases:
        """bases[i] = [i + 1] G for i < n, made on the device (bzh_bases_walk); g_xy: 8 limbs of one affine point"""
        g = np.ascontiguousarray(g_xy, dtype=np.uint64).reshape(8)
        h = ctypes.c_void_p()
        L = load()
        L.bzh_bases_walk.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.POINTER(ctypes.c_void_p)]
        self._check(L.bzh_bases_walk(self.handle, curve, ctypes.c_void_p(g.ctypes.data), form, n, ctypes.byref(h)), "bzh_bases_walk")
        return Bases(self, h, curve, n)

    def bases_points(self, bases: Bases, first: int, count: int) -> np.ndarray:
        """points [first, first + count) of a table as (count, 8) canonical limbs (bzh_bases_points)"""
        out = np.zeros((count, 8), dtype=np.uint64)
        L = load()
        L.bzh_bases_points.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_void_p]
        self._check(L.bzh_bases_points(self.handle, bases.handle, first, count, ctypes.c_void_p(out.ctypes.data)), "bzh_bases_points")
        return out

    # ---- MSM ----
    def msm(self, bases: Bases, scalars: np.ndarray, form: int = FORM_CANONICAL) -> np.ndarray:
        """best_multiexp for `batch` scalar vectors: scalars (batch, n, 4) or (n, 4) uint64 -> (batch, 12) Jacobian."""
        s = np.ascontiguousarray(scalars, dtype=np.uint64)
        if s.ndim == 2:
            s = s.reshape(1, *s.shape)
        batch, n = s.shape[0], s.shape[1]
        assert s.shape[2] == 4
        out = np.zeros((batch, 12), dtype=np.uint64)
        rc = load().bzh_msm(self.handle, bases.handle, ctypes.c_void_p(s.ctypes.data), n, batch, form, MEM_HOST,
                            ctypes.c_void_p(out.ctypes.data))
        self._check(rc, "bzh_msm")
        return out

    def msm_device(self, bases: Bases, scalars_ptr: int, n: int, batch: int, out_ptr: int, form: int = FORM_MONTGOMERY):
        """Device-pointer form: enqueues on the ctx stream, no copies, no sync."""
        rc = load().bzh_msm(self.handle, bases.handle, ctypes.c_void_p(scalars_ptr), n, batch, form, MEM_DEVICE,
                            ctypes.c_void_p(out_ptr))
        self._check(rc, "bzh_msm")

    # ---- NTT ----
    def ntt(self, field: int, data: np.ndarray, omega: int | None = None, inverse: bool = False,
            coset_shift: int | None = None, form: int = FORM_CANONICAL) -> np.ndarray:
        """best_fft over (batch, n, 4) or (n, 4) uint64; returns a new array."""
        a = np.ascontiguousarray(data, dtype=np.uint64).copy()
        shape = a.shape
        if a.ndim == 2:
            a = a.reshape(1, *a.shape)
        batch, n = a.shape[0], a.shape[1]
        log_n = n.bit_length() - 1
        if n == 0 or (1 << log_n) != n:
            raise BzhError(E_ARG, "bzh_ntt", "length must be a power of two")
        w = field_omega(field, log_n, form) if omega is None else int_to_limbs(omega)
        cs = None if coset_shift is None else int_to_limbs(coset_shift)
        rc = load().bzh_ntt(self.handle, field, ctypes.c_void_p(a.ctypes.data), log_n, batch, _u64(w),
                            _u64(cs) if cs is not None else None, int(inverse), form, MEM_HOST)
        self._check(rc, "bzh_ntt")
        return a.reshape(shape)

    def coeff_to_extended(self, field: int, coeffs: np.ndarray, log_ext: int, omega_ext: int | None = None,
                          coset_shift: int | None = None, form: int = FORM_CANONICAL) -> np.ndarray:
        """EvaluationDomain::coeff_to_extended over (batch, n, 4) or (n, 4) uint64 coefficients -> (batch, 2^log_ext, 4)."""
        a = np.ascontiguousarray(coeffs, dtype=np.uint64)
        squeeze = a.ndim == 2
        if squeeze:
            a = a.reshape(1, *a.shape)
        batch, n = a.shape[0], a.shape[1]
        log_n = n.bit_length() - 1
        if n != 1 << log_n:
            raise BzhError(E_ARG, "bzh_coeff_to_extended", "length must be a power of two")
        w = field_omega(field, log_ext, form) if omega_ext is None else int_to_limbs(omega_ext)
        sh = None if coset_shift is None else int_to_limbs(coset_shift)
        out = np.zeros((batch, 1 << log_ext, 4), dtype=np.uint64)
        L = load()
        L.bzh_coeff_to_extended.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_uint, ctypes.c_void_p, ctypes.c_uint,
                                            ctypes.c_size_t, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64),
                                            ctypes.c_int, ctypes.c_int]
        rc = L.bzh_coeff_to_extended(self.handle, field, ctypes.c_void_p(a.ctypes.data), log_n, ctypes.c_void_p(out.ctypes.data), log_ext,
                                     batch, _u64(w), _u64(sh) if sh is not None else None, form, MEM_HOST)
        self._check(rc, "bzh_coeff_to_extended")
        return out[0] if squeeze else out

    def ntt_device(self, field: int, data_ptr: int, log_n: int, batch: int, omega: np.ndarray,
                   coset_shift: np.ndarray | None = None, inverse: bool = False, form: int = FORM_MONTGOMERY):
        rc = load().bzh_ntt(self.handle, field, ctypes.c_void_p(data_ptr), log_n, batch, _u64(omega),
                            _u64(coset_shift) if coset_shift is not None else None, int(inverse), form, MEM_DEVICE)
        self._check(rc, "bzh_ntt")


# ---- host helpers -----------------------------------------------------------
def jacobian_to_affine(curve: int, xyz: np.ndarray, form: int = FORM_CANONICAL) -> np.ndarray:
    a = np.ascontiguousarray(xyz, dtype=np.uint64).reshape(-1, 12)
    out = np.zeros((a.shape[0], 8), dtype=np.uint64)
    rc = load().bzh_jacobian_to_affine(curve, _u64(a), a.shape[0], form, _u64(out))
    if rc != OK:
        raise BzhError(rc, "bzh_jacobian_to_affine")
    return out


def jacobian_sum(curve: int, xyz: np.ndarray, form: int = FORM_CANONICAL) -> np.ndarray:
    """Sum of Jacobian points on the host (the combine step of an MSM split over several GPUs)."""
    a = np.ascontiguousarray(xyz, dtype=np.uint64).reshape(-1, 12)
    out = np.zeros(12, dtype=np.uint64)
    L = load()
    L.bzh_jacobian_sum.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_uint64), ctypes.c_size_t, ctypes.c_int, ctypes.POINTER(ctypes.c_uint64)]
    rc = L.bzh_jacobian_sum(curve, _u64(a), a.shape[0], form, _u64(out))
    if rc != OK:
        raise BzhError(rc, "bzh_jacobian_sum")
    return out


def affine_compress(curve: int, xy: np.ndarray, form: int = FORM_CANONICAL) -> list:
    a = np.ascontiguousarray(xy, dtype=np.uint64).reshape(-1, 8)
    out = np.zeros((a.shape[0], 32), dtype=np.uint8)
    rc = load().bzh_affine_compress(curve, _u64(a), a.shape[0], form, out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)))
    if rc != OK:
        raise BzhError(rc, "bzh_affine_compress")
    return [bytes(r) for r in out]


EXPORTS += ["bzh_batch_sqrt", "bzh_affine_decompress", "bzh_pk_verify_select", "bzh_pk_verify_selected"]
POINT_OK, POINT_IDENTITY, POINT_INVALID = 0, 1, 2


def _bind_sqrt():
    L = load()
    vp, u8p = ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint8)
    L.bzh_batch_sqrt.argtypes = [vp, ctypes.c_int, vp, ctypes.c_size_t, ctypes.c_int, ctypes.c_int, u8p]
    L.bzh_affine_decompress.argtypes = [vp, ctypes.c_int, vp, ctypes.c_size_t, ctypes.c_int, ctypes.c_int, vp, u8p]
    return L


def batch_sqrt(field: int, data, form: int = FORM_CANONICAL, ctx=None):
    """ff::Field::sqrt per element (bzh_batch_sqrt; the root pasta_curves 0.4.1 returns): (roots, status) -- status (n,) uint8,
    1 = a square (its root is in `roots`), 0 = not a square (the element is handed back unchanged).  ctx None: on the host."""
    a = np.ascontiguousarray(data, dtype=np.uint64).reshape(-1, 4).copy()
    st = np.zeros(a.shape[0], dtype=np.uint8)
    rc = _bind_sqrt().bzh_batch_sqrt(ctx.handle if ctx is not None else None, field, ctypes.c_void_p(a.ctypes.data), a.shape[0], form, MEM_HOST,
                                     st.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)))
    if rc != OK:
        raise BzhError(rc, "bzh_batch_sqrt")
    return a, st


def affine_decompress(curve: int, in32, form: int = FORM_CANONICAL, ctx=None, check: bool = False):
    """pasta_curves from_bytes for a list of 32-byte strings (bzh_affine_decompress): (xy, status) -- xy (n, 8) uint64 in `form`,
    status (n,) uint8 of POINT_OK / POINT_IDENTITY / POINT_INVALID (zeros in xy unless POINT_OK).  check=True passes no status
    buffer: BzhError E_RANGE if any string is not a point.  ctx None: on the host."""
    raw = b"".join(bytes(b) for b in in32)
    assert len(raw) % 32 == 0
    n = len(raw) // 32
    buf = np.frombuffer(raw, dtype=np.uint8).copy() if n else np.zeros(0, dtype=np.uint8)
    xy = np.zeros((n, 8), dtype=np.uint64)
    st = np.zeros(n, dtype=np.uint8)
    rc = _bind_sqrt().bzh_affine_decompress(ctx.handle if ctx is not None else None, curve, ctypes.c_void_p(buf.ctypes.data), n, form, MEM_HOST,
                                            ctypes.c_void_p(xy.ctypes.data), None if check else st.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)))
    if rc != OK:
        raise BzhError(rc, "bzh_affine_decompress")
    return xy, st


EXPORTS += ["bzh_batch_normalize", "bzh_affine_compress_batch", "bzh_batch_normalize_plan"]


def _bind_normalize():
    L = load()
    vp, u8p, szp = ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_size_t)
    L.bzh_batch_normalize.argtypes = [vp, ctypes.c_int, vp, ctypes.c_size_t, ctypes.c_int, ctypes.c_int, vp, vp, vp]
    L.bzh_affine_compress_batch.argtypes = [vp, ctypes.c_int, vp, ctypes.c_size_t, ctypes.c_int, ctypes.c_int, vp]
    L.bzh_batch_normalize_plan.argtypes = [ctypes.c_size_t, szp, szp]
    return L


def batch_normalize_plan(n: int):
    """(lanes, chain) of the launch bzh_batch_normalize makes for n points: lane t owns the points t, t + lanes, ..., at most
    `chain` of them (bzh_batch_normalize_plan)."""
    lanes, chain = ctypes.c_size_t(), ctypes.c_size_t()
    rc = _bind_normalize().bzh_batch_normalize_plan(n, ctypes.byref(lanes), ctypes.byref(chain))
    if rc != OK:
        raise BzhError(rc, "bzh_batch_normalize_plan")
    return lanes.value, chain.value


def batch_normalize(curve: int, xyz, *, ctx=None, form: int = FORM_CANONICAL, mem: int = MEM_HOST, want_xy: bool = True,
                    want_bytes: bool = False, want_status: bool = False, n: int | None = None, out_xy: int | None = None,
                    out32: int | None = None, status: int | None = None):
    """Curve::batch_normalize and to_bytes for Jacobian points in `form` (bzh_batch_normalize); ctx None: on the host.
    MEM_HOST: xyz is an (n, 12) uint64 array; returns (xy, enc, status) -- xy (n, 8) uint64 in `form`, enc (n, 32) uint8, status
    (n,) uint8 of POINT_OK / POINT_IDENTITY (zeros) --, None for what was not wanted.  A canonical coordinate that is not below p
    raises BzhError E_RANGE before anything is computed (host operands are checked first).
    MEM_DEVICE: xyz, out_xy, out32 and status are device pointers (ints, 16-byte aligned; out_xy or out32 may be None) and n the
    number of points; with a status pointer the call only enqueues on the ctx's stream (ctx.sync()).  Returns None."""
    L = _bind_normalize()
    h = ctx.handle if ctx is not None else None
    if mem == MEM_DEVICE:
        assert n is not None
        rc = L.bzh_batch_normalize(h, curve, ctypes.c_void_p(int(xyz)), n, form, mem, ctypes.c_void_p(out_xy) if out_xy else None,
                                   ctypes.c_void_p(out32) if out32 else None, ctypes.c_void_p(status) if status else None)
        if rc != OK:
            raise BzhError(rc, "bzh_batch_normalize", load().bzh_last_error(h).decode() if h else "")
        return None
    a = np.ascontiguousarray(xyz, dtype=np.uint64).reshape(-1, 12)
    cnt = a.shape[0]
    xy = np.zeros((cnt, 8), dtype=np.uint64) if want_xy else None
    enc = np.zeros((cnt, 32), dtype=np.uint8) if want_bytes else None
    st = np.zeros(cnt, dtype=np.uint8) if want_status else None
    rc = L.bzh_batch_normalize(h, curve, _vp(a), cnt, form, mem, *(None if o is None else _vp(o) for o in (xy, enc, st)))
    if rc != OK:
        raise BzhError(rc, "bzh_batch_normalize", load().bzh_last_error(h).decode() if h else "")
    return xy, enc, st


def affine_compress_batch(curve: int, xy, *, ctx=None, form: int = FORM_CANONICAL, mem: int = MEM_HOST, n: int | None = None,
                          out32: int | None = None):
    """to_bytes for affine points in `form` (bzh_affine_compress_batch): an (n, 32) uint8 array; ctx None: on the host.
    MEM_DEVICE: xy and out32 are device pointers (ints, 16-byte aligned), n the number of points; enqueues only, returns None."""
    L = _bind_normalize()
    h = ctx.handle if ctx is not None else None
    if mem == MEM_DEVICE:
        assert n is not None
        rc = L.bzh_affine_compress_batch(h, curve, ctypes.c_void_p(int(xy)), n, form, mem, ctypes.c_void_p(out32) if out32 else None)
        enc = None
    else:
        a = np.ascontiguousarray(xy, dtype=np.uint64).reshape(-1, 8)
        enc = np.zeros((a.shape[0], 32), dtype=np.uint8)
        rc = L.bzh_affine_compress_batch(h, curve, _vp(a), a.shape[0], form, mem, _vp(enc))
    if rc != OK:
        raise BzhError(rc, "bzh_affine_compress_batch", load().bzh_last_error(h).decode() if h else "")
    return enc


def field_omega(field: int, log_n: int, form: int = FORM_CANONICAL) -> np.ndarray:
    out = np.zeros(4, dtype=np.uint64)
    rc = load().bzh_field_omega(field, log_n, form, _u64(out))
    if rc != OK:
        raise BzhError(rc, "bzh_field_omega")
    return out


# ---- prover-stage vector primitives (host-buffer forms; see include/bzh2.h) --------------------
def _vp(a: np.ndarray):
    return ctypes.c_void_p(a.ctypes.data)


def _bind_poly(L):
    vp = ctypes.c_void_p
    L.bzh_batch_invert.argtypes = [vp, ctypes.c_int, vp, ctypes.c_size_t, ctypes.c_int, ctypes.c_int]
    L.bzh_prefix_product.argtypes = [vp, ctypes.c_int, vp, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_int, ctypes.c_int]
    L.bzh_eval_polynomial.argtypes = [vp, ctypes.c_int, vp, ctypes.c_size_t, ctypes.c_size_t, vp, ctypes.c_size_t, ctypes.c_int,
                                      ctypes.c_int, vp]
    L.bzh_inner_product.argtypes = [vp, ctypes.c_int, vp, vp, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_int, ctypes.c_int, vp]
    L.bzh_fold.argtypes = [vp, ctypes.c_int, vp, ctypes.c_size_t, ctypes.c_size_t, vp, ctypes.c_size_t, ctypes.c_int, ctypes.c_int, vp]
    L.bzh_vec_mul.argtypes = [vp, ctypes.c_int, vp, vp, ctypes.c_size_t, ctypes.c_int, ctypes.c_int]


EXPORTS += ["bzh_field_convert", "bzh_random_field", "bzh_batch_invert", "bzh_prefix_product", "bzh_eval_polynomial", "bzh_inner_product", "bzh_fold", "bzh_vec_mul"]
TIMER_NAMES[5] = "poly"
TIMER_NAMES[6] = "quotient"


def _as_elems(a):
    a = np.ascontiguousarray(a, dtype=np.uint64)
    assert a.shape[-1] == 4
    return a


def _ctx_batch_invert(self, field: int, data, form: int = FORM_CANONICAL) -> np.ndarray:
    a = _as_elems(data).copy()
    _bind_poly(load())
    self._check(load().bzh_batch_invert(self.handle, field, _vp(a), a.size // 4, form, MEM_HOST), "bzh_batch_invert")
    return a


def _ctx_prefix_product(self, field: int, data, form: int = FORM_CANONICAL) -> np.ndarray:
    a = _as_elems(data).copy()
    n = a.shape[-2]
    batch = a.size // 4 // n if n else 0
    _bind_poly(load())
    self._check(load().bzh_prefix_product(self.handle, field, _vp(a), n, batch, form, MEM_HOST), "bzh_prefix_product")
    return a


def _ctx_eval_polynomial(self, field: int, coeffs, xs, form: int = FORM_CANONICAL) -> np.ndarray:
    c = _as_elems(coeffs)
    if c.ndim == 2:
        c = c.reshape(1, *c.shape)
    x = _as_elems(xs).reshape(-1, 4)
    out = np.zeros((c.shape[0], 4), dtype=np.uint64)
    _bind_poly(load())
    rc = load().bzh_eval_polynomial(self.handle, field, _vp(c), c.shape[1], c.shape[0], _vp(x), x.shape[0], form, MEM_HOST, _vp(out))
    self._check(rc, "bzh_eval_polynomial")
    return out


def _ctx_inner_product(self, field: int, a, b, form: int = FORM_CANONICAL) -> np.ndarray:
    a, b = _as_elems(a), _as_elems(b)
    if a.ndim == 2:
        a, b = a.reshape(1, *a.shape), b.reshape(1, *b.shape)
    out = np.zeros((a.shape[0], 4), dtype=np.uint64)
    _bind_poly(load())
    rc = load().bzh_inner_product(self.handle, field, _vp(a), _vp(b), a.shape[1], a.shape[0], form, MEM_HOST, _vp(out))
    self._check(rc, "bzh_inner_product")
    return out


def _ctx_fold(self, field: int, v, u, form: int = FORM_CANONICAL) -> np.ndarray:
    v = _as_elems(v)
    if v.ndim == 2:
        v = v.reshape(1, *v.shape)
    u = _as_elems(u).reshape(-1, 4)
    half = v.shape[1] // 2
    out = np.zeros((v.shape[0], half, 4), dtype=np.uint64)
    _bind_poly(load())
    rc = load().bzh_fold(self.handle, field, _vp(v), half, v.shape[0], _vp(u), u.shape[0], form, MEM_HOST, _vp(out))
    self._check(rc, "bzh_fold")
    return out


def _ctx_vec_mul(self, field: int, a, b, form: int = FORM_CANONICAL) -> np.ndarray:
    a, b = _as_elems(a).copy(), _as_elems(b)
    _bind_poly(load())
    self._check(load().bzh_vec_mul(self.handle, field, _vp(a), _vp(b), a.size // 4, form, MEM_HOST), "bzh_vec_mul")
    return a


Context.batch_invert = _ctx_batch_invert
Context.prefix_product = _ctx_prefix_product
Context.eval_polynomial = _ctx_eval_polynomial
Context.inner_product = _ctx_inner_product
Context.fold = _ctx_fold
Context.vec_mul = _ctx_vec_mul


# ---- transcript (host) ---------------------------------------------------------------------------
EXPORTS += ["bzh_pk_quotient_select", "bzh_pk_quotient_selected", "bzh_quotient_source_for_circuit", "bzh_builtin_quotients",
            "bzh_quotient_degree_histogram", "bzh_pk_lookup_select", "bzh_pk_lookup_selected", "bzh_pk_quotient_loads",
            "bzh_quotient_program_for_circuit"]
EXPORTS += ["bzh_record_stride", "bzh_record_encode", "bzh_record_decode", "bzh_record_to_json", "bzh_record_from_json"]
EXPORTS += ["bzh_transcript_new", "bzh_transcript_free", "bzh_transcript_common_point", "bzh_transcript_common_scalar",
            "bzh_transcript_write_point", "bzh_transcript_write_scalar", "bzh_transcript_squeeze_challenge",
            "bzh_transcript_proof"]


class Transcript:
    """Blake2bWrite + Challenge255 (bzh_transcript_*); ints in, ints out."""

    def __init__(self, challenge_field: int = FIELD_FP):
        L = load()
        vp = ctypes.c_void_p
        L.bzh_transcript_new.argtypes = [ctypes.c_int, ctypes.POINTER(vp)]
        for f in ("bzh_transcript_free",):
            getattr(L, f).argtypes = [vp]
        for f in ("bzh_transcript_common_point", "bzh_transcript_common_scalar", "bzh_transcript_write_scalar",
                  "bzh_transcript_squeeze_challenge"):
            getattr(L, f).argtypes = [vp, ctypes.POINTER(ctypes.c_uint64)]
        L.bzh_transcript_write_point.argtypes = [vp, ctypes.c_int, ctypes.POINTER(ctypes.c_uint64)]
        L.bzh_transcript_proof.argtypes = [vp, ctypes.POINTER(ctypes.POINTER(ctypes.c_uint8)), ctypes.POINTER(ctypes.c_size_t)]
        self.h = vp()
        rc = L.bzh_transcript_new(challenge_field, ctypes.byref(self.h))
        if rc != OK:
            raise BzhError(rc, "bzh_transcript_new")

    @staticmethod
    def _pt(pt):
        x, y = (0, 0) if pt is None else pt
        return np.concatenate([int_to_limbs(x), int_to_limbs(y)])

    def common_point(self, pt):
        rc = load().bzh_transcript_common_point(self.h, _u64(self._pt(pt)))
        if rc != OK:
            raise BzhError(rc, "bzh_transcript_common_point")

    def common_scalar(self, s: int):
        rc = load().bzh_transcript_common_scalar(self.h, _u64(int_to_limbs(s)))
        if rc != OK:
            raise BzhError(rc, "bzh_transcript_common_scalar")

    def write_point(self, curve: int, pt):
        rc = load().bzh_transcript_write_point(self.h, curve, _u64(self._pt(pt)))
        if rc != OK:
            raise BzhError(rc, "bzh_transcript_write_point")

    def write_scalar(self, s: int):
        rc = load().bzh_transcript_write_scalar(self.h, _u64(int_to_limbs(s)))
        if rc != OK:
            raise BzhError(rc, "bzh_transcript_write_scalar")

    def squeeze_challenge(self) -> int:
        out = np.zeros(4, dtype=np.uint64)
        rc = load().bzh_transcript_squeeze_challenge(self.h, _u64(out))
        if rc != OK:
            raise BzhError(rc, "bzh_transcript_squeeze_challenge")
        return limbs_to_int(out)

    def proof(self) -> bytes:
        p = ctypes.POINTER(ctypes.c_uint8)()
        n = ctypes.c_size_t()
        load().bzh_transcript_proof(self.h, ctypes.byref(p), ctypes.byref(n))
        return bytes(ctypes.string_at(p, n.value)) if n.value else b""

    def close(self):
        if self.h is not None:
            load().bzh_transcript_free(self.h)
            self.h = None


# ---- batched transcripts (host-resident or on the device) ----------------------------------------
EXPORTS += ["bzh_transcript_batch_new", "bzh_transcript_batch_free", "bzh_transcript_batch_common_points",
            "bzh_transcript_batch_write_points", "bzh_transcript_batch_write_jacobian", "bzh_transcript_batch_common_scalars",
            "bzh_transcript_batch_write_scalars", "bzh_transcript_batch_squeeze", "bzh_transcript_batch_proofs",
            "bzh_transcript_batch_status", "bzh_transcript_batch_from_host", "bzh_transcript_batch_to_host"]


def _bind_transcript_batch():
    L = load()
    vp, sz, ci = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
    L.bzh_transcript_batch_new.argtypes = [vp, ci, sz, sz, ctypes.POINTER(vp)]
    L.bzh_transcript_batch_free.argtypes = [vp]
    for f in ("common_points", "write_points", "write_jacobian", "common_scalars", "write_scalars"):
        getattr(L, "bzh_transcript_batch_" + f).argtypes = [vp, vp, sz, sz, ci, ci]
    L.bzh_transcript_batch_squeeze.argtypes = [vp, ci, ci, vp]
    L.bzh_transcript_batch_proofs.argtypes = [vp, ci, vp, sz, ctypes.POINTER(sz)]
    L.bzh_transcript_batch_status.argtypes = [vp, vp]
    L.bzh_transcript_batch_from_host.argtypes = [vp, ctypes.POINTER(vp)]
    L.bzh_transcript_batch_to_host.argtypes = [vp, ctypes.POINTER(vp)]
    return L


class TranscriptBatch:
    """`batch` Blake2bWrite + Challenge255 transcripts in lockstep (bzh_transcript_batch_*): on ctx's device, or host-resident
    (ctx None, the same step code on the host).  `curve` fixes the fields: coordinates in its base field, scalars and challenges
    in its scalar field.  Every call gives every transcript the same number of items.
    MEM_HOST: operands are uint64 arrays of shape (batch, n, limbs) -- 8 limbs for an affine point, 12 for a Jacobian point, 4
    for a scalar --, in `form`; a canonical operand that is not below its modulus raises BzhError E_RANGE and absorbs nothing.
    MEM_DEVICE: operands are device pointers (ints, 16-byte aligned) with `n` items per transcript, transcript b reading the
    items b * stride + i (stride defaults to n); the call only enqueues on the ctx's stream."""
    ITEM_LIMBS = {"common_points": 8, "write_points": 8, "write_jacobian": 12, "common_scalars": 4, "write_scalars": 4}

    def __init__(self, curve: int, batch: int, proof_cap: int, ctx: "Context | None" = None):
        L = _bind_transcript_batch()
        self.ctx, self.curve, self.batch, self.proof_cap = ctx, curve, batch, proof_cap
        self.h = ctypes.c_void_p()
        rc = L.bzh_transcript_batch_new(ctx.handle if ctx is not None else None, curve, batch, proof_cap, ctypes.byref(self.h))
        if rc != OK:
            self.h = None
            raise BzhError(rc, "bzh_transcript_batch_new", self._detail())

    def _detail(self) -> str:
        return load().bzh_last_error(self.ctx.handle).decode() if self.ctx is not None and self.ctx.handle is not None else ""

    def _check(self, rc: int, where: str):
        if rc != OK:
            raise BzhError(rc, where, self._detail())

    def _absorb(self, op: str, data, form: int, mem: int, n, stride):
        fn = getattr(_bind_transcript_batch(), "bzh_transcript_batch_" + op)
        if mem == MEM_DEVICE:
            assert n is not None
            ptr = ctypes.c_void_p(int(data))
        else:
            a = np.ascontiguousarray(data, dtype=np.uint64).reshape(self.batch, -1, self.ITEM_LIMBS[op])
            n = a.shape[1]
            ptr = _vp(a)
        self._check(fn(self.h, ptr, n, n if stride is None else stride, form, mem), "bzh_transcript_batch_" + op)

    def common_points(self, xy, *, form: int = FORM_CANONICAL, mem: int = MEM_HOST, n: int | None = None, stride: int | None = None):
        self._absorb("common_points", xy, form, mem, n, stride)

    def write_points(self, xy, *, form: int = FORM_CANONICAL, mem: int = MEM_HOST, n: int | None = None, stride: int | None = None):
        self._absorb("write_points", xy, form, mem, n, stride)

    def write_jacobian(self, xyz, *, form: int = FORM_CANONICAL, mem: int = MEM_HOST, n: int | None = None, stride: int | None = None):
        self._absorb("write_jacobian", xyz, form, mem, n, stride)

    def common_scalars(self, s, *, form: int = FORM_CANONICAL, mem: int = MEM_HOST, n: int | None = None, stride: int | None = None):
        self._absorb("common_scalars", s, form, mem, n, stride)

    def write_scalars(self, s, *, form: int = FORM_CANONICAL, mem: int = MEM_HOST, n: int | None = None, stride: int | None = None):
        self._absorb("write_scalars", s, form, mem, n, stride)

    def squeeze(self, *, form: int = FORM_CANONICAL, mem: int = MEM_HOST, out: int | None = None):
        """one challenge per transcript: a (batch, 4) uint64 array in `form`, or, with MEM_DEVICE, into the device pointer `out`
        (batch x 4 limbs; enqueues only, returns None)"""
        L = _bind_transcript_batch()
        if mem == MEM_DEVICE:
            self._check(L.bzh_transcript_batch_squeeze(self.h, form, mem, ctypes.c_void_p(out) if out else None), "bzh_transcript_batch_squeeze")
            return None
        a = np.zeros((self.batch, 4), dtype=np.uint64)
        self._check(L.bzh_transcript_batch_squeeze(self.h, form, mem, _vp(a)), "bzh_transcript_batch_squeeze")
        return a

    def proof_len(self) -> int:
        n = ctypes.c_size_t()
        self._check(_bind_transcript_batch().bzh_transcript_batch_proofs(self.h, MEM_HOST, None, 0, ctypes.byref(n)), "bzh_transcript_batch_proofs")
        return n.value

    def proofs(self, *, mem: int = MEM_HOST, out: int | None = None, out_stride: int | None = None):
        """the proof bytes written so far: a list of `batch` byte strings, or, with MEM_DEVICE, into rows of out_stride bytes at
        the device pointer `out` (enqueues only; returns the length of each)"""
        L = _bind_transcript_batch()
        n = self.proof_len()
        if mem == MEM_DEVICE:
            self._check(L.bzh_transcript_batch_proofs(self.h, mem, ctypes.c_void_p(out) if out else None, n if out_stride is None else out_stride,
                                                      None), "bzh_transcript_batch_proofs")
            return n
        a = np.zeros((self.batch, max(n, 1)), dtype=np.uint8)
        self._check(L.bzh_transcript_batch_proofs(self.h, mem, _vp(a), a.shape[1], None), "bzh_transcript_batch_proofs")
        return [a[b, :n].tobytes() for b in range(self.batch)]

    def status(self) -> np.ndarray:
        """(batch,) uint8: the largest POINT_* status each transcript has seen; waits for the stream"""
        st = np.zeros(self.batch, dtype=np.uint8)
        self._check(_bind_transcript_batch().bzh_transcript_batch_status(self.h, _vp(st)), "bzh_transcript_batch_status")
        return st

    def _handles(self, transcripts):
        assert len(transcripts) == self.batch
        return (ctypes.c_void_p * self.batch)(*[t.h for t in transcripts])

    def from_host(self, transcripts):
        """take over the state and proof bytes of `batch` Transcript objects (bzh_transcript_batch_from_host)"""
        self._check(_bind_transcript_batch().bzh_transcript_batch_from_host(self.h, self._handles(transcripts)), "bzh_transcript_batch_from_host")

    def to_host(self, transcripts):
        """overwrite the state and proof bytes of `batch` Transcript objects (bzh_transcript_batch_to_host)"""
        self._check(_bind_transcript_batch().bzh_transcript_batch_to_host(self.h, self._handles(transcripts)), "bzh_transcript_batch_to_host")

    def ipa_open(self, bases: "Bases", polys, blinds, x3s, rng, *, form: int = FORM_CANONICAL, mem: int = MEM_HOST, out_v=None,
                 status=None, rng_stride: int | None = None, batch: int | None = None):
        """`batch` openings against this device-resident batch (bzh_ipa_open_batch_device): S, (L_j, R_j)*, c, f go into the
        transcripts, byte for byte what Context.ipa_open_batch writes into host transcripts.
        MEM_HOST: polys (batch, n, 4) uint64 in `form`; blinds, x3s: (batch, 4) uint64 in `form`, or lists of ints; rng: one byte
        string of 64 * (n + 1 + 2k) draws per proof.  Returns (v, status): (batch, 4) uint64 in `form` and (batch,) uint8 -- nonzero
        where a round challenge was zero.
        MEM_DEVICE: every operand is a device pointer (int, 16-byte aligned; `status` any alignment, or None), the draws of proof b
        at rng + b * rng_stride; out_v is required.  Enqueues only, returns None.
        The number of openings is the number of rng strings (MEM_HOST) or `batch` (MEM_DEVICE, default: this batch's size); the
        library refuses one that is not this batch's size."""
        L = load()
        vp, sz, ci = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
        L.bzh_ipa_open_batch_device.argtypes = [vp, vp, vp, ci, ci, sz, vp, vp, vp, sz, vp, vp, vp]
        ctxh = self.ctx.handle if self.ctx is not None else None
        bh = bases.handle if bases is not None else None
        where = "bzh_ipa_open_batch_device"
        if mem == MEM_DEVICE:
            ptr = lambda v: ctypes.c_void_p(int(v)) if v else None  # noqa: E731
            self._check(L.bzh_ipa_open_batch_device(ctxh, bh, ptr(polys), form, mem, self.batch if batch is None else batch, ptr(blinds),
                                                    ptr(x3s), ptr(rng), rng_stride or 0, self.h, ptr(out_v), ptr(status)), where)
            return None
        B = len(rng)

        def limbs(v):
            if isinstance(v, np.ndarray):
                return np.ascontiguousarray(v, dtype=np.uint64).reshape(B, 4)
            return np.ascontiguousarray(np.stack([int_to_limbs(x) for x in v]))

        p = np.ascontiguousarray(np.asarray(polys, dtype=np.uint64).reshape(B, -1, 4))
        bl, xs = limbs(blinds), limbs(x3s)
        stride = len(rng[0])
        assert all(len(r) == stride for r in rng)
        raw = np.frombuffer(b"".join(rng), dtype=np.uint8)
        v = np.zeros((B, 4), dtype=np.uint64)
        st = np.zeros(B, dtype=np.uint8)
        self._check(L.bzh_ipa_open_batch_device(ctxh, bh, _vp(p), form, mem, B, _vp(bl), _vp(xs), _vp(raw), stride, self.h, _vp(v), _vp(st)),
                    where)
        return v, st

    def multiopen(self, bases: "Bases", k: int, polys, blinds, points, queries, rng_list, *, shared=None, shared_blinds=None,
                  form: int = FORM_CANONICAL, mem: int = MEM_HOST, status=None, rng_stride: int | None = None, batch: int | None = None,
                  npolys_own: int | None = None, npolys_shared: int = 0, npoints: int | None = None):
        """the multiopen argument of `batch` proofs against this device-resident batch (bzh_multiopen_batch_device): x1, x2, the
        commitment of f, x3, every q_s(x3), x4 and the opening of p at x3 go through the transcripts, with no host trip in between.
        queries: (poly, point number) pairs; ids below the number of own polynomials are a proof's own, the rest `shared`.
        MEM_HOST: polys (batch, npolys_own, n, 4) uint64 in `form`; blinds (batch, npolys_own, 4); points (batch, npoints, 4);
        shared (npolys_shared, n, 4) and shared_blinds (npolys_shared, 4) or None; rng_list: one byte string of
        64 * (n + 2 + 2k) draws per proof.  Returns the status bytes, (batch,) uint8: bit 0 -- two points of a set coincide in
        that proof, bit 1 -- a zero round challenge in the opening.
        MEM_DEVICE: every operand is a device pointer (int, 16-byte aligned; `status` any alignment, or None), rng_list the pointer
        to the draws (proof b at + b * rng_stride); npolys_own and npoints are required, npolys_shared defaults to 0.  Enqueues
        only, returns None."""
        L = load()
        vp, sz, ci = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
        L.bzh_multiopen_batch_device.argtypes = [vp, vp, sz, ctypes.c_uint, vp, sz, vp, sz, vp, vp, vp, sz, vp, sz, ci, ci, vp, sz, vp, vp]
        ctxh = self.ctx.handle if self.ctx is not None else None
        bh = bases.handle if bases is not None else None
        where = "bzh_multiopen_batch_device"
        q = _query_array(queries)
        if mem == MEM_DEVICE:
            ptr = lambda v: ctypes.c_void_p(int(v)) if v else None  # noqa: E731
            self._check(L.bzh_multiopen_batch_device(ctxh, bh, self.batch if batch is None else batch, k, ptr(polys), npolys_own or 0,
                                                     ptr(shared), npolys_shared, ptr(blinds), ptr(shared_blinds), ptr(points), npoints or 0,
                                                     _vp(q), len(q), form, mem, ptr(rng_list), rng_stride or 0, self.h, ptr(status)), where)
            return None
        B, n = len(rng_list), 1 << k
        p = np.ascontiguousarray(np.asarray(polys, dtype=np.uint64).reshape(B, -1, n, 4))
        own = p.shape[1]
        bl = np.ascontiguousarray(np.asarray(blinds, dtype=np.uint64).reshape(B, own, 4))
        pt = np.ascontiguousarray(np.asarray(points, dtype=np.uint64).reshape(B, -1, 4))
        sh = sb = None
        nsh = 0
        if shared is not None:
            sh = np.ascontiguousarray(np.asarray(shared, dtype=np.uint64).reshape(-1, n, 4))
            nsh = sh.shape[0]
            sb = np.ascontiguousarray(np.asarray(shared_blinds, dtype=np.uint64).reshape(nsh, 4))
        stride = len(rng_list[0])
        assert all(len(r) == stride for r in rng_list)
        raw = np.frombuffer(b"".join(rng_list), dtype=np.uint8)
        st = np.zeros(B, dtype=np.uint8)
        self._check(L.bzh_multiopen_batch_device(ctxh, bh, B, k, _vp(p), own, _vp(sh) if nsh else None, nsh, _vp(bl), _vp(sb) if nsh else None,
                                                 _vp(pt), pt.shape[1], _vp(q), len(q), form, mem, _vp(raw), stride, self.h, _vp(st)), where)
        return st

    def evaluations(self, k: int, polys, queries, *, shared=None, h_pieces=None, h_blinds=None, npieces: int = 0, h_stride: int | None = None,
                    form: int = FORM_CANONICAL, mem: int = MEM_HOST, out_points=None, out_evals=None, out_h=None, out_h_blind=None,
                    batch: int | None = None, npolys_own: int | None = None, npolys_shared: int = 0):
        """the evaluation phase of `batch` proofs against this device-resident batch (bzh_evaluations_batch_device): x is squeezed,
        every query's value poly(x * omega^rotation) written in the order given, and h(X) = sum_i x^(n i) piece_i built, with no
        host trip in between.  queries: (poly, rotation) pairs; ids below the number of own polynomials are a proof's own, the
        rest `shared`.  The outputs chain into multiopen(): points is its `points` operand, h and h_blind one more own polynomial.
        MEM_HOST: polys (batch, npolys_own, n, 4) uint64 in `form`; shared (npolys_shared, n, 4) or None; with npieces > 0,
        h_pieces (batch, h_stride, 4) -- piece i of a proof at elements [i * n, (i + 1) * n) of its row, h_stride >= npieces * n --
        and h_blinds (batch, npieces, 4).  Returns (points, evals, h, h_blind): (batch, nrotations, 4), (batch, nqueries, 4),
        (batch, n, 4) and (batch, 4) uint64 in `form`, the rotations numbered as evaluations_plan numbers them; h and h_blind are
        None without pieces.
        MEM_DEVICE: every operand and output is a device pointer (int, 16-byte aligned); npolys_own is required, and so are
        h_stride and the two h outputs with npieces > 0; out_evals may be None.  Enqueues only, returns None."""
        L = load()
        vp, sz, ci = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
        L.bzh_evaluations_batch_device.argtypes = [vp, sz, ctypes.c_uint, vp, sz, vp, sz, vp, sz, vp, sz, sz, vp, ci, ci, vp, vp, vp, vp, vp]
        ctxh = self.ctx.handle if self.ctx is not None else None
        where = "bzh_evaluations_batch_device"
        q = _eval_query_array(queries)
        if mem == MEM_DEVICE:
            ptr = lambda v: ctypes.c_void_p(int(v)) if v else None  # noqa: E731
            self._check(L.bzh_evaluations_batch_device(ctxh, self.batch if batch is None else batch, k, ptr(polys), npolys_own or 0, ptr(shared),
                                                       npolys_shared, _vp(q), len(q), ptr(h_pieces), npieces, h_stride or 0, ptr(h_blinds), form,
                                                       mem, self.h, ptr(out_points), ptr(out_evals), ptr(out_h), ptr(out_h_blind)), where)
            return None
        n = 1 << k
        p = np.ascontiguousarray(np.asarray(polys, dtype=np.uint64))
        B = p.shape[0]
        p = p.reshape(B, -1, n, 4)
        sh, nsh = None, 0
        if shared is not None:
            sh = np.ascontiguousarray(np.asarray(shared, dtype=np.uint64).reshape(-1, n, 4))
            nsh = sh.shape[0]
        hp = hb = h = hbl = None
        stride = 0
        if npieces:
            hp = np.ascontiguousarray(np.asarray(h_pieces, dtype=np.uint64).reshape(B, -1, 4))
            stride = hp.shape[1] if h_stride is None else h_stride
            hb = np.ascontiguousarray(np.asarray(h_blinds, dtype=np.uint64).reshape(B, npieces, 4))
            h, hbl = np.zeros((B, n, 4), dtype=np.uint64), np.zeros((B, 4), dtype=np.uint64)
        nrot = len({int(r) for r in q["rotation"]})
        pts, ev = np.zeros((B, max(nrot, 1), 4), dtype=np.uint64), np.zeros((B, max(len(q), 1), 4), dtype=np.uint64)
        opt = lambda a: _vp(a) if a is not None else None  # noqa: E731
        self._check(L.bzh_evaluations_batch_device(ctxh, B, k, _vp(p), p.shape[1], opt(sh), nsh, _vp(q), len(q), opt(hp), npieces, stride, opt(hb),
                                                   form, mem, self.h, _vp(pts), _vp(ev), opt(h), opt(hbl)), where)
        return pts[:, :nrot], ev[:, :len(q)], h, hbl

    def vanishing(self, pk, advice_polys, instance_polys, lookup_polys, z_polys, theta, beta, gamma, rng_list, *, form: int = FORM_CANONICAL,
                  mem: int = MEM_HOST, out_random=None, out_random_blind=None, out_h=None, out_h_blinds=None, status=None,
                  rng_stride: int | None = None, batch: int | None = None, shape=None):
        """the vanishing argument of `batch` proofs against this device-resident batch (bzh_vanishing_batch_device): the commitment
        of the random polynomial is written, y squeezed, the quotient evaluated in the flavour `pk` (a NativeProvingKey) has
        selected, and the commitments of its pieces written, with no host trip in between.  The outputs chain into evaluations():
        h is its h_pieces with h_stride = the extended size, h_blinds its h_blinds, random one more own polynomial.
        MEM_HOST: advice_polys (batch, num_advice, n, 4), instance_polys (batch, num_instance, n, 4), lookup_polys
        (batch, lookups, 2, n, 4) and z_polys (batch, nz, n, 4) uint64 coefficients in `form` (None where the count is 0); theta,
        beta, gamma (batch, 4); rng_list: one byte string of 64 * (n + 1 + npieces) draws per proof.  Returns (random,
        random_blind, h, h_blinds, status): (batch, n, 4), (batch, 4), (batch, en, 4), (batch, npieces, 4) uint64 in `form` and
        (batch,) uint8 -- bit 0: a quotient coefficient at or above npieces * n is non-zero.  `shape`: the first element of
        vanishing_plan(), which sizes the outputs; None: pk.vanishing_plan()[0], computed for this call.
        MEM_DEVICE: every operand and output is a device pointer (int, 16-byte aligned; `status` any alignment, or None),
        rng_list the pointer to the draws (proof b at + b * rng_stride).  Enqueues only, returns None."""
        L = load()
        vp, sz, ci = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
        L.bzh_vanishing_batch_device.argtypes = [vp, vp, sz, vp, vp, vp, vp, vp, vp, vp, ci, ci, vp, sz, vp, vp, vp, vp, vp, vp]
        ctxh = self.ctx.handle if self.ctx is not None else None
        pkh = pk.handle if hasattr(pk, "handle") else pk
        where = "bzh_vanishing_batch_device"
        if mem == MEM_DEVICE:
            ptr = lambda v: ctypes.c_void_p(int(v)) if v else None  # noqa: E731
            self._check(L.bzh_vanishing_batch_device(ctxh, pkh, self.batch if batch is None else batch, ptr(advice_polys), ptr(instance_polys),
                                                     ptr(lookup_polys), ptr(z_polys), ptr(theta), ptr(beta), ptr(gamma), form, mem, ptr(rng_list),
                                                     rng_stride or 0, self.h, ptr(out_random), ptr(out_random_blind), ptr(out_h),
                                                     ptr(out_h_blinds), ptr(status)), where)
            return None
        B = len(rng_list)
        if shape is None:
            if not hasattr(pk, "vanishing_plan"):
                raise TypeError("TranscriptBatch.vanishing: `shape` is required when pk is a bare handle")
            shape = pk.vanishing_plan()[0]
        n, en, _, _, _, _, npieces, _ = shape
        arr = lambda a: None if a is None else np.ascontiguousarray(np.asarray(a, dtype=np.uint64))  # noqa: E731
        opt = lambda a: _vp(a) if a is not None and a.size else None  # noqa: E731
        ops = [arr(a) for a in (advice_polys, instance_polys, lookup_polys, z_polys, theta, beta, gamma)]
        stride = len(rng_list[0])
        assert all(len(r) == stride for r in rng_list)
        raw = np.frombuffer(b"".join(rng_list), dtype=np.uint8)
        rp, rb = np.zeros((B, n, 4), dtype=np.uint64), np.zeros((B, 4), dtype=np.uint64)
        h, hb = np.zeros((B, en, 4), dtype=np.uint64), np.zeros((B, npieces, 4), dtype=np.uint64)
        st = np.zeros(B, dtype=np.uint8)
        self._check(L.bzh_vanishing_batch_device(ctxh, pkh, B, *[opt(a) for a in ops], form, mem, _vp(raw), stride, self.h, _vp(rp), _vp(rb),
                                                 _vp(h), _vp(hb), _vp(st)), where)
        return rp, rb, h, hb, st

    def grand_products(self, pk, advice, instance, lookup_compressed, lookup_permuted, beta, gamma, rng_list, *, form: int = FORM_CANONICAL,
                       mem: int = MEM_HOST, out_z=None, out_z_polys=None, out_z_blinds=None, status=None, rng_stride: int | None = None,
                       batch: int | None = None, shape=None, want_z: bool = True):
        """the permutation and lookup grand products of `batch` proofs against this device-resident batch
        (bzh_grand_products_batch_device): every product is built from beta and gamma where they lie, and its commitment written,
        with no host trip in between.  The outputs chain into vanishing(): z_polys is its z_polys operand.
        MEM_HOST: advice (batch, num_advice, n, 4) and instance (batch, num_instance, n, 4) uint64 evaluations over the domain in
        `form`, blinding rows in place; lookup_compressed and lookup_permuted (batch, lookups, 2, n, 4) (None where the count is
        0); beta, gamma (batch, 4); rng_list: one byte string of 64 * nz * (bf + 1) draws per proof.  Returns (z, z_polys,
        z_blinds, status): (batch, nz, n, 4) twice (z is None with want_z false) and (batch, nz, 4) uint64 in `form`, and
        (batch,) uint8 -- 1: a product of that proof does not close.  `shape`: grand_products_plan(), which sizes the outputs;
        None: pk.grand_products_plan(), computed for this call.
        MEM_DEVICE: every operand and output is a device pointer (int, 16-byte aligned; `status` any alignment, or None; out_z may
        be None), rng_list the pointer to the draws (proof b at + b * rng_stride).  Enqueues only, returns None."""
        L = load()
        vp, sz, ci = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
        L.bzh_grand_products_batch_device.argtypes = [vp, vp, sz, vp, vp, vp, vp, vp, vp, ci, ci, vp, sz, vp, vp, vp, vp, vp]
        ctxh = self.ctx.handle if self.ctx is not None else None
        pkh = pk.handle if hasattr(pk, "handle") else pk
        where = "bzh_grand_products_batch_device"
        if mem == MEM_DEVICE:
            ptr = lambda v: ctypes.c_void_p(int(v)) if v else None  # noqa: E731
            self._check(L.bzh_grand_products_batch_device(ctxh, pkh, self.batch if batch is None else batch, ptr(advice), ptr(instance),
                                                          ptr(lookup_compressed), ptr(lookup_permuted), ptr(beta), ptr(gamma), form, mem,
                                                          ptr(rng_list), rng_stride or 0, self.h, ptr(out_z), ptr(out_z_polys),
                                                          ptr(out_z_blinds), ptr(status)), where)
            return None
        B = len(rng_list)
        if shape is None:
            if not hasattr(pk, "grand_products_plan"):
                raise TypeError("TranscriptBatch.grand_products: `shape` is required when pk is a bare handle")
            shape = pk.grand_products_plan()
        n, nz = shape[0], shape[5]
        arr = lambda a: None if a is None else np.ascontiguousarray(np.asarray(a, dtype=np.uint64))  # noqa: E731
        opt = lambda a: _vp(a) if a is not None and a.size else None  # noqa: E731
        ops = [arr(a) for a in (advice, instance, lookup_compressed, lookup_permuted, beta, gamma)]
        stride = len(rng_list[0])
        assert all(len(r) == stride for r in rng_list)
        raw = np.frombuffer(b"".join(rng_list), dtype=np.uint8)
        z = np.zeros((B, nz, n, 4), dtype=np.uint64) if want_z else None
        zp, zb = np.zeros((B, nz, n, 4), dtype=np.uint64), np.zeros((B, nz, 4), dtype=np.uint64)
        st = np.zeros(B, dtype=np.uint8)
        self._check(L.bzh_grand_products_batch_device(ctxh, pkh, B, *[opt(a) for a in ops], form, mem, _vp(raw), stride, self.h,
                                                      _vp(z) if want_z else None, _vp(zp), _vp(zb), _vp(st)), where)
        return z, zp, zb, st

    COMMITMENTS_OUT = ("advice", "instance", "lookup_compressed", "lookup_permuted", "advice_polys", "instance_polys", "lookup_polys",
                       "advice_blinds", "lookup_blinds", "theta", "beta", "gamma")

    def commitments(self, pk, advice, instances, rng_list, *, form: int = FORM_CANONICAL, mem: int = MEM_HOST, out=None, status=None,
                    instance_rows: int | None = None, rng_stride: int | None = None, batch: int | None = None, shape=None):
        """the witness commitments of `batch` proofs against this device-resident batch (bzh_commitments_batch_device): the instance
        commitments are absorbed, the advice commitments written, theta squeezed, the lookups compressed with theta where it lies,
        permuted and committed, beta and gamma squeezed, with no host trip in between.  The key's vk_repr is not absorbed here:
        common_scalars it first.  The outputs chain into grand_products() and vanishing().
        MEM_HOST: advice (batch, num_advice, n, 4) and instances (batch, num_instance, instance_rows, 4) uint64 in `form` (None
        where the count is 0); rng_list: one byte string of 64 * nd draws per proof.  Returns (outputs, status): a dict of uint64
        arrays in `form` by the names of COMMITMENTS_OUT -- advice (batch, na, n, 4), instance (batch, ni, n, 4),
        lookup_compressed, lookup_permuted and lookup_polys (batch, nl, 2, n, 4), advice_polys, instance_polys, advice_blinds
        (batch, na, 4), lookup_blinds (batch, nl, 2, 4), theta, beta, gamma (batch, 4) -- and (batch,) uint8 -- bit 0: a lookup
        input of that proof is not in its table.  `shape`: commitments_plan(), which sizes the outputs; None:
        pk.commitments_plan(), computed for this call.
        MEM_DEVICE: advice, instances and rng_list are device pointers (ints, 16-byte aligned; proof b's draws at + b *
        rng_stride), `out` a dict of device pointers by the names of COMMITMENTS_OUT (a missing name is NULL), `status` a device
        pointer of any alignment or None, instance_rows the rows per instance column.  Enqueues only, returns None."""
        L = load()
        vp, sz, ci = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
        L.bzh_commitments_batch_device.argtypes = [vp, vp, sz, vp, vp, sz, ci, ci, vp, sz, vp, vp, vp]
        ctxh = self.ctx.handle if self.ctx is not None else None
        pkh = pk.handle if hasattr(pk, "handle") else pk
        where = "bzh_commitments_batch_device"
        if mem == MEM_DEVICE:
            ptr = lambda v: ctypes.c_void_p(int(v)) if v else None  # noqa: E731
            o = (ctypes.c_void_p * 12)(*[ptr((out or {}).get(name)) for name in self.COMMITMENTS_OUT])
            self._check(L.bzh_commitments_batch_device(ctxh, pkh, self.batch if batch is None else batch, ptr(advice), ptr(instances),
                                                       instance_rows or 0, form, mem, ptr(rng_list), rng_stride or 0, self.h,
                                                       ctypes.cast(o, vp) if out is not None else None, ptr(status)), where)
            return None
        B = len(rng_list)
        if shape is None:
            if not hasattr(pk, "commitments_plan"):
                raise TypeError("TranscriptBatch.commitments: `shape` is required when pk is a bare handle")
            shape = pk.commitments_plan()
        n, _, _, na, ni, nl = shape[:6]
        arr = lambda a: None if a is None else np.ascontiguousarray(np.asarray(a, dtype=np.uint64))  # noqa: E731
        opt = lambda a: _vp(a) if a is not None and a.size else None  # noqa: E731
        adv, inst = arr(advice), arr(instances)
        if instance_rows is None:
            instance_rows = inst.reshape(B, ni, -1, 4).shape[2] if inst is not None and inst.size else 0
        stride = len(rng_list[0])
        assert all(len(r) == stride for r in rng_list)
        raw = np.frombuffer(b"".join(rng_list), dtype=np.uint8)
        dims = {"advice": (na, n), "instance": (ni, n), "lookup_compressed": (nl, 2, n), "lookup_permuted": (nl, 2, n), "advice_polys": (na, n),
                "instance_polys": (ni, n), "lookup_polys": (nl, 2, n), "advice_blinds": (na,), "lookup_blinds": (nl, 2), "theta": (), "beta": (),
                "gamma": ()}
        res = {name: np.zeros((B,) + dims[name] + (4,), dtype=np.uint64) for name in self.COMMITMENTS_OUT}
        o = (ctypes.c_void_p * 12)(*[opt(res[name]) for name in self.COMMITMENTS_OUT])
        st = np.zeros(B, dtype=np.uint8)
        self._check(L.bzh_commitments_batch_device(ctxh, pkh, B, opt(adv), opt(inst), instance_rows, form, mem, _vp(raw), stride, self.h,
                                                   ctypes.cast(o, vp), _vp(st)), where)
        return res, st

    def close(self):
        if self.h is not None:
            load().bzh_transcript_batch_free(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


# ---- IPA opening --------------------------------------------------------------------------------
EXPORTS += ["bzh_ipa_open", "bzh_ipa_open_batch", "bzh_ipa_open_batch_device", "bzh_ipa_verify"]
EXPORTS += ["bzh_multiopen_plan", "bzh_multiopen_batch_device"]
MULTIOPEN_MAX_POINTS = 8


def _query_array(queries) -> np.ndarray:
    """(poly, point number) pairs as the bzh_open_query array the library reads"""
    return np.ascontiguousarray(np.asarray(list(queries), dtype=np.uint32).reshape(-1, 2))


def multiopen_plan(queries, npolys: int, npoints: int):
    """upstream's construct_intermediate_sets on (poly, point number) pairs (bzh_multiopen_plan, host only): returns
    (point_sets, groups, set_of_poly) -- point_sets[s]: the point numbers of set s, ascending; groups[s]: its polynomials in
    first-seen order; set_of_poly[p]: the set of polynomial p, or None if it is never queried."""
    L = load()
    vp, sz = ctypes.c_void_p, ctypes.c_size_t
    L.bzh_multiopen_plan.argtypes = [vp, sz, sz, sz, vp, vp, vp, vp, ctypes.POINTER(sz)]
    q = _query_array(queries)
    room = max(npolys, 1)
    set_of, order, sizes = (np.zeros(room, dtype=np.uint32) for _ in range(3))
    pts = np.zeros((room, MULTIOPEN_MAX_POINTS), dtype=np.uint32)
    nsets = sz(0)
    rc = L.bzh_multiopen_plan(_vp(q), len(q), npolys, npoints, _vp(set_of), _vp(order), _vp(sizes), _vp(pts), ctypes.byref(nsets))
    if rc != OK:
        raise BzhError(rc, "bzh_multiopen_plan")
    ns = nsets.value
    point_sets = [[int(x) for x in pts[s, :sizes[s]]] for s in range(ns)]
    groups = [[] for _ in range(ns)]
    for pid in order[:npolys]:
        if pid != 0xffffffff:
            groups[int(set_of[pid])].append(int(pid))
    return point_sets, groups, [None if x == 0xffffffff else int(x) for x in set_of[:npolys]]


EXPORTS += ["bzh_evaluations_plan", "bzh_evaluations_batch_device"]
EVAL_MAX_ROTATIONS = 8
_EVAL_QUERY = np.dtype([("poly", np.uint32), ("rotation", np.int32)])


def _eval_query_array(queries) -> np.ndarray:
    """(poly, rotation) pairs as the bzh_eval_query array the library reads"""
    return np.array([(int(p), int(r)) for p, r in queries], dtype=_EVAL_QUERY)


def evaluations_plan(queries, npolys: int):
    """what the evaluation phase derives from its (poly, rotation) queries (bzh_evaluations_plan, host only): returns
    (rotations, point_of_query, poly_order, rot_count) -- the distinct rotations in first-seen order; per query the index of its
    rotation in that list; the queried polynomials in first-seen order; per polynomial id the number of its distinct rotations
    (0: never queried)."""
    L = load()
    vp, sz = ctypes.c_void_p, ctypes.c_size_t
    L.bzh_evaluations_plan.argtypes = [vp, sz, sz, vp, ctypes.POINTER(sz), vp, vp, vp]
    q = _eval_query_array(queries)
    rots = np.zeros(max(len(q), 1), dtype=np.int32)
    point = np.zeros(max(len(q), 1), dtype=np.uint32)
    order, count = (np.zeros(max(npolys, 1), dtype=np.uint32) for _ in range(2))
    nrot = sz(0)
    rc = L.bzh_evaluations_plan(_vp(q), len(q), npolys, _vp(rots), ctypes.byref(nrot), _vp(point), _vp(order), _vp(count))
    if rc != OK:
        raise BzhError(rc, "bzh_evaluations_plan")
    return ([int(r) for r in rots[:nrot.value]], [int(j) for j in point[:len(q)]], [int(i) for i in order[:npolys] if i != 0xffffffff],
            [int(c) for c in count[:npolys]])


EXPORTS += ["bzh_vanishing_plan", "bzh_vanishing_batch_device"]
_VANISHING_CONST = np.dtype([("challenge", np.int32), ("exponent", np.uint32), ("value", np.uint32, 8)])


def vanishing_plan(curve: int, circuit_blob: bytes):
    """what the vanishing argument derives from a circuit (bzh_vanishing_plan, host only): returns (shape, consts) -- shape:
    (n, extended size, num_advice, num_instance, nz, lookups, npieces, draws per proof); consts: one (challenge, exponent, value)
    per entry of the quotient program's constant table, challenge -1 for a literal, else 0 .. 3 for theta, beta, gamma, y, the
    entry meaning value * challenge^exponent, value a Montgomery-form int."""
    L = load()
    vp, sz = ctypes.c_void_p, ctypes.c_size_t
    L.bzh_vanishing_plan.argtypes = [ctypes.c_int, ctypes.c_char_p, sz, vp, vp, sz, ctypes.POINTER(sz)]
    L.bzh_quotient_program_for_circuit.argtypes = [ctypes.c_int, ctypes.c_char_p, sz, vp, sz, ctypes.POINTER(sz), vp, sz, ctypes.POINTER(sz),
                                                   ctypes.POINTER(ctypes.c_uint32)]
    blob = bytes(circuit_blob)
    nops, nc = sz(0), sz(0)
    rc = L.bzh_quotient_program_for_circuit(curve, blob, len(blob), None, 0, ctypes.byref(nops), None, 0, ctypes.byref(nc), None)
    if rc != OK:
        raise BzhError(rc, "bzh_vanishing_plan")
    shape = np.zeros(8, dtype=np.uint32)
    consts = np.zeros(max(nc.value, 1), dtype=_VANISHING_CONST)
    got = sz(0)
    rc = L.bzh_vanishing_plan(curve, blob, len(blob), _vp(shape), _vp(consts), nc.value, ctypes.byref(got))
    if rc != OK:
        raise BzhError(rc, "bzh_vanishing_plan")
    value = lambda w: sum(int(x) << (32 * i) for i, x in enumerate(w))  # noqa: E731
    return tuple(int(x) for x in shape), [(int(c["challenge"]), int(c["exponent"]), value(c["value"])) for c in consts[:got.value]]


EXPORTS += ["bzh_grand_products_plan", "bzh_grand_products_batch_device"]


def grand_products_plan(curve: int, circuit_blob: bytes):
    """what the grand products derive from a circuit (bzh_grand_products_plan, host only): (n, usable rows, blinding factors,
    permutation sets, lookups, nz = sets + lookups, columns per set, draws per proof = nz * (blinding factors + 1))"""
    L = load()
    L.bzh_grand_products_plan.argtypes = [ctypes.c_int, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_void_p]
    blob = bytes(circuit_blob)
    shape = np.zeros(8, dtype=np.uint32)
    rc = L.bzh_grand_products_plan(curve, blob, len(blob), _vp(shape))
    if rc != OK:
        raise BzhError(rc, "bzh_grand_products_plan")
    return tuple(int(x) for x in shape)


EXPORTS += ["bzh_commitments_plan", "bzh_commitments_batch_device"]


def commitments_plan(curve: int, circuit_blob: bytes):
    """what the witness commitments derive from a circuit (bzh_commitments_plan, host only): (n, usable rows, blinding factors bf,
    num_advice na, num_instance ni, lookups nl, draws per proof = na * (bf + 1) + na + nl * (2 * (bf + 1) + 2), proof bytes
    appended = 32 * (na + 2 * nl))"""
    L = load()
    L.bzh_commitments_plan.argtypes = [ctypes.c_int, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_void_p]
    blob = bytes(circuit_blob)
    shape = np.zeros(8, dtype=np.uint32)
    rc = L.bzh_commitments_plan(curve, blob, len(blob), _vp(shape))
    if rc != OK:
        raise BzhError(rc, "bzh_commitments_plan")
    return tuple(int(x) for x in shape)


EXPORTS += ["bzh_prove_device_plan", "bzh_prove_batch_device", "bzh_prove_batch_device_seeded"]


def prove_device_plan(curve: int, circuit_blob: bytes):
    """(commitments draws, grand-products draws, vanishing draws, multiopen draws, their sum = rng_bytes / 64, proof bytes, nown, largest
    batch) of bzh_prove_batch_device for a circuit blob (host only): the draws per proof of the four drawing leaves in chain order,
    the polynomials of a proof that get opened, and 65535 // max(na, ni, 2 nl, nz, npieces)"""
    L = load()
    L.bzh_prove_device_plan.argtypes = [ctypes.c_int, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_void_p]
    shape = np.zeros(8, dtype=np.uint32)
    rc = L.bzh_prove_device_plan(curve, circuit_blob, len(circuit_blob), ctypes.c_void_p(shape.ctypes.data))
    if rc:
        raise BzhError(rc, "bzh_prove_device_plan")
    return tuple(int(v) for v in shape)


EXPORTS += ["bzh_pk_create", "bzh_pk_free", "bzh_pk_set_lagrange", "bzh_pk_quotient_stats", "bzh_pk_quotient_source", "bzh_pk_set_quotient_module", "bzh_pk_info", "bzh_prove_batch", "bzh_prove_batch_seeded", "bzh_rng_expand", "bzh_verify_batch",
            "bzh_vk_digest", "bzh_pk_vk_repr"]
EXPORTS += ["bzh_vk_create", "bzh_vk_from_pk", "bzh_vk_write", "bzh_vk_read", "bzh_vk_info", "bzh_vk_vk_repr", "bzh_vk_device_bytes",
            "bzh_pk_device_bytes", "bzh_vk_free", "bzh_verify_batch_vk"]
EXPORTS += ["bzh_pk_verify_pass_select", "bzh_pk_verify_pass_selected", "bzh_verify_batch_vk_with"]
# Params::new (bzh2/params.py)
EXPORTS += ["bzh_hash_to_curve", "bzh_params_generators", "bzh_group_ifft", "bzh_params_create", "bzh_params_free", "bzh_params_bases",
            "bzh_params_points"]
EXPORTS += ["bzh_hash_to_curve_batch", "bzh_map_to_curve_batch", "bzh_params_generators_device", "bzh_params_create_with"]
EXPORTS += ["bzh_params_file_info", "bzh_params_encode", "bzh_params_write", "bzh_params_read"]
# circuit front end (bzh2/circuits.py)
EXPORTS += ["bzh_circuit_create", "bzh_circuit_free", "bzh_circuit_last_error", "bzh_circuit_blob", "bzh_circuit_describe",
            "bzh_circuit_info", "bzh_synthesize_shot", "bzh_synthesize_board", "bzh_synthesize_bitify_test", "bzh_board_witness",
            "bzh_shot_serialize", "bzh_pedersen_commit_host", "bzh_fixed_base_tables", "bzh_circuit_set_vk_repr", "bzh_circuit_vk_repr",
            "bzh_pedersen_commit_batch"]
EXPORTS += ["bzh_synthesize_shot_with", "bzh_synthesize_board_with"]
# game inputs in, proofs out, in one device-resident call (NativeProvingKey.prove_shots_device / prove_boards_device)
EXPORTS += ["bzh_prove_shots_device", "bzh_prove_boards_device"]
# records in, accept / reject out, in one device-resident call (NativeVerifyingKey.verify_records)
EXPORTS += ["bzh_verify_records_device"]
EXPORTS += ["bzh_verify_records_accumulated", "bzh_verify_batch_vk_accumulated", "bzh_accumulation_weights", "bzh_ipa_check_accumulated"]
E_VERIFY = -6


def _ctx_ipa_open(self, bases: Bases, poly, blind: int, x3: int, rng_bytes: bytes, transcript: "Transcript",
                  form: int = FORM_CANONICAL) -> int:
    """poly::commitment::create_proof: appends S, (L_j, R_j)*, c, f to `transcript`; returns v = p(x3)."""
    L = load()
    vp = ctypes.c_void_p
    L.bzh_ipa_open.argtypes = [vp, vp, vp, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_uint64),
                               ctypes.POINTER(ctypes.c_uint64), ctypes.c_char_p, ctypes.c_size_t, vp,
                               ctypes.POINTER(ctypes.c_uint64)]
    p = _as_elems(poly)
    out = np.zeros(4, dtype=np.uint64)
    rc = L.bzh_ipa_open(self.handle, bases.handle, _vp(p), form, MEM_HOST, _u64(int_to_limbs(blind)), _u64(int_to_limbs(x3)),
                        rng_bytes, len(rng_bytes), transcript.h, _u64(out))
    self._check(rc, "bzh_ipa_open")
    return limbs_to_int(out)


def _ctx_ipa_verify(self, bases: Bases, commitment, x3: int, v: int, proof: bytes, transcript: "Transcript", g0_u_w) -> bool:
    """True iff the opening proof verifies (bzh_ipa_verify); raises on any other error."""
    L = load()
    vp = ctypes.c_void_p
    u64p = ctypes.POINTER(ctypes.c_uint64)
    L.bzh_ipa_verify.argtypes = [vp, vp, u64p, u64p, u64p, ctypes.c_char_p, ctypes.c_size_t, vp, u64p]
    cm = Transcript._pt(commitment)
    trip = np.concatenate([Transcript._pt(p) for p in g0_u_w])
    rc = L.bzh_ipa_verify(self.handle, bases.handle, _u64(cm), _u64(int_to_limbs(x3)), _u64(int_to_limbs(v)), proof, len(proof),
                          transcript.h, _u64(trip))
    if rc == E_VERIFY:
        return False
    self._check(rc, "bzh_ipa_verify")
    return True


def _ctx_ipa_open_batch(self, bases: Bases, polys, blinds, x3s, rng_list, transcripts, form: int = FORM_CANONICAL):
    """`len(transcripts)` openings in lockstep (bzh_ipa_open_batch); polys: (batch, n, 4) uint64; returns the v's."""
    L = load()
    vp = ctypes.c_void_p
    u64p = ctypes.POINTER(ctypes.c_uint64)
    L.bzh_ipa_open_batch.argtypes = [vp, vp, vp, ctypes.c_int, ctypes.c_int, ctypes.c_size_t, u64p, u64p, ctypes.c_char_p,
                                     ctypes.c_size_t, ctypes.POINTER(vp), u64p]
    B = len(transcripts)
    p = np.ascontiguousarray(np.asarray(polys, dtype=np.uint64).reshape(B, -1, 4))
    stride = len(rng_list[0])
    assert all(len(r) == stride for r in rng_list)
    bl = np.ascontiguousarray(np.stack([int_to_limbs(v) for v in blinds]))
    xs = np.ascontiguousarray(np.stack([int_to_limbs(v) for v in x3s]))
    out = np.zeros((B, 4), dtype=np.uint64)
    trs = (vp * B)(*[t.h for t in transcripts])
    rc = L.bzh_ipa_open_batch(self.handle, bases.handle, _vp(p), form, MEM_HOST, B, _u64(bl), _u64(xs), b"".join(rng_list), stride,
                              trs, _u64(out))
    self._check(rc, "bzh_ipa_open_batch")
    return [limbs_to_int(o) for o in out]


Context.ipa_open = _ctx_ipa_open
Context.ipa_open_batch = _ctx_ipa_open_batch
Context.ipa_verify = _ctx_ipa_verify


# ---- gate-expression evaluation (row a13) ------------------------------------------------------
EXPORTS += ["bzh_expr_eval", "bzh_expr_eval_batch"]


def _ctx_expr_eval(self, field: int, program, columns, form: int = FORM_CANONICAL) -> np.ndarray:
    """Evaluate a straight-line program (bzh_expr_op records: anything with .as_array() -> ctypes array of them, .ops, .consts,
    .result_slot; tests/helpers/expr.py compiles expression trees into one) at every row; columns: list of (size, 4) uint64 arrays."""
    L = load()
    vp = ctypes.c_void_p
    L.bzh_expr_eval.argtypes = [vp, ctypes.c_int, vp, ctypes.c_size_t, ctypes.POINTER(vp), ctypes.c_size_t,
                                vp, ctypes.c_size_t, ctypes.c_uint, ctypes.c_int, ctypes.c_int, ctypes.c_int, vp]
    cols = [_as_elems(c) for c in columns]
    size = cols[0].shape[0] if cols else 1
    log_size = size.bit_length() - 1
    assert all(c.shape[0] == size for c in cols) and (1 << log_size) == size
    ptrs = (vp * max(len(cols), 1))(*[c.ctypes.data for c in cols])
    consts = np.ascontiguousarray(np.stack([int_to_limbs(v) for v in program.consts]) if program.consts
                                  else np.zeros((1, 4), dtype=np.uint64))
    out = np.zeros((size, 4), dtype=np.uint64)
    ops = program.as_array()
    rc = L.bzh_expr_eval(self.handle, field, ctypes.cast(ops, vp), len(program.ops), ptrs, len(cols), _vp(consts), len(program.consts), log_size,
                         program.result_slot, form, MEM_HOST, _vp(out))
    self._check(rc, "bzh_expr_eval")
    return out


Context.expr_eval = _ctx_expr_eval

EXPORTS += ["bzh_vm2_eval"]
# one 16-byte VM v2 instruction word (csrc/vm2_isa.hpp; what bzh_quotient_program_for_circuit hands out)
VM2_OP_DTYPE = np.dtype([("code", "u1"), ("a_kind", "u1"), ("b_kind", "u1"), ("pad", "u1"), ("a_idx", "<i4"), ("b_idx", "<i4"),
                         ("a_rot", "<i2"), ("b_rot", "<i2")])


def _ctx_vm2_eval(self, field: int, ops, columns, consts, size: int, batch: int = 1, nlds: int = 0, column_strides=None,
                  const_stride: int = 0, form: int = FORM_CANONICAL, mem: int = MEM_HOST, out=None, nconsts: int | None = None):
    """Run a VM v2 program (bzh_vm2_eval; `ops`: VM2_OP_DTYPE records) over `batch` vectors of `size` rows and return register r0 of
    every row, (batch * size, 4) uint64.  columns: (n, 4) uint64 arrays, vector v of column c starting column_strides[c] elements
    after vector v - 1 (0: shared); consts: (n, 4) uint64 (host), vector v's const_stride elements after (0: shared), nconsts of
    them per vector (default: all of them, or const_stride).  With MEM_DEVICE the columns and `out` are device addresses.  `out` (MEM_HOST: a (batch * size, 4) uint64 array) is filled and returned when given."""
    L = load()
    vp = ctypes.c_void_p
    L.bzh_vm2_eval.argtypes = [vp, ctypes.c_int, vp, ctypes.c_size_t, ctypes.POINTER(vp), ctypes.POINTER(ctypes.c_size_t), ctypes.c_size_t,
                               vp, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_uint, ctypes.c_size_t, ctypes.c_int, ctypes.c_int,
                               ctypes.c_int, vp]
    ops = np.ascontiguousarray(ops, dtype=VM2_OP_DTYPE)
    if mem == MEM_HOST:
        columns = [_as_elems(c) for c in columns]
        if out is None:
            out = np.zeros((batch * size, 4), dtype=np.uint64)
    ncols = len(columns)
    ptrs = (vp * max(ncols, 1))(*[c.ctypes.data if mem == MEM_HOST else int(c) for c in columns])
    strides = (ctypes.c_size_t * max(ncols, 1))(*(column_strides if column_strides is not None else [0] * ncols))
    cv = _as_elems(consts) if len(consts) else np.zeros((1, 4), dtype=np.uint64)
    if nconsts is None:
        nconsts = (const_stride or cv.shape[0]) if len(consts) else 0
    log_size = max(size.bit_length() - 1, 0)
    assert (1 << log_size) == size, "size must be a power of two"
    rc = L.bzh_vm2_eval(self.handle, field, _vp(ops), len(ops), ptrs, strides, ncols, _vp(cv), nconsts, const_stride, log_size, batch,
                        nlds, form, mem, _vp(out) if mem == MEM_HOST else vp(int(out)))
    self._check(rc, "bzh_vm2_eval")
    return out


Context.vm2_eval = _ctx_vm2_eval

EXPORTS += ["bzh_vm2_eval_cosets", "bzh_pk_workspace_select", "bzh_pk_workspace_selected", "bzh_workspace_plan", "bzh_workspace_plan_items", "bzh_pk_workspace_peak"]


def _ctx_vm2_eval_cosets(self, field: int, ops, columns, column_extended, consts, log_n: int, batch: int = 1, nlds: int = 0,
                         column_strides=None, const_stride: int = 0, form: int = FORM_CANONICAL, mem: int = MEM_HOST, out=None,
                         nconsts: int | None = None, out_size: int | None = None):
    """Run a VM v2 program coset by coset (bzh_vm2_eval_cosets) over `batch` vectors of 8 * 2^log_n rows and return register r0 of
    every row, (batch * 8 * 2^log_n, 4) uint64 -- what vm2_eval returns over the same data.  column_extended[c] true: column c as
    for vm2_eval, 8 n rows per vector; false: eight blocks of n rows per vector, block j = rows j, j + 8, ... (coset j), vector v
    of block j at j * batch * stride + v * stride elements (a shared column: at j * n).  The rest as for vm2_eval; out_size
    (default 8 * 2^log_n) is what the call is told `out` holds per vector."""
    L = load()
    vp, sz = ctypes.c_void_p, ctypes.c_size_t
    L.bzh_vm2_eval_cosets.argtypes = [vp, ctypes.c_int, vp, sz, ctypes.POINTER(vp), ctypes.POINTER(sz), ctypes.c_char_p, sz, vp, sz, sz,
                                      ctypes.c_uint, sz, sz, ctypes.c_int, ctypes.c_int, ctypes.c_int, vp]
    ops = np.ascontiguousarray(ops, dtype=VM2_OP_DTYPE)
    size = 8 << log_n
    if mem == MEM_HOST:
        columns = [_as_elems(c) for c in columns]
        if out is None:
            out = np.zeros((batch * size, 4), dtype=np.uint64)
    ncols = len(columns)
    ptrs = (vp * max(ncols, 1))(*[c.ctypes.data if mem == MEM_HOST else int(c) for c in columns])
    strides = (sz * max(ncols, 1))(*(column_strides if column_strides is not None else [0] * ncols))
    flags = bytes(1 if f else 0 for f in column_extended) or b"\0"
    cv = _as_elems(consts) if len(consts) else np.zeros((1, 4), dtype=np.uint64)
    if nconsts is None:
        nconsts = (const_stride or cv.shape[0]) if len(consts) else 0
    out_ptr = (out.ctypes.data if isinstance(out, np.ndarray) else int(out))
    rc = L.bzh_vm2_eval_cosets(self.handle, field, _vp(ops), len(ops), ptrs, strides, flags, ncols, _vp(cv), nconsts, const_stride, log_n,
                               size if out_size is None else out_size, batch, nlds, form, mem, vp(out_ptr))
    self._check(rc, "bzh_vm2_eval_cosets")
    return out


Context.vm2_eval_cosets = _ctx_vm2_eval_cosets


# ---- multiopen / lookup helpers ---------------------------------------------------------------------
EXPORTS += ["bzh_kate_division", "bzh_kate_division_batch", "bzh_permute_expression_pair"]


def _ctx_kate_division(self, field: int, coeffs, x: int, form: int = FORM_CANONICAL) -> np.ndarray:
    """arithmetic::kate_division: quotient of p(X) by (X - x) (n-1 coefficients)."""
    c = _as_elems(coeffs)
    n = c.shape[0]
    out = np.zeros((max(n - 1, 0), 4), dtype=np.uint64)
    L = load()
    vp = ctypes.c_void_p
    L.bzh_kate_division.argtypes = [vp, ctypes.c_int, vp, ctypes.c_size_t, ctypes.POINTER(ctypes.c_uint64), ctypes.c_int, ctypes.c_int, vp]
    self._check(L.bzh_kate_division(self.handle, field, _vp(c), n, _u64(int_to_limbs(x)), form, MEM_HOST, _vp(out)), "bzh_kate_division")
    return out


Context.kate_division = _ctx_kate_division


def _ctx_kate_division_batch(self, field: int, coeffs, xs, form: int = FORM_CANONICAL) -> np.ndarray:
    """`batch` kate divisions in one pass: coeffs (batch, n, 4), xs a list of `batch` integers; returns (batch, n-1, 4)."""
    c = np.ascontiguousarray(coeffs, dtype=np.uint64)
    batch, n = c.shape[0], c.shape[1]
    out = np.zeros((batch, max(n - 1, 0), 4), dtype=np.uint64)
    xv = np.ascontiguousarray(np.stack([int_to_limbs(x) for x in xs]), dtype=np.uint64)
    L = load()
    vp = ctypes.c_void_p
    L.bzh_kate_division_batch.argtypes = [vp, ctypes.c_int, vp, ctypes.c_size_t, ctypes.c_size_t, vp, ctypes.c_int, ctypes.c_int, vp]
    self._check(L.bzh_kate_division_batch(self.handle, field, _vp(c), n, batch, _vp(xv), form, MEM_HOST, _vp(out)),
                "bzh_kate_division_batch")
    return out


Context.kate_division_batch = _ctx_kate_division_batch


EXPORTS += ["bzh_batch_invert_plan", "bzh_kate_division_plan"]


def batch_invert_plan(count: int) -> int:
    """threads of the launch bzh_batch_invert makes for `count` elements: thread t owns the elements t, t + nthreads, ...
    (bzh_batch_invert_plan)."""
    L = load()
    L.bzh_batch_invert_plan.argtypes = [ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t)]
    nthreads = ctypes.c_size_t()
    rc = L.bzh_batch_invert_plan(count, ctypes.byref(nthreads))
    if rc != OK:
        raise BzhError(rc, "bzh_batch_invert_plan")
    return nthreads.value


def kate_division_plan(n: int, batch: int = 1):
    """(threads, L, S) of the launch bzh_kate_division_batch makes for `batch` polynomials of n coefficients: S workgroups of
    `threads` threads per polynomial, L quotient coefficients per thread (bzh_kate_division_plan)."""
    L = load()
    szp = ctypes.POINTER(ctypes.c_size_t)
    L.bzh_kate_division_plan.argtypes = [ctypes.c_size_t, ctypes.c_size_t, ctypes.POINTER(ctypes.c_uint), szp, szp]
    threads, seg, spans = ctypes.c_uint(), ctypes.c_size_t(), ctypes.c_size_t()
    rc = L.bzh_kate_division_plan(n, batch, ctypes.byref(threads), ctypes.byref(seg), ctypes.byref(spans))
    if rc != OK:
        raise BzhError(rc, "bzh_kate_division_plan")
    return threads.value, seg.value, spans.value


EXPORTS += ["bzh_permute_expression_pair_batch"]


def _bind_permute_batch():
    L = load()
    vp = ctypes.c_void_p
    L.bzh_permute_expression_pair_batch.argtypes = [vp, ctypes.c_int, vp, vp, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_int,
                                                    ctypes.c_int, vp, vp, ctypes.POINTER(ctypes.c_int32)]
    return L


def _ctx_permute_expression_pair_batch(self, field: int, input_vals, table_vals, usable_rows: int, form: int = FORM_CANONICAL,
                                       check: bool = True, out=None):
    """lookup::prover::permute_expression_pair for `batch` pairs on the device (bzh_permute_expression_pair_batch).
    input_vals / table_vals: (batch, stride, 4) uint64 in `form`; returns (permuted_input, permuted_table, status): the
    outputs have the inputs' shape with rows usable_rows .. stride zero, status is (batch,) int32 -- 0, or E_RANGE for a pair
    with an input value missing from its table.  check=True raises BzhError on such a pair; check=False hands the status
    words and the other pairs' results back.  out: a pair of C-contiguous uint64 arrays of that shape to write into."""
    a = np.ascontiguousarray(input_vals, dtype=np.uint64)
    t = np.ascontiguousarray(table_vals, dtype=np.uint64)
    if a.ndim != 3 or a.shape != t.shape or a.shape[2] != 4:
        raise BzhError(E_ARG, "bzh_permute_expression_pair_batch", "input and table must both be (batch, stride, 4)")
    batch, stride = a.shape[0], a.shape[1]
    oa, ot = (np.zeros_like(a), np.zeros_like(t)) if out is None else out
    if any(o.shape != a.shape or o.dtype != np.uint64 or not o.flags.c_contiguous for o in (oa, ot)):
        raise BzhError(E_ARG, "bzh_permute_expression_pair_batch", "out arrays must match the inputs")
    status = np.zeros(batch, dtype=np.int32)
    rc = _bind_permute_batch().bzh_permute_expression_pair_batch(self.handle, field, _vp(a), _vp(t), stride, usable_rows, batch, form, MEM_HOST,
                                                                  _vp(oa), _vp(ot), status.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)))
    if rc != OK and (check or rc != E_RANGE):
        self._check(rc, "bzh_permute_expression_pair_batch")
    return oa, ot, status


def _ctx_permute_expression_pair_batch_device(self, field: int, input_ptr: int, table_ptr: int, stride: int, usable_rows: int, batch: int,
                                              out_input_ptr: int, out_table_ptr: int, form: int = FORM_MONTGOMERY, check: bool = True):
    """Device-pointer form: every array is batch x stride elements in HBM; returns the (batch,) int32 status words."""
    vp = ctypes.c_void_p
    status = np.zeros(batch, dtype=np.int32)
    rc = _bind_permute_batch().bzh_permute_expression_pair_batch(self.handle, field, vp(input_ptr), vp(table_ptr), stride, usable_rows, batch,
                                                                  form, MEM_DEVICE, vp(out_input_ptr), vp(out_table_ptr),
                                                                  status.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)))
    if rc != OK and (check or rc != E_RANGE):
        self._check(rc, "bzh_permute_expression_pair_batch")
    return status


Context.permute_expression_pair_batch = _ctx_permute_expression_pair_batch
Context.permute_expression_pair_batch_device = _ctx_permute_expression_pair_batch_device


def permute_expression_pair(field: int, input_vals, table_vals, usable_rows: int, form: int = FORM_CANONICAL):
    """lookup::prover::permute_expression_pair over the first usable_rows rows -> (permuted_input, permuted_table)."""
    a, t = _as_elems(input_vals), _as_elems(table_vals)
    oa = np.zeros((usable_rows, 4), dtype=np.uint64)
    ot = np.zeros((usable_rows, 4), dtype=np.uint64)
    L = load()
    vp = ctypes.c_void_p
    L.bzh_permute_expression_pair.argtypes = [ctypes.c_int, vp, vp, ctypes.c_size_t, ctypes.c_int, vp, vp]
    rc = L.bzh_permute_expression_pair(field, _vp(a), _vp(t), usable_rows, form, _vp(oa), _vp(ot))
    if rc != OK:
        raise BzhError(rc, "bzh_permute_expression_pair")
    return oa, ot


def __getattr__(name):
    # bzh2.NativeVerifyingKey: the verifying key of bzh2.native (which imports this module, hence resolved on first use)
    if name == "NativeVerifyingKey":
        from .native import NativeVerifyingKey
        return NativeVerifyingKey
    if name == "accumulation_weights":   # likewise: the weights of NativeVerifyingKey.verify_records_accumulated / verify_batch_accumulated
        from .native import accumulation_weights
        return accumulation_weights
    raise AttributeError("module %r has no attribute %r" % (__name__, name))
