"""Params::new (halo2_proofs poly::commitment::Params; benches/shot.rs:58, benches/board.rs:51) through the C ABI
(include/bzh2.h, csrc/params.hip): hash-to-curve SRS on the host -- or, opt-in, on the device (csrc/hash_to_curve.hip) --,
g_lagrange by a group FFT on the device, both cached on disk keyed by (curve, k)."""
from __future__ import annotations

import ctypes

import numpy as np

from . import CURVE_PALLAS, CURVE_VESTA, FORM_CANONICAL, MEM_HOST, Bases, BzhError, Context, limbs_to_int, load

_VP = ctypes.c_void_p


def _bind():
    L = load()
    if getattr(L, "_bzh_params_bound", False):
        return L
    L.bzh_hash_to_curve.argtypes = [ctypes.c_int, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_size_t, _VP]
    L.bzh_params_generators.argtypes = [ctypes.c_uint, _VP, _VP, _VP, ctypes.c_uint]
    L.bzh_group_ifft.argtypes = [_VP, ctypes.c_int, _VP, ctypes.c_uint, _VP]
    L.bzh_params_create.argtypes = [_VP, ctypes.c_uint, ctypes.c_char_p, ctypes.c_int, ctypes.POINTER(_VP)]
    L.bzh_params_free.argtypes = [_VP, _VP]
    L.bzh_params_bases.argtypes = [_VP, ctypes.POINTER(_VP), ctypes.POINTER(_VP)]
    L.bzh_params_points.argtypes = [_VP, _VP, _VP, _VP, _VP, ctypes.POINTER(ctypes.c_int)]
    u8p = ctypes.POINTER(ctypes.c_uint8)
    L.bzh_hash_to_curve_batch.argtypes = [_VP, ctypes.c_int, ctypes.c_char_p, _VP, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_int, ctypes.c_int,
                                          _VP, u8p]
    L.bzh_map_to_curve_batch.argtypes = [_VP, ctypes.c_int, _VP, ctypes.c_size_t, ctypes.c_int, ctypes.c_int, _VP, u8p]
    L.bzh_params_generators_device.argtypes = [_VP, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_int, ctypes.c_int, _VP]
    L.bzh_params_create_with.argtypes = [_VP, ctypes.c_uint, ctypes.c_char_p, ctypes.c_int, ctypes.c_int, ctypes.POINTER(_VP)]
    szp = ctypes.POINTER(ctypes.c_size_t)
    L.bzh_params_file_info.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_uint), szp]
    L.bzh_params_encode.argtypes = [ctypes.c_uint, _VP, _VP, _VP, _VP, _VP, ctypes.c_size_t, szp]
    L.bzh_params_write.argtypes = [_VP, _VP, _VP, ctypes.c_size_t, szp]
    L.bzh_params_read.argtypes = [_VP, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_int, ctypes.POINTER(_VP), _VP]
    L._bzh_params_bound = True
    return L


def hash_to_curve(curve: int, domain_prefix: str, message: bytes):
    """CurveExt::hash_to_curve(domain_prefix)(message) -> affine (x, y) ints (host)."""
    out = np.zeros(8, dtype=np.uint64)
    rc = _bind().bzh_hash_to_curve(curve, domain_prefix.encode(), message, len(message), _VP(out.ctypes.data))
    if rc:
        raise BzhError(rc, "bzh_hash_to_curve")
    return limbs_to_int(out[:4]), limbs_to_int(out[4:])


def generators(k: int, threads: int = 0):
    """(g, w, u) of Params::new(k): g as an (n, 8) uint64 array of canonical limbs, w / u as (x, y) ints."""
    n = 1 << k
    g, w, u = np.zeros((n, 8), dtype=np.uint64), np.zeros(8, dtype=np.uint64), np.zeros(8, dtype=np.uint64)
    rc = _bind().bzh_params_generators(k, _VP(g.ctypes.data), _VP(w.ctypes.data), _VP(u.ctypes.data), threads)
    if rc:
        raise BzhError(rc, "bzh_params_generators")
    return g, (limbs_to_int(w[:4]), limbs_to_int(w[4:])), (limbs_to_int(u[:4]), limbs_to_int(u[4:]))


GENERATORS_HOST, GENERATORS_DEVICE = 0, 1
_GENERATORS = {"host": GENERATORS_HOST, "device": GENERATORS_DEVICE}


def hash_to_curve_batch(ctx, curve: int, domain_prefix: str, messages, form: int = FORM_CANONICAL):
    """CurveExt::hash_to_curve(domain_prefix)(m) for a list of equally long byte strings (bzh_hash_to_curve_batch): (xy, status)
    -- xy (n, 8) uint64 in `form`, status (n,) uint8 of POINT_OK / POINT_IDENTITY.  ctx=None runs on the host, a Context on its
    device."""
    messages = list(messages)
    n = len(messages)
    msg_len = len(messages[0]) if n else 0
    if any(len(m) != msg_len for m in messages):
        raise ValueError("hash_to_curve_batch: the messages of one call have one length")
    buf = np.frombuffer(b"".join(messages), dtype=np.uint8).copy() if n * msg_len else np.zeros(1, dtype=np.uint8)
    out, st = np.zeros((n, 8), dtype=np.uint64), np.zeros(n, dtype=np.uint8)
    rc = _bind().bzh_hash_to_curve_batch(ctx.handle if ctx is not None else None, curve, domain_prefix.encode(), _VP(buf.ctypes.data), msg_len, n,
                                         form, MEM_HOST, _VP(out.ctypes.data), st.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)))
    if rc:
        raise BzhError(rc, "bzh_hash_to_curve_batch")
    return out, st


def map_to_curve_batch(ctx, curve: int, u_pairs, form: int = FORM_CANONICAL):
    """iso_map(swu(u0) + swu(u1)) for an (n, 8) uint64 array of pairs u0 || u1 in `form` (bzh_map_to_curve_batch): (xy, status)."""
    u = np.ascontiguousarray(u_pairs, dtype=np.uint64).reshape(-1, 8)
    n = u.shape[0]
    out, st = np.zeros((n, 8), dtype=np.uint64), np.zeros(n, dtype=np.uint8)
    rc = _bind().bzh_map_to_curve_batch(ctx.handle if ctx is not None else None, curve, _VP(u.ctypes.data), n, form, MEM_HOST,
                                        _VP(out.ctypes.data), st.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)))
    if rc:
        raise BzhError(rc, "bzh_map_to_curve_batch")
    return out, st


def generators_device(ctx: Context, first: int, count: int, form: int = FORM_CANONICAL) -> np.ndarray:
    """g[first : first + count] of Params::new made on the device (bzh_params_generators_device): (count, 8) uint64 in `form`."""
    out = np.zeros((count, 8), dtype=np.uint64)
    ctx._check(_bind().bzh_params_generators_device(ctx.handle, first, count, form, MEM_HOST, _VP(out.ctypes.data)), "bzh_params_generators_device")
    return out


def group_ifft(ctx: Context, g: np.ndarray) -> np.ndarray:
    """The inverse group FFT of n = 2^k Vesta points (bzh_group_ifft): (n, 8) uint64 canonical limbs x || y in and out, (0, 0) the
    identity.  g is left as it is."""
    g = np.ascontiguousarray(g, dtype=np.uint64)
    if g.ndim != 2 or g.shape[1] != 8:
        raise ValueError("group_ifft: g is an (n, 8) array of canonical limbs, got shape %r" % (g.shape,))
    n = g.shape[0]
    if n < 1 or n & (n - 1):
        raise ValueError("group_ifft: the number of points is a power of two, got %d" % n)
    k = n.bit_length() - 1
    out = np.zeros((n, 8), dtype=np.uint64)
    ctx._check(_bind().bzh_group_ifft(ctx.handle, CURVE_VESTA, _VP(g.ctypes.data), k, _VP(out.ctypes.data)), "bzh_group_ifft")
    return out


E_RANGE = -4
CHECK_POINTS, CHECK_LAGRANGE, CHECK_FULL = 0, 1, 2
_CHECKS = {"points": CHECK_POINTS, "lagrange": CHECK_LAGRANGE, "full": CHECK_FULL}
BAD_DECODE, BAD_LAGRANGE, BAD_GENERATORS = 1, 2, 4
SECTIONS = ("g", "g_lagrange", "w", "u")


class ParamsFileError(ValueError):
    """bzh_params_read refused a params file: the fields of its bzh_params_verdict -- bits (BAD_DECODE, or BAD_LAGRANGE |
    BAD_GENERATORS), and section (index into SECTIONS), first_bad, n_bad of the offending points (include/bzh2.h)."""

    def __init__(self, bits: int, section: int, first_bad: int, n_bad: int, detail: str = ""):
        self.bits, self.section, self.first_bad, self.n_bad = bits, section, first_bad, n_bad
        super().__init__(detail or "params file refused: bits %d, %s[%d], %d bad" % (bits, SECTIONS[section & 3], first_bad, n_bad))


def file_info(data: bytes):
    """(k, n) of a params file's header after the length check (bzh_params_file_info, host only)"""
    data = bytes(data)
    k, n = ctypes.c_uint(), ctypes.c_size_t()
    rc = _bind().bzh_params_file_info(data, len(data), ctypes.byref(k), ctypes.byref(n))
    if rc:
        raise BzhError(rc, "bzh_params_file_info")
    return k.value, n.value


def encode(k: int, g, g_lagrange, w, u) -> bytes:
    """halo2_proofs' Params::write for points given as canonical limbs (bzh_params_encode, host only): g, g_lagrange (n, 8) uint64,
    w, u (8,) uint64."""
    arrs = [np.ascontiguousarray(a, dtype=np.uint64) for a in (g, g_lagrange, w, u)]
    n = 1 << k
    if arrs[0].shape != (n, 8) or arrs[1].shape != (n, 8) or arrs[2].size != 8 or arrs[3].size != 8:
        raise ValueError("encode: g and g_lagrange are (2^k, 8) arrays, w and u 8 limbs")
    L, size = _bind(), ctypes.c_size_t()
    ptrs = [_VP(a.ctypes.data) for a in arrs]
    rc = L.bzh_params_encode(k, *ptrs, None, 0, ctypes.byref(size))
    if rc:
        raise BzhError(rc, "bzh_params_encode")
    out = np.zeros(size.value, dtype=np.uint8)
    rc = L.bzh_params_encode(k, *ptrs, _VP(out.ctypes.data), out.size, ctypes.byref(size))
    if rc:
        raise BzhError(rc, "bzh_params_encode")
    return out.tobytes()


class Params:
    """Params::<vesta::Affine>::new(k): the two commitment-base tables live on the device."""

    def __init__(self, ctx: Context, k: int, cache_dir: str | None = None, window_bits: int = 0, generators: str = "host"):
        """generators: who makes g on a cache miss -- "host" (threads) or "device" (csrc/hash_to_curve.hip); the same points."""
        L = _bind()
        h = _VP()
        if generators not in _GENERATORS:
            raise ValueError("Params: generators is 'host' or 'device'")
        ctx._check(L.bzh_params_create_with(ctx.handle, k, None if cache_dir is None else cache_dir.encode(), window_bits,
                                            _GENERATORS[generators], ctypes.byref(h)), "bzh_params_create_with")
        self._attach(ctx, h, k)

    def _attach(self, ctx: Context, h, k: int):
        """take over a bzh_params handle, whoever made it"""
        self.ctx, self.handle, self.k, self.n = ctx, h, k, 1 << k
        g, gl = _VP(), _VP()
        _bind().bzh_params_bases(h, ctypes.byref(g), ctypes.byref(gl))
        self.bases = Bases(ctx, g, CURVE_VESTA, self.n + 2)
        self.bases_lagrange = Bases(ctx, gl, CURVE_VESTA, self.n + 3)    # (g_lagrange | u | w | g_0)
        self._borrowers = []     # weak references to the proving keys built on these tables (they borrow, include/bzh2.h)

    @classmethod
    def from_bytes(cls, ctx: Context, data: bytes, check: str = "full", window_bits: int = 0) -> "Params":
        """halo2_proofs' Params::read (bzh_params_read): the byte string Params::write / to_bytes gives -> Params on ctx's device,
        as __init__ would have made them for the same points.  check: "points" (every string is a point other than the identity),
        "lagrange" (and g_lagrange is the inverse group FFT of g), "full" (and g, w, u are Params::new(k)'s -- the default, the only
        level that protects soundness).  A refused file raises ParamsFileError; a malformed one (length, k) BzhError."""
        if check not in _CHECKS:
            raise ValueError("Params.from_bytes: check is 'points', 'lagrange' or 'full'")
        data = bytes(data)
        h, v = _VP(), np.zeros(4, dtype=np.uint32)
        rc = _bind().bzh_params_read(ctx.handle, data, len(data), window_bits, _CHECKS[check], ctypes.byref(h), _VP(v.ctypes.data))
        if rc == E_RANGE and v[0]:
            raise ParamsFileError(*(int(x) for x in v), detail=load().bzh_last_error(ctx.handle).decode())
        ctx._check(rc, "bzh_params_read")
        self = cls.__new__(cls)
        self._attach(ctx, h, file_info(data)[0])
        return self

    def to_bytes(self) -> bytes:
        """halo2_proofs' Params::write (bzh_params_write): k | g | g_lagrange | w | u, 32 bytes a point."""
        L, size = _bind(), ctypes.c_size_t()
        self.ctx._check(L.bzh_params_write(self.ctx.handle, self.handle, None, 0, ctypes.byref(size)), "bzh_params_write")
        out = np.zeros(size.value, dtype=np.uint8)
        self.ctx._check(L.bzh_params_write(self.ctx.handle, self.handle, _VP(out.ctypes.data), out.size, ctypes.byref(size)), "bzh_params_write")
        return out.tobytes()

    @classmethod
    def from_file(cls, ctx: Context, path, check: str = "full", window_bits: int = 0) -> "Params":
        with open(path, "rb") as f:
            return cls.from_bytes(ctx, f.read(), check=check, window_bits=window_bits)

    def to_file(self, path):
        with open(path, "wb") as f:
            f.write(self.to_bytes())

    def points(self, want_g: bool = True, want_lagrange: bool = True):
        """host copies: (g, g_lagrange, w, u, from_cache) -- arrays of canonical limbs, w / u as (x, y) ints"""
        g = np.zeros((self.n, 8), dtype=np.uint64) if want_g else None
        gl = np.zeros((self.n, 8), dtype=np.uint64) if want_lagrange else None
        w, u = np.zeros(8, dtype=np.uint64), np.zeros(8, dtype=np.uint64)
        fc = ctypes.c_int()
        _bind().bzh_params_points(self.handle, _VP(g.ctypes.data) if want_g else None, _VP(gl.ctypes.data) if want_lagrange else None,
                                  _VP(w.ctypes.data), _VP(u.ctypes.data), ctypes.byref(fc))
        return g, gl, (limbs_to_int(w[:4]), limbs_to_int(w[4:])), (limbs_to_int(u[:4]), limbs_to_int(u[4:])), bool(fc.value)

    def close(self, strict: bool = False):
        """bzh_params_free.  Proving keys borrow the tables: freeing them under a live key would leave it reading freed window
        tables.  close() is what cleanup paths (`finally:`) call, so by default the keys still open on these Params are closed
        first, with a warning -- raising here would mask the exception that skipped their close() and leak the device tables.
        strict=True keeps the hard error for callers that want the ordering enforced."""
        if self.handle is not None:
            live = [r() for r in self._borrowers if r() is not None and r().handle is not None]
            self._borrowers = []          # dead references are dropped either way
            if live and strict:
                self._borrowers = [__import__("weakref").ref(k) for k in live]
                raise RuntimeError("Params.close(strict=True): a NativeProvingKey built on these Params is still open; close the key first")
            if live:
                import warnings
                warnings.warn("Params.close(): closing %d NativeProvingKey(s) still open on these Params first" % len(live), ResourceWarning, stacklevel=2)
                for key in live:
                    key.close()
            _bind().bzh_params_free(self.ctx.handle, self.handle)
            self.handle = None
            self.bases.handle = None            # the tables went with the params
            self.bases_lagrange.handle = None
