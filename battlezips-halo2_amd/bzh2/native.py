"""Binding of the native whole-proof entry points (include/bzh2.h: bzh_pk_create / bzh_prove_batch).

The reference-side call this stands behind is halo2_proofs::plonk::{keygen_pk, create_proof} (benches/shot.rs:58-71,
benches/board.rs:51-71); the circuit crosses the boundary as data (bzh2.circuit_data.serialize_circuit, or a blob of bzh2.circuits.CircuitLayout)."""
from __future__ import annotations

import ctypes

import numpy as np

from . import CURVE_SCALAR_FIELD, FORM_CANONICAL, FORM_MONTGOMERY, MEM_DEVICE, MEM_HOST, Bases, BzhError, Context, int_to_limbs, load
from .circuit_data import MODULI, Circuit, serialize_circuit

_VP = ctypes.c_void_p


def _bind():
    L = load()
    if getattr(L, "_bzh_native_bound", False):
        return L
    L.bzh_pk_create.argtypes = [_VP, _VP, ctypes.c_char_p, ctypes.c_size_t, ctypes.POINTER(_VP)]
    L.bzh_pk_free.argtypes = [_VP, _VP]
    L.bzh_pk_set_lagrange.argtypes = [_VP, _VP]
    L.bzh_pk_info.argtypes = [_VP, ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(ctypes.c_uint32),
                              ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32)]
    L.bzh_verify_batch.argtypes = [_VP, _VP, ctypes.c_size_t, _VP, ctypes.c_size_t, _VP, ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t), _VP,
                                   ctypes.POINTER(ctypes.c_int)]
    L.bzh_prove_batch.argtypes = [_VP, _VP, ctypes.c_size_t, _VP, ctypes.c_int, ctypes.c_int, _VP, ctypes.c_size_t, ctypes.c_char_p,
                                  ctypes.c_size_t, _VP, ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t)]
    L.bzh_prove_batch_seeded.argtypes = [_VP, _VP, ctypes.c_size_t, _VP, ctypes.c_int, ctypes.c_int, _VP, ctypes.c_size_t, ctypes.c_char_p,
                                         _VP, ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t)]
    L.bzh_rng_expand.argtypes = [ctypes.c_char_p, ctypes.c_uint64, ctypes.c_size_t, _VP]
    L.bzh_prove_batch_device.argtypes = [_VP, _VP, ctypes.c_size_t, _VP, ctypes.c_int, ctypes.c_int, _VP, ctypes.c_size_t, _VP,
                                         ctypes.c_size_t, _VP, ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t), _VP]
    L.bzh_prove_batch_device_seeded.argtypes = [_VP, _VP, ctypes.c_size_t, _VP, ctypes.c_int, ctypes.c_int, _VP, ctypes.c_size_t,
                                                ctypes.c_char_p, _VP, ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t), _VP]
    L.bzh_prove_shots_device.argtypes = [_VP, _VP, _VP, ctypes.c_size_t, _VP, _VP, _VP, _VP, ctypes.c_char_p, _VP, _VP, ctypes.c_size_t,
                                         ctypes.POINTER(ctypes.c_size_t), _VP]
    L.bzh_prove_boards_device.argtypes = [_VP, _VP, _VP, ctypes.c_size_t, _VP, _VP, _VP, ctypes.c_char_p, _VP, _VP, ctypes.c_size_t,
                                          ctypes.POINTER(ctypes.c_size_t), _VP]
    L.bzh_pk_vk_repr.argtypes = [_VP, _VP, ctypes.POINTER(ctypes.c_int)]
    szp, u32p = ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(ctypes.c_uint32)
    L.bzh_vk_create.argtypes = [_VP, _VP, ctypes.c_char_p, ctypes.c_size_t, ctypes.POINTER(_VP)]
    L.bzh_vk_from_pk.argtypes = [_VP, _VP, ctypes.POINTER(_VP)]
    L.bzh_vk_write.argtypes = [_VP, _VP, ctypes.c_size_t, szp]
    L.bzh_vk_read.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.POINTER(_VP)]
    L.bzh_vk_info.argtypes = [_VP, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_uint), u32p, u32p, u32p, szp]
    L.bzh_vk_vk_repr.argtypes = [_VP, _VP, ctypes.POINTER(ctypes.c_int)]
    L.bzh_vk_device_bytes.argtypes = [_VP, szp, szp]
    L.bzh_pk_device_bytes.argtypes = [_VP, szp, szp]
    L.bzh_vk_free.argtypes = [_VP]
    L.bzh_verify_batch_vk.argtypes = [_VP, _VP, _VP, _VP, ctypes.c_size_t, _VP, ctypes.c_size_t, _VP, ctypes.c_size_t,
                                      ctypes.POINTER(ctypes.c_size_t), _VP, ctypes.POINTER(ctypes.c_int)]
    L.bzh_verify_batch_vk_with.argtypes = [_VP, _VP, _VP, _VP, ctypes.c_int, ctypes.c_size_t, _VP, ctypes.c_size_t, _VP, ctypes.c_size_t,
                                           ctypes.POINTER(ctypes.c_size_t), _VP, ctypes.POINTER(ctypes.c_int)]
    L.bzh_verify_records_device.argtypes = [_VP, _VP, _VP, _VP, ctypes.c_size_t, ctypes.c_size_t, _VP, ctypes.c_size_t, _VP,
                                            ctypes.POINTER(ctypes.c_int), _VP]
    L.bzh_verify_records_accumulated.argtypes = [_VP, _VP, _VP, _VP, ctypes.c_size_t, ctypes.c_size_t, _VP, ctypes.c_size_t, _VP,
                                                 ctypes.c_char_p, ctypes.POINTER(ctypes.c_int), _VP, ctypes.POINTER(ctypes.c_int)]
    L.bzh_verify_batch_vk_accumulated.argtypes = [_VP, _VP, _VP, _VP, ctypes.c_size_t, _VP, ctypes.c_size_t, _VP, ctypes.c_size_t,
                                                  ctypes.POINTER(ctypes.c_size_t), _VP, ctypes.c_char_p, ctypes.POINTER(ctypes.c_int),
                                                  ctypes.POINTER(ctypes.c_int)]
    L.bzh_accumulation_weights.argtypes = [ctypes.c_int, ctypes.c_char_p, ctypes.c_size_t, _VP]
    L.bzh_ipa_check_accumulated.argtypes = [_VP, _VP, ctypes.c_size_t, ctypes.c_size_t, _VP, _VP, _VP, _VP, _VP, ctypes.POINTER(ctypes.c_int)]
    L.bzh_pk_verify_pass_select.argtypes = [_VP, ctypes.c_int]
    L.bzh_pk_verify_pass_selected.argtypes = [_VP, ctypes.POINTER(ctypes.c_int)]
    L._bzh_native_bound = True
    return L


def rng_expand(seed: bytes, first_draw: int, draws: int) -> bytes:
    """draws [first_draw, first_draw + draws) of the ChaCha20 stream bzh_prove_batch_seeded derives from `seed` (64 bytes each)"""
    assert len(seed) == 32
    out = np.zeros(draws * 64, dtype=np.uint8)
    rc = _bind().bzh_rng_expand(seed, first_draw, draws, _VP(out.ctypes.data))
    if rc:
        raise BzhError(rc, "bzh_rng_expand")
    return out.tobytes()


def accumulation_weights(curve: int, seed: bytes, batch: int) -> list:
    """the weights of an accumulated batch verification (bzh_accumulation_weights): draw b of rng_expand(seed, b, 1) reduced into
    the scalar field of `curve` as a 512-bit little-endian integer; a list of ints.  The seed must be unpredictable to the proofs'
    author: see the SECURITY paragraph in include/bzh2.h."""
    assert len(seed) == 32
    out = np.zeros((max(batch, 1), 4), dtype=np.uint64)
    rc = _bind().bzh_accumulation_weights(curve, seed, batch, _VP(out.ctypes.data))
    if rc:
        raise BzhError(rc, "bzh_accumulation_weights")
    return [int.from_bytes(out[b].tobytes(), "little") for b in range(batch)]


QUOTIENT_INTERPRETER, QUOTIENT_BUILTIN, QUOTIENT_MODULE = 0, 1, 2
LOOKUP_HOST, LOOKUP_DEVICE = 0, 1
WORKSPACE_EXTENDED, WORKSPACE_COSETWISE = 0, 1


class _WorkspaceItems(ctypes.Structure):
    _fields_ = [(name, ctypes.c_uint64) for name in ("n", "extended", "columns", "column_bytes", "cosets_bytes", "cosets_extended_bytes",
                                                      "witness_bytes", "quotient_bytes", "tail_bytes", "staging_bytes", "total_bytes")]


def workspace_plan(curve: int, circuit_blob: bytes, batch: int, mode: int = WORKSPACE_EXTENDED) -> int:
    """arena bytes one prove call of `batch` proofs takes in `mode` (bzh_workspace_plan; host only, needs no GPU)"""
    L = load()
    L.bzh_workspace_plan.argtypes = [ctypes.c_int, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_int,
                                     ctypes.POINTER(ctypes.c_size_t)]
    blob, out = bytes(circuit_blob), ctypes.c_size_t()
    _check(L.bzh_workspace_plan(curve, blob, len(blob), batch, mode, ctypes.byref(out)), "bzh_workspace_plan")
    return out.value


def workspace_plan_items(curve: int, circuit_blob: bytes, batch: int, mode: int = WORKSPACE_EXTENDED) -> dict:
    """the items bzh_workspace_plan sums (bzh_workspace_plan_items: the fields of bzh_workspace_items, include/bzh2.h)"""
    L = load()
    L.bzh_workspace_plan_items.argtypes = [ctypes.c_int, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_int,
                                           ctypes.POINTER(_WorkspaceItems)]
    blob, it = bytes(circuit_blob), _WorkspaceItems()
    _check(L.bzh_workspace_plan_items(curve, blob, len(blob), batch, mode, ctypes.byref(it)), "bzh_workspace_plan_items")
    return {name: int(getattr(it, name)) for name, _ in _WorkspaceItems._fields_}
VERIFY_POINTS_HOST, VERIFY_POINTS_DEVICE = 0, 1
VERIFY_PASS_HOST, VERIFY_PASS_DEVICE = 0, 1

_QUOTIENT_CODE = {}   # source hash -> code object (several keys of one circuit in a process share one compilation)


def compile_quotient_source(src: str, cache_dir: str | None = None, use_cache: bool = True) -> bytes | None:
    """hipcc --genco of a bzh_pk_quotient_source text against csrc/field.cuh; the code object, or None."""
    import hashlib
    import os
    import shutil
    import subprocess
    import tempfile
    pkg = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    h = hashlib.sha256(src.encode())
    for hdr in ("field.cuh", "field_mul_fips.inc"):   # the code object also depends on the arithmetic it is compiled against
        try:
            h.update(open(os.path.join(pkg, "csrc", hdr), "rb").read())
        except OSError:
            return None
    key = h.hexdigest()[:24]
    if use_cache and key in _QUOTIENT_CODE:
        return _QUOTIENT_CODE[key]
    cache_dir = cache_dir or os.environ.get("BZH_CACHE_DIR") or os.path.join(os.path.dirname(pkg), ".bzh2_cache")
    path = os.path.join(cache_dir, "quotient_%s_gfx950.hsaco" % key)
    if use_cache and os.path.exists(path):
        _QUOTIENT_CODE[key] = open(path, "rb").read()
        return _QUOTIENT_CODE[key]
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        return None
    with tempfile.TemporaryDirectory() as td:
        srcp, outp = os.path.join(td, "quotient.hip"), os.path.join(td, "quotient.hsaco")
        open(srcp, "w").write(src)
        # hipcc is a driver that execs clang through a shell: it must not inherit a profiler's preload (rocprofv3 sets LD_PRELOAD /
        # tool-library variables; a preloaded tool initialises the GPU in every child and the exec chain is then refused on this pool)
        env = {k: v for k, v in os.environ.items()
               if k not in ("LD_PRELOAD", "HSA_TOOLS_LIB", "ROCP_TOOL_LIBRARIES") and not k.startswith(("ROCPROFILER_", "ROCPROF_", "ROCP_"))}
        r = subprocess.run([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "--genco", "-I", os.path.join(pkg, "csrc"), srcp, "-o", outp],
                           capture_output=True, text=True, env=env)
        if r.returncode != 0 or not os.path.exists(outp):
            return None
        code = open(outp, "rb").read()
    try:
        os.makedirs(cache_dir, exist_ok=True)
        tmp = "%s.tmp%d" % (path, os.getpid())
        open(tmp, "wb").write(code)
        os.replace(tmp, path)
    except OSError:
        pass
    _QUOTIENT_CODE[key] = code
    return code


class NativeProvingKey:
    """keygen_pk on the device.  g: the n SRS points, w / u: Params.w / Params.u (affine canonical int pairs)."""

    def __init__(self, ctx: Context, circuit: Circuit, curve: int, g=None, w=None, u=None, vk_repr: int = 0x1234, window_bits: int = 0,
                 params=None):
        """SRS either as explicit points (g, w, u) or as a bzh2.params.Params (Params::new(k): its tables are used as they
        are, and commitments the upstream prover makes in the Lagrange basis are made in it)."""
        self.ctx, self.c, self.curve = ctx, circuit, curve
        self.field = CURVE_SCALAR_FIELD[curve]
        self.p = MODULI[self.field]
        self._own_bases = params is None
        if params is None:
            tbl = np.stack([np.concatenate([int_to_limbs(pt[0]), int_to_limbs(pt[1])]) for pt in list(g) + [u, w]])
            self.bases: Bases = ctx.upload_bases(curve, tbl).precompute(window_bits)
            self._g0_u_w = np.ascontiguousarray(np.stack([tbl[0], tbl[-2], tbl[-1]]))
        else:
            import weakref
            self._params = params                      # keep the borrowed tables alive as long as the key
            params._borrowers.append(weakref.ref(self))
            self.bases = params.bases
            gp, _, wp, up, _ = params.points(want_lagrange=False)
            self._g0_u_w = np.ascontiguousarray(np.stack([gp[0], np.concatenate([int_to_limbs(up[0]), int_to_limbs(up[1])]),
                                                          np.concatenate([int_to_limbs(wp[0]), int_to_limbs(wp[1])])]))
        # a circuit built by the C++ front end (bzh2.circuits.CircuitLayout.blob()) arrives already serialised
        blob = bytes(circuit) if isinstance(circuit, (bytes, bytearray)) else serialize_circuit(circuit, self.p, vk_repr)
        self.blob = blob
        L = _bind()
        h = _VP()
        ctx._check(L.bzh_pk_create(ctx.handle, self.bases.handle, blob, len(blob), ctypes.byref(h)), "bzh_pk_create")
        self.handle = h
        rb, mp = ctypes.c_size_t(), ctypes.c_size_t()
        na, nr, ur = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32()
        ctx._check(L.bzh_pk_info(h, ctypes.byref(rb), ctypes.byref(mp), ctypes.byref(na), ctypes.byref(nr), ctypes.byref(ur)), "bzh_pk_info")
        self.rng_bytes, self.max_proof_bytes, self.num_advice, self.n, self.usable_rows = rb.value, mp.value, na.value, nr.value, ur.value
        if params is not None:
            self.set_lagrange(params.bases_lagrange)

    def vk_repr(self):
        """(the verifying-key digest this key absorbs first, whether it is still the library's placeholder)"""
        out, ph = (ctypes.c_uint8 * 32)(), ctypes.c_int()
        self.ctx._check(_bind().bzh_pk_vk_repr(self.handle, out, ctypes.byref(ph)), "bzh_pk_vk_repr")
        return int.from_bytes(bytes(out), "little"), bool(ph.value)

    def vanishing_plan(self):
        """(shape, consts) of bzh2.vanishing_plan for this key's circuit: what TranscriptBatch.vanishing takes as `shape`"""
        from . import vanishing_plan
        return vanishing_plan(self.curve, self.blob)

    def grand_products_plan(self):
        """the shape of bzh2.grand_products_plan for this key's circuit: what TranscriptBatch.grand_products takes as `shape`"""
        from . import grand_products_plan
        return grand_products_plan(self.curve, self.blob)

    def commitments_plan(self):
        """the shape of bzh2.commitments_plan for this key's circuit: what TranscriptBatch.commitments takes as `shape`"""
        from . import commitments_plan
        return commitments_plan(self.curve, self.blob)

    def prove_device_plan(self):
        """the shape of bzh2.prove_device_plan for this key's circuit: the leaves' draws, their sum, the proof bytes, nown, the largest batch"""
        from . import prove_device_plan
        return prove_device_plan(self.curve, self.blob)

    def quotient_stats(self) -> dict:
        L = _bind()
        L.bzh_pk_quotient_stats.argtypes = [_VP] + [ctypes.POINTER(ctypes.c_uint32)] * 4
        v = [ctypes.c_uint32() for _ in range(4)]
        self.ctx._check(L.bzh_pk_quotient_stats(self.handle, *[ctypes.byref(x) for x in v]), "bzh_pk_quotient_stats")
        L.bzh_pk_quotient_loads.argtypes = [_VP] + [ctypes.POINTER(ctypes.c_uint32)] * 2
        w = [ctypes.c_uint32() for _ in range(2)]
        self.ctx._check(L.bzh_pk_quotient_loads(self.handle, *[ctypes.byref(x) for x in w]), "bzh_pk_quotient_loads")
        return {"ops": v[0].value, "multiplications_per_row": v[1].value, "lds_slots": v[2].value, "hoisted_columns": v[3].value,
                "loads_per_row": w[0].value, "leaf_slots": w[1].value}

    # ---- the quotient evaluator as compiled code -------------------------------------------------------------
    def quotient_source(self) -> str:
        """the evaluator program as straight-line HIP source (BzhError E_RANGE if the circuit does not fit the evaluator)"""
        L = _bind()
        L.bzh_pk_quotient_source.argtypes = [_VP, ctypes.c_char_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t)]
        n = ctypes.c_size_t()
        self.ctx._check(L.bzh_pk_quotient_source(self.handle, None, 0, ctypes.byref(n)), "bzh_pk_quotient_source")
        buf = ctypes.create_string_buffer(n.value + 1)
        self.ctx._check(L.bzh_pk_quotient_source(self.handle, buf, n.value + 1, ctypes.byref(n)), "bzh_pk_quotient_source")
        return buf.value.decode()

    def set_quotient_module(self, code_object: bytes | None):
        L = _bind()
        L.bzh_pk_set_quotient_module.argtypes = [_VP, _VP, ctypes.c_char_p, ctypes.c_size_t]
        self.ctx._check(L.bzh_pk_set_quotient_module(self.ctx.handle, self.handle, code_object, len(code_object) if code_object else 0),
                        "bzh_pk_set_quotient_module")

    def quotient_selected(self):
        """(flavour, builtin_available): which quotient evaluator the key runs -- QUOTIENT_INTERPRETER (k_expr_vm2),
        QUOTIENT_BUILTIN (kernel generated when libbzh2.so was built: the reference's Shot / Board circuits) or
        QUOTIENT_MODULE (a code object installed with set_quotient_module)"""
        L = _bind()
        L.bzh_pk_quotient_selected.argtypes = [_VP, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]
        f, b = ctypes.c_int(), ctypes.c_int()
        self.ctx._check(L.bzh_pk_quotient_selected(self.handle, ctypes.byref(f), ctypes.byref(b)), "bzh_pk_quotient_selected")
        return f.value, bool(b.value)

    def quotient_select(self, flavour: int):
        L = _bind()
        L.bzh_pk_quotient_select.argtypes = [_VP, ctypes.c_int]
        self.ctx._check(L.bzh_pk_quotient_select(self.handle, flavour), "bzh_pk_quotient_select")

    # ---- where the lookup argument's columns are permuted ----------------------------------------------------
    def lookup_selected(self) -> int:
        """LOOKUP_DEVICE (csrc/lookup_permute.hip on the ctx's stream; every new key's default) or LOOKUP_HOST (pinned round
        trip + host sorts).  A key on which lookup_select was never called reports LOOKUP_DEVICE and takes the host path for
        batches of fewer than 8 proofs (include/bzh2.h)"""
        L = _bind()
        L.bzh_pk_lookup_selected.argtypes = [_VP, ctypes.POINTER(ctypes.c_int)]
        w = ctypes.c_int()
        self.ctx._check(L.bzh_pk_lookup_selected(self.handle, ctypes.byref(w)), "bzh_pk_lookup_selected")
        return w.value

    def lookup_select(self, where: int):
        L = _bind()
        L.bzh_pk_lookup_select.argtypes = [_VP, ctypes.c_int]
        self.ctx._check(L.bzh_pk_lookup_select(self.handle, where), "bzh_pk_lookup_select")

    # ---- where the quotient reads the per-proof columns -------------------------------------------------------
    def workspace_selected(self) -> int:
        """WORKSPACE_EXTENDED (every per-proof column on the whole extended coset; every new key's default) or
        WORKSPACE_COSETWISE (n-sized buffers, the quotient coset by coset through the interpreter whatever quotient_select
        says: include/bzh2.h)"""
        L = _bind()
        L.bzh_pk_workspace_selected.argtypes = [_VP, ctypes.POINTER(ctypes.c_int)]
        w = ctypes.c_int()
        self.ctx._check(L.bzh_pk_workspace_selected(self.handle, ctypes.byref(w)), "bzh_pk_workspace_selected")
        return w.value

    def workspace_select(self, mode: int):
        L = _bind()
        L.bzh_pk_workspace_select.argtypes = [_VP, ctypes.c_int]
        self.ctx._check(L.bzh_pk_workspace_select(self.handle, mode), "bzh_pk_workspace_select")

    def workspace_peak(self) -> int:
        """the most arena bytes the key's last call held at once (bzh_pk_workspace_peak): what workspace_plan estimates"""
        L = _bind()
        L.bzh_pk_workspace_peak.argtypes = [_VP, ctypes.POINTER(ctypes.c_size_t)]
        out = ctypes.c_size_t()
        self.ctx._check(L.bzh_pk_workspace_peak(self.handle, ctypes.byref(out)), "bzh_pk_workspace_peak")
        return out.value

    def workspace_plan(self, batch: int, mode: int | None = None) -> int:
        """arena bytes one prove call of `batch` proofs of this key's circuit takes (bzh2.workspace_plan), in `mode` or the
        key's current mode"""
        return workspace_plan(self.curve, self.blob, batch, self.workspace_selected() if mode is None else mode)

    # ---- where bzh_verify_batch decompresses the proofs' points ----------------------------------------------
    def verify_selected(self) -> int:
        """VERIFY_POINTS_HOST (inside the per-proof host pass) or VERIFY_POINTS_DEVICE (one k_decompress launch per batch)"""
        L = _bind()
        L.bzh_pk_verify_selected.argtypes = [_VP, ctypes.POINTER(ctypes.c_int)]
        w = ctypes.c_int()
        self.ctx._check(L.bzh_pk_verify_selected(self.handle, ctypes.byref(w)), "bzh_pk_verify_selected")
        return w.value

    def verify_select(self, where: int):
        L = _bind()
        L.bzh_pk_verify_select.argtypes = [_VP, ctypes.c_int]
        self.ctx._check(L.bzh_pk_verify_select(self.handle, where), "bzh_pk_verify_select")

    # ---- where bzh_verify_batch runs the per-proof pass ------------------------------------------------------
    def verify_pass_selected(self) -> int:
        """VERIFY_PASS_HOST (host threads, one proof each) or VERIFY_PASS_DEVICE (the key's scalar program, one lane per proof)"""
        w = ctypes.c_int()
        self.ctx._check(_bind().bzh_pk_verify_pass_selected(self.handle, ctypes.byref(w)), "bzh_pk_verify_pass_selected")
        return w.value

    def verify_pass_select(self, where: int):
        self.ctx._check(_bind().bzh_pk_verify_pass_select(self.handle, where), "bzh_pk_verify_pass_select")

    def compile_quotient(self, cache_dir: str | None = None) -> bool:
        """Make the key run its quotient program as compiled code.  The reference's circuits have a kernel inside libbzh2.so
        (generated at build time): selected, nothing to compile.  Any other circuit: quotient_source() through hipcc (a child
        process; ~5 s, cached on disk by the hash of the source), installed with set_quotient_module.  False (the interpreter
        stays) when there is neither a builtin kernel nor a working hipcc."""
        if self.quotient_selected()[1]:
            self.quotient_select(QUOTIENT_BUILTIN)
            return True
        try:
            src = self.quotient_source()
        except BzhError:
            return False          # the circuit does not fit the VM v2 evaluator
        for attempt in (0, 1):
            code = compile_quotient_source(src, cache_dir, use_cache=attempt == 0)
            if code is None:
                return False
            try:
                self.set_quotient_module(code)
                return True
            except BzhError:
                continue   # a stale or damaged cached code object: compile afresh once
        return False

    def set_lagrange(self, bases_lagrange):
        """Params::commit_lagrange for the columns upstream commits in the Lagrange basis (None: back to coefficients)."""
        self.ctx._check(_bind().bzh_pk_set_lagrange(self.handle, bases_lagrange.handle if bases_lagrange is not None else None),
                        "bzh_pk_set_lagrange")

    def device_bytes(self):
        """(key_bytes, workspace_bytes): device memory the key owns for its lifetime, and the per-ctx workspaces grown so far"""
        kb, wb = ctypes.c_size_t(), ctypes.c_size_t()
        self.ctx._check(_bind().bzh_pk_device_bytes(self.handle, ctypes.byref(kb), ctypes.byref(wb)), "bzh_pk_device_bytes")
        return kb.value, wb.value

    def close(self):
        """bzh_pk_free.  Refused (BzhError, the key stays open) while a prove / verify call on the key has started on any ctx and
        not returned -- also one that still waits for its ctx: the key's workspaces and code belong to every ctx that uses it.
        Once this has returned, no thread may start a call on the key."""
        if self.handle is not None:
            self.ctx._check(_bind().bzh_pk_free(self.ctx.handle, self.handle), "bzh_pk_free")
            self.handle = None
            if self._own_bases:
                self.bases.free()

    def _instances(self, instances):
        B = len(instances)
        rows = max([len(col) for cols in instances for col in cols] + [0])
        inst = np.zeros((B, max(len(instances[0]), 1), max(rows, 1), 4), dtype=np.uint64)
        for b, cols in enumerate(instances):
            for i, col in enumerate(cols):
                for r, v in enumerate(col):
                    inst[b, i, r] = int_to_limbs(int(v) % self.p)
        return inst, rows

    def verify_batch(self, instances, proofs, ctx: Context | None = None) -> list:
        """plonk::verify_proof for each (instances[b], proofs[b]); returns a list of bools.  ctx: the context (stream) to run on --
        the key is shared, read-only state; every ctx that uses it gets its own workspace inside the library."""
        L = _bind()
        ctx = ctx or self.ctx
        B = len(proofs)
        inst, rows = self._instances(instances)
        stride = max(max(len(pr) for pr in proofs), 1)
        buf = np.zeros((B, stride), dtype=np.uint8)
        lens = (ctypes.c_size_t * B)(*[len(pr) for pr in proofs])
        for b, pr in enumerate(proofs):
            buf[b, :len(pr)] = np.frombuffer(pr, dtype=np.uint8)
        res = (ctypes.c_int * B)()
        rc = L.bzh_verify_batch(ctx.handle, self.handle, B, _VP(inst.ctypes.data), rows, _VP(buf.ctypes.data), stride, lens,
                                _VP(self._g0_u_w.ctypes.data), res)
        ctx._check(rc, "bzh_verify_batch")
        return [bool(v) for v in res]

    def prove_batch(self, advice, instances, rng_list, device_ptr: int | None = None, seeds=None, ctx: Context | None = None) -> list:
        """advice: (B, num_advice, n, 4) uint64 canonical host array (or, with device_ptr, a device pointer to Montgomery
        limbs of that shape); instances: B lists of instance columns (equal lengths); rng_list: B byte strings of
        rng_bytes each -- or None with seeds = B 32-byte strings: the library expands each into its proof's stream on the
        device (bzh_prove_batch_seeded; the same proofs as rng_list = [rng_expand(s, 0, rng_bytes // 64) for s in seeds]).
        ctx: the context (device stream) to prove on, default the one the key was created through; several host threads may
        prove on ONE key concurrently, each through its own ctx."""
        L = _bind()
        ctx = ctx or self.ctx
        seeded = rng_list is None
        if seeded:
            assert seeds is not None and all(len(sd) == 32 for sd in seeds)
            rng_list = list(seeds)
        B = len(rng_list)
        stride = len(rng_list[0])
        assert all(len(r) == stride for r in rng_list) and (seeded or stride >= self.rng_bytes), (stride, self.rng_bytes)
        inst, rows = self._instances(instances)
        proofs = np.zeros((B, self.max_proof_bytes), dtype=np.uint8)
        lens = (ctypes.c_size_t * B)()
        if device_ptr is not None:
            adv_p, form, mem = _VP(device_ptr), FORM_MONTGOMERY, MEM_DEVICE
        else:
            a = np.ascontiguousarray(advice, dtype=np.uint64)
            assert a.shape == (B, self.num_advice, self.n, 4), a.shape
            adv_p, form, mem = _VP(a.ctypes.data), FORM_CANONICAL, MEM_HOST
        if seeded:
            rc = L.bzh_prove_batch_seeded(ctx.handle, self.handle, B, adv_p, form, mem, _VP(inst.ctypes.data), rows,
                                          b"".join(rng_list), _VP(proofs.ctypes.data), self.max_proof_bytes, lens)
        else:
            rc = L.bzh_prove_batch(ctx.handle, self.handle, B, adv_p, form, mem, _VP(inst.ctypes.data), rows, b"".join(rng_list), stride,
                                   _VP(proofs.ctypes.data), self.max_proof_bytes, lens)
        ctx._check(rc, "bzh_prove_batch")
        return [bytes(proofs[b, :lens[b]]) for b in range(B)]

    def prove_batch_device(self, advice, instances, rng_list=None, *, seeds=None, device_ptr: int | None = None,
                           rng_device_ptr: int | None = None, ctx: Context | None = None, want_status: bool = True,
                           batch: int | None = None, rng_stride: int | None = None, proof_stride: int | None = None):
        """prove_batch as the chain of the device-resident leaves in one call (bzh_prove_batch_device / _seeded): the same
        arguments, marshalled the same way, and (proofs, status) back -- status one byte per proof (bit 0 lookup, 1 grand product,
        2 degree check, 3 multiopen / opening), or None with want_status=False, when a flagged proof fails the whole batch with
        BZH_E_RANGE.  rng_device_ptr (with device_ptr): the draws already in device memory, rng_stride bytes apart (default
        rng_bytes), `batch` proofs.  proof_stride: room per proof in the result buffer, default max_proof_bytes."""
        L = _bind()
        ctx = ctx or self.ctx
        seeded = rng_list is None and rng_device_ptr is None
        if seeded:
            assert seeds is not None and all(len(sd) == 32 for sd in seeds)
            rng_list = list(seeds)
        if rng_device_ptr is not None:
            B = batch if batch is not None else len(instances)
            stride = self.rng_bytes if rng_stride is None else rng_stride
            rng_p = _VP(rng_device_ptr)
        else:
            B = batch if batch is not None else len(rng_list)
            stride = len(rng_list[0]) if rng_stride is None else rng_stride
            assert all(len(r) == len(rng_list[0]) for r in rng_list)
            raw = np.frombuffer(b"".join(rng_list), dtype=np.uint8)
            rng_p = _VP(raw.ctypes.data)
        inst, rows = self._instances(instances)
        pstride = self.max_proof_bytes if proof_stride is None else proof_stride
        proofs = np.zeros((B, max(pstride, 1)), dtype=np.uint8)
        lens = (ctypes.c_size_t * max(B, 1))()
        status = np.zeros(max(B, 1), dtype=np.uint8)
        st_p = _VP(status.ctypes.data) if want_status else None
        if device_ptr is not None:
            adv_p, form, mem = _VP(device_ptr), FORM_MONTGOMERY, MEM_DEVICE
        else:
            a = np.ascontiguousarray(advice, dtype=np.uint64)
            adv_p, form, mem = _VP(a.ctypes.data), FORM_CANONICAL, MEM_HOST
        if seeded:
            rc = L.bzh_prove_batch_device_seeded(ctx.handle, self.handle, B, adv_p, form, mem, _VP(inst.ctypes.data), rows, raw.tobytes(),
                                                 _VP(proofs.ctypes.data), pstride, lens, st_p)
        else:
            rc = L.bzh_prove_batch_device(ctx.handle, self.handle, B, adv_p, form, mem, _VP(inst.ctypes.data), rows, rng_p, stride,
                                          _VP(proofs.ctypes.data), pstride, lens, st_p)
        ctx._check(rc, "bzh_prove_batch_device")
        return [bytes(proofs[b, :lens[b]]) for b in range(B)], (status[:B].copy() if want_status else None)

    def _prove_game_device(self, layout, circuits, seeds, ctx, want_status, shot):
        from .circuits import _limbs
        L = _bind()
        ctx = ctx or self.ctx
        B = len(circuits)
        assert len(seeds) == B and all(len(sd) == 32 for sd in seeds)
        rows = layout.num_instance_rows
        inst = np.zeros((max(B, 1), max(rows, 1), 4), dtype=np.uint64)
        proofs = np.zeros((max(B, 1), max(self.max_proof_bytes, 1)), dtype=np.uint8)
        lens = (ctypes.c_size_t * max(B, 1))()
        status = np.zeros(max(B, 1), dtype=np.uint8)
        st_p = _VP(status.ctypes.data) if want_status else None
        boards = _limbs([c.board.value for c in circuits])
        traps = _limbs([c.board_commitment_trapdoor for c in circuits])
        tail = (b"".join(seeds), _VP(inst.ctypes.data), _VP(proofs.ctypes.data), self.max_proof_bytes, lens, st_p)
        if shot:
            shots, hits = _limbs([c.shot.value for c in circuits]), _limbs([c.hit.value for c in circuits])
            rc = L.bzh_prove_shots_device(ctx.handle, self.handle, layout.handle, B, _VP(boards.ctypes.data), _VP(traps.ctypes.data),
                                          _VP(shots.ctypes.data), _VP(hits.ctypes.data), *tail)
        else:
            ships = _limbs([s.value for c in circuits for s in c.ship_commitments])
            rc = L.bzh_prove_boards_device(ctx.handle, self.handle, layout.handle, B, _VP(ships.ctypes.data), _VP(boards.ctypes.data),
                                           _VP(traps.ctypes.data), *tail)
        ctx._check(rc, "bzh_prove_shots_device" if shot else "bzh_prove_boards_device")
        from . import limbs_to_int
        instances = [[[limbs_to_int(inst[b, r]) for r in range(rows)]] for b in range(B)]
        return instances, [bytes(proofs[b, :lens[b]]) for b in range(B)], (status[:B].copy() if want_status else None)

    def prove_shots_device(self, layout, circuits, seeds, ctx: Context | None = None, want_status: bool = True):
        """game inputs in, proofs out, in one device-resident call (bzh_prove_shots_device): `circuits` are bzh2.circuits.ShotCircuit,
        `layout` the Shot CircuitLayout this key was made from, `seeds` 32 bytes per proof (the SECURITY note of prove_batch's seeds
        holds).  Returns (instances, proofs, status): the instances as CircuitLayout.synthesize returns them, the proofs
        byte-identical to layout.synthesize(where="device") followed by prove_batch_device(seeds=...), status one byte per proof
        -- bits 0 .. 3 as prove_batch_device's, bits 4 .. 6 the synthesis status (exceptional addition, window point with x = 0,
        non-canonical message) -- or None with want_status=False, when a flagged proof fails the whole batch with BZH_E_RANGE."""
        return self._prove_game_device(layout, circuits, seeds, ctx, want_status, True)

    def prove_boards_device(self, layout, circuits, seeds, ctx: Context | None = None, want_status: bool = True):
        """prove_shots_device for bzh2.circuits.BoardCircuit and the Board layout (bzh_prove_boards_device)"""
        return self._prove_game_device(layout, circuits, seeds, ctx, want_status, False)


def _check(rc: int, where: str):
    if rc:
        raise BzhError(rc, where)


def _g0_u_w(params):
    gp, _, wp, up, _ = params.points(want_lagrange=False)
    return np.ascontiguousarray(np.stack([gp[0], np.concatenate([int_to_limbs(up[0]), int_to_limbs(up[1])]),
                                          np.concatenate([int_to_limbs(wp[0]), int_to_limbs(wp[1])])]))


class NativeVerifyingKey:
    """keygen_vk / pk.get_vk() / VerifyingKey::{write, read} (bzh_vk): host memory only, tied to no ctx and no device.  Make one
    with create, from_pk or from_bytes; verify_batch takes the ctx and the SRS it runs against."""

    def __init__(self, handle):
        self.handle = handle
        self.p = MODULI[CURVE_SCALAR_FIELD[self.info()["curve"]]]

    @classmethod
    def create(cls, ctx: Context, params_or_bases, blob: bytes) -> "NativeVerifyingKey":
        """keygen_vk for a circuit blob against an SRS: a bzh2.params.Params, or a Bases table (g | u | w) with its window table"""
        bases = getattr(params_or_bases, "bases", params_or_bases)
        h = _VP()
        ctx._check(_bind().bzh_vk_create(ctx.handle, bases.handle, bytes(blob), len(blob), ctypes.byref(h)), "bzh_vk_create")
        return cls(h)

    @classmethod
    def from_pk(cls, pk: NativeProvingKey, ctx: Context | None = None) -> "NativeVerifyingKey":
        ctx = ctx or pk.ctx
        h = _VP()
        ctx._check(_bind().bzh_vk_from_pk(ctx.handle, pk.handle, ctypes.byref(h)), "bzh_vk_from_pk")
        return cls(h)

    @classmethod
    def from_bytes(cls, b: bytes) -> "NativeVerifyingKey":
        """bzh_vk_read: host only; BzhError E_ARG / E_RANGE for anything but a well-formed "BZV1" key"""
        h = _VP()
        _check(_bind().bzh_vk_read(bytes(b), len(b), ctypes.byref(h)), "bzh_vk_read")
        return cls(h)

    def to_bytes(self) -> bytes:
        L = _bind()
        n = ctypes.c_size_t()
        _check(L.bzh_vk_write(self.handle, None, 0, ctypes.byref(n)), "bzh_vk_write")
        buf = (ctypes.c_uint8 * n.value)()
        _check(L.bzh_vk_write(self.handle, buf, n.value, ctypes.byref(n)), "bzh_vk_write")
        return bytes(buf)

    def info(self) -> dict:
        curve, k, mp = ctypes.c_int(), ctypes.c_uint(), ctypes.c_size_t()
        ni, nf, npm = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32()
        _check(_bind().bzh_vk_info(self.handle, ctypes.byref(curve), ctypes.byref(k), ctypes.byref(ni), ctypes.byref(nf), ctypes.byref(npm),
                                   ctypes.byref(mp)), "bzh_vk_info")
        return {"curve": curve.value, "k": k.value, "num_instance": ni.value, "num_fixed_commitments": nf.value,
                "num_permutation_commitments": npm.value, "max_proof_bytes": mp.value}

    def vk_repr(self):
        """(the verifying-key digest the key absorbs first, whether it is still the library's placeholder)"""
        out, ph = (ctypes.c_uint8 * 32)(), ctypes.c_int()
        _check(_bind().bzh_vk_vk_repr(self.handle, out, ctypes.byref(ph)), "bzh_vk_vk_repr")
        return int.from_bytes(bytes(out), "little"), bool(ph.value)

    def device_bytes(self):
        """(key_bytes, workspace_bytes): see NativeProvingKey.device_bytes; key_bytes is 0 for a verifying key"""
        kb, wb = ctypes.c_size_t(), ctypes.c_size_t()
        _check(_bind().bzh_vk_device_bytes(self.handle, ctypes.byref(kb), ctypes.byref(wb)), "bzh_vk_device_bytes")
        return kb.value, wb.value

    def verify_batch(self, ctx: Context, params, instances, proofs, lagrange: bool = True, g0_u_w=None, pass_where: int | None = None) -> list:
        """plonk::verify_proof(&params, &vk, ..) for each (instances[b], proofs[b]); returns a list of bools.  params: a
        bzh2.params.Params -- with lagrange its g_lagrange table commits the instance columns -- or a Bases table (g | u | w)
        together with g0_u_w (3 x 8 canonical limbs).  pass_where: VERIFY_PASS_HOST / VERIFY_PASS_DEVICE through
        bzh_verify_batch_vk_with; None: bzh_verify_batch_vk."""
        L = _bind()
        bases = getattr(params, "bases", params)
        lag = getattr(params, "bases_lagrange", None) if lagrange else None
        g0 = np.ascontiguousarray(g0_u_w, dtype=np.uint64) if g0_u_w is not None else _g0_u_w(params)
        B = len(proofs)
        inst, rows = NativeProvingKey._instances(self, instances)
        stride = max(max(len(pr) for pr in proofs), 1)
        buf = np.zeros((B, stride), dtype=np.uint8)
        lens = (ctypes.c_size_t * B)(*[len(pr) for pr in proofs])
        for b, pr in enumerate(proofs):
            buf[b, :len(pr)] = np.frombuffer(pr, dtype=np.uint8)
        res = (ctypes.c_int * B)()
        lagh = lag.handle if lag is not None else None
        if pass_where is None:
            rc = L.bzh_verify_batch_vk(ctx.handle, self.handle, bases.handle, lagh, B, _VP(inst.ctypes.data), rows, _VP(buf.ctypes.data), stride,
                                       lens, _VP(g0.ctypes.data), res)
        else:
            rc = L.bzh_verify_batch_vk_with(ctx.handle, self.handle, bases.handle, lagh, pass_where, B, _VP(inst.ctypes.data), rows,
                                            _VP(buf.ctypes.data), stride, lens, _VP(g0.ctypes.data), res)
        ctx._check(rc, "bzh_verify_batch_vk")
        return [bool(v) for v in res]

    def verify_records(self, ctx: Context, params, records, n_inputs: int, g0_u_w=None, want_status: bool = True, record_stride: int | None = None):
        """verify_board / verify_shot for a batch of binary records in one device-resident call (bzh_verify_records_device).
        records: equal-length byte strings in the layout of bzh2.wire.Record.encode (or one contiguous uint8 array of
        len(records) rows); n_inputs: 4 for Shot, 2 for Board; params: a bzh2.params.Params -- its g_lagrange table commits the
        inputs.  g0_u_w (3 x 8 canonical limbs): checked against the SRS on the device when given; None: not checked, G_0 U W are
        the SRS table's.  Returns (results, status): a list of bools, and one byte per record -- bit 0: refused before
        verification (corrupt header, another n_inputs, another proof length, a non-canonical input) -- or None with
        want_status=False."""
        L = _bind()
        bases = getattr(params, "bases", params)
        lag = getattr(params, "bases_lagrange", None)
        B = len(records)
        buf = np.ascontiguousarray(np.frombuffer(b"".join(bytes(r) for r in records), dtype=np.uint8)) if B else np.zeros(1, dtype=np.uint8)
        stride = record_stride if record_stride is not None else (len(records[0]) if B else 0)
        assert all(len(r) == stride for r in records) or record_stride is not None
        g0 = np.ascontiguousarray(g0_u_w, dtype=np.uint64) if g0_u_w is not None else None
        res = (ctypes.c_int * max(B, 1))()
        status = np.zeros(max(B, 1), dtype=np.uint8)
        rc = L.bzh_verify_records_device(ctx.handle, self.handle, bases.handle, lag.handle if lag is not None else None, B, n_inputs,
                                         _VP(buf.ctypes.data), stride, _VP(g0.ctypes.data) if g0 is not None else None, res,
                                         _VP(status.ctypes.data) if want_status else None)
        ctx._check(rc, "bzh_verify_records_device")
        return [bool(res[b]) for b in range(B)], (status[:B].copy() if want_status else None)

    def verify_records_accumulated(self, ctx: Context, params, records, n_inputs: int, seed: bytes | None = None, g0_u_w=None,
                                   record_stride: int | None = None):
        """verify_records with ONE accumulated opening check for the batch (bzh_verify_records_accumulated).  seed: 32 bytes that
        the records' authors cannot predict, fresh per call; None draws os.urandom(32).  Returns (results, status, path): results
        and status as verify_records returns them; path 0: the accumulated check accepted the included records, 1: it did not and
        the per-record check ran as well."""
        import os
        L = _bind()
        bases = getattr(params, "bases", params)
        lag = getattr(params, "bases_lagrange", None)
        B = len(records)
        buf = np.ascontiguousarray(np.frombuffer(b"".join(bytes(r) for r in records), dtype=np.uint8)) if B else np.zeros(1, dtype=np.uint8)
        stride = record_stride if record_stride is not None else (len(records[0]) if B else 0)
        assert all(len(r) == stride for r in records) or record_stride is not None
        g0 = np.ascontiguousarray(g0_u_w, dtype=np.uint64) if g0_u_w is not None else None
        seed = os.urandom(32) if seed is None else bytes(seed)
        assert len(seed) == 32
        res = (ctypes.c_int * max(B, 1))()
        status = np.zeros(max(B, 1), dtype=np.uint8)
        path = ctypes.c_int(0)
        rc = L.bzh_verify_records_accumulated(ctx.handle, self.handle, bases.handle, lag.handle if lag is not None else None, B, n_inputs,
                                              _VP(buf.ctypes.data), stride, _VP(g0.ctypes.data) if g0 is not None else None, seed, res,
                                              _VP(status.ctypes.data), ctypes.byref(path))
        ctx._check(rc, "bzh_verify_records_accumulated")
        return [bool(res[b]) for b in range(B)], status[:B].copy(), path.value

    def verify_batch_accumulated(self, ctx: Context, params, instances, proofs, seed: bytes | None = None, lagrange: bool = True, g0_u_w=None):
        """verify_batch under the device pass with ONE accumulated opening check (bzh_verify_batch_vk_accumulated); seed as in
        verify_records_accumulated.  Returns (results, path)."""
        import os
        L = _bind()
        bases = getattr(params, "bases", params)
        lag = getattr(params, "bases_lagrange", None) if lagrange else None
        g0 = np.ascontiguousarray(g0_u_w, dtype=np.uint64) if g0_u_w is not None else _g0_u_w(params)
        B = len(proofs)
        inst, rows = NativeProvingKey._instances(self, instances)
        stride = max(max(len(pr) for pr in proofs), 1)
        buf = np.zeros((B, stride), dtype=np.uint8)
        lens = (ctypes.c_size_t * B)(*[len(pr) for pr in proofs])
        for b, pr in enumerate(proofs):
            buf[b, :len(pr)] = np.frombuffer(pr, dtype=np.uint8)
        seed = os.urandom(32) if seed is None else bytes(seed)
        assert len(seed) == 32
        res = (ctypes.c_int * B)()
        path = ctypes.c_int(0)
        rc = L.bzh_verify_batch_vk_accumulated(ctx.handle, self.handle, bases.handle, lag.handle if lag is not None else None, B,
                                               _VP(inst.ctypes.data), rows, _VP(buf.ctypes.data), stride, lens, _VP(g0.ctypes.data), seed, res,
                                               ctypes.byref(path))
        ctx._check(rc, "bzh_verify_batch_vk_accumulated")
        return [bool(v) for v in res], path.value

    def close(self):
        """bzh_vk_free.  Refused (BzhError, the key stays open) while a verify_batch on the key has started on any ctx and not
        returned -- also one that still waits for its ctx.  Once this has returned, no thread may start a call on the key."""
        if self.handle is not None:
            _check(_bind().bzh_vk_free(self.handle), "bzh_vk_free")
            self.handle = None
