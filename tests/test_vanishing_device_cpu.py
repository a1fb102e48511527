"""The vanishing argument on device-resident transcripts (bzh_vanishing_plan, bzh_vanishing_batch_device) without a device: the
header / exports agreement for the two names, the plan against the quotient program and the oracle's constraint system, the
argument refusals that need no device, and the lane body (csrc/vanishing_scalars.hpp) run lane by lane on the host against
fe_mul / h_pow_u64 (tests/helpers/vanishing_scalars_check.hip, a stand-alone program under the host's address and
undefined-behaviour sanitizers)."""
import ctypes
import os
import random
import re
import shutil
import subprocess

import numpy as np
import pytest

import halo2_oracle as H
import pasta as O
import sample_circuit as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("bzh_vanishing_plan", "bzh_vanishing_batch_device")
E_ARG, E_RANGE = -1, -4
SY_BD0, SY_YPOW0 = 8, 4096                    # csrc/expr_compiler.hpp, csrc/quotient_compiler.hpp
CONST_DTYPE = np.dtype([("sym", "<i4"), ("pad", "<u4"), ("val", "<u4", (8,))])   # bzh_quotient_program_for_circuit's constants
F = O.FP


def test_header_and_exports_name_the_entry_points():
    import bzh2
    header = open(os.path.join(ROOT, "include", "bzh2.h")).read()
    for name in NAMES:
        assert re.search(r"\bint %s\(" % name, header) and name in bzh2.EXPORTS
        getattr(bzh2.load(), name)
    assert header.index("int bzh_evaluations_batch_device(") < header.index("int bzh_vanishing_plan(") < header.index("int bzh_vanishing_batch_device(")
    assert re.search(r"typedef struct \{\s*int32_t challenge;[^}]*uint32_t exponent;\s*uint32_t value\[8\];[^}]*\} bzh_vanishing_const;", header)
    assert hasattr(bzh2.TranscriptBatch, "vanishing") and callable(bzh2.vanishing_plan)


def _blobs():
    """(name, blob, the oracle's ConstraintSystem): the reference's two circuits and the sample circuit with and without a lookup"""
    import blob as Bm
    from bzh2 import circuit_data as P, circuits as Cm
    out = []
    for name, kind, k in (("shot", Cm.SHOT, 11), ("board", Cm.BOARD, 12)):
        lay = Cm.CircuitLayout(kind, k)
        blob = lay.blob()
        lay.close()
        c = Bm.decode(blob)
        cs = H.ConstraintSystem(c.k, c.num_advice, c.num_fixed, c.num_instance, c.gates, c.perm_columns, c.lookups, degree=c.min_degree,
                                queries=c.queries)
        out.append((name, blob, cs))
    for with_lookup in (False, True):
        # (k = 6 without a lookup: degree 3 extends the domain twofold, and VM v2 needs 128 rows)
        cs, fixed, copies, _, _ = S.build(k=5 if with_lookup else 6, seed=3, with_lookup=with_lookup)
        circ = P.Circuit(cs.k, cs.num_advice, cs.num_fixed, cs.num_instance, cs.gates, cs.perm_columns, cs.lookups, fixed, copies)
        out.append(("sample%d" % with_lookup, P.serialize_circuit(circ, F.p, 0x1234), cs))
    return out


def _program_consts(L, blob):
    vp, sz = ctypes.c_void_p, ctypes.c_size_t
    L.bzh_quotient_program_for_circuit.argtypes = [ctypes.c_int, ctypes.c_char_p, sz, vp, sz, ctypes.POINTER(sz), vp, sz, ctypes.POINTER(sz),
                                                   ctypes.POINTER(ctypes.c_uint32)]
    nops, nc = sz(), sz()
    assert L.bzh_quotient_program_for_circuit(0, blob, len(blob), None, 0, ctypes.byref(nops), None, 0, ctypes.byref(nc), None) == 0
    consts = np.zeros(nc.value, CONST_DTYPE)
    assert L.bzh_quotient_program_for_circuit(0, blob, len(blob), None, 0, ctypes.byref(nops), consts.ctypes.data, consts.nbytes,
                                              ctypes.byref(nc), None) == 0
    return consts


def test_plan_against_the_program_and_the_constraint_system():
    """shape8 is the oracle ConstraintSystem's numbers; every descriptor is the program's {symbol, value} entry, literals bit for
    bit and symbols mapped as the header says, delta^j against Domain.delta; evaluated at seeded theta, beta, gamma, y the
    descriptors give what Prover::vanishing puts into env: the challenges, y^m for m <= 64 and beta * delta^j"""
    import bzh2
    L = bzh2.load()
    p, R = F.p, F.R
    rng = random.Random(20262)
    for name, blob, cs in _blobs():
        shape, consts = bzh2.vanishing_plan(bzh2.CURVE_VESTA, blob)
        dom = H.Domain(cs, F)
        nsets = (len(cs.perm_columns) + cs.chunk_len - 1) // cs.chunk_len if cs.perm_columns else 0
        npieces = cs.degree - 1
        assert shape == (cs.n, dom.en, cs.num_advice, cs.num_instance, nsets + len(cs.lookups), len(cs.lookups), npieces,
                         cs.n + 1 + npieces), name
        prog = _program_consts(L, blob)
        assert len(consts) == len(prog), name
        ch = [rng.randrange(p) for _ in range(4)]                      # theta, beta, gamma, y
        env = {i: ch[i] for i in range(4)}
        for m in range(2, 65):
            env[SY_YPOW0 + m] = pow(ch[3], m, p)
        for j in range(len(cs.perm_columns)):
            env[SY_BD0 + j] = ch[1] * pow(dom.delta, j, p) % p
        seen = set()
        for (c, e, v), ent in zip(consts, prog):
            sym, lit = int(ent["sym"]), sum(int(w) << (32 * i) for i, w in enumerate(ent["val"]))
            if sym < 0:
                assert (c, v) == (-1, lit), name                        # a literal, bit for bit
                continue
            seen.add(sym)
            if sym < 4:
                assert (c, e, v) == (sym, 1, R % p), name
            elif sym >= SY_YPOW0:
                assert (c, e, v) == (3, sym - SY_YPOW0, R % p) and e <= 64, name
            else:
                assert (c, e, v) == (1, 1, pow(dom.delta, sym - SY_BD0, p) * R % p), name
            assert v * pow(R, -1, p) * pow(ch[c], e, p) % p == env[sym], (name, sym)
        assert {1, 2, 3}.issubset(seen) and any(SY_BD0 <= s < SY_YPOW0 for s in seen), name   # beta, gamma, y and a beta * delta^j


def test_plan_refusals():
    import bzh2
    L = bzh2.load()
    vp, sz = ctypes.c_void_p, ctypes.c_size_t
    L.bzh_vanishing_plan.argtypes = [ctypes.c_int, ctypes.c_char_p, sz, vp, vp, sz, ctypes.POINTER(sz)]
    blob = _blobs()[3][1]
    nc = len(bzh2.vanishing_plan(bzh2.CURVE_VESTA, blob)[1])
    shape = np.full(8, 5, dtype=np.uint32)
    consts = np.full(nc * 10, 5, dtype=np.uint32)
    got = sz(5)
    args = [0, blob, len(blob), vp(shape.ctypes.data), vp(consts.ctypes.data), nc, ctypes.byref(got)]
    untouched = lambda: got.value == 5 and (shape == 5).all() and (consts == 5).all()   # noqa: E731
    for i in (1, 3, 4, 6):                                              # each pointer in turn NULL
        a = list(args)
        a[i] = None
        assert L.bzh_vanishing_plan(*a) == E_ARG and untouched()
    a = list(args)
    a[5] = nc - 1                                                       # capacity one short
    assert L.bzh_vanishing_plan(*a) == E_ARG and untouched()
    a = list(args)
    a[2] = len(blob) // 2                                               # a truncated blob
    assert L.bzh_vanishing_plan(*a) == E_ARG and untouched()
    a = list(args)
    a[0] = 7                                                            # no such curve
    assert L.bzh_vanishing_plan(*a) == E_ARG and untouched()
    assert L.bzh_vanishing_plan(*args) == 0 and got.value == nc and shape[0] == 32


def test_argument_refusals_without_a_device():
    """every refusal that needs no device, on made-up non-NULL handles that a refusal must not read through; a host-resident batch is
    left as it was and the output arrays are untouched"""
    import bzh2
    L = bzh2.load()
    vp, sz, ci = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
    L.bzh_vanishing_batch_device.argtypes = [vp, vp, sz, vp, vp, vp, vp, vp, vp, vp, ci, ci, vp, sz, vp, vp, vp, vp, vp, vp]
    B, n = 2, 4
    ops = [np.zeros((B, 1, n, 4), dtype=np.uint64) for _ in range(4)]
    chs = [np.zeros((B, 4), dtype=np.uint64) for _ in range(3)]
    raw = np.zeros(B * 64 * 16, dtype=np.uint8)
    outs = [np.full((B, m, 4), 7, dtype=np.uint64) for m in (n, 1, 2 * n, 2)]
    st = np.full(B, 7, dtype=np.uint8)
    fake = vp(0x1000)
    with bzh2.TranscriptBatch(bzh2.CURVE_VESTA, B, 256) as tb, bzh2.TranscriptBatch(bzh2.CURVE_VESTA, B, 256) as twin:   # host-resident

        def call(**kw):
            a = dict(ctx=fake, pk=fake, batch=B, adv=vp(ops[0].ctypes.data), inst=vp(ops[1].ctypes.data), lk=vp(ops[2].ctypes.data),
                     z=vp(ops[3].ctypes.data), theta=vp(chs[0].ctypes.data), beta=vp(chs[1].ctypes.data), gamma=vp(chs[2].ctypes.data),
                     form=bzh2.FORM_CANONICAL, mem=bzh2.MEM_HOST, rng=vp(raw.ctypes.data), stride=64 * 16, trs=tb.h,
                     o0=vp(outs[0].ctypes.data), o1=vp(outs[1].ctypes.data), o2=vp(outs[2].ctypes.data), o3=vp(outs[3].ctypes.data),
                     st=vp(st.ctypes.data))
            a.update(kw)
            return L.bzh_vanishing_batch_device(*a.values())

        assert call() == E_ARG                                   # a host-resident batch: the made-up ctx and key are not read
        for kw in (dict(ctx=None), dict(pk=None), dict(trs=None), dict(rng=None), dict(theta=None), dict(beta=None), dict(gamma=None),
                   dict(o0=None), dict(o1=None), dict(o2=None), dict(o3=None), dict(adv=None), dict(inst=None), dict(lk=None), dict(z=None),
                   dict(batch=0), dict(batch=65536), dict(form=2), dict(mem=2)):
            assert call(**kw) == E_ARG, kw
        with pytest.raises(bzh2.BzhError) as e:                  # the Python mirror on a host-resident batch: refused the same way
            tb.vanishing(fake, ops[0], ops[1], ops[2], ops[3], chs[0], chs[1], chs[2], [bytes(64 * 16)] * B, shape=(n, 2 * n, 1, 1, 1, 1, 2, 7))
        assert e.value.status == E_ARG
        assert all((o == 7).all() for o in outs) and (st == 7).all() and tb.proof_len() == 0
        assert (tb.squeeze() == twin.squeeze()).all()   # the batch is as it was


def test_lane_body_against_the_host_arithmetic_standalone_under_host_sanitizers(tmp_path):
    """vn_const_lane against fe_mul / h_pow_u64, word for word, for Fp and Fq, both operand forms and both table formats (the fe29
    slot against fe29_from_sat_reduced of the host result); exponents 0, 1, 2, 63, 64; challenges random, 0, 1 and p - 1; literals"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    csrc = os.path.join(ROOT, "battlezips-halo2_amd", "csrc")
    exe = str(tmp_path / "vanishing_scalars_check")
    subprocess.check_call([hipcc, "-O1", "-g", "-std=c++17", "--offload-arch=gfx950", "-Wno-unused-function",
                           "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                           "-I", csrc, os.path.join(ROOT, "tests", "helpers", "vanishing_scalars_check.hip"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(out.stdout[-3000:])
    assert out.returncode == 0 and out.stdout.strip().endswith("vanishing_scalars_check: ok"), out.stdout[-3000:] + out.stderr[-3000:]
    # per run: 4 proofs x (4 challenges x 5 exponents + beta * value + 2 literals); 2 forms x 2 table formats x 2 fields
    assert int(re.search(r"(\d+) lanes", out.stdout).group(1)) == 4 * 23 * 8
