"""bzh_prove_batch_device / bzh_prove_batch_device_seeded on the GPU: the five device-resident leaves as ONE call must give, proof
for proof and byte for byte, the oracle prover's proofs and bzh_prove_batch's, report failures per proof, and refuse what
bzh_prove_batch refuses with everything left as it was.  Every comparison is exact.

The vanishing leaf needs the key's VM v2 quotient program and an extended domain of at least one 128-row workgroup
(bzh_vanishing_batch_device), so a degree-3 circuit -- the sample circuit without its lookup -- enters the call from k = 6 on
(en = 2 n = 128): the circuit without instance column and lookup (ni = 0, nl = 0) runs at k = 6, and its k = 4 key is the
BZH_E_RANGE refusal of test_refusals_leave_everything_as_it_was.  The k = 4 cases run the circuit with its lookup at min_degree 6
(en = 8 n = 128; at its own degree 5 the extended domain is 4 n = 64 rows)."""
import numpy as np
import pytest

import pasta as O
import sample_circuit as S
from helpers import commitments_cases as K
from helpers import vanishing_cases as V
from helpers.real_parity import accelerated_oracle

pytestmark = pytest.mark.gpu

E_ARG, E_RANGE = -1, -4
F = O.FP
P = F.p
MONT = lambda x: x * F.R % P          # noqa: E731


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64).copy()).to("cuda")


def make_key(ctx, case):
    import bzh2
    from bzh2 import native as N
    return N.NativeProvingKey(ctx, case[2], bzh2.CURVE_VESTA, *case[3])


def operands(pk, bounds):
    """(canonical advice array, instances as lists, one draw stream of rng_bytes per proof) of a case's captured proofs"""
    adv, _ = K.operand_arrays(bounds, pk.n)
    streams = [s.v.rbytes[:pk.rng_bytes] for s in bounds]
    assert all(len(s) == pk.rng_bytes for s in streams)
    return adv, [s.instance for s in bounds], streams


def against_prove_batch(ctx, case, lagrange=None):
    """the one call against bzh_prove_batch on the same key, witness and draws; returns the proofs"""
    bounds = case[4]
    B = len(bounds)
    pk = make_key(ctx, case)
    try:
        if lagrange is not None:
            pk.set_lagrange(lagrange)
        assert pk.prove_device_plan()[4] * 64 == pk.rng_bytes and pk.prove_device_plan()[5] == len(case[5][0])
        adv, insts, streams = operands(pk, bounds)
        got, st = pk.prove_batch_device(adv, insts, streams)
        assert not st.any()
        assert got == pk.prove_batch(adv, insts, streams)
        assert pk.verify_batch(insts, got) == [True] * B
        pk.set_lagrange(None)
        return got
    finally:
        pk.close()


@accelerated_oracle
def test_parity_with_the_oracle_and_prove_batch(gpu_ctx, oracle_c):
    """k = 5 with the lookup, B = 3.  Host operands in canonical form: proofs and lengths are the oracle's, equal pk.prove_batch's
    on the same key and draws, verify, status all zero.  The same with Montgomery device operands and the draws in device memory
    (a stride above the stream's length)."""
    case = K.case(5, True, None, 3)
    bounds, proofs = case[4], case[5]
    B = 3
    pk = make_key(gpu_ctx, case)
    try:
        adv, insts, streams = operands(pk, bounds)
        got, st = pk.prove_batch_device(adv, insts, streams)
        assert st.tolist() == [0] * B
        for b in range(B):
            assert len(got[b]) == len(proofs[b]) and got[b] == proofs[b], "proof %d against the oracle" % b
        assert got == pk.prove_batch(adv, insts, streams)
        assert pk.verify_batch(insts, got) == [True] * B
        adv_m, _ = K.operand_arrays(bounds, pk.n, MONT)
        d_adv = dev(adv_m)
        stride = pk.rng_bytes + 64
        d_rng = dev(np.frombuffer(b"".join(s + bytes(64) for s in streams), dtype=np.uint8).view(np.uint64))
        got_d, st_d = pk.prove_batch_device(None, insts, device_ptr=d_adv.data_ptr(), rng_device_ptr=d_rng.data_ptr(), rng_stride=stride)
        assert got_d == got and st_d.tolist() == [0] * B
        got_h, _ = pk.prove_batch_device(None, insts, streams, device_ptr=d_adv.data_ptr())      # device advice, host draws
        assert got_h == got
    finally:
        pk.close()


@pytest.mark.parametrize("which", ["no_instance_k6", "two_column", "degree6", "single"])
@accelerated_oracle
def test_shapes_that_move_the_tables(gpu_ctx, oracle_c, which):
    """the circuit without instance column and lookup (ni = 0, nl = 0: empty runs in the blind table and the source table); the
    two-column lookup with a rotation; min_degree 6 (another npieces: 5 pieces in a row of 8 n, copied side by side); B = 1"""
    case = {"no_instance_k6": lambda: K.no_instance_case(6, 2), "two_column": lambda: K.two_column_case(), "degree6": lambda: K.case(5, True, 6, 3),
            "single": lambda: K.case(5, True, None, 3)}[which]()
    if which == "single":
        case = case[:4] + (case[4][:1], case[5][:1], case[6][:1])
    got = against_prove_batch(gpu_ctx, case)
    assert got == list(case[5])                               # (the oracle's proofs come with the case)


def _many(k, B):
    """B witnesses of the sample circuit with its lookup, as (advice array, instances)"""
    adv, insts = [], []
    for b in range(B):
        _, _, _, a, inst = S.build(k=k, seed=5000 + 3 * b, with_lookup=True)
        adv.append(np.stack([V.lim((list(c) + [0] * (1 << k))[:1 << k]) for c in a]))
        insts.append(inst)
    return np.stack(adv), insts


@accelerated_oracle
def test_more_proofs_than_a_wave(gpu_ctx, oracle_c):
    """B = 65 at k = 4: the lane kernels take a second workgroup.  Against the host path, which verifies them"""
    import random
    case = K.case(4, True, 6, 1)
    B = 65
    pk = make_key(gpu_ctx, case)
    try:
        adv, insts = _many(4, B)
        rng = random.Random(65)
        streams = [bytes(rng.getrandbits(8) for _ in range(pk.rng_bytes)) for _ in range(B)]
        got, st = pk.prove_batch_device(adv, insts, streams)
        assert not st.any() and got == pk.prove_batch(adv, insts, streams)
        assert pk.verify_batch(insts, got) == [True] * B
    finally:
        pk.close()


@pytest.mark.parametrize("k,B", [(5, 3), (4, 2)])
@accelerated_oracle
def test_a_key_with_g_lagrange_gives_the_same_bytes(gpu_ctx, oracle_c, k, B):
    """with bzh_pk_set_lagrange every witness commitment and the grand products' are made against g_lagrange (the products' rows
    are dense) -- the same bytes as without, and as bzh_prove_batch's"""
    from test_gpu_commitments_device import _Lagrange
    case = K.case(k, True, 6 if k == 4 else None, B)
    lag = _Lagrange(gpu_ctx, case)
    try:
        plain = against_prove_batch(gpu_ctx, case)
        with_table = against_prove_batch(gpu_ctx, case, lag.bases)
        assert plain == with_table == list(case[5])
    finally:
        lag.bases.free()


@accelerated_oracle
def test_seeded(gpu_ctx, oracle_c):
    """bzh_prove_batch_device_seeded equals bzh_prove_batch_seeded on the same seeds, and bzh_prove_batch_device fed with
    bzh_rng_expand"""
    from bzh2 import native as N
    case = K.case(5, True, None, 3)
    pk = make_key(gpu_ctx, case)
    try:
        adv, insts, _ = operands(pk, case[4])
        seeds = [bytes([17 * b + i for i in range(32)]) for b in range(3)]
        got, st = pk.prove_batch_device(adv, insts, seeds=seeds)
        assert not st.any()
        assert got == pk.prove_batch(adv, insts, None, seeds=seeds)
        expanded = [N.rng_expand(s, 0, pk.rng_bytes // 64) for s in seeds]
        assert got == pk.prove_batch_device(adv, insts, expanded)[0]
        assert pk.verify_batch(insts, got) == [True] * 3
    finally:
        pk.close()


def _broken(case, what):
    """proof 1's witness broken so that exactly one leaf flags it (sample_circuit.build): (advice columns per proof, instances)"""
    cs, keys, bounds = case[0], case[1], case[4]
    advice = [[list(c) + [0] * (cs.n - len(c)) for c in b.advice] for b in bounds]
    insts = [[list(c) for c in b.instance] for b in bounds]
    nb = max(1, min(3, cs.usable_rows - 4))
    if what == "lookup":
        # the recomposed value, its copy in the looked-up cell and its copy in the instance all become a value the table (0 .. 7)
        # does not hold: every copy constraint still holds, the lookup input is not in its table
        rows = [r for r in range(cs.usable_rows) if keys.fixed[3][r]]
        assert rows == [nb + 2]
        advice[1][2][nb] = advice[1][0][nb + 2] = insts[1][0][0] = 1 << 40
    elif what == "copy":
        advice[1][2][nb] = (advice[1][2][nb] + 1) % P         # copied to advice 0 and the instance: both constraints break
    else:
        assert keys.fixed[0][nb + 1] == 1                     # the multiplication row: a0 * a1 = a2 no longer holds; no copy, no lookup
        advice[1][0][nb + 1] = (advice[1][0][nb + 1] + 1) % P
    return advice, insts


@pytest.mark.parametrize("what,degree,bit", [("lookup", None, 1), ("copy", None, 2), ("gate", 6, 4)])
@accelerated_oracle
def test_one_bad_proof_in_a_batch(gpu_ctx, oracle_c, what, degree, bit):
    """B = 3, k = 5, a witness broken in proof 1 only.  With `status`: BZH_OK, status[1] is exactly the expected bit, status[0] ==
    status[2] == 0, proofs 0 and 2 are the all-good run's, verify_batch says [True, False, True].  With status=None the same batch
    is BZH_E_RANGE and the next call on the key gives the good proofs.  The broken gate runs at min_degree 6, where coefficients
    above npieces * n exist and k_vn_degree runs (at degrees 3, 5 and 9 the pieces fill the extended domain and bit 2 cannot be
    set: there the gate broken by the "copy" and "lookup" cases goes unnoticed by the prover and is left to the verifier).

    The "lookup" case leaves every copy constraint intact (the changed value is written to every cell of its cycle), and the
    device permutation keeps a failed pair's columns permutations of the compressed ones, so the lookup's own grand product
    closes and bit 0 stands alone."""
    import bzh2
    case = K.case(5, True, degree, 3)
    bounds = case[4]
    pk = make_key(gpu_ctx, case)
    try:
        adv, insts, streams = operands(pk, bounds)
        good, st = pk.prove_batch_device(adv, insts, streams)
        assert not st.any() and good == list(case[5])
        advice, bad_insts = _broken(case, what)
        bad_adv, _ = K.operand_arrays(bounds, pk.n, advice=advice)
        got, st = pk.prove_batch_device(bad_adv, bad_insts, streams)
        print("status", st.tolist())
        assert st.tolist() == [0, bit, 0]
        assert got[0] == good[0] and got[2] == good[2] and len(got[1]) == len(good[1]) and got[1] != good[1]
        assert pk.verify_batch(bad_insts, got) == [True, False, True]
        with pytest.raises(bzh2.BzhError) as e:
            pk.prove_batch_device(bad_adv, bad_insts, streams, want_status=False)
        assert e.value.status == E_RANGE
        assert "proof 1" in str(e.value)                      # bzh_last_error names the first flagged proof
        assert pk.prove_batch_device(adv, insts, streams, want_status=False)[0] == good
    finally:
        pk.close()


@accelerated_oracle
def test_refusals_leave_everything_as_it_was(gpu_ctx, oracle_c):
    """batch 0 and a batch above the plan's limit, instance_rows > usable, a proof_stride one byte short, unknown form and mem, a
    misaligned device pointer, a short rng_stride, a key of a circuit without a VM v2 workgroup (k = 4, degree 3): each is refused
    with its status, and after each a good call on the same key and ctx gives the reference bytes"""
    import ctypes
    import bzh2
    from bzh2 import native as N
    case = K.case(5, True, None, 3)
    bounds = case[4]
    pk = make_key(gpu_ctx, case)
    small = make_key(gpu_ctx, K.no_instance_case())
    try:
        adv, insts, streams = operands(pk, bounds)
        good = list(case[5])
        limit = pk.prove_device_plan()[7]
        L = N._bind()
        vp = ctypes.c_void_p
        B = 3
        inst_arr, rows = pk._instances(insts)
        raw = np.frombuffer(b"".join(streams), dtype=np.uint8)
        d_adv = dev(K.operand_arrays(bounds, pk.n, MONT)[0])

        def call(status, **kw):
            proofs = np.full((B, pk.max_proof_bytes), 7, dtype=np.uint8)
            lens, st = (ctypes.c_size_t * B)(9, 9, 9), np.full(B, 7, dtype=np.uint8)
            a = dict(ctx=gpu_ctx.handle, pk=pk.handle, batch=B, adv=vp(adv.ctypes.data), form=bzh2.FORM_CANONICAL, mem=bzh2.MEM_HOST,
                     inst=vp(inst_arr.ctypes.data), rows=rows, rng=vp(raw.ctypes.data), stride=pk.rng_bytes, proofs=vp(proofs.ctypes.data),
                     pstride=pk.max_proof_bytes, lens=lens, st=vp(st.ctypes.data))
            a.update(kw)
            assert L.bzh_prove_batch_device(*a.values()) == status, kw
            assert (proofs == 7).all() and list(lens) == [9, 9, 9] and (st == 7).all(), kw       # nothing written
            assert pk.prove_batch_device(adv, insts, streams)[0] == good, kw                     # the key and the ctx are usable

        call(E_ARG, batch=0)
        call(E_ARG, batch=limit + 1)                    # refused before anything is read: the operands need not hold that many proofs
        call(E_ARG, rows=pk.usable_rows + 1)
        assert pk.prove_device_plan()[5] == len(good[0])
        call(E_RANGE, pstride=len(good[0]) - 1)
        call(E_ARG, form=2)
        call(E_ARG, mem=2)
        call(E_ARG, stride=pk.rng_bytes - 64)
        call(E_ARG, inst=None)                          # instance rows without an instance
        call(E_ARG, mem=bzh2.MEM_DEVICE, form=bzh2.FORM_MONTGOMERY, adv=vp(d_adv.data_ptr() + 8))
        call(E_ARG, mem=bzh2.MEM_DEVICE, form=bzh2.FORM_CANONICAL, adv=vp(d_adv.data_ptr()))
        call(E_RANGE, pk=small.handle)                  # degree 3 at k = 4: the extended domain is below VM v2's workgroup
    finally:
        small.close()
        pk.close()


def test_one_real_circuit(gpu_ctx, oracle_c):
    """Shot at k = 11, B = 2, in the key's default quotient flavour (the kernel generated at build time; the key of _setup has
    g_lagrange set): the proofs are bzh_prove_batch's for the same draws"""
    from bzh2 import circuits as Cm, native as N
    from helpers import real_parity as R
    from test_gpu_real_circuit_parity import _setup
    lay, prm, pk = _setup(gpu_ctx, "shot", 11)
    try:
        assert pk.quotient_selected() == (N.QUOTIENT_BUILTIN, True)
        adv, insts = lay.synthesize(R.shot_circuits(Cm, 1107, 2))
        streams = [R.rng_stream("prove-device-shot-%d" % b, pk.rng_bytes) for b in range(2)]
        got, st = pk.prove_batch_device(adv, insts, streams)
        assert not st.any() and got == pk.prove_batch(adv, insts, streams)
        assert pk.verify_batch(insts, got) == [True, True]
    finally:
        pk.close()
        prm.close()
        lay.close()
