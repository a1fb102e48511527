"""TEST HELPER: proofs and damaged proofs for the verifier's device pass (tests/test_verify_pass_cpu.py,
tests/test_gpu_verify_pass.py): tests/helpers/vk_cases.py's k = 5 sample circuit with 0, 1 and 2 instance columns, keys and
proofs from the ORACLE (oracle/halo2_oracle.py), and the list of damages with what each does to a proof."""
import functools
import random
import struct

import halo2_oracle as H
import pasta as O

from helpers import vk_cases as V

F, CV = O.FP, O.VESTA
R_MOD, P_MOD = O.FP.p, O.VESTA.p          # scalar field (evaluations, c, f) and base field (coordinates) of Vesta


@functools.lru_cache(maxsize=None)
def oracle_keys(num_instance, k=V.K):
    cs, fixed, copies, _, _, _ = V.circuit(k, 70, num_instance)
    g, w, u = V.srs(k)
    return H.Keys(cs, H.Domain(cs, F), CV, g, w, u, fixed, copies)


@functools.lru_cache(maxsize=None)
def oracle_proof(num_instance, b, k=V.K):
    """(instances, proof bytes) of witness b from the oracle prover"""
    keys = oracle_keys(num_instance, k)
    _, _, _, adv, inst, _ = V.circuit(k, 70 + b, num_instance)
    r = random.Random(1000 * num_instance + b + 17 * k)
    rs = [r.randrange(R_MOD) for _ in range(8192)]
    return [list(c) for c in inst], H.create_proof(keys, adv, inst, rs, O.Blake2bTranscript(F))


def oracle_accepts(num_instance, inst, proof, k=V.K) -> bool:
    return bool(H.verify_proof(oracle_keys(num_instance, k), inst, proof, O.Blake2bTranscript(F)))


def instance_commitments(num_instance, inst) -> bytes:
    """what the verifier absorbs for `inst`: commit_lagrange of every column with blind 1, 64 bytes each (one zero block when the
    circuit has no instance column)"""
    keys = oracle_keys(num_instance)
    n = keys.cs.n
    out = b""
    for c in inst:
        pt = keys.commit(keys.dom.lagrange_to_coeff(list(c) + [0] * (n - len(c))), 1)
        out += int(pt[0]).to_bytes(32, "little") + int(pt[1]).to_bytes(32, "little")
    return out or b"\x00" * 64


def layout(num_instance):
    """byte offsets inside a proof of the k = 5 sample circuit: first advice commitment, first evaluation, L_1, c, f, total"""
    cs, _, _, _, _, circ = V.circuit(V.K, 70, num_instance)
    nl, nsets, npieces = len(cs.lookups), -(-len(cs.perm_columns) // circ.chunk_len), circ.degree - 1
    evals_at = 32 * (cs.num_advice + 3 * nl + nsets + 1 + npieces)
    return {"advice": 0, "eval": evals_at}


def _off_curve_x():
    x = 1
    while pow((x * x * x + 5) % P_MOD, (P_MOD - 1) // 2, P_MOD) == 1:
        x += 1
    return x


def damaged(num_instance, proof: bytes, other_k_proof: bytes | None = None):
    """[(name, proof bytes, host_pass)]: host_pass says what the per-proof pass makes of it BEFORE the IPA check -- 1 it parses
    (the check then fails), 0 it is refused, 2 either.  None of them verifies."""
    lay = layout(num_instance)
    ln = len(proof)
    c_at, f_at, l1_at = ln - 64, ln - 32, ln - 64 - 64 * V.K
    flip = lambda at: proof[:at] + bytes([proof[at] ^ 0x10]) + proof[at + 1:]
    put = lambda at, b: proof[:at] + b + proof[at + len(b):]
    out = [("a flipped bit in an advice commitment", flip(lay["advice"] + 5), 2),
           ("a flipped bit in an evaluation", flip(lay["eval"] + 32 * 2 + 5), 1),
           ("a flipped bit in an L_j", flip(l1_at + 3), 2),
           ("a flipped bit in c", flip(c_at + 7), 1),
           ("a flipped bit in f", flip(f_at + 7), 1),
           ("a point whose x is the modulus", put(32, P_MOD.to_bytes(32, "little")), 0),
           ("a point off the curve", put(32, _off_curve_x().to_bytes(32, "little")), 0),
           ("32 zero bytes where a point stands", put(64, b"\x00" * 32), 0),
           ("an evaluation equal to the modulus", put(lay["eval"] + 32, R_MOD.to_bytes(32, "little")), 0),
           ("c equal to the modulus", put(c_at, R_MOD.to_bytes(32, "little")), 0),
           ("one byte short", proof[:-1], 0),
           ("one byte long", proof + b"\x00", 0)]
    if other_k_proof is not None:
        out.append(("a proof of the k = 6 key", other_k_proof, 0))
    return out


def check_file(circuits) -> bytes:
    """circuits: [(key bytes, points per instance block, [(expectation, instance commitments, proof)])] as
    tests/helpers/verify_pass_check.hip reads them"""
    out = struct.pack("<I", len(circuits))
    for kb, ni1, proofs in circuits:
        out += struct.pack("<I", len(kb)) + kb + struct.pack("<II", ni1, len(proofs))
        for expect, ic, pr in proofs:
            assert len(ic) == 64 * ni1
            out += struct.pack("<I", expect) + ic + struct.pack("<I", len(pr)) + pr
    return out
