"""TEST HELPER: the verifying-key tests' circuit, SRS, oracle commitments, the "BZV1" bytes built in Python from the layout
documented at the top of csrc/verifying_key.hpp, and the hostile variants of those bytes (tests/test_vk_cpu.py replays them
through bzh_vk_read in a child process and through tests/helpers/vk_check.hip under the host sanitizers)."""
import functools
import random
import struct
import zlib

import halo2_oracle as H
import pasta as O
import sample_circuit as S
from bzh2 import circuit_data as P

E_ARG, E_RANGE = -1, -4
ANY_ERROR, MUST_ROUND_TRIP = 0, 1        # what a replayed case expects besides the two statuses above
PLACEHOLDER = 0x1234
OTHER_REPR = 0x0123456789abcdef0123456789abcdef0123456789abcdef
K = 5


def circuit(k=K, seed=70, num_instance=1):
    """(cs, fixed, copies, advice, instances, bzh2 Circuit): oracle/sample_circuit.py -- 4 gates, a lookup, 4 permutation columns (one of
    them the instance column), 4 fixed columns.  num_instance = 0 drops the instance column (and its copy constraint), 2 adds a
    second one that nothing constrains."""
    cs, fixed, copies, adv, inst = S.build(k=k, seed=seed, with_lookup=True)
    perm = list(cs.perm_columns)
    if num_instance == 0:
        perm = [c for c in perm if c[0] != 'instance']
        copies = [c for c in copies if c[0][0] < len(perm) and c[1][0] < len(perm)]
        inst = []
    elif num_instance == 2:
        inst = [inst[0], [7, 8, 9]]
    if num_instance != 1:
        cs = H.ConstraintSystem(k, 3, 4, num_instance, cs.gates, perm, cs.lookups)
    circ = P.Circuit(cs.k, cs.num_advice, cs.num_fixed, cs.num_instance, cs.gates, cs.perm_columns, cs.lookups, fixed, copies)
    return cs, fixed, copies, adv, inst, circ


@functools.lru_cache(maxsize=None)
def srs(k=K, seed=7):
    """(g, w, u): 2^k + 2 random Vesta points"""
    r = random.Random(seed * 1000 + k)
    g = [O.VESTA.random_point(r) for _ in range(1 << k)]
    return g, O.VESTA.random_point(r), O.VESTA.random_point(r)


@functools.lru_cache(maxsize=None)
def oracle_commitments(k=K, seed=70, num_instance=1):
    """(fixed commitments, permutation commitments) of circuit(...) on srs(k): the oracle's keygen, blind 1"""
    cs, fixed, copies, _, _, _ = circuit(k, seed, num_instance)
    g, w, u = srs(k)
    keys = H.Keys(cs, H.Domain(cs, O.FP), O.VESTA, g, w, u, fixed, copies)
    return list(keys.fixed_commitments), list(keys.sigma_commitments)


def constraint_system_bytes(circ, p, vk_repr):
    """the circuit blob without copy constraints and with empty fixed columns"""
    bare = P.Circuit(circ.k, circ.num_advice, circ.num_fixed, circ.num_instance, circ.gates, circ.perm_columns, circ.lookups,
                     [[] for _ in range(circ.num_fixed)], [])
    return P.serialize_circuit(bare, p, vk_repr, min_degree=circ.degree)


def with_crc(body: bytes) -> bytes:
    return body + struct.pack("<I", zlib.crc32(body) & 0xffffffff)


def bzv1(circ, fixed_commitments, sigma_commitments, vk_repr=PLACEHOLDER, curve=0) -> bytes:
    p = O.FP.p
    cs = constraint_system_bytes(circ, p, vk_repr)
    pt = lambda q: int(q[0]).to_bytes(32, "little") + int(q[1]).to_bytes(32, "little")
    body = b"BZV1" + struct.pack("<II", circ.k, curve) + (vk_repr % p).to_bytes(32, "little")
    body += struct.pack("<IIII", 1 if vk_repr % p == PLACEHOLDER else 0, len(fixed_commitments), len(sigma_commitments), len(cs))
    body += b"".join(pt(q) for q in fixed_commitments) + b"".join(pt(q) for q in sigma_commitments) + cs
    return with_crc(body)


@functools.lru_cache(maxsize=None)
def golden(vk_repr=PLACEHOLDER) -> bytes:
    """the BZV1 bytes of circuit() on srs() with the oracle's commitments"""
    fc, sc = oracle_commitments()
    return bzv1(circuit()[5], fc, sc, vk_repr)


# field name -> (offset, size) of the header and the counts
HEADER_FIELDS = {"magic": (0, 4), "k": (4, 4), "curve": (8, 4), "vk_repr": (12, 32), "placeholder": (44, 4), "num_fixed": (48, 4),
                 "num_permutation": (52, 4), "cs_len": (56, 4)}
HEADER_BYTES = 60


def hostile(good: bytes):
    """[(name, bytes, expectation)]: expectation is E_ARG, E_RANGE or ANY_ERROR (negative, whichever)"""
    out = []
    body = good[:-4]
    patch = lambda b, off, new: b[:off] + new + b[off + len(new):]
    for ln in range(len(good)):                                   # every truncation
        out.append(("truncated to %d" % ln, good[:ln], E_ARG))
    out.append(("one byte too many", good + b"\x00", E_ARG))
    for name, (off, size) in HEADER_FIELDS.items():               # one flipped bit per field, checksum stale and checksum mended
        for bit in (0, 8 * size - 1):
            flipped = patch(body, off + bit // 8, bytes([body[off + bit // 8] ^ (1 << (bit % 8))]))
            out.append(("%s bit %d flipped" % (name, bit), flipped + good[-4:], E_ARG))
            out.append(("%s bit %d flipped, checksum mended" % (name, bit), with_crc(flipped), ANY_ERROR))
    for name in ("num_fixed", "num_permutation", "cs_len"):       # a count inflated to 2^31
        out.append(("%s = 2^31" % name, with_crc(patch(body, HEADER_FIELDS[name][0], struct.pack("<I", 1 << 31))), E_ARG))
    nf = struct.unpack_from("<I", good, 48)[0]
    pbase = O.VESTA.p
    for which, off in (("first fixed", HEADER_BYTES), ("first permutation", HEADER_BYTES + 64 * nf)):
        for coord, o in (("x", 0), ("y", 32)):
            out.append(("%s commitment %s = p" % (which, coord), with_crc(patch(body, off + o, pbase.to_bytes(32, "little"))), E_RANGE))
            out.append(("%s commitment %s = 2^256 - 1" % (which, coord), with_crc(patch(body, off + o, b"\xff" * 32)), E_RANGE))
        y = int.from_bytes(body[off + 32:off + 64], "little")
        out.append(("%s commitment off the curve" % which, with_crc(patch(body, off + 32, ((y + 1) % pbase).to_bytes(32, "little"))), E_RANGE))
        out.append(("%s commitment the identity" % which, with_crc(patch(body, off, b"\x00" * 64)), E_RANGE))
    out.append(("wrong checksum", body + struct.pack("<I", (zlib.crc32(body) ^ 1) & 0xffffffff), E_ARG))
    # inside the constraint-system bytes (checksum mended): a bad magic, an expression tag out of range, a column out of range
    cs_off = len(body) - struct.unpack_from("<I", good, 56)[0]
    out.append(("constraint system: magic", with_crc(patch(body, cs_off, b"BZC9")), E_ARG))
    out.append(("constraint system: k", with_crc(patch(body, cs_off + 4, struct.pack("<I", 6))), E_ARG))
    out.append(("constraint system: num_advice = 2^31", with_crc(patch(body, cs_off + 8, struct.pack("<I", 1 << 31))), E_ARG))
    out.append(("constraint system: first expression tag", with_crc(patch(body, cs_off + 60, b"\x09")), E_ARG))
    for i in range(cs_off + 56, len(body), 7):                    # a byte smashed here and there: any error, or a key that round-trips
        out.append(("constraint system: byte %d smashed" % i, with_crc(patch(body, i, bytes([body[i] ^ 0xff]))), None))
    return out


def replay_file(cases) -> bytes:
    """the cases as a file for the replayers: per case i32 expectation (E_ARG, E_RANGE, ANY_ERROR, MUST_ROUND_TRIP, or 2 = either an
    error or a key that round-trips), u32 length, bytes"""
    return b"".join(struct.pack("<iI", 2 if exp is None else exp, len(b)) + b for _, b, exp in cases)
