"""The host side of libbzh2.so multiplies field elements too (witness synthesis, Jacobian -> affine read-backs, challenge
algebra): csrc/field.cuh gives the host pass a 64-bit-limb Montgomery product.  tests/helpers/host_field_check.hip compiles
against the library's own header and compares it with the 32-bit CIOS on all four fields (host code only: no GPU needed).  tests/helpers/host_field_edges.hip runs
the host fe_add / fe_sub / fe_neg and both host products over the adversarial operand table of tests/helpers/field_edges.py.
tests/helpers/host_field_helpers.hip drives the helpers of csrc/host_field.hpp (square root, Jacobi symbol, point decompression,
roots of unity, batch inversion, interpolation, Jacobian / XYZZ -> affine), which the library otherwise reaches only around GPU work, against oracle/pasta.py."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_host_64_bit_field_product_equals_the_32_bit_one(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    exe = str(tmp_path / "host_field_check")
    subprocess.check_call([hipcc, "-O2", "-std=c++17", "--offload-arch=gfx950", "-Wno-unused-function",
                           "-I", os.path.join(ROOT, "battlezips-halo2_amd", "csrc"),
                           os.path.join(ROOT, "tests", "helpers", "host_field_check.hip"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = [ln for ln in out.stdout.splitlines() if ln.strip()]
    assert len(lines) == 4 and all(ln.endswith("-> OK") for ln in lines), out.stdout
    assert all("64-bit limbs" in ln for ln in lines), "the host pass did not take the 64-bit path:\n" + out.stdout


@pytest.fixture(scope="module")
def edge_programs(tmp_path_factory):
    """tests/helpers/host_field_edges.hip built twice: the 64-bit-limb host product and, with -DBZH_NO_HOST_MUL64, the 32-bit CIOS"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    d = tmp_path_factory.mktemp("host_field_edges")
    exes = {}
    for name, flags in (("64-bit limbs", []), ("32-bit limbs", ["-DBZH_NO_HOST_MUL64"])):
        exe = str(d / ("edges_" + name[:2]))
        subprocess.check_call([hipcc, "-O2", "-std=c++17", "--offload-arch=gfx950", "-Wno-unused-function", *flags,
                               "-I", os.path.join(ROOT, "battlezips-halo2_amd", "csrc"),
                               os.path.join(ROOT, "tests", "helpers", "host_field_edges.hip"), "-o", exe])
        exes[name] = exe
    return d, exes


@pytest.mark.parametrize("fid", [0, 1, 2, 3])
def test_host_twins_on_the_edge_operand_table(edge_programs, fid):
    """fe_add, fe_sub, fe_neg and both host fe_mul paths on all 256 x 256 ordered pairs of the adversarial operand set
    (tests/helpers/field_edges.py) and on the targeted products, bit-exact against Python integers: the vector set and its
    reference are sound before a GPU is involved, and the host code is pinned at the same corners as the device asm."""
    import random

    from helpers import field_edges as E
    d, exes = edge_programs
    p = E.MODULI[fid]
    a, b = E.all_pairs(E.edge_values(p))
    trip = E.targeted_products(p, random.Random(5 + fid))
    a += [t[0] for t in trip]
    b += [t[1] for t in trip]
    want = {op: [E.reference(op, x, y, p) for x, y in zip(a, b)] for op in ("add", "sub", "neg", "mul")}
    assert want["mul"][65536:] == [t[2] for t in trip]
    fin, fout = str(d / ("in%d.bin" % fid)), str(d / ("out%d.bin" % fid))
    with open(fin, "wb") as f:
        f.write(b"".join(x.to_bytes(32, "little") + y.to_bytes(32, "little") for x, y in zip(a, b)))
    for path, exe in exes.items():
        out = subprocess.run([exe, str(fid), fin, fout], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0 and out.stdout.strip() == path, (out.returncode, out.stdout, out.stderr)
        raw = open(fout, "rb").read()
        assert len(raw) == 128 * len(a)
        for k, op in enumerate(("add", "sub", "neg", "mul")):
            got = [int.from_bytes(raw[128 * i + 32 * k: 128 * i + 32 * k + 32], "little") for i in range(len(a))]
            msg = E.first_mismatch(got, want[op], a, b, "field %d host fe_%s (%s)" % (fid, op, path))
            assert msg is None, msg


# ---------------------------------------------------------------------------------------------------------------------
# csrc/host_field.hpp against oracle/pasta.py
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def helper_program(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    d = tmp_path_factory.mktemp("host_field_helpers")
    exe = str(d / "host_field_helpers")
    subprocess.check_call([hipcc, "-O2", "-std=c++17", "--offload-arch=gfx950", "-Wno-unused-function",
                           "-I", os.path.join(ROOT, "battlezips-halo2_amd", "csrc"),
                           os.path.join(ROOT, "tests", "helpers", "host_field_helpers.hip"), "-o", exe])

    def ask(commands):
        """one answer line (split into words) per command line"""
        path = str(d / "commands.txt")
        with open(path, "w") as f:
            f.write("".join(c + "\n" for c in commands))
        out = subprocess.run([exe, path], capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
        lines = out.stdout.splitlines()
        assert len(lines) == len(commands), (len(lines), len(commands))
        return [ln.split() for ln in lines]
    return ask


def _oracle():
    import sys
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import pasta
    return pasta


def _hx(v):
    return "%064x" % v


@pytest.mark.parametrize("fid", [0, 1, 2, 3])
def test_host_sqrt_against_the_oracle(helper_program, fid):
    """h_sqrt on 0, 1, the edge operands (residues and non-residues alike), squares of even and of odd roots, and the
    multiplicative generator times squares (never a residue): a root is reported exactly where the oracle finds one, and it
    squares to the operand."""
    import random

    from helpers import field_edges as E
    O = _oracle()
    F = O.FIELD_BY_ID[fid]
    p = F.p
    assert p == E.MODULI[fid]
    rng = random.Random(100 + fid)
    edges = E.edge_values(p)
    roots = [r for r in edges[:48]] + [2 * rng.randrange(1, p // 2) for _ in range(8)] + [2 * rng.randrange(p // 2) + 1 for _ in range(8)]
    vals = [0, 1] + edges + [r * r % p for r in roots] + [F.g] + [F.g * r * r % p for r in roots[1:17] if r]
    want = [F.sqrt(a) for a in vals]
    assert sum(w is None for w in want) >= 17 and sum(w is not None for w in want) >= 64
    assert F.sqrt(F.g) is None
    got = helper_program(["sqrt %d %s" % (fid, _hx(a)) for a in vals])
    for a, w, g in zip(vals, want, got):
        if w is None:
            assert g == ["none"], "field %d: sqrt(%#x) reported for a non-residue: %s" % (fid, a, g)
        else:
            assert g[0] == "ok", "field %d: no sqrt(%#x), the oracle has %#x" % (fid, a, w)
            r = int(g[1], 16)
            assert r < p and r in (w, (p - w) % p) and r * r % p == a, "field %d: sqrt(%#x) = %#x, the oracle has +-%#x" % (fid, a, r, w)


@pytest.mark.parametrize("fid", [0, 1, 2, 3])
def test_host_omega_against_the_oracle(helper_program, fid):
    O = _oracle()
    F = O.FIELD_BY_ID[fid]
    got = helper_program(["omega %d %d" % (fid, k) for k in range(F.S + 1)])
    assert [int(g[0], 16) for g in got] == [F.omega(k) for k in range(F.S + 1)]


@pytest.mark.parametrize("fid", [0, 1, 2, 3])
def test_host_batch_inversion_with_zeros(helper_program, fid):
    """h_batch_invert: every non-zero edge operand inverted; zeros in first, middle and last place stay zero when the caller
    asks for them to be skipped and make the call fail, with nothing written, when it does not"""
    from helpers import field_edges as E
    O = _oracle()
    F = O.FIELD_BY_ID[fid]
    nz = [v for v in E.edge_values(F.p) if v]
    holes = [0] + nz[:7] + [0, 0] + nz[7:20] + [0]
    cases = [(0, nz), (1, nz), (1, holes), (0, holes), (1, [0, 0, 0]), (0, [0]), (1, [0]), (0, []), (1, []), (0, nz[:1]), (1, [0, nz[3]])]
    got = helper_program(["binv %d %d %d %s" % (fid, skip, len(v), " ".join(_hx(x) for x in v)) for skip, v in cases])
    for (skip, v), g in zip(cases, got):
        if 0 in v and not skip:
            assert g == ["fail"], g[:1]
        else:
            assert g[0] == "ok" and [int(x, 16) for x in g[1:]] == [F.inv(x) for x in v], "field %d skip %d n %d" % (fid, skip, len(v))


def _interpolate(F, xs, ys):
    """coefficients, lowest first, of the polynomial of degree < len(xs) through the points: Lagrange's formula in exact integers"""
    p = F.p
    out = [0] * len(xs)
    for j, (xj, yj) in enumerate(zip(xs, ys)):
        num, den = [1], 1
        for mm, xm in enumerate(xs):
            if mm != j:
                num = [((num[i - 1] if i else 0) - xm * (num[i] if i < len(num) else 0)) % p for i in range(len(num) + 1)]
                den = den * (xj - xm) % p
        cf = yj * F.inv(den) % p
        out = [(o + cf * c) % p for o, c in zip(out, num)]
    return out


@pytest.mark.parametrize("fid", [0, 1])
def test_host_interpolation_against_exact_integers(helper_program, fid):
    """h_interpolate (the multiopen remainders) through 1, 2, 3 and 4 points of Fp and Fq: points at 0, 1 and p - 1, evaluations
    of 0 (all of them, and one among others), edge and random operands, coefficient by coefficient against Lagrange's formula
    in Python integers; the result takes the given values at the given points, and two equal points make the inversion fail"""
    import random

    from helpers import field_edges as E
    O = _oracle()
    F = O.FIELD_BY_ID[fid]
    p = F.p
    rng = random.Random(400 + fid)
    edges = E.edge_values(p)
    cases = []
    for np_ in (1, 2, 3, 4):
        special = [0, 1, p - 1, 2][:np_]
        cases.append((special, [rng.randrange(p) for _ in range(np_)]))
        cases.append((special[::-1], [0] * np_))
        cases.append(([p - 1, rng.randrange(2, p - 1), 0, 1][:np_], [rng.randrange(p), 0, p - 1, 1][:np_]))
        cases.append(([rng.randrange(p) for _ in range(np_)], [rng.randrange(p) for _ in range(np_)]))
        cases.append((rng.sample(edges, np_), rng.sample(edges, np_)))
    assert all(len(set(xs)) == len(xs) for xs, _ in cases)
    got = helper_program(["interp %d %d %s" % (fid, len(xs), " ".join(_hx(v) for v in xs + ys)) for xs, ys in cases])
    for (xs, ys), g in zip(cases, got):
        want = _interpolate(F, xs, ys)
        assert [sum(c * pow(x, i, p) for i, c in enumerate(want)) % p for x in xs] == ys   # (the reference itself)
        assert g[0] == "ok" and [int(c, 16) for c in g[1:]] == want, "field %d, %d points %s" % (fid, len(xs), [hex(x) for x in xs])
    twice = helper_program(["interp %d 3 %s" % (fid, " ".join(_hx(v) for v in [5, 7, 5, 1, 2, 3]))])
    assert twice == [["fail"]]


def _decompress(O, curve, raw):
    """pasta_curves from_bytes restated on the oracle's field: (x, y), None for the identity, or "reject" """
    v = int.from_bytes(raw, "little")
    sign, x = v >> 255, v & ((1 << 255) - 1)
    if x == 0:
        return "reject" if sign else None
    if x >= curve.p:
        return "reject"
    y = curve.base.sqrt((x * x * x + curve.b) % curve.p)
    if y is None:
        return "reject"
    return (x, y if (y & 1) == sign else curve.p - y)


@pytest.mark.parametrize("cid", [0, 1, 2])
def test_host_point_decompression_against_the_oracle(helper_program, cid):
    """h_decompress on both sign bits of edge and random x (on and off the curve), x >= p, and the identity with and
    without the sign bit.  Rejected: x >= p, x^3 + b a non-residue, the sign bit on the identity."""
    import random

    from helpers import field_edges as E
    O = _oracle()
    cv = O.CURVE_BY_ID[cid]
    p = cv.p
    rng = random.Random(200 + cid)
    xs = [x for x in E.edge_values(p)[:96] if x] + [rng.randrange(1, p) for _ in range(32)]
    on = [x for x in xs if cv.base.sqrt((x ** 3 + cv.b) % p) is not None]
    off = [x for x in xs if cv.base.sqrt((x ** 3 + cv.b) % p) is None]
    assert len(on) >= 32 and len(off) >= 32
    too_big = [p, p + 1, p + on[0], (1 << 255) - 1] + [x + p for x in on[:4] if x + p < 1 << 255]
    enc = [(x | s << 255).to_bytes(32, "little") for x in on + off + too_big for s in (0, 1)]
    enc += [bytes(32), bytes(31) + b"\x80"]
    want = [_decompress(O, cv, e) for e in enc]
    for x in off + too_big:
        for s in (0, 1):
            assert want[enc.index((x | s << 255).to_bytes(32, "little"))] == "reject"
    assert want[-2] is None and want[-1] == "reject"
    got = helper_program(["decompress %d %s" % (cid, e.hex()) for e in enc])
    for e, w, g in zip(enc, want, got):
        if w == "reject":
            assert g == ["reject"], "curve %d: %s accepted as %s" % (cid, e.hex(), g)
        else:
            assert g[0] == "ok", "curve %d: %s rejected" % (cid, e.hex())
            pt = (int(g[1], 16), int(g[2], 16))
            assert pt == (w or (0, 0)), "curve %d: %s" % (cid, e.hex())
            if w is not None:
                assert cv.is_on_curve(pt) and cv.compress(pt) == e


@pytest.mark.parametrize("cid", [0, 1, 2])
def test_host_jacobian_to_affine_with_identities(helper_program, cid):
    """h_jac_to_affine over batches that hold identities (Z = 0 with arbitrary X, Y) in first, middle and last place, only
    identities, one point and none, with Z drawn from the edge operands, in every combination of input and output form"""
    import random

    from helpers import field_edges as E
    O = _oracle()
    cv = O.CURVE_BY_ID[cid]
    p = cv.p
    R = E.R % p
    rng = random.Random(300 + cid)
    zs = [z for z in E.edge_values(p) if z]

    def jac(pt, z):
        if pt is None:
            return (rng.randrange(p), rng.randrange(p), 0)
        return (pt[0] * z * z % p, pt[1] * z * z * z % p, z)
    pts = [cv.random_point(rng) for _ in range(24)]
    batches = [
        [jac(pt, zs[i]) for i, pt in enumerate(pts)],
        [jac(None, 0)] + [jac(pt, zs[30 + i]) for i, pt in enumerate(pts[:9])] + [jac(None, 0)] * 2 + [jac(pt, zs[60 + i]) for i, pt in enumerate(pts[9:])] + [jac(None, 0)],
        [jac(None, 0)] * 3, [jac(None, 0)], [jac(pts[0], p - 1)], [],
    ]
    cases = [(fi, fo, b) for b in batches for fi in (0, 1) for fo in (0, 1)]
    got = helper_program(["jac %d %d %d %d %s" % (cid, fi, fo, len(b), " ".join(_hx(c * R % p if fi else c) for t in b for c in t)) for fi, fo, b in cases])
    for (fi, fo, b), g in zip(cases, got):
        want = []
        for X, Y, Z in b:
            if Z == 0:
                want += [0, 0]
            else:
                zi = cv.base.inv(Z)
                want += [X * zi * zi % p, Y * zi * zi * zi % p]
        assert [int(x, 16) for x in g] == [w * R % p if fo else w for w in want], "curve %d forms %d -> %d, %d points" % (cid, fi, fo, len(b))
    # the non-identity points of the first batch come back as the oracle's own affine points
    assert [int(x, 16) for x in got[0]] == [c for pt in pts for c in pt]


@pytest.mark.parametrize("fid", [0, 1])
def test_host_jacobi_symbol_against_eulers_criterion(helper_program, fid):
    """h_jacobi (the circuit's fixed-base tables ask it per entry) on 0, 1, p - 1, the edge operands, and the generator of the
    2-Sylow subgroup (never a square) and its square: +1, -1 or 0 exactly as a^((p-1)/2) says"""
    from helpers import field_edges as E
    O = _oracle()
    F = O.FIELD_BY_ID[fid]
    p = F.p
    root = F.omega(F.S)
    assert pow(root, 1 << (F.S - 1), p) == p - 1        # order exactly 2^S
    vals = [0, 1, p - 1, root, root * root % p] + E.edge_values(p)
    want = [{0: 0, 1: 1, p - 1: -1}[pow(a, (p - 1) // 2, p)] for a in vals]
    assert want[:5] == [0, 1, 1, -1, 1] and want.count(-1) >= 64 and want.count(1) >= 64
    got = helper_program(["jacobi %d %s" % (fid, _hx(a)) for a in vals])
    assert [int(g[0]) for g in got] == want, [hex(a) for a, w, g in zip(vals, want, got) if int(g[0]) != w][:4]


@pytest.mark.parametrize("cid", [0, 1])
def test_host_xyzz_to_affine_with_one_shared_inversion(helper_program, cid):
    """h_xyzz_to_affine over a vector holding the identity (ZZ = 0 with arbitrary X, Y), a point, its negative and the doubled
    point, each scaled by another z (X = x z^2, Y = y z^3, ZZ = z^2, ZZZ = z^3), z from the edge operands and p - 1; the identity
    first, in the middle, last and alone, and the empty vector"""
    import random

    from helpers import field_edges as E
    O = _oracle()
    cv = O.CURVE_BY_ID[cid]
    p = cv.p
    rng = random.Random(500 + cid)
    zs = [z for z in E.edge_values(p) if z] + [p - 1]
    pt = cv.random_point(rng)
    assert cv.is_on_curve(cv.add(pt, pt)) and cv.add(pt, cv.neg(pt)) is None
    quad = [None, pt, cv.neg(pt), cv.add(pt, pt)]

    def xyzz(q, z):
        if q is None:
            return (rng.randrange(p), rng.randrange(p), 0, 0)
        return (q[0] * z * z % p, q[1] * z ** 3 % p, z * z % p, z ** 3 % p)
    batches = [quad, quad[1:] + [None], [pt, None, None, cv.neg(pt)], [None], [cv.add(pt, pt)], []]
    batches += [[quad[(i + j) % 4] for j in range(4)] for i in range(8)]
    cases = [[(q, zs[(7 * bi + 3 * i) % len(zs)] if bi else zs[-1 - i]) for i, q in enumerate(b)] for bi, b in enumerate(batches)]
    got = helper_program(["xyzz %d %d %s" % (cid, len(b), " ".join(_hx(c) for q, z in b for c in xyzz(q, z))) for b in cases])
    for b, g in zip(cases, got):
        assert [int(x, 16) for x in g] == [c for q, _ in b for c in (q or (0, 0))], "curve %d, %d points" % (cid, len(b))


def test_circuit_value_types_accept_exactly_the_canonical_encodings():
    """The circuit front end's Fp / Fq (csrc/circuit/hostfield.hpp) read limbs through the library's is_canonical: from_repr
    (bzh_circuit_set_vk_repr) and from_limbs (bzh_pedersen_commit_host: an Fp message, an Fq trapdoor) take 0 and p - 1 and refuse
    p, p + 1 and 2^256 - 1 with BZH_E_RANGE.  The accepted commitments are the oracle's: [0]V + [0]R is the identity (0, 0), which
    the window sums reach by adding a point to its negative."""
    import bzh2
    from bzh2 import BzhError, circuits as Cm
    O = _oracle()
    p, q = O.FP.p, O.FQ.p
    assert p < q
    lay = Cm.CircuitLayout(Cm.SHOT, 11)
    try:
        for good in (0, p - 1):
            lay.set_vk_repr(good)
            assert lay.vk_repr() == (good, False)
        for bad in (p, p + 1, (1 << 256) - 1):
            with pytest.raises(BzhError) as e:
                lay.set_vk_repr(bad)
            assert e.value.status == bzh2.E_RANGE
        assert lay.vk_repr() == (p - 1, False)
    finally:
        lay.close()
    for m, t in ((0, 0), (p - 1, q - 1), (0, q - 1), (p - 1, 0)):
        assert Cm.pedersen_commit_host(m, t) == (O.pedersen_commit(m, t) or (0, 0)), (hex(m), hex(t))
    for m, t in [(bad, 1) for bad in (p, p + 1, (1 << 256) - 1)] + [(1, bad) for bad in (q, q + 1, (1 << 256) - 1)]:
        with pytest.raises(BzhError) as e:
            Cm.pedersen_commit_host(m, t)
        assert e.value.status == bzh2.E_RANGE, (hex(m), hex(t))
