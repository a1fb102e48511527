"""The host side of libbzh2.so multiplies field elements too (witness synthesis, Jacobian -> affine read-backs, challenge
algebra): csrc/field.cuh gives the host pass a 64-bit-limb Montgomery product.  tests/helpers/host_field_check.hip compiles
against the library's own header and compares it with the 32-bit CIOS on all four fields (host code only: no GPU needed).  tests/helpers/host_field_edges.hip runs
the host fe_add / fe_sub / fe_neg and both host products over the adversarial operand table of tests/helpers/field_edges.py."""
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
