"""The runtime state both keys hold -- csrc/key_runtime.hpp: the key's mutex, one arena per ctx serial, the count of running calls,
the call guard and retire() -- without a device: tests/helpers/key_runtime_check.hip drives the struct directly (an arena with no
blocks never reaches the HIP runtime), as a stand-alone program under the host's sanitizers."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(tmp_path, name, sanitize):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    exe = str(tmp_path / name)
    cmd = [hipcc, "-O1", "-g", "-std=c++17", "--offload-arch=gfx950", "-Wno-unused-function", "-pthread",
           "-Xarch_host", "-fsanitize=" + sanitize, "-Xarch_host", "-fno-sanitize-recover=undefined",
           "-I", os.path.join(ROOT, "battlezips-halo2_amd", "csrc"), os.path.join(ROOT, "tests", "helpers", "key_runtime_check.hip"), "-o", exe]
    return exe, subprocess.run(cmd, capture_output=True, text=True)


def test_guards_retire_serials_and_arenas_standalone_under_host_sanitizers(tmp_path):
    """retire() refuses while a guard is alive and succeeds after it is gone; 8 threads x 10 000 guards against a thread that
    keeps calling retire(): every refusal with a guard alive, exactly one success, with none; ctx serials never collide, over
    threads and over contexts that reuse an address; arena_for keeps one arena per serial and makes a fresh one, on the new
    ctx's device, for a new serial.  Address and undefined-behaviour sanitizers."""
    exe, built = _build(tmp_path, "key_runtime_check", "address,undefined")
    assert built.returncode == 0, built.stderr[-3000:]
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(out.stdout[-3000:])
    assert out.returncode == 0 and out.stdout.strip().endswith("key_runtime_check: ok"), out.stdout[-3000:] + out.stderr[-3000:]
    m = re.search(r"(\d+) guards, (\d+) refusals, (\d+) success", out.stdout)
    assert int(m.group(1)) == 8 * 10000 and int(m.group(2)) >= 1 and int(m.group(3)) == 1


def test_threaded_part_under_the_thread_sanitizer(tmp_path):
    """The same guards-against-retire race under the thread sanitizer, where this toolchain links it."""
    exe, built = _build(tmp_path, "key_runtime_check_threads", "thread")
    if built.returncode != 0:
        # only a missing sanitizer runtime is a reason to skip: a compile error in the helper is a failure here as above
        assert re.search(r"tsan|unsupported option '-fsanitize=thread'", built.stderr), built.stderr[-3000:]
        pytest.skip("the thread sanitizer does not link on this toolchain")
    out = subprocess.run([exe, "threads"], capture_output=True, text=True, timeout=600)
    print(out.stdout[-3000:])
    assert out.returncode == 0 and out.stdout.strip().endswith("key_runtime_check: ok"), out.stdout[-3000:] + out.stderr[-3000:]
    assert "ThreadSanitizer" not in out.stderr
