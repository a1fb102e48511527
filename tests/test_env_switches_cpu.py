"""Every BZH_* variable the library reads has a row in INTEGRATION.md's table, and every one that selects a code path is a
setting of tests/test_gpu_env_paths.py, which pins that path bit for bit against the default: no path is reachable only
through an untested switch."""
import importlib.util
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "battlezips-halo2_amd", "csrc")
NOT_PATHS = {"BZH_CACHE_DIR", "BZH_PROVE_TRACE", "BZH_HOST_THREADS", "BZH_VM2_DEBUG"}   # read, but compute the same way


def _read(path):
    with open(path, encoding="utf-8") as f:
        return f.read()


def _library_switches():
    names = set()
    for d, _, files in os.walk(CSRC):
        for fn in files:
            if fn.endswith((".hip", ".hpp", ".cuh", ".cpp", ".h", ".inc")):
                names |= set(re.findall(r'getenv\("(BZH_\w+)"\)', _read(os.path.join(d, fn))))
    return names


def test_every_switch_is_documented_and_env_tested():
    names = _library_switches()
    assert "BZH_ACC_SATURATED" in names   # (the scan itself works)
    table = _read(os.path.join(ROOT, "INTEGRATION.md")).split("## Environment variables", 1)[1].split("\n## ", 1)[0]
    documented = {n for ln in table.splitlines() if ln.startswith("| `") for n in re.findall(r"`(BZH_\w+)`", ln.split("|")[1])}
    spec = importlib.util.spec_from_file_location("env_paths", os.path.join(ROOT, "tests", "test_gpu_env_paths.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    tested = {k for setting in m.SETTINGS for k in setting}
    assert sorted(names - documented) == [], "missing from INTEGRATION.md's table of environment variables"
    assert sorted(names - NOT_PATHS - tested) == [], "selects a path that tests/test_gpu_env_paths.py does not pin"
