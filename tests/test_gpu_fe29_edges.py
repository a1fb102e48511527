"""The DEVICE build of the unsaturated 9 x 29-bit field and curve code (csrc/fe29.cuh, csrc/curve29.cuh), operation by operation,
with operands on the documented bounds: the operand files of tests/test_fe29_edges_cpu.py through tests/helpers/fe29_ops.hip
--device, judged by the same integer model (tests/helpers/fe29_model.py).  The device build is not the host build
(fe29_p8_opaque is inline assembly, the special cases are __noinline__ callees, xyzz29_add_nocall hides its operands, the
multiply-adds are lowered differently), so besides the model the device limbs must equal the host limbs word for word: both are
deterministic integer code.  xyzz29_add_quad, xyzz29_from_sat_quad and xyzz29_shfl_down exist on the device only and are judged
by the model alone; the four lanes of a quad must hold identical results.

The program runs in a child process under a time limit.  A non-zero status, a signal or a timeout fails the test, and after
that no test of this module starts another device run."""
import subprocess

import pytest

from helpers import fe29_model as M

pytestmark = pytest.mark.gpu

COMPILE_TIMEOUT = 210     # seconds: three times the first measured compile of this program (68 s)
RUN_TIMEOUT = 10          # seconds: the slowest measured device run of one group took 0.33 s (three times that is 1 s); the rest
                          # is room for the start of a process that opens the device on a shared machine
HOST_TIMEOUT = 10         # the host run of a group took 0.02 s
GROUPS = dict(M.FIELD_GROUPS, **M.CURVE_GROUPS)
_stopped = []


@pytest.fixture(scope="module")
def program(gpu_ctx, tmp_path_factory):
    # gpu_ctx only so that the suite's gating of GPU tests applies; the program opens the device itself
    exe = M.build_program(str(tmp_path_factory.mktemp("fe29_ops") / "fe29_ops"), COMPILE_TIMEOUT)
    assert exe is not None, "no hipcc"
    return exe


def device_run(program, field, ops, workdir):
    if _stopped:
        pytest.fail("no further device run: an earlier one of this module failed (%s)" % _stopped[0])
    try:
        return M.run_program(program, "device", field, ops, workdir, RUN_TIMEOUT)
    except (RuntimeError, subprocess.TimeoutExpired) as e:
        _stopped.append(str(e)[:300])
        raise


@pytest.mark.parametrize("group", sorted(GROUPS))
@pytest.mark.parametrize("field", ["fp", "fq"])
def test_device_build_against_the_model_and_the_host_build(program, tmp_path, field, group):
    secs, dev = device_run(program, field, GROUPS[group], str(tmp_path))
    M.check_results(secs, dev, field)
    _, host = M.run_program(program, "host", field, GROUPS[group], str(tmp_path), HOST_TIMEOUT)
    for op, cs, param in secs:
        d, h = dev[(op, param)], host[(op, param)]
        bad = [i for i in range(len(cs)) if d[i] != h[i]]
        assert not bad, "%s/%s: device and host words differ in %d of %d cases; first: case %d, inputs %s, device %s, host %s" % (
            op, field, len(bad), len(cs), bad[0], cs.ins[bad[0]], d[bad[0]], h[bad[0]])


@pytest.mark.parametrize("field", ["fp", "fq"])
def test_device_only_operations_against_the_model(program, tmp_path, field):
    secs, dev = device_run(program, field, M.DEVICE_GROUPS["quad"], str(tmp_path))
    assert {op for op, _, _ in secs} == set(M.DEVICE_ONLY) and len(secs) == 2 + len(M.SHFL_DISTANCES)
    M.check_results(secs, dev, field)          # includes: the four lanes of every quad hold identical words
