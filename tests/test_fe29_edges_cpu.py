"""The unsaturated 9 x 29-bit field and curve code (csrc/fe29.cuh, csrc/curve29.cuh) on the host, operation by operation, with
operands ON the documented bounds: tests/helpers/fe29_ops.hip applies one operation to every case of an operand file and
tests/helpers/fe29_model.py -- Python integers only -- says what the result must be: the exact value or residue, the documented
output bounds, and for the curve operations the affine point of oracle/pasta.py's group law.  The model asserts the documented
precondition on every case it emits.  The device build of the same functions: tests/test_gpu_fe29_edges.py."""
import pytest

from helpers import fe29_model as M

COMPILE_TIMEOUT = 210     # seconds: three times the first measured compile of this program (68 s)
RUN_TIMEOUT = 10          # seconds: the slowest measured host run of one group took 0.2 s (three times that is under 1 s) plus room
                          # for a loaded machine
GROUPS = dict(M.FIELD_GROUPS, **M.CURVE_GROUPS)


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = M.build_program(str(tmp_path_factory.mktemp("fe29_ops") / "fe29_ops"), COMPILE_TIMEOUT)
    if exe is None:
        pytest.skip("no hipcc")
    return exe


@pytest.mark.parametrize("group", sorted(GROUPS))
@pytest.mark.parametrize("field", ["fp", "fq"])
def test_host_build_against_the_integer_model(program, tmp_path, field, group):
    secs, res = M.run_program(program, "host", field, GROUPS[group], str(tmp_path), RUN_TIMEOUT)
    M.check_results(secs, res, field)


@pytest.mark.parametrize("field", ["fp", "fq"])
def test_every_operation_has_cases_on_a_bound(field):
    for group in list(GROUPS.values()) + list(M.DEVICE_GROUPS.values()):
        for op, (n, on) in M.census(group, field).items():
            assert n > 0 and on > 0, (op, n, on)
    # the special-case filters: every reachable multiple of p at their edges shows in limb 0 of some case with equal x
    assert {5, 17} <= M.cases("madd_q29", field).filter_ks and 18 not in M.cases("madd_q29", field).filter_ks
    for op in ("add", "add_nocall", "add_quad"):
        assert M.cases(op, field).filter_ks == {3, 4, 5}, op


def test_the_program_refuses_a_device_only_operation_on_the_host(program, tmp_path):
    with pytest.raises(RuntimeError):
        M.run_program(program, "host", "fp", ["from_sat_quad"], str(tmp_path), RUN_TIMEOUT)
