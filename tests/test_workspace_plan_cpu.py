"""bzh_workspace_plan / bzh_workspace_plan_items (host only): the arena bytes one prove call takes under BZH_WORKSPACE_EXTENDED and
BZH_WORKSPACE_COSETWISE for the Shot and Board circuits.  The figures are computed, not measured; what is checked is their shape:
strictly increasing in the batch, COSETWISE below EXTENDED, and the two apart by exactly 7/8 of the extended-coset term the plan
itself itemises.  Also the header / exports / Python-mirror agreement for the new names."""
import ctypes
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCHES = (1, 2, 3, 8, 64, 65, 1000)
NAMES = ("bzh_pk_workspace_select", "bzh_pk_workspace_selected", "bzh_workspace_plan", "bzh_workspace_plan_items", "bzh_pk_workspace_peak",
         "bzh_vm2_eval_cosets")
_blobs = {}


def blob(name):
    if name not in _blobs:
        from bzh2 import circuits as Cm
        lay = Cm.CircuitLayout(Cm.SHOT if name == "shot" else Cm.BOARD, 11 if name == "shot" else 12)
        _blobs[name] = lay.blob()
        lay.close()
    return _blobs[name]


def test_names_are_declared_exported_and_mirrored():
    import bzh2
    from bzh2 import native as N
    header = open(os.path.join(ROOT, "include", "bzh2.h")).read()
    for name in NAMES:
        assert "int %s(" % name in header and name in bzh2.EXPORTS
    assert (N.WORKSPACE_EXTENDED, N.WORKSPACE_COSETWISE) == (0, 1)
    assert "BZH_WORKSPACE_EXTENDED = 0, BZH_WORKSPACE_COSETWISE = 1" in header
    for attr in ("workspace_select", "workspace_selected", "workspace_plan", "workspace_peak"):
        assert hasattr(N.NativeProvingKey, attr)
    assert hasattr(bzh2.Context, "vm2_eval_cosets")


@pytest.mark.parametrize("name", ["shot", "board"])
def test_the_plan_grows_with_the_batch_and_cosetwise_is_below_extended(name):
    import bzh2
    from bzh2 import native as N
    b = blob(name)
    last = {N.WORKSPACE_EXTENDED: 0, N.WORKSPACE_COSETWISE: 0}
    for batch in BATCHES:
        ext, cw = (N.workspace_plan(bzh2.CURVE_VESTA, b, batch, m) for m in (N.WORKSPACE_EXTENDED, N.WORKSPACE_COSETWISE))
        assert ext > last[N.WORKSPACE_EXTENDED] and cw > last[N.WORKSPACE_COSETWISE] and 0 < cw < ext
        last = {N.WORKSPACE_EXTENDED: ext, N.WORKSPACE_COSETWISE: cw}
        ie, ic = (N.workspace_plan_items(bzh2.CURVE_VESTA, b, batch, m) for m in (N.WORKSPACE_EXTENDED, N.WORKSPACE_COSETWISE))
        assert ie["total_bytes"] == ext and ic["total_bytes"] == cw
        for it in (ie, ic):
            assert it["total_bytes"] == it["cosets_bytes"] + it["witness_bytes"] + it["quotient_bytes"] + it["tail_bytes"] + it["staging_bytes"]
            assert it["extended"] == 8 * it["n"] and it["n"] == 1 << (11 if name == "shot" else 12)
        # the term the mode changes: per-proof columns where the quotient reads them
        assert ie["cosets_bytes"] == ie["cosets_extended_bytes"] == ic["cosets_extended_bytes"]
        assert ie["cosets_bytes"] == batch * ie["columns"] * ie["column_bytes"] and ie["column_bytes"] == 32 * ie["extended"]
        assert ic["cosets_bytes"] == batch * ic["columns"] * ic["column_bytes"] and ic["column_bytes"] == 32 * ic["n"]
        assert ie["cosets_extended_bytes"] % 8 == 0
        assert ext - cw == ie["cosets_extended_bytes"] // 8 * 7
        for key in ("witness_bytes", "quotient_bytes", "tail_bytes", "staging_bytes", "columns"):
            assert ie[key] == ic[key]


def test_refusals():
    import bzh2
    from bzh2 import native as N
    b = blob("shot")
    for mode in (2, -1, 7):
        with pytest.raises(bzh2.BzhError) as e:
            N.workspace_plan(bzh2.CURVE_VESTA, b, 3, mode)
        assert e.value.status == bzh2.E_ARG
    for cut in (0, 1, 16, len(b) // 2, len(b) - 1):
        for mode in (N.WORKSPACE_EXTENDED, N.WORKSPACE_COSETWISE):
            with pytest.raises(bzh2.BzhError) as e:
                N.workspace_plan(bzh2.CURVE_VESTA, b[:cut], 3, mode)
            assert e.value.status == bzh2.E_ARG, "blob cut to %d bytes" % cut
    for batch in (0, 65536):
        with pytest.raises(bzh2.BzhError) as e:
            N.workspace_plan(bzh2.CURVE_VESTA, b, batch, N.WORKSPACE_COSETWISE)
        assert e.value.status == bzh2.E_ARG
    L = bzh2.load()
    L.bzh_workspace_plan.argtypes = [ctypes.c_int, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    assert L.bzh_workspace_plan(bzh2.CURVE_VESTA, b, len(b), 3, 0, None) == bzh2.E_ARG
    assert L.bzh_workspace_plan(bzh2.CURVE_VESTA, None, len(b), 3, 0, None) == bzh2.E_ARG
