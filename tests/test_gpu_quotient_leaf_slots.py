"""Column leaves in slots (csrc/quotient_compiler.hpp, Compiler2::select_leaves; BZH_VM2_LEAF) change no proof byte: the
builtin kernel generated from the leaf-slot program, the interpreter running that same program, and the interpreter running
the BZH_VM2_LEAF=0 program (every use of a column loads it, as before) give the same proofs of the reference's real circuits
at their smallest tables -- ShotCircuit k = 11 (benches/shot.rs:22), BoardCircuit k = 12 (benches/board.rs:22) -- for the same
witnesses and randomness streams, and bzh_verify_batch accepts them.  (Byte equality with the ORACLE prover at these sizes:
tests/test_gpu_real_circuit_parity.py, which runs on the leaf-slot program since it is the default.)  The program is compiled
when a key is created and BZH_VM2_LEAF is read then, so one process holds both keys."""
import os

import pytest

from helpers import real_parity as R

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("kind,k", [("shot", 11), ("board", 12)])
def test_leaf_slot_program_changes_no_proof_byte(gpu_ctx, kind, k):
    import bzh2
    from bzh2 import circuits as Cm, native as N, params as Pm
    lay = Cm.CircuitLayout(Cm.SHOT if kind == "shot" else Cm.BOARD, k)
    prm = Pm.Params(gpu_ctx, k)
    old = os.environ.pop("BZH_VM2_LEAF", None)
    pks = []
    try:
        pk = N.NativeProvingKey(gpu_ctx, lay.blob(), bzh2.CURVE_VESTA, params=prm)
        pks.append(pk)
        os.environ["BZH_VM2_LEAF"] = "0"
        pk0 = N.NativeProvingKey(gpu_ctx, lay.blob(), bzh2.CURVE_VESTA, params=prm)
        pks.append(pk0)
        del os.environ["BZH_VM2_LEAF"]
        st, st0 = pk.quotient_stats(), pk0.quotient_stats()
        assert st["leaf_slots"] > 0 and st0["leaf_slots"] == 0
        assert st["loads_per_row"] < st0["loads_per_row"] and st["multiplications_per_row"] == st0["multiplications_per_row"]
        assert pk.quotient_selected() == (N.QUOTIENT_BUILTIN, True), "the key did not pick up the kernel generated at build time"
        assert pk0.quotient_selected() == (N.QUOTIENT_INTERPRETER, False)   # another program: no builtin kernel
        circuits = (R.shot_circuits if kind == "shot" else R.board_circuits)(Cm, 500 * k + 3, 2)
        adv, insts = lay.synthesize(circuits)
        streams = [R.rng_stream("leaf-slots-%s-%d-%d" % (kind, k, b), pk.rng_bytes) for b in range(2)]
        builtin = pk.prove_batch(adv, insts, streams)
        without = pk0.prove_batch(adv, insts, streams)
        pk.quotient_select(N.QUOTIENT_INTERPRETER)
        interp = pk.prove_batch(adv, insts, streams)
        assert builtin == without, "builtin kernel (leaf slots) against the interpreter on the BZH_VM2_LEAF=0 program"
        assert builtin == interp, "builtin kernel against the interpreter on the same leaf-slot program"
        assert len(set(builtin)) == 2
        assert pk.verify_batch(insts, builtin) == [True, True] and pk0.verify_batch(insts, without) == [True, True]
    finally:
        os.environ.pop("BZH_VM2_LEAF", None)
        if old is not None:
            os.environ["BZH_VM2_LEAF"] = old
        for p in pks:
            p.close()
        prm.close()
        lay.close()
