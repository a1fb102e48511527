"""The lookup argument's permutation runs on the device on every new key (csrc/lookup_permute.hip), and the prover reads the
per-proof status words only when the lookup's commitments come back: the reference's ShotCircuit (k = 11, 10-bit range lookup),
seeded proofs, an untouched key against a key switched to LOOKUP_HOST.

An untouched key chooses per call -- the device from 8 proofs up, the host path below (kLookupDeviceMinBatch, csrc/prover.hpp) --
so the batches of 3 and 1 on it are joined by a batch of 8, and the failure cases also run on a key switched to LOOKUP_DEVICE,
where a batch of 3 takes the device path and its deferred status.

One key of each kind, one synthesis and one set of host-path proofs serve every test of the module."""
import pytest

import pasta as O
from helpers import field_edges as FE

pytestmark = pytest.mark.gpu


def _eval(e, adv, fixed, row, n, p):
    tag = e[0]
    if tag == "const":
        return e[1] % p
    if tag in ("advice", "fixed"):
        col = adv[e[1]] if tag == "advice" else fixed[e[1]]
        return col[(row + e[2]) % n]
    assert tag != "instance"
    if tag == "neg":
        return -_eval(e[1], adv, fixed, row, n, p) % p
    if tag == "scale":
        return _eval(e[1], adv, fixed, row, n, p) * e[2] % p
    x, y = _eval(e[1], adv, fixed, row, n, p), _eval(e[2], adv, fixed, row, n, p)
    return (x + y) % p if tag == "add" else x * y % p


def _advice_queries(e, out):
    if e[0] == "advice":
        out.append((e[1], e[2]))
    elif e[0] in ("neg", "scale"):
        _advice_queries(e[1], out)
    elif e[0] in ("add", "mul"):
        _advice_queries(e[1], out)
        _advice_queries(e[2], out)
    return out


class _Case:
    pass


@pytest.fixture(scope="module")
def case(gpu_ctx):
    import blob as Bm
    import bzh2
    from bzh2 import circuits as Cm, native as N, params as Pm
    from helpers import real_parity as RP
    c = _Case()
    c.N = N
    lay = Cm.CircuitLayout(Cm.SHOT, 11)
    prm = Pm.Params(gpu_ctx, 11)
    c.fresh = N.NativeProvingKey(gpu_ctx, lay.blob(), bzh2.CURVE_VESTA, params=prm)     # lookup_select is never called on it
    host = N.NativeProvingKey(gpu_ctx, lay.blob(), bzh2.CURVE_VESTA, params=prm)
    c.device = N.NativeProvingKey(gpu_ctx, lay.blob(), bzh2.CURVE_VESTA, params=prm)
    try:
        c.selected_at_creation = c.fresh.lookup_selected()
        c.adv, c.insts = lay.synthesize(RP.shot_circuits(Cm, 77, 3))
        c.seeds = [bytes([17 + b]) * 32 for b in range(3)]
        host.lookup_select(N.LOOKUP_HOST)
        assert host.lookup_selected() == N.LOOKUP_HOST
        c.device.lookup_select(N.LOOKUP_DEVICE)
        c.host = host
        c.host3 = host.prove_batch(c.adv, c.insts, None, seeds=c.seeds)
        c.host1 = host.prove_batch(c.adv[:1], c.insts[:1], None, seeds=c.seeds[:1])
        c.circ = Bm.decode(lay.blob())
        yield c
    finally:
        host.close()
        c.device.close()
        c.fresh.close()
        prm.close()
        lay.close()


def _bad_advice(c, proof):
    """the batch's advice with one lookup input of `proof` pushed out of the table: one cell of the column the lookup reads, on
    a row where the lookup is enabled (tests/test_gpu_lookup_permute.py builds it the same way)"""
    circ, adv = c.circ, c.adv
    p, n, usable = O.FP.p, circ.n, c.fresh.usable_rows
    (ins, tabs), = circ.lookups
    assert len(ins) == 1
    cols = [FE.array_to_ints(adv[proof, k]) for k in range(adv.shape[1])]
    table = {_eval(tabs[0], cols, circ.fixed, r, n, p) for r in range(usable)}
    values = [_eval(ins[0], cols, circ.fixed, r, n, p) for r in range(usable)]
    assert all(v in table for v in values)
    row = next(r for r in range(usable) if values[r])
    col = next(k for k, rot in _advice_queries(ins[0], []) if rot == 0)
    cols[col][row] = (cols[col][row] + (1 << 100)) % p
    assert _eval(ins[0], cols, circ.fixed, row, n, p) not in table
    bad = adv.copy()
    bad[proof, col, row] = FE.ints_to_array([cols[col][row]])[0]
    return bad


def test_a_fresh_key_permutes_on_the_device_and_gives_the_host_paths_bytes(case):
    c = case
    assert c.selected_at_creation == c.N.LOOKUP_DEVICE and c.fresh.lookup_selected() == c.N.LOOKUP_DEVICE
    proofs = c.fresh.prove_batch(c.adv, c.insts, None, seeds=c.seeds)
    assert proofs == c.host3 and len(set(proofs)) == 3
    assert c.fresh.verify_batch(c.insts, proofs) == [True] * 3


def test_a_batch_of_one_on_a_fresh_key_gives_the_host_paths_bytes(case):
    c = case
    proofs = c.fresh.prove_batch(c.adv[:1], c.insts[:1], None, seeds=c.seeds[:1])
    assert proofs == c.host1
    assert c.fresh.verify_batch(c.insts[:1], proofs) == [True]
    assert c.fresh.lookup_selected() == c.N.LOOKUP_DEVICE


def test_a_batch_at_the_device_threshold_on_a_fresh_key_gives_the_host_paths_bytes(case):
    """8 proofs (the 3 witnesses cycled, a seed of its own each): the untouched key takes the device path"""
    c = case
    idx = [b % 3 for b in range(8)]
    adv, insts = c.adv[idx], [c.insts[i] for i in idx]
    seeds = [bytes([40 + b]) * 32 for b in range(8)]
    proofs = c.fresh.prove_batch(adv, insts, None, seeds=seeds)
    assert proofs == c.host.prove_batch(adv, insts, None, seeds=seeds) and len(set(proofs)) == 8
    assert c.fresh.verify_batch(insts, proofs) == [True] * 8
    bad = adv.copy()
    bad[7] = _bad_advice(c, 1)[1]            # proof 7 is witness 1 again
    import bzh2
    with pytest.raises(bzh2.BzhError) as e:
        c.fresh.prove_batch(bad, insts, None, seeds=seeds)
    assert e.value.status == bzh2.E_RANGE
    assert c.fresh.prove_batch(adv, insts, None, seeds=seeds) == proofs


@pytest.mark.parametrize("key", ["fresh", "device"])
def test_a_failed_lookup_is_e_range_and_leaves_nothing_behind(case, key):
    """proof 1 of 3 fails; the same key and context then give the earlier bytes twice: no pending read-back, no stale status"""
    import bzh2
    c = case
    pk = getattr(c, key)
    with pytest.raises(bzh2.BzhError) as e:
        pk.prove_batch(_bad_advice(c, 1), c.insts, None, seeds=c.seeds)
    assert e.value.status == bzh2.E_RANGE
    assert pk.prove_batch(c.adv, c.insts, None, seeds=c.seeds) == c.host3
    assert pk.prove_batch(c.adv, c.insts, None, seeds=c.seeds) == c.host3


@pytest.mark.parametrize("key", ["fresh", "device"])
@pytest.mark.parametrize("proof", [2, 0])
def test_the_deferred_status_is_read_for_every_proof(case, proof, key):
    """the failing proof last and first in the batch: the status words are looked at per proof after they have landed"""
    import bzh2
    c = case
    pk = getattr(c, key)
    with pytest.raises(bzh2.BzhError) as e:
        pk.prove_batch(_bad_advice(c, proof), c.insts, None, seeds=c.seeds)
    assert e.value.status == bzh2.E_RANGE
    assert pk.prove_batch(c.adv, c.insts, None, seeds=c.seeds) == c.host3
