"""The verifier's per-proof pass on the device (BZH_VERIFY_PASS_DEVICE: csrc/verify_pass.hip over the key's scalar program,
one transcript batch, one decompression launch) against the host pass and the oracle's verifier: tests/helpers/vk_cases.py's
k = 5 sample circuit with 0, 1 and 2 instance columns, batches of 1, 3 and 65 (one full wave and one lane), through a proving
key and through a verifying key with and without g_lagrange, with the damaged proofs of tests/helpers/verify_pass_cases.py at
lane 0, at lane 64 and between valid neighbours; and the reference's Shot circuit at k = 11."""
import numpy as np
import pytest

import coracle as C
from helpers import real_parity as R
from helpers import verify_pass_cases as VP
from helpers import vk_cases as V

pytestmark = pytest.mark.gpu
E_ARG = -1


class _Srs:
    def __init__(self, ctx, k):
        import bzh2
        from bzh2 import params as Pm
        g, w, u = V.srs(k)
        self.g, self.w, self.u = g, w, u
        garr = C.points_to_array(g)
        uw = C.points_to_array([u, w])
        self.bases = ctx.upload_bases(bzh2.CURVE_VESTA, np.concatenate([garr, uw])).precompute(0)
        self.bases_lagrange = ctx.upload_bases(bzh2.CURVE_VESTA, np.concatenate([Pm.group_ifft(ctx, garr), uw])).precompute(0)
        self.g0_u_w = np.ascontiguousarray(np.stack([garr[0], uw[0], uw[1]]))

    def close(self):
        self.bases.free()
        self.bases_lagrange.free()


def _prove(ctx, srs, k, num_instance, count):
    import bzh2
    from bzh2 import native as N
    cases = [V.circuit(k, 70 + b, num_instance) for b in range(count)]
    pk = N.NativeProvingKey(ctx, cases[0][5], bzh2.CURVE_VESTA, srs.g, srs.w, srs.u)
    n = 1 << k
    adv = np.stack([np.stack([C.ints_to_array(list(col) + [0] * (n - len(col))) for col in cse[3]]) for cse in cases])
    insts = [[list(col) for col in cse[4]] for cse in cases]
    rbs = [R.rng_stream("vpass-%d-%d-%d" % (k, num_instance, b), pk.rng_bytes) for b in range(count)]
    return pk, insts, pk.prove_batch(adv, insts, rbs)


@pytest.fixture(scope="module")
def world(gpu_ctx):
    """per instance-column count: (pk, vk, instances, proofs) of three valid proofs from the library's prover; one k = 6 proof"""
    from bzh2 import native as N
    srs5, srs6 = _Srs(gpu_ctx, V.K), _Srs(gpu_ctx, 6)
    pk6, _, proofs6 = _prove(gpu_ctx, srs6, 6, 1, 1)
    pk6.close()
    srs6.close()
    w = {"srs": srs5, "k6": proofs6[0]}
    for ni in (0, 1, 2):
        pk, insts, proofs = _prove(gpu_ctx, srs5, V.K, ni, 3)
        assert pk.verify_pass_selected() == N.VERIFY_PASS_HOST                  # every new key's default
        w[ni] = (pk, N.NativeVerifyingKey.from_pk(pk), insts, proofs)
    yield w
    for ni in (0, 1, 2):
        w[ni][1].close()
        w[ni][0].close()
    srs5.close()


def _both_ways(ctx, w, ni, insts, proofs):
    """results[] of one batch: (host pass through the pk, device pass through the pk, the vk with g_lagrange, the vk without)"""
    from bzh2 import native as N
    pk, vk, _, _ = w[ni]
    srs = w["srs"]
    host = pk.verify_batch(insts, proofs)
    pk.verify_pass_select(N.VERIFY_PASS_DEVICE)
    try:
        assert pk.verify_pass_selected() == N.VERIFY_PASS_DEVICE
        dev = pk.verify_batch(insts, proofs)
    finally:
        pk.verify_pass_select(N.VERIFY_PASS_HOST)
    assert pk.verify_pass_selected() == N.VERIFY_PASS_HOST
    vk_lag = vk.verify_batch(ctx, srs, insts, proofs, lagrange=True, g0_u_w=srs.g0_u_w, pass_where=N.VERIFY_PASS_DEVICE)
    vk_coeff = vk.verify_batch(ctx, srs, insts, proofs, lagrange=False, g0_u_w=srs.g0_u_w, pass_where=N.VERIFY_PASS_DEVICE)
    vk_host = vk.verify_batch(ctx, srs, insts, proofs, g0_u_w=srs.g0_u_w, pass_where=N.VERIFY_PASS_HOST)
    assert vk_host == host == vk.verify_batch(ctx, srs, insts, proofs, g0_u_w=srs.g0_u_w)
    return host, dev, vk_lag, vk_coeff


def _batches(w, ni, batch):
    """[(name, instances, proofs, expected)]: expected by construction -- a valid proof with its own instances verifies, nothing
    else does (test_the_oracle_verifier_decides_the_same pins that against the oracle)"""
    _, _, insts, proofs = w[ni]
    bad = [pr for _, pr, _ in VP.damaged(ni, proofs[1], w["k6"])]
    out = []
    if batch == 1:
        out.append(("a valid proof", [insts[0]], [proofs[0]], [True]))
        for d in (bad[1], bad[5], bad[10]):
            out.append(("a damaged proof alone", [insts[1]], [d], [False]))
    elif batch == 3:
        for i, d in enumerate(bad):
            out.append(("damaged %d between valid neighbours" % i, [insts[0], insts[1], insts[2]], [proofs[0], d, proofs[2]], [True, False, True]))
        out.append(("damaged at lane 0", [insts[1], insts[0], insts[2]], [bad[3], proofs[0], proofs[2]], [False, True, True]))
        if ni:
            out.append(("instances swapped", [insts[1], insts[0], insts[2]], list(proofs), [False, False, True]))
        out.append(("every proof damaged", [insts[1]] * 3, [bad[0], bad[8], bad[11]], [False] * 3))
    else:
        ii = [insts[b % 3] for b in range(65)]
        pp = [proofs[b % 3] for b in range(65)]
        want = [True] * 65
        lanes = [0, 64] + list(range(2, 2 * len(bad) - 2, 2))              # lane 0, lane 64, then every other lane: valid neighbours
        for lane, d in zip(lanes, bad):
            ii[lane], pp[lane], want[lane] = insts[1], d, False
        if ni:                                                             # two neighbours' instances swapped, far from the rest
            ii[40], ii[41], want[40], want[41] = ii[41], ii[40], False, False
        out.append(("one wave and one lane", ii, pp, want))
    return out


@pytest.mark.parametrize("batch", [1, 3, 65])
@pytest.mark.parametrize("num_instance", [0, 1, 2])
def test_device_pass_equals_host_pass(gpu_ctx, world, num_instance, batch):
    for name, ii, pp, want in _batches(world, num_instance, batch):
        host, dev, vk_lag, vk_coeff = _both_ways(gpu_ctx, world, num_instance, ii, pp)
        assert host == want, (name, host, want)
        assert dev == host and vk_lag == host and vk_coeff == host, (name, dev, vk_lag, vk_coeff, host)


def test_the_oracle_verifier_decides_the_same(gpu_ctx, world):
    """the oracle's verify_proof on the valid proofs of every circuit and on every damaged proof of the one-instance-column
    circuit: what _batches expects by construction is what the oracle decides"""
    for ni in (0, 1, 2):
        _, _, insts, proofs = world[ni]
        assert VP.oracle_accepts(ni, insts[0], proofs[0])
    _, _, insts, proofs = world[1]
    assert not VP.oracle_accepts(1, insts[0], proofs[1])                   # the neighbour's instances
    for name, pr, _ in VP.damaged(1, proofs[1], world["k6"]):
        assert not VP.oracle_accepts(1, insts[1], pr), name


def test_selector(gpu_ctx, world):
    from bzh2 import BzhError, native as N
    pk = world[1][0]
    assert pk.verify_pass_selected() == N.VERIFY_PASS_HOST
    pk.verify_pass_select(N.VERIFY_PASS_DEVICE)
    for bad in (2, -1, 7):
        with pytest.raises(BzhError) as e:
            pk.verify_pass_select(bad)
        assert e.value.status == E_ARG and pk.verify_pass_selected() == N.VERIFY_PASS_DEVICE
    pk.verify_pass_select(N.VERIFY_PASS_HOST)
    with pytest.raises(BzhError) as e:
        pk.verify_pass_select(2)
    assert e.value.status == E_ARG and pk.verify_pass_selected() == N.VERIFY_PASS_HOST
    with pytest.raises(BzhError):
        pk.verify_select(2)                                                # the points selector keeps its two values
    # the pass implies device decompression whatever the points selector says
    _, _, insts, proofs = world[1]
    for points in (N.VERIFY_POINTS_DEVICE, N.VERIFY_POINTS_HOST):
        pk.verify_select(points)
        pk.verify_pass_select(N.VERIFY_PASS_DEVICE)
        try:
            assert pk.verify_batch(insts, proofs) == [True] * 3
        finally:
            pk.verify_pass_select(N.VERIFY_PASS_HOST)
    vk, srs = world[1][1], world["srs"]
    with pytest.raises(BzhError) as e:
        vk.verify_batch(gpu_ctx, srs, insts, proofs, g0_u_w=srs.g0_u_w, pass_where=2)
    assert e.value.status == E_ARG
    assert vk.device_bytes()[0] == 0                                       # the program's device copy is workspace, not key


def test_the_references_shot_circuit(gpu_ctx):
    import bzh2
    from bzh2 import circuits as Cm, native as N, params as Pm
    lay = Cm.CircuitLayout(Cm.SHOT, 11)
    prm = Pm.Params(gpu_ctx, 11)
    keys = []
    try:
        adv, insts = lay.synthesize(R.shot_circuits(Cm, 911, 2))
        seeds = [R.rng_stream("vpass-shot-%d" % b, 32) for b in range(2)]
        pk = N.NativeProvingKey(gpu_ctx, lay.blob(), bzh2.CURVE_VESTA, params=prm)
        keys.append(pk)
        proofs = pk.prove_batch(adv, insts, None, seeds=seeds)
        tampered = [proofs[0], proofs[1][:200] + bytes([proofs[1][200] ^ 1]) + proofs[1][201:]]
        vk = N.NativeVerifyingKey.from_pk(pk)
        keys.append(vk)
        for pp, want in ((proofs, [True, True]), (tampered, [True, False])):
            host = vk.verify_batch(gpu_ctx, prm, insts, pp, pass_where=N.VERIFY_PASS_HOST)
            dev = vk.verify_batch(gpu_ctx, prm, insts, pp, pass_where=N.VERIFY_PASS_DEVICE)
            assert host == dev == want, (host, dev, want)
    finally:
        for k_ in keys:
            k_.close()
        prm.close()
        lay.close()
