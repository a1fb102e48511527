"""bzh_prove_shots_device / bzh_prove_boards_device on the GPU: game inputs in, proofs out, in one device-resident call, against
the two paths that exist -- device synthesis (bzh_synthesize_*_with, BZH_SYNTH_DEVICE) followed by bzh_prove_batch_device_seeded,
and host synthesis followed by bzh_prove_batch_seeded -- on the same inputs and seeds.  Every comparison is exact: proofs, lengths,
instances and status bytes.  Shot runs at k = 11 and Board at k = 12, the smallest sizes the circuits fit; one Params and one key
per circuit serve the module.  The game inputs are tests/helpers/prove_game_cases.py's, every candidate classified alone through
the host path."""
import copy

import pytest

from helpers import prove_game_cases as G

pytestmark = pytest.mark.gpu

E_ARG, E_RANGE = -1, -4
SYNTHESIS_TEXTS = {"incomplete addition: exceptional case": 1 << 4, "fixed-base mul: window point with x = 0": 2 << 4,
                   "pedersen_commit: message repr is not a canonical scalar": 4 << 4}


class Side:
    """one circuit kind: layout, Params, key, the classified candidates"""

    def __init__(self, ctx, kind, k):
        import bzh2
        from bzh2 import circuits as Cm, native as N, params as Pm
        self.ctx, self.kind, self.shot = ctx, kind, kind == "shot"
        self.lay = Cm.CircuitLayout(Cm.SHOT if self.shot else Cm.BOARD, k)
        self.prm = Pm.Params(ctx, k)
        self.pk = N.NativeProvingKey(ctx, self.lay.blob(), bzh2.CURVE_VESTA, params=self.prm)
        game = G.games()
        self.ok, self.bad = G.classify(self.lay, G.shot_cases(game) if self.shot else G.board_cases(game))
        assert len(self.ok) >= 8, "the host path accepts the valid games and the canonical trapdoors"
        # the accepted operands whose witness also satisfies the circuit (the others, a hit claimed on a miss or a board without
        # its ships, synthesize and prove, and the verifier rejects them)
        self.valid = [c for c in self.ok if G.is_valid_game(c, game)]
        assert len(self.valid) >= 8

    def new_key(self):
        import bzh2
        from bzh2 import native as N
        return N.NativeProvingKey(self.ctx, self.lay.blob(), bzh2.CURVE_VESTA, params=self.prm)

    def close(self):
        self.pk.close()
        self.prm.close()
        self.lay.close()

    def one_call(self, circuits, seeds, pk=None, lay=None, want_status=True):
        pk, lay = pk or self.pk, lay or self.lay
        fn = pk.prove_shots_device if self.shot else pk.prove_boards_device
        return fn(lay, circuits, seeds, ctx=self.ctx, want_status=want_status)

    def two_calls(self, circuits, seeds, pk=None):
        """device synthesis into a tensor of the test's, then bzh_prove_batch_device_seeded on it"""
        import torch
        dev = torch.empty((len(circuits), self.lay.num_advice, self.lay.n, 4), dtype=torch.int64, device="cuda")
        dev.fill_(-1)
        torch.cuda.synchronize()
        _, insts = self.lay.synthesize(circuits, ctx=self.ctx, device_ptr=dev.data_ptr(), where="device")
        proofs, st = (pk or self.pk).prove_batch_device(None, insts, seeds=seeds, device_ptr=dev.data_ptr())
        return insts, proofs, st

    def host_path(self, circuits, seeds):
        adv, insts = self.lay.synthesize(circuits)
        return insts, self.pk.prove_batch(adv, insts, None, seeds=seeds)


def seeds_for(n, salt):
    return [bytes((salt + 31 * b + 7 * i) & 0xff for i in range(32)) for b in range(n)]


@pytest.fixture(scope="module")
def sides(gpu_ctx):
    out = {"shot": Side(gpu_ctx, "shot", 11), "board": Side(gpu_ctx, "board", 12)}
    yield out
    for s in out.values():
        s.close()


def cycle(cases, n, first=0):
    return [cases[(first + i) % len(cases)] for i in range(n)]


@pytest.mark.parametrize("kind,batch,host", [("shot", 1, False), ("shot", 3, True), ("shot", 65, False), ("board", 2, True)])
def test_parity_with_the_two_call_path_and_the_host_path(sides, kind, batch, host):
    """proofs, lengths and instances of the one call equal device synthesis + bzh_prove_batch_device_seeded under the same seeds
    (Shot B = 65: a second, partial wave on every one-lane kernel); for Shot B = 3 and Board B = 2 also host synthesis +
    bzh_prove_batch_seeded; the verifier accepts every proof.  The games are the accepted candidates that are valid games."""
    S = sides[kind]
    circuits, seeds = cycle(S.valid, batch, first=batch), seeds_for(batch, batch)
    insts, proofs, st = S.one_call(circuits, seeds)
    print("status", st.tolist(), "lengths", sorted({len(p) for p in proofs}))
    winsts, wproofs, wst = S.two_calls(circuits, seeds)
    assert st.tolist() == [0] * batch and wst.tolist() == [0] * batch
    assert insts == winsts
    assert [len(p) for p in proofs] == [len(p) for p in wproofs] and proofs == wproofs
    if host:
        hinsts, hproofs = S.host_path(circuits, seeds)
        assert insts == hinsts and proofs == hproofs
    assert S.pk.verify_batch(insts, proofs) == [True] * batch


def test_a_wrong_hit_claim_is_its_own_proofs_affair(sides):
    """a hit claim of 1 on a miss at position 1 of 3: the status byte and the proof bytes are the two-call path's for that witness,
    the verifier rejects that proof alone, and the other two equal their single-proof runs"""
    from bzh2 import circuits as Cm
    S = sides["shot"]
    state = S.valid[0].board
    miss = next(i for i in range(100) if not state.value >> i & 1)
    wrong = Cm.ShotCircuit(state, 0x77aa55, G.bv(1 << miss), G.bv(1))
    circuits, seeds = [S.valid[1], wrong, S.valid[5]], seeds_for(3, 40)
    insts, proofs, st = S.one_call(circuits, seeds)
    winsts, wproofs, wst = S.two_calls(circuits, seeds)
    print("status", st.tolist(), "two-call status", wst.tolist())
    assert st.tolist() == wst.tolist() and insts == winsts and proofs == wproofs
    assert insts[1][0][3] == 1
    assert S.pk.verify_batch(insts, proofs) == [True, False, True]
    for b in (0, 2):
        i1, p1, s1 = S.one_call([circuits[b]], [seeds[b]])
        assert (i1[0], p1[0], s1.tolist()) == (insts[b], proofs[b], [0])


@pytest.mark.parametrize("kind", ["shot", "board"])
def test_a_proof_flagged_by_the_synthesis(sides, kind):
    """An operand the host path refuses AFTER running the synthesis (one of the three status-word refusals) at positions 0 and 2
    of a batch of 3: with `status` the call returns OK, that proof alone carries the matching bit at 4 .. 6, the clean proof's
    bytes are those of its own run; with status=None the call is BZH_E_RANGE with the host's text and nothing comes back.

    None of the classified candidates (tests/helpers/prove_game_cases.py) has such a refusal today: the only one the host path
    refuses is the trapdoor 2^255 - 1, on sight ("trapdoor is not a canonical scalar"), which is
    test_input_only_refusals_carry_the_hosts_text's subject.  Reaching an exceptional addition or a window point with x = 0 needs a
    scalar chosen against the fixed bases' discrete logarithms, and a Shot message is 128 bits and always canonical.  Until a
    candidate has one, the cover of bits 4 .. 6 is the fold's CPU test (tests/test_prove_game_cpu.py, all 8 x 16 combinations) and
    this test only checks the classification it rests on."""
    import bzh2
    S = sides[kind]
    flagged = [(c, text) for c, st, text in S.bad if any(t in text for t in SYNTHESIS_TEXTS)]
    assert all(st == E_RANGE for _, st, _ in S.bad)
    for c, text in flagged[:1]:
        bit = next(v for t, v in SYNTHESIS_TEXTS.items() if t in text)
        circuits, seeds = [c, S.ok[2], c], seeds_for(3, 50)
        insts, proofs, st = S.one_call(circuits, seeds)
        print("status", st.tolist())
        assert st[1] == 0 and (st[0] & 0x70) == bit and (st[2] & 0x70) == bit
        assert all(len(p) == len(proofs[1]) for p in proofs)
        i1, p1, _ = S.one_call([circuits[1]], [seeds[1]])
        assert (insts[1], proofs[1]) == (i1[0], p1[0])
        with pytest.raises(bzh2.BzhError) as e:
            S.one_call(circuits, seeds, want_status=False)
        assert e.value.status == E_RANGE and "proof 0" in str(e.value) and str(e.value).endswith(text.split(": ", 2)[2])


@pytest.mark.parametrize("kind", ["shot", "board"])
def test_input_only_refusals_carry_the_hosts_text(sides, kind):
    """a trapdoor equal to q and one equal to 2^256 - 1 at positions 0, 2 and 4 of 5: BZH_E_RANGE with the host path's text, and
    after each refusal a clean batch on the same ctx and key proves correctly"""
    import bzh2
    S = sides[kind]
    clean, cseeds = S.ok[:2], seeds_for(2, 60)
    want = S.one_call(clean, cseeds)
    assert want[1] == S.two_calls(clean, cseeds)[1]
    for bad in (G.FQ, (1 << 256) - 1):
        for pos in (0, 2, 4):
            group = [copy.copy(c) for c in S.ok[:5]]
            group[pos].board_commitment_trapdoor = bad
            with pytest.raises(bzh2.BzhError) as host:
                S.lay.synthesize(group)
            with pytest.raises(bzh2.BzhError) as dev:
                S.one_call(group, seeds_for(5, 61))
            assert host.value.status == E_RANGE and dev.value.status == E_RANGE
            assert "trapdoor is not a canonical scalar" in str(host.value)
            assert str(dev.value).split(": ", 1)[1] == str(host.value).split(": ", 1)[1]
            got = S.one_call(clean, cseeds)
            assert got[0] == want[0] and got[1] == want[1] and got[2].tolist() == [0, 0]


def test_a_circuit_that_is_not_the_keys_is_refused(sides):
    """a Board layout with the Shot key, and a Shot layout at k = 12 with the k = 11 key: BZH_E_ARG, the key usable afterwards"""
    import bzh2
    from bzh2 import circuits as Cm
    S, Bd = sides["shot"], sides["board"]
    circuits, seeds = S.valid[:2], seeds_for(2, 70)
    want = S.one_call(circuits, seeds)
    with pytest.raises(bzh2.BzhError) as e:
        S.pk.prove_boards_device(Bd.lay, Bd.ok[:2], seeds, ctx=S.ctx)
    assert e.value.status == E_ARG
    shot12 = Cm.CircuitLayout(Cm.SHOT, 12)
    try:
        with pytest.raises(bzh2.BzhError) as e:
            S.one_call(circuits, seeds, lay=shot12)
        assert e.value.status == E_ARG
    finally:
        shot12.close()
    got = S.one_call(circuits, seeds)
    assert got[0] == want[0] and got[1] == want[1]
    assert S.pk.verify_batch(got[0], got[1]) == [True, True]


def test_a_cold_workspace(sides):
    """a key that has served no call: batches of 3, then 5 (the first call leaves the workspace as a list of blocks, the second
    merges them and grows), then bzh_prove_batch_device_seeded on the same key and ctx; all against the module's warm key.  The
    operands are all the accepted candidates, valid games or not: the comparison is of bytes"""
    S = sides["shot"]
    pk = S.new_key()
    try:
        for batch in (3, 5):
            circuits, seeds = cycle(S.ok, batch, first=9), seeds_for(batch, 80 + batch)
            insts, proofs, st = S.one_call(circuits, seeds, pk=pk)
            winsts, wproofs, _ = S.two_calls(circuits, seeds)
            assert st.tolist() == [0] * batch and insts == winsts and proofs == wproofs
        circuits, seeds = cycle(S.ok, 2, first=3), seeds_for(2, 90)
        _, proofs, st = S.two_calls(circuits, seeds, pk=pk)
        assert st.tolist() == [0, 0] and proofs == S.one_call(circuits, seeds)[1]
    finally:
        pk.close()
