"""BZH_WORKSPACE_COSETWISE (bzh_pk_workspace_select) on the GPU: the quotient evaluated coset by coset out of n-sized buffers is
the same polynomial as the quotient over the whole extended coset, so every proof must come out byte for byte as under
BZH_WORKSPACE_EXTENDED -- through bzh_prove_batch_seeded, bzh_prove_batch_device_seeded and bzh_prove_shots_device on the real
Shot circuit at k = 11 (batch 3), and through bzh_prove_batch_seeded on the Board circuit at k = 12 (batch 2) -- and an
unsatisfied witness must be reported as it is today.  Every comparison is exact.  One Params and one key per circuit serve the
module; the game inputs are tests/helpers/prove_game_cases.py's."""
import pytest

from helpers import prove_game_cases as G

pytestmark = pytest.mark.gpu


class Side:
    def __init__(self, ctx, kind, k):
        import bzh2
        from bzh2 import circuits as Cm, native as N, params as Pm
        self.ctx, self.shot = ctx, kind == "shot"
        self.lay = Cm.CircuitLayout(Cm.SHOT if self.shot else Cm.BOARD, k)
        self.prm = Pm.Params(ctx, k)
        self.pk = N.NativeProvingKey(ctx, self.lay.blob(), bzh2.CURVE_VESTA, params=self.prm)
        self.fresh_mode = self.pk.workspace_selected()
        game = G.games()
        cases = G.shot_cases(game) if self.shot else G.board_cases(game)
        self.game, self.valid = game, [c for c in cases if G.is_valid_game(c, game) and self.accepts(c)]

    def accepts(self, c):
        import bzh2
        try:
            self.lay.synthesize([c], form=bzh2.FORM_MONTGOMERY)
            return True
        except bzh2.BzhError:
            return False

    def close(self):
        self.pk.close()
        self.prm.close()
        self.lay.close()

    def host_path(self, circuits, seeds):
        adv, insts = self.lay.synthesize(circuits)
        return insts, self.pk.prove_batch(adv, insts, None, seeds=seeds)

    def device_chain(self, circuits, seeds):
        import torch
        dev = torch.empty((len(circuits), self.lay.num_advice, self.lay.n, 4), dtype=torch.int64, device="cuda")
        _, insts = self.lay.synthesize(circuits, ctx=self.ctx, device_ptr=dev.data_ptr(), where="device")
        proofs, st = self.pk.prove_batch_device(None, insts, seeds=seeds, device_ptr=dev.data_ptr())
        return insts, proofs, st.tolist()

    def one_call(self, circuits, seeds):
        insts, proofs, st = self.pk.prove_shots_device(self.lay, circuits, seeds, ctx=self.ctx, want_status=True)
        return insts, proofs, st.tolist()


def seeds_for(n, salt):
    return [bytes((salt + 31 * b + 7 * i) & 0xff for i in range(32)) for b in range(n)]


@pytest.fixture(scope="module")
def shot(gpu_ctx):
    s = Side(gpu_ctx, "shot", 11)
    yield s
    s.close()


def under(S, mode, fn):
    """fn() with the key in `mode`; the key goes back to EXTENDED"""
    from bzh2 import native as N
    S.pk.workspace_select(mode)
    try:
        assert S.pk.workspace_selected() == mode
        return fn()
    finally:
        S.pk.workspace_select(N.WORKSPACE_EXTENDED)


def test_a_fresh_key_is_extended_and_the_switch_reports_and_refuses(shot):
    import bzh2
    from bzh2 import native as N
    assert shot.fresh_mode == N.WORKSPACE_EXTENDED
    assert under(shot, N.WORKSPACE_COSETWISE, shot.pk.workspace_selected) == N.WORKSPACE_COSETWISE
    assert shot.pk.workspace_selected() == N.WORKSPACE_EXTENDED
    with pytest.raises(bzh2.BzhError) as e:
        shot.pk.workspace_select(2)
    assert e.value.status == bzh2.E_ARG and shot.pk.workspace_selected() == N.WORKSPACE_EXTENDED


def test_shot_proofs_are_the_same_bytes_through_the_three_provers(shot):
    """batch 3 at k = 11: bzh_prove_batch_seeded, bzh_prove_batch_device_seeded and bzh_prove_shots_device, each under both
    modes; the proofs verify; then the flavour BUILTIN with COSETWISE (the interpreter runs, the choice is still reported), and
    EXTENDED again on the same key"""
    from bzh2 import native as N
    circuits, seeds = shot.valid[:3], seeds_for(3, 3)
    want = {name: fn(circuits, seeds) for name, fn in (("host", shot.host_path), ("chain", shot.device_chain), ("one", shot.one_call))}
    assert want["host"][1] == want["chain"][1] == want["one"][1]
    assert shot.pk.verify_batch(want["host"][0], want["host"][1]) == [True] * 3
    for name, fn in (("host", shot.host_path), ("chain", shot.device_chain), ("one", shot.one_call)):
        got = under(shot, N.WORKSPACE_COSETWISE, lambda: fn(circuits, seeds))
        assert got[0] == want[name][0], name
        assert [len(p) for p in got[1]] == [len(p) for p in want[name][1]] and got[1] == want[name][1], name
        assert got[2:] == want[name][2:], name
        assert shot.pk.verify_batch(got[0], got[1]) == [True] * 3
    flavour, builtin = shot.pk.quotient_selected()
    if builtin:
        shot.pk.quotient_select(N.QUOTIENT_BUILTIN)
        try:
            got = under(shot, N.WORKSPACE_COSETWISE, lambda: (shot.pk.quotient_selected()[0], shot.host_path(circuits, seeds)))
            assert got[0] == N.QUOTIENT_BUILTIN and got[1] == want["host"]
            assert shot.host_path(circuits, seeds) == want["host"]      # EXTENDED again, the builtin kernel
        finally:
            shot.pk.quotient_select(flavour)
    assert builtin, "the Shot circuit has a kernel generated at build time"
    for name, fn in (("host", shot.host_path), ("chain", shot.device_chain)):
        assert fn(circuits, seeds) == want[name], "%s after the return to EXTENDED" % name


def test_a_broken_witness_in_the_middle_is_reported_as_today(shot):
    """a hit claimed on a miss at position 1 of 3: bzh_prove_batch_seeded's outcome (the proofs, or the status and text it
    raises) and the device chain's proofs and per-proof status bytes are those of EXTENDED"""
    import bzh2
    from bzh2 import circuits as Cm, native as N
    state = shot.valid[0].board
    miss = next(i for i in range(100) if not state.value >> i & 1)
    wrong = Cm.ShotCircuit(state, 0x77aa55, G.bv(1 << miss), G.bv(1))
    circuits, seeds = [shot.valid[1], wrong, shot.valid[5]], seeds_for(3, 40)

    def host():
        try:
            return ("ok",) + tuple(shot.host_path(circuits, seeds))
        except bzh2.BzhError as e:
            return ("raised", e.status, str(e))

    want_host, want_chain, want_one = host(), shot.device_chain(circuits, seeds), shot.one_call(circuits, seeds)
    print("host", want_host[:2], "chain status", want_chain[2], "one-call status", want_one[2])
    assert under(shot, N.WORKSPACE_COSETWISE, host) == want_host
    assert under(shot, N.WORKSPACE_COSETWISE, lambda: shot.device_chain(circuits, seeds)) == want_chain
    assert under(shot, N.WORKSPACE_COSETWISE, lambda: shot.one_call(circuits, seeds)) == want_one
    assert shot.pk.verify_batch(want_chain[0], want_chain[1]) == [True, False, True]


def test_board_proofs_are_the_same_bytes(gpu_ctx):
    """Board at k = 12, batch 2, through bzh_prove_batch_seeded"""
    from bzh2 import native as N
    S = Side(gpu_ctx, "board", 12)
    try:
        circuits, seeds = S.valid[:2], seeds_for(2, 12)
        want = S.host_path(circuits, seeds)
        got = under(S, N.WORKSPACE_COSETWISE, lambda: S.host_path(circuits, seeds))
        assert got == want and S.pk.verify_batch(want[0], want[1]) == [True, True]
    finally:
        S.close()


def test_the_mode_is_honoured_and_the_plan_covers_the_arena(shot):
    """A key of its own (its arena has served no call), the interpreter in both modes so that both read saturated columns, batch 3
    through bzh_prove_batch_seeded.  bzh_pk_workspace_peak is the arena's high-water mark of the last call.
      * COSETWISE holds less: were the switch ignored, the two peaks would be equal.
      * Past the quotient the two modes allocate the same buffers in the same order, and the call's peak lies there (the evaluation
        gather and the multiopen's buffers on top of everything the earlier phases left), so the peaks differ by the plan's coset
        term -- 7/8 of cosets_extended_bytes -- less what COSETWISE alone allocates besides: the shift table, one 4-byte word per
        column of the quotient's registry, rounded to the arena's 256 bytes (under 4 KiB for any circuit of up to 1 000 columns).
      * bzh_workspace_plan is meant to size batches: it must not be below the peak.  Its items count the column-sized buffers
        one by one and add an allowance for what the launches stage (staging_bytes), so it may be above the peak by that
        allowance and no more."""
    import bzh2
    from bzh2 import native as N
    pk = N.NativeProvingKey(shot.ctx, shot.lay.blob(), bzh2.CURVE_VESTA, params=shot.prm)
    try:
        pk.quotient_select(N.QUOTIENT_INTERPRETER)
        assert pk.workspace_peak() == 0
        circuits, seeds = shot.valid[:3], seeds_for(3, 9)
        adv, insts = shot.lay.synthesize(circuits)
        peak, plan, proofs = {}, {}, {}
        for mode in (N.WORKSPACE_EXTENDED, N.WORKSPACE_COSETWISE, N.WORKSPACE_EXTENDED):
            pk.workspace_select(mode)
            proofs[mode] = pk.prove_batch(adv, insts, None, seeds=seeds)
            peak[mode] = pk.workspace_peak()
            plan[mode] = N.workspace_plan_items(bzh2.CURVE_VESTA, pk.blob, 3, mode)
            print("mode %d: arena peak %d, plan %d (cosets %d, witness %d, quotient %d, tail %d, staging %d)" % (
                mode, peak[mode], plan[mode]["total_bytes"], plan[mode]["cosets_bytes"], plan[mode]["witness_bytes"],
                plan[mode]["quotient_bytes"], plan[mode]["tail_bytes"], plan[mode]["staging_bytes"]))
        assert proofs[N.WORKSPACE_EXTENDED] == proofs[N.WORKSPACE_COSETWISE]
        e, c = N.WORKSPACE_EXTENDED, N.WORKSPACE_COSETWISE
        assert peak[c] < peak[e]
        term = plan[e]["cosets_bytes"] - plan[c]["cosets_bytes"]
        assert term == plan[e]["cosets_extended_bytes"] // 8 * 7
        assert 0 <= term - (peak[e] - peak[c]) <= 4096
        for mode in (e, c):
            assert plan[mode]["total_bytes"] >= peak[mode], "the plan is below what the call held"
            assert plan[mode]["total_bytes"] - peak[mode] <= plan[mode]["staging_bytes"], "the plan counts buffers the call never held"
            assert pk.workspace_plan(3, mode) == plan[mode]["total_bytes"]
    finally:
        pk.close()
