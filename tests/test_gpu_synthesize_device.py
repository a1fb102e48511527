"""Witness synthesis on the device (bzh_synthesize_{shot,board}_with, BZH_SYNTH_DEVICE; csrc/synthesize_device.hip) against the
host path: the whole (batch, num_advice, 2^k) tensor read back from the device and the instances, word for word, for valid games
and for operands that steer the fixed-base multiplications and the complete additions; the same status where the host path
refuses an input (which inputs it refuses is taken from the host path at test time); refusals of a non-canonical trapdoor with
the host's text; proofs from a device witness byte-identical to those from the host witness; argument refusals."""
import ctypes
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

E_ARG, E_RANGE = -1, -4
FQ = 0x40000000000000000000000000000000224698fc0994a8dd8c46eb2100000001
SHIPS = [(3, 3, True), (5, 4, False), (0, 1, False), (0, 5, True), (6, 1, False)]   # pattern #1 of the reference's tests


def _windows(ws):
    return sum(w << (3 * i) for i, w in enumerate(ws))


TRAPDOORS = [0, 1, FQ - 1, (1 << 254) - 1, 1 << 252, 0x5eed,
             _windows([7] * 85),                                   # every window 7: 2^255 - 1
             _windows([7 * (i & 1) for i in range(85)]), _windows([7 * ((i + 1) & 1) for i in range(84)])]


def _bv(v):
    from bzh2.game import BinaryValue
    return BinaryValue(v)


@pytest.fixture(scope="module")
def game():
    from bzh2 import circuits as Cm
    ships, state = Cm.board_witness(SHIPS, None)
    ships2, state2 = Cm.board_witness([(0, 0, False), (2, 2, False), (4, 4, False), (6, 6, False), (8, 8, False)], None)
    return (ships, state), (ships2, state2)


@pytest.fixture(scope="module")
def shot_cases(game):
    """ShotCircuits: valid games (hit and miss), every trapdoor, the boards 0, 2^100 - 1 and a single bit"""
    from bzh2 import circuits as Cm
    (_, state), (_, state2) = game
    hit = next(i for i in range(100) if state.value >> i & 1)
    miss = next(i for i in range(100) if not state.value >> i & 1)
    out = [Cm.ShotCircuit(state, t, _bv(1 << hit), _bv(1)) for t in TRAPDOORS]
    out.append(Cm.ShotCircuit(state, 0x1234567, _bv(1 << miss), _bv(0)))
    out.append(Cm.ShotCircuit(state2, FQ - 2, Cm.shot_serialize([9], [9]), _bv(1)))
    for board in (0, (1 << 100) - 1, 1 << 99):
        out.append(Cm.ShotCircuit(_bv(board), 0, _bv(1 << 99), _bv((board >> 99) & 1)))
        out.append(Cm.ShotCircuit(_bv(board), FQ - 1, _bv(1), _bv(board & 1)))
    return out


@pytest.fixture(scope="module")
def board_cases(game):
    from bzh2 import circuits as Cm
    (ships, state), (ships2, state2) = game
    zeros = [_bv(0)] * 10
    out = [Cm.BoardCircuit(ships, state, t) for t in TRAPDOORS]
    out.append(Cm.BoardCircuit(ships2, state2, FQ - 2))
    for board in (0, (1 << 100) - 1, 1 << 99):
        out.append(Cm.BoardCircuit(zeros, _bv(board), 0))                 # ship commitments of all zeros
        out.append(Cm.BoardCircuit(ships, _bv(board), (1 << 254) - 1))
    return out


@pytest.fixture(scope="module")
def layouts():
    from bzh2 import circuits as Cm
    lays = {"shot11": Cm.CircuitLayout(Cm.SHOT, 11), "board12": Cm.CircuitLayout(Cm.BOARD, 12), "board14": Cm.CircuitLayout(Cm.BOARD, 14)}
    yield lays
    for lay in lays.values():
        lay.close()


def _host(lay, circuits):
    """(status, advice, instances) of the host path: host memory, Montgomery form"""
    import bzh2
    try:
        adv, insts = lay.synthesize(circuits, form=bzh2.FORM_MONTGOMERY)
        return 0, adv, insts
    except bzh2.BzhError as e:
        return e.status, None, str(e)


def _device(lay, circuits, ctx):
    import torch
    import bzh2
    dev = torch.empty((len(circuits), lay.num_advice, lay.n, 4), dtype=torch.int64, device="cuda")
    dev.fill_(-1)                                                        # stale contents must be overwritten / zeroed
    torch.cuda.synchronize()
    try:
        _, insts = lay.synthesize(circuits, ctx=ctx, device_ptr=dev.data_ptr(), where="device")
    except bzh2.BzhError as e:
        return e.status, None, str(e)
    return 0, dev.cpu().numpy().view(np.uint64), insts


@pytest.fixture(scope="module")
def classified(layouts, shot_cases, board_cases):
    """every operand alone through the host path: (accepted, refused with their status)"""
    out = {}
    for name, lay, cases in (("shot", layouts["shot11"], shot_cases), ("board", layouts["board12"], board_cases)):
        ok, bad = [], []
        for c in cases:
            st, _, text = _host(lay, [c])
            (bad.append((c, st, text)) if st else ok.append(c))
        assert len(ok) >= 8, "the host path accepts the valid games and the canonical trapdoors"
        out[name] = (ok, bad)
    return out


def _compare(lay, circuits, ctx):
    st, want, winst = _host(lay, circuits)
    assert st == 0
    st, got, ginst = _device(lay, circuits, ctx)
    assert st == 0
    assert got.shape == want.shape
    diff = np.argwhere(got != want)
    assert diff.size == 0, "first differing words (proof, column, row, limb): %s" % diff[:5].tolist()
    assert ginst == winst


@pytest.mark.parametrize("batch", [1, 2, 65])
@pytest.mark.parametrize("kind", ["shot", "board"])
def test_device_witness_equals_host_witness(gpu_ctx, layouts, classified, kind, batch):
    """every operand the host path accepts, cycled into batches of 1, 2 and 65 (more than one wave of tail lanes): Shot at
    k = 11, Board at k = 12"""
    lay = layouts["shot11" if kind == "shot" else "board12"]
    ok = classified[kind][0]
    if batch == 65:
        groups = [[ok[i % len(ok)] for i in range(65)]]
    else:
        groups = [ok[i:i + batch] for i in range(0, len(ok), batch)]
    for g in groups:
        _compare(lay, g, gpu_ctx)


def test_board_at_k14_stride_and_zero_fill(gpu_ctx, layouts, classified):
    ok = classified["board"][0]
    _compare(layouts["board14"], [ok[0], ok[len(ok) // 2], ok[-1]], gpu_ctx)


@pytest.mark.parametrize("kind", ["shot", "board"])
def test_status_parity_on_operands_the_host_path_refuses(gpu_ctx, layouts, classified, kind):
    lay = layouts["shot11" if kind == "shot" else "board12"]
    for c, st, _ in classified[kind][1]:
        got, _, _ = _device(lay, [c], gpu_ctx)
        assert got == st


@pytest.mark.parametrize("kind", ["shot", "board"])
def test_non_canonical_trapdoor_is_refused_with_the_hosts_text_and_the_ctx_goes_on(gpu_ctx, layouts, classified, kind):
    import copy
    lay = layouts["shot11" if kind == "shot" else "board12"]
    ok = classified[kind][0]
    for bad in (FQ, (1 << 256) - 1):
        for pos in (0, 2, 4):
            group = [copy.copy(c) for c in ok[:5]]
            group[pos].board_commitment_trapdoor = bad
            hst, _, htext = _host(lay, group)
            dst, _, dtext = _device(lay, group, gpu_ctx)
            assert hst == E_RANGE and dst == E_RANGE
            assert "trapdoor is not a canonical scalar" in htext and dtext.split(": ", 1)[1] == htext.split(": ", 1)[1]
    _compare(lay, ok[:5], gpu_ctx)


def test_device_witness_gives_the_host_witness_proofs(gpu_ctx, layouts, classified):
    """one Shot batch of 2 at k = 11 through bzh_prove_batch: byte-identical proofs under the same randomness, accepted"""
    import torch
    import bzh2
    from bzh2 import native as N, params as Pm
    lay = layouts["shot11"]
    circuits = [classified["shot"][0][5], classified["shot"][0][-1]]
    prm = Pm.Params(gpu_ctx, 11)
    pk = N.NativeProvingKey(gpu_ctx, lay.blob(), bzh2.CURVE_VESTA, params=prm)
    try:
        rng = random.Random(2024)
        rbs = [rng.randbytes(pk.rng_bytes) for _ in circuits]
        adv, insts = lay.synthesize(circuits)
        want = pk.prove_batch(adv, insts, rbs)
        dev = torch.empty((2, lay.num_advice, lay.n, 4), dtype=torch.int64, device="cuda")
        dev.fill_(-1)
        torch.cuda.synchronize()
        _, insts2 = lay.synthesize(circuits, ctx=gpu_ctx, device_ptr=dev.data_ptr(), where="device")
        assert insts2 == insts
        got = pk.prove_batch(None, insts2, rbs, device_ptr=dev.data_ptr())
        assert got == want
        assert pk.verify_batch(insts2, got) == [True, True]
    finally:
        pk.close()
        prm.close()


def test_argument_refusals_and_host_through_the_new_entry_point(gpu_ctx, layouts, classified):
    import torch
    import bzh2
    from bzh2 import circuits as Cm
    L = Cm._bind()
    VP = ctypes.c_void_p
    lay = layouts["shot11"]
    c = classified["shot"][0][0]
    words = [np.ascontiguousarray(bzh2.int_to_limbs(v)) for v in (c.board.value, c.board_commitment_trapdoor, c.shot.value, c.hit.value)]
    ptrs = [VP(w.ctypes.data) for w in words]
    host = np.zeros((1, lay.num_advice, lay.n, 4), dtype=np.uint64)
    inst = np.zeros((4, 4), dtype=np.uint64)
    dev = torch.zeros((1, lay.num_advice, lay.n, 4), dtype=torch.int64, device="cuda")

    def call(ctx, adv, form, mem, where):
        return L.bzh_synthesize_shot_with(ctx, lay.handle, 1, *ptrs, adv, form, mem, VP(inst.ctypes.data), 1, where)

    assert call(gpu_ctx.handle, VP(host.ctypes.data), bzh2.FORM_MONTGOMERY, bzh2.MEM_HOST, Cm.SYNTH_DEVICE) == E_ARG
    assert call(gpu_ctx.handle, VP(dev.data_ptr()), bzh2.FORM_CANONICAL, bzh2.MEM_DEVICE, Cm.SYNTH_DEVICE) == E_ARG
    assert call(None, VP(dev.data_ptr()), bzh2.FORM_MONTGOMERY, bzh2.MEM_DEVICE, Cm.SYNTH_DEVICE) == E_ARG
    assert call(gpu_ctx.handle, VP(dev.data_ptr()), bzh2.FORM_MONTGOMERY, bzh2.MEM_DEVICE, 2) == E_ARG
    assert call(None, VP(host.ctypes.data), bzh2.FORM_MONTGOMERY, bzh2.MEM_HOST, Cm.SYNTH_HOST) == 0
    want, winst = np.zeros_like(host), np.zeros_like(inst)
    assert L.bzh_synthesize_shot(None, lay.handle, 1, *ptrs, VP(want.ctypes.data), bzh2.FORM_MONTGOMERY, bzh2.MEM_HOST, VP(winst.ctypes.data), 1) == 0
    assert (host == want).all() and (inst == winst).all()
