"""The game inputs of tests/test_gpu_prove_game.py: the case builders of tests/test_gpu_synthesize_device.py (valid hit and miss
games, every trapdoor that steers the fixed-base multiplications, the boards 0, 2^100 - 1 and a single bit), and the
classification of every candidate, alone, through the host path."""
FQ = 0x40000000000000000000000000000000224698fc0994a8dd8c46eb2100000001
SHIPS = [(3, 3, True), (5, 4, False), (0, 1, False), (0, 5, True), (6, 1, False)]   # pattern #1 of the reference's tests


def _windows(ws):
    return sum(w << (3 * i) for i, w in enumerate(ws))


TRAPDOORS = [0, 1, FQ - 1, (1 << 254) - 1, 1 << 252, 0x5eed,
             _windows([7] * 85),                                   # every window 7: 2^255 - 1
             _windows([7 * (i & 1) for i in range(85)]), _windows([7 * ((i + 1) & 1) for i in range(84)])]


def bv(v):
    from bzh2.game import BinaryValue
    return BinaryValue(v)


def games():
    from bzh2 import circuits as Cm
    ships, state = Cm.board_witness(SHIPS, None)
    ships2, state2 = Cm.board_witness([(0, 0, False), (2, 2, False), (4, 4, False), (6, 6, False), (8, 8, False)], None)
    return (ships, state), (ships2, state2)


def shot_cases(game):
    """ShotCircuits: valid games (hit and miss), every trapdoor, the boards 0, 2^100 - 1 and a single bit"""
    from bzh2 import circuits as Cm
    (_, state), (_, state2) = game
    hit = next(i for i in range(100) if state.value >> i & 1)
    miss = next(i for i in range(100) if not state.value >> i & 1)
    out = [Cm.ShotCircuit(state, t, bv(1 << hit), bv(1)) for t in TRAPDOORS]
    out.append(Cm.ShotCircuit(state, 0x1234567, bv(1 << miss), bv(0)))
    out.append(Cm.ShotCircuit(state2, FQ - 2, Cm.shot_serialize([9], [9]), bv(1)))
    for board in (0, (1 << 100) - 1, 1 << 99):
        out.append(Cm.ShotCircuit(bv(board), 0, bv(1 << 99), bv((board >> 99) & 1)))
        out.append(Cm.ShotCircuit(bv(board), FQ - 1, bv(1), bv(board & 1)))
    return out


def board_cases(game):
    from bzh2 import circuits as Cm
    (ships, state), (ships2, state2) = game
    zeros = [bv(0)] * 10
    out = [Cm.BoardCircuit(ships, state, t) for t in TRAPDOORS]
    out.append(Cm.BoardCircuit(ships2, state2, FQ - 2))
    for board in (0, (1 << 100) - 1, 1 << 99):
        out.append(Cm.BoardCircuit(zeros, bv(board), 0))                 # ship commitments of all zeros
        out.append(Cm.BoardCircuit(ships, bv(board), (1 << 254) - 1))
    return out


def is_valid_game(c, game):
    """whether a candidate's witness satisfies its circuit, so that the verifier accepts its proof: a Shot of one cell with the
    true hit claim (the Shot circuit takes any board state); a Board whose ship commitments and state are one of the two games'"""
    if hasattr(c, "shot"):
        shot, board = c.shot.value, c.board.value
        return bin(shot).count("1") == 1 and shot < 1 << 100 and c.hit.value == (1 if board & shot else 0)
    return any([s.value for s in c.ship_commitments] == [s.value for s in ships] and c.board.value == state.value for ships, state in game)


def classify(lay, cases):
    """every operand alone through the host path: (accepted, [(refused, status, text)])"""
    import bzh2
    ok, bad = [], []
    for c in cases:
        try:
            lay.synthesize([c], form=bzh2.FORM_MONTGOMERY)
            ok.append(c)
        except bzh2.BzhError as e:
            bad.append((c, e.status, str(e)))
    return ok, bad
