"""Stone lists on the CPU env oracle (shared by tests/test_positions_host.py and tests/test_gpu_positions.py).

A forced-colour stone is reproduced through RefGame's public API: set ``maker_turn`` to the stone's colour, ``make_move``, put
the side back.  Graph, ``alive`` and response sets come out as the reference's ``make_move(v, force_color=...)`` leaves them; only
the oracle's ``total_num_moves`` counts the forced stones too, so ``OracleGame`` keeps the count the reference would hold."""
import numpy as np


class OracleGame:
    """A RefGame plus the move count under forced-colour stones."""

    def __init__(self, hexref, size, maker_turn=True):
        self.game = hexref.RefGame(size)
        self.game.maker_turn = maker_turn
        self.moves = 0
        self.size = size

    def apply(self, vertex, colour, remove=False):
        """One stone; ValueError (the oracle's) for an illegal one.  Returns who_won()."""
        g = self.game
        if colour == "turn":
            g.make_move(int(vertex), bool(remove))
            self.moves += 1
        else:
            side = g.maker_turn
            g.maker_turn = colour == "m"
            try:
                g.make_move(int(vertex), bool(remove))
            finally:
                g.maker_turn = side
        return g.who_won()

    def responses(self):
        """(resp_maker, resp_breaker) int16 [nv], -1 = none: the device's layout."""
        nv = self.game.nv
        out = np.full((2, nv), -1, dtype=np.int16)
        for v in range(nv):
            for row, for_maker in ((0, True), (1, False)):
                r = self.game.get_response(v, for_maker)
                if r is not None:
                    out[row, v] = r
        return out[0], out[1]


def assert_env_equals(st, i, og, tag=""):
    """Env i of ``Env_manager._state()`` against an OracleGame: boards, side, move count and response sets, exactly."""
    adj, alive = og.game.dump()
    assert np.array_equal(st["alive"][i], alive), "%s env %d: alive set differs" % (tag, i)
    assert np.array_equal(st["adj"][i], adj), "%s env %d: adjacency differs" % (tag, i)
    assert bool(st["maker_turn"][i]) == og.game.maker_turn, "%s env %d: side" % (tag, i)
    assert int(st["total_moves"][i]) == og.moves, "%s env %d: move count %d, oracle %d" % (tag, i, st["total_moves"][i], og.moves)
    rm, rb = og.responses()
    assert np.array_equal(st["resp_maker"][i], rm), "%s env %d: maker response set" % (tag, i)
    assert np.array_equal(st["resp_breaker"][i], rb), "%s env %d: breaker response set" % (tag, i)


def random_stone_list(og, rng, length):
    """Draw up to ``length`` stones on the oracle (and apply them there): a random live cell, a random colour among
    m / b / turn, a random remove flag; the list stops when the position is decided.  Returns the list."""
    out = []
    for _ in range(length):
        acts = og.game.get_actions()
        if len(acts) == 0:
            break
        v = int(acts[rng.integers(len(acts))])
        colour = ("m", "b", "turn")[int(rng.integers(3))]
        remove = bool(rng.integers(2))
        out.append((v, colour, remove))
        if og.apply(v, colour, remove) is not None:
            break
    return out
