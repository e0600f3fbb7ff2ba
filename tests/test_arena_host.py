"""CPU: the match-play entry points refuse bad arguments before touching the device, and the host side of
gnn_hex_amd.arena.Elo_handler: rating arithmetic, the unique opening moves, the capping of a match's game count, and what it
refuses to play."""
import ctypes
import random

import pytest


def _handler(size):
    """An Elo_handler without a device (nothing below plays a game)."""
    from gnn_hex_amd.arena import Elo_handler
    return Elo_handler(size, device="cuda")


def test_match_play_entry_points_validate_arguments_without_gpu():
    from gnn_hex_amd import _lib
    L = _lib.lib()
    buf = (ctypes.c_char * 64)()
    p = ctypes.addressof(buf)             # host memory standing in for every required pointer: never dereferenced
    S = L.hexgnn_sample_actions
    assert S(-1, p, p, p, 0, 1.0, p, p, p, None, None) == -1
    assert S(4, p, p, p, 3, 1.0, p, p, p, None, None) == -1 and S(4, p, p, p, -1, 1.0, p, p, p, None, None) == -1
    assert S(4, None, p, p, 0, 1.0, p, p, p, None, None) == -1 and S(4, p, p, p, 0, 1.0, p, p, None, None, None) == -1
    assert S(4, p, None, p, 0, 1.0, None, p, p, None, None) == -1          # GREEDY needs q
    assert S(4, p, None, p, 2, 1.0, p, p, p, None, None) == -1             # SOFTMAX needs q
    assert S(4, p, p, p, 1, 1.0, None, p, p, None, None) == -1             # UNIFORM needs u
    assert S(4, p, p, p, 2, 1.0, None, p, p, None, None) == -1             # SOFTMAX needs u
    for bad_t in (0.0, -1.0, float("inf"), float("nan")):
        assert S(4, p, p, p, 2, bad_t, p, p, p, None, None) == -1
    assert S(0, None, None, None, 0, 1.0, None, None, None, None, None) == 0     # an empty batch: nothing to do
    A = L.hexgnn_arena_ply
    ok = dict(h=p, gptr=p, q=p, backmap=p, mode=0, t=1.0, u=p, forced=None, rmt=0, game=p, log=p, result=p, live=p)

    def ply(**kw):
        a = dict(ok, **kw)
        return A(a["h"], a["gptr"], a["q"], a["backmap"], a["mode"], a["t"], a["u"], a["forced"], a["rmt"], a["game"], a["log"],
                 a["result"], a["live"], None)
    for name in ("h", "gptr", "backmap", "game", "log", "result", "live"):
        assert ply(**{name: None}) == -1, name
    assert ply(mode=3) == -1 and ply(mode=-1) == -1
    assert ply(q=None) == -1 and ply(q=None, mode=2) == -1
    assert ply(u=None, mode=1) == -1 and ply(u=None, mode=2) == -1
    for bad_t in (0.0, -0.5, float("inf"), float("nan")):
        assert ply(mode=2, t=bad_t) == -1


def test_rating_arithmetic():
    """One score_some_statistics: a rated player moves by K (score - expectation) / games over its matches against rated
    opponents, a player without a rating receives its performance rating, a fixed one stays."""
    e = _handler(5)
    e.add_player(name="random", set_rating=0, rating_fixed=True)
    e.add_player(name="maker", set_rating=1500, rating_fixed=False)
    e.add_player(name="huff", set_rating=None, rating_fixed=False)
    stats = [{"random": 6, "maker": 6}, {"huff": 2, "maker": 10}, {"huff": 4, "random": 8}]
    perf = e.get_performances_from_stats(stats)
    assert perf["huff"] == 550.0                                    # (1500*12 + 400*(4-12) + 0*12 + 400*(8-12)) / 24
    assert perf["maker"] == 0.0 and perf["random"] == pytest.approx(1500.0)      # against their rated opponents alone
    e.score_some_statistics(stats)
    assert e.get_rating("maker") == pytest.approx(1495.0017779632385, rel=1e-12)
    assert e.get_rating("huff") == 550.0
    assert e.get_rating("random") == 0
    assert e.get_rating_table() == (["name", "rating"], [["maker", e.get_rating("maker")], ["huff", 550.0], ["random", 0]])
    # not per game: the whole K (score - expectation)
    e2 = _handler(5)
    e2.add_player(name="a", set_rating=1000)
    e2.add_player(name="b", set_rating=1000)
    e2.score_some_statistics([{"a": 9, "b": 3}], game_num_independent=False)
    assert e2.get_rating("a") == pytest.approx(1030.0) and e2.get_rating("b") == pytest.approx(970.0)
    e2.reset(new_hex_size=7, keep_players=["a"])
    assert list(e2.players) == ["a"] and e2.size == 7


@pytest.mark.parametrize("size,count", [(5, 15), (7, 28), (11, 66), (13, 91)])
def test_opening_moves(size, count):
    e = _handler(size)
    moves = e.opening_moves()
    assert len(moves) == count == size * (size + 1) // 2 and len(set(moves)) == count
    cells = [m - 2 for m in moves]
    assert cells == [i * size + j for i in range(size) for j in range(i, size)]
    # together with their images under the board's point symmetry they cover every cell
    assert sorted(set(cells) | {size * size - 1 - c for c in cells}) == list(range(size * size))


@pytest.mark.parametrize("size", [5, 7])
def test_match_plan_caps_the_game_count(size):
    e = _handler(size)
    unique = size * (size + 1) // 2
    for asked, per_leg in ((None, unique), (2 * unique + 10, unique), (2 * unique, unique), (10, 5), (11, 5), (1, 0)):
        random.seed(size)
        got, openings = e._match_plan(asked, False)
        random.seed(size)
        want = e.opening_moves()
        random.shuffle(want)
        assert got == per_leg
        assert openings[0] == openings[1] == want[:per_leg]           # game i of either leg opens with the i-th shuffled move
    # a random first move lifts the cap; every opening is a board cell
    random.seed(1)
    got, openings = e._match_plan(4 * unique, True)
    assert got == 2 * unique and all(len(o) == got for o in openings)
    assert all(2 <= v < size * size + 2 for o in openings for v in o) and openings[0] != openings[1]
    assert e._match_plan(None, True)[0] == unique


def test_unsupported_players_are_refused():
    e = _handler(5)
    e.add_player(name="rnd", model="random", simple=True)
    e.add_player(name="cnn", model=object(), cnn=True)
    e.add_player(name="gao", model=object(), gao_style=True)
    e.add_player(name="walker", model=lambda games: [0 for _ in games], simple=True)
    for other in ("cnn", "gao", "walker"):
        with pytest.raises(NotImplementedError):
            e.play_some_games("rnd", other, 4, 0)
        with pytest.raises(NotImplementedError):
            e.play_some_games(other, "rnd", 4, 0)
    with pytest.raises(NotImplementedError):
        e.play_some_games("rnd", "rnd", 4, 0, log_sgfs=True)
    assert e._player_for_arena("rnd") == "random"
