"""CPU: the playout rule (include/hexgnn.h: hexgnn_playout_values; gnn_hex_amd/playouts.py) on the host.
(a) "the maker wins iff the terminals are connected inside the maker's vertices" against sequential play on the C env oracle,
(b) the selection sampling takes exactly ceil(m / 2) rows, (c) the greedy playout player of tests/playout_oracle.py beats uniformly
random moves, (d) the entry point's declaration, its ctypes mirror and its argument checks.  Nothing here touches a GPU."""
import ctypes
import os
import random
import re

import numpy as np
import pytest

import playout_oracle as po

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EUNSUPPORTED = -1, -2


def _play_out(game, bm, own_rows, rng):
    """Sequential play of one playout: the side to move owns the vertices of ``own_rows``, the other side the rest; both play
    theirs in a random order, alternating, without dead/captured removal, until somebody has won."""
    mine = [int(bm[r]) for r in range(2, len(bm)) if own_rows[r]]
    theirs = [int(bm[r]) for r in range(2, len(bm)) if not own_rows[r]]
    rng.shuffle(mine)
    rng.shuffle(theirs)
    assert len(mine) - len(theirs) in (0, 1)
    g = game.copy()
    for j in range(len(mine) + len(theirs)):
        if g.who_won() is not None:
            break
        g.make_move(mine[j // 2] if j % 2 == 0 else theirs[j // 2], False)
    return g.who_won()


@pytest.mark.parametrize("size,maker_turn", [(5, True), (5, False), (7, True), (7, False)])
def test_connection_rule_equals_sequential_play(hexref, size, maker_turn):
    """(a) 4 x 55 = 220 reduced positions, three playouts each."""
    rng = random.Random(100 * size + maker_turn)
    for g in range(55):
        game = hexref.random_position(size, 1000 * size + g, maker_turn)
        assert game.maker_turn == maker_turn and game.who_won() is None
        adj, bm = po.game_adjacency(game)
        n = adj.shape[0]
        own = po.mover_sets(n, 3, po.graph_base(size, g, 0))
        free = np.arange(n) >= 2
        makers = own if maker_turn else (~own & free[None, :])
        want = po.connected(adj, makers)
        for p in range(3):
            won = _play_out(game, bm, own[p], rng)
            assert won is not None
            assert (won == "m") == bool(want[p]), "Hex-%d position %d playout %d" % (size, g, p)


def test_selection_sampling_takes_half_rounded_up():
    """(b) exactly ceil(m / 2) rows for m = 0 .. 70, never a terminal."""
    for m in range(71):
        own = po.mover_sets(m + 2, 40, po.graph_base(7, m, 3))
        assert (own.sum(1) == (m + 1) // 2).all(), m
        assert not own[:, :2].any()
    # the sets differ between playouts, graphs and counters, and depend on the low counter word only
    a = po.mover_sets(30, 16, po.graph_base(1, 0, 0))
    assert len({r.tobytes() for r in a}) > 8
    assert not np.array_equal(a, po.mover_sets(30, 16, po.graph_base(1, 0, 1)))
    assert not np.array_equal(a, po.mover_sets(30, 16, po.graph_base(1, 1, 0)))
    assert np.array_equal(a, po.mover_sets(30, 16, po.graph_base(1, 1 << 32, 0)))


def test_hash_values():
    """The hash is the published 'lowbias32' mixer: pinned on a few inputs computed by hand-expanded integer arithmetic."""
    def ref(x):
        x &= 0xFFFFFFFF
        x ^= x >> 16
        x = (x * 0x7feb352d) & 0xFFFFFFFF
        x ^= x >> 15
        x = (x * 0x846ca68b) & 0xFFFFFFFF
        x ^= x >> 16
        return x
    xs = [0, 1, 2, 0x9e3779b9, 0xFFFFFFFF, 123456789]
    assert [int(v) for v in po.h32(np.array(xs, dtype=np.uint64))] == [ref(x) for x in xs]
    assert ref(0) == 0 and ref(1) != 1


def test_oracle_player_beats_random_moves(hexref):
    """(c) R = 256, greedy first maximum, dead/captured removal on: at least 30 of 40 Hex-5 games against uniform moves."""
    rng = random.Random(2024)
    won = 0
    calls = 0
    for mc_is_maker in (True, False):
        for mc_first in (True, False):
            for _ in range(10):
                game = hexref.RefGame(5)
                game.maker_turn = mc_is_maker == mc_first
                while game.who_won() is None:
                    if game.maker_turn == mc_is_maker:
                        adj, bm = po.game_adjacency(game)
                        scores = po.playout_graph(adj, game.maker_turn, 256, seed=5, counter=calls)[0]
                        calls += 1
                        v = int(bm[po.pick(scores)])
                    else:
                        acts = game.get_actions()
                        v = int(acts[rng.randrange(len(acts))])
                    game.make_move(v, True)
                won += game.who_won() == ("m" if mc_is_maker else "b")
    assert won >= 30, "the playout player won %d of 40" % won


def test_playout_call_is_declared_exported_and_mirrored():
    """(d) the header, the library and the ctypes table agree."""
    from gnn_hex_amd import _lib
    header = open(os.path.join(ROOT, "include", "hexgnn.h")).read()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    assert re.search(r"\bint\s+hexgnn_playout_values\s*\(\s*const\s+hexgnn_playout_call\s*\*\s*\w+\s*,\s*hexgnn_stream_t\s+\w+\s*\)",
                     header)
    assert hasattr(raw, "hexgnn_playout_values") and "hexgnn_playout_values" in _lib.exported_symbols()
    assert _lib.lib().hexgnn_abi_version() == 8
    m = re.search(r"typedef\s+struct\s+hexgnn_playout_call\s*\{(.*?)\}\s*hexgnn_playout_call\s*;", header, re.S)
    kinds = {"size_t": ctypes.c_size_t, "int": ctypes.c_int, "uint32_t": ctypes.c_uint32}
    want = []
    for decl in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(";"):
        decl = decl.strip()
        if not decl:
            continue
        head = re.match(r"(?:const\s+)?(\w+)", decl)
        for item in decl[head.end():].split(","):
            name = re.search(r"(\w+)\s*$", item).group(1)
            want.append((name, ctypes.c_void_p if "*" in item else kinds[head.group(1)]))
    assert [(n, t) for n, t in _lib.PlayoutCall._fields_] == want
    assert [n for n, _ in want] == ["struct_bytes", "b", "playouts", "max_nodes", "maker_to_move", "seed", "gptr", "rowptr", "col",
                                    "counter", "scores", "value", "tables", "wins", "status"]
    assert int(re.search(r"#define\s+HEXGNN_PLAYOUT_MAX_NODES\s+(\d+)", header).group(1)) == _lib.PLAYOUT_MAX_NODES == 640


def _call(_lib, p, **kw):
    call = _lib.PlayoutCall(struct_bytes=ctypes.sizeof(_lib.PlayoutCall), b=2, playouts=16, max_nodes=27, maker_to_move=1, seed=3,
                            gptr=p, rowptr=p, col=p, counter=None, scores=p, value=p, tables=None, wins=None, status=p)
    for k, v in kw.items():
        setattr(call, k, v)
    return call


def test_playout_refusals_that_need_no_device():
    """(d) every refusal comes from the host checks, before anything is launched."""
    from gnn_hex_amd import _lib
    L = _lib.lib()
    buf = (ctypes.c_char * 4096)()
    p = ctypes.addressof(buf)
    assert L.hexgnn_playout_values(None, None) == EINVAL
    assert L.hexgnn_playout_values(ctypes.byref(_call(_lib, p, struct_bytes=ctypes.sizeof(_lib.PlayoutCall) - 8)), None) == EINVAL
    assert L.hexgnn_playout_values(ctypes.byref(_call(_lib, p, struct_bytes=0)), None) == EINVAL
    for bad in (0, -1, (1 << 24) + 1):
        assert L.hexgnn_playout_values(ctypes.byref(_call(_lib, p, playouts=bad)), None) == EINVAL, bad
    for bad in (1, 0, -5):
        assert L.hexgnn_playout_values(ctypes.byref(_call(_lib, p, max_nodes=bad)), None) == EINVAL, bad
    assert L.hexgnn_playout_values(ctypes.byref(_call(_lib, p, b=-1)), None) == EINVAL
    for bad in (641, 2048):
        assert L.hexgnn_playout_values(ctypes.byref(_call(_lib, p, max_nodes=bad)), None) == EUNSUPPORTED, bad
    assert L.hexgnn_playout_values(ctypes.byref(_call(_lib, p, max_nodes=641, playouts=0)), None) == EINVAL   # the order of the checks
    for name in ("gptr", "rowptr", "col", "scores", "status"):
        assert L.hexgnn_playout_values(ctypes.byref(_call(_lib, p, **{name: None})), None) == EINVAL, name
    # nothing to do: OK without a launch, whatever the pointers
    assert L.hexgnn_playout_values(ctypes.byref(_call(_lib, None, b=0, max_nodes=640)), None) == 0


def test_player_object_without_a_device():
    from gnn_hex_amd.playouts import MonteCarloPlayer
    from gnn_hex_amd.observation import live_norm_of
    pl = MonteCarloPlayer(64, seed=-1)
    assert pl.playouts == 64 and pl.seed == 0xFFFFFFFF
    assert pl.train() is pl and pl.eval() is pl and pl.to("cuda") is pl and callable(pl)
    assert live_norm_of(pl) is False
    pl.set_counter(7)
    assert pl.counter() == 7
    pl.status()
    with pytest.raises(ValueError):
        pl.set_counter(-1)
    with pytest.raises(ValueError):
        MonteCarloPlayer(0)
