"""GPU: Monte-Carlo playout values (gnn_hex_amd/csrc/playout.hip, gnn_hex_amd/playouts.py) against the numpy restatement of the
rule in tests/playout_oracle.py: exact integer tables and bit-equal fp32 scores at the word-count edges of the kernel, capacity-sized
targets, the size limit, the counter discipline, whole arena games replayed on the host, and the surfaces a player drops into."""
import numpy as np
import pytest
import torch

import playout_oracle as po

pytestmark = pytest.mark.gpu

DEV = "cuda"
# word-count edges of the kernel's instantiations (64 / 128 / 192 / 256 rows) and the limit
SIZES = [2, 3, 4, 63, 64, 65, 66, 127, 128, 129, 130, 192, 193, 256, 257, 640]
BIG_COUNTER = (1 << 32) * 3 + 5           # only the low word counts


def _random_graph(n, rng, extra=1.5, joined=True):
    """int64 [2, E]: a random connected symmetric graph on n rows (a random tree plus ``extra * n`` random edges), both
    directions listed; for n == 2 the one possible edge is there when ``joined``."""
    if n == 2:
        pairs = [(0, 1)] if joined else []
    else:
        order = rng.permutation(n)
        pairs = [(int(order[i]), int(order[rng.integers(i)])) for i in range(1, n)]
        for _ in range(int(extra * n)):
            a, b = (int(v) for v in rng.integers(n, size=2))
            if a != b:
                pairs.append((a, b))
    e = np.array(pairs, dtype=np.int64).reshape(-1, 2).T
    return np.concatenate([e, e[::-1]], axis=1)


def _batch(graphs, sizes, maker):
    """Device tensors ``(x, edge_index, ptr)`` of a collated batch of local edge lists."""
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    ei = np.concatenate([g + off[i] for i, g in enumerate(graphs)], axis=1) if graphs else np.zeros((2, 0), dtype=np.int64)
    x = torch.zeros((int(off[-1]), 3), dtype=torch.float32, device=DEV)
    x[:, 2] = float(maker)
    return x, torch.from_numpy(ei).to(DEV), torch.from_numpy(off).to(DEV)


_GRAPHS = {}


def _graph(n, tag=0):
    key = (n, tag)
    if key not in _GRAPHS:
        e = _random_graph(n, np.random.default_rng(1000 * n + tag), joined=tag % 2 == 0)
        _GRAPHS[key] = (e, po.dense_adjacency(n, e))
    return _GRAPHS[key]


_WANT = {}


def _oracle(keys, adjs, maker, R, seed, counter):
    """The oracle's answer for a batch, computed once per (batch, side, R, seed, counter)."""
    key = (keys, maker, R, seed, counter & 0xFFFFFFFF)
    if key not in _WANT:
        _WANT[key] = po.playout_batch(adjs, maker, R, seed, counter)
    return _WANT[key]


def _bits(t):
    return t.detach().cpu().numpy().view(np.int32)


def _check(got, want, what):
    scores, value, tables, wins = got
    w_scores, w_value, w_tables, w_wins = want
    n = w_scores.shape[0]
    assert np.array_equal(wins.cpu().numpy(), w_wins), "%s: wins %s, oracle %s" % (what, wins.cpu().numpy(), w_wins)
    assert np.array_equal(tables.cpu().numpy()[:n], w_tables), "%s: own / won tables" % what
    assert np.array_equal(_bits(scores)[:n], w_scores.view(np.int32)), "%s: scores are not bit-equal" % what
    assert np.array_equal(_bits(value), w_value.view(np.int32)), "%s: values are not bit-equal" % what


def _run(x, ei, ptr, R, maker, seed, counter, **kw):
    from gnn_hex_amd.playouts import playout_values
    ctr = torch.tensor([counter], dtype=torch.int64, device=DEV) if counter is not None else None
    return playout_values(x, ei, ptr, R, seed=seed, counter=ctr, is_maker=maker, tables=True, **kw)


# ---- 1. the kernel against the oracle --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("maker", [True, False])
@pytest.mark.parametrize("n", SIZES)
def test_single_graph_every_word_count(n, maker):
    """b = 1; every R on the graphs up to 130 rows, the playout-count edges of a wave and of the workgroup on the larger ones."""
    for tag in ((0, 1) if n == 2 else (0,)):           # two terminals alone: joined and not
        e, adj = _graph(n, tag)
        x, ei, ptr = _batch([e], [n], maker)
        for R in ((1, 63, 64, 65, 256, 1000) if n <= 130 else (1, 65, 257)):
            for counter in ((0, BIG_COUNTER) if R == 65 else (0,)):
                got = _run(x, ei, ptr, R, maker, 11, counter)
                _check(got, _oracle((n, tag), [adj], maker, R, 11, counter), "n=%d R=%d counter=%d" % (n, R, counter))
                assert int(got[3][0]) <= R and int(got[2][:, 0].max()) <= R
                if n > 2:
                    assert int(got[2][2:, 0].sum()) == R * ((n - 1) // 2)       # every playout hands out ceil(m / 2) rows
                else:
                    assert int(got[3][0]) == (R if (tag == 0) == maker else 0)


@pytest.mark.parametrize("maker", [True, False])
def test_ragged_batch_of_all_sizes(maker):
    graphs = [_graph(n)[0] for n in SIZES]
    adjs = [_graph(n)[1] for n in SIZES]
    x, ei, ptr = _batch(graphs, SIZES, maker)
    for counter in (0, BIG_COUNTER):
        got = _run(x, ei, ptr, 65, maker, 3, counter)
        _check(got, _oracle(tuple(SIZES), adjs, maker, 65, 3, counter), "ragged counter=%d" % counter)
    # the counter is read from the device: NULL means 0, the high word does not count, another low word gives other draws
    zero = _run(x, ei, ptr, 65, maker, 3, 0)
    none = _run(x, ei, ptr, 65, maker, 3, None)
    high = _run(x, ei, ptr, 65, maker, 3, 1 << 32)
    other = _run(x, ei, ptr, 65, maker, 3, 1)
    assert torch.equal(zero[2], none[2]) and torch.equal(zero[2], high[2]) and not torch.equal(zero[2], other[2])
    assert np.array_equal(_bits(zero[0]), _bits(none[0]))


@pytest.mark.parametrize("maker", [True, False])
def test_more_graphs_than_compute_units(maker):
    rng = np.random.default_rng(5)
    sizes = [int(v) for v in rng.integers(2, 41, size=300)]
    built = [_graph(n, tag=1 + i) for i, n in enumerate(sizes)]
    x, ei, ptr = _batch([b[0] for b in built], sizes, maker)
    got = _run(x, ei, ptr, 64, maker, 8, 2)
    _check(got, _oracle(("b300",), [b[1] for b in built], maker, 64, 8, 2), "b=300")


@pytest.mark.parametrize("size,R", [(5, 256), (5, 1000), (11, 256), (25, 64)])
def test_start_positions_from_the_env(size, R):
    """The Hex start graphs as ``Env_manager.observe()`` emits them (the env builder's CSR), both sides to move."""
    from gnn_hex_amd.multi_env_manager import Env_manager
    from gnn_hex_amd.playouts import playout_values
    mgr = Env_manager(2, size)
    obs = mgr.observe()
    b = obs.to_batch()
    n = size * size + 2
    assert obs.node_off == [0, n, 2 * n]
    ei = b.edge_index.cpu().numpy()
    adjs = [po.dense_adjacency(n, ei[:, (ei[0] >= g * n) & (ei[0] < (g + 1) * n)] - g * n) for g in range(2)]
    for maker in (True, False):
        got = playout_values(b.x, b.edge_index, b.ptr, R, seed=size, is_maker=maker, tables=True)
        _check(got, _oracle(("hex", size), adjs, maker, R, size, 0), "Hex-%d R=%d maker=%s" % (size, R, maker))
    # the hints of the observation give the same call (maker to move at the start)
    hinted = playout_values(b.x, b.edge_index, b.ptr, R, seed=size)
    assert np.array_equal(_bits(hinted[0]), _oracle(("hex", size), adjs, True, R, size, 0)[0].view(np.int32))


# ---- 2. capacity-sized target ----------------------------------------------------------------------------------------------------

def _host_csr(graphs, sizes):
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    rowptr, col = [0], []
    for i, (g, n) in enumerate(zip(graphs, sizes)):
        adj = po.dense_adjacency(n, g)
        for r in range(n):
            nb = np.nonzero(adj[r])[0] + off[i]
            col.extend(nb.tolist())
            rowptr.append(len(col))
    return off, np.array(rowptr, dtype=np.int32), np.array(col, dtype=np.int32)


@pytest.mark.parametrize("maker", [True, False])
def test_capacity_sized_target_keeps_its_tail(maker):
    from gnn_hex_amd import ops
    from gnn_hex_amd.playouts import playout_values
    sizes = [27, 2, 66, 130, 9]
    graphs = [_graph(n, tag=7)[0] for n in sizes]
    off, rowptr, col = _host_csr(graphs, sizes)
    N, E, b = int(off[-1]), len(col), len(sizes)
    n_cap, e_cap = N + 300, E + 500
    rng = np.random.default_rng(1)
    rp = np.concatenate([rowptr, rng.integers(-(1 << 30), 1 << 30, size=n_cap - N).astype(np.int32)])     # stale rows
    cl = np.concatenate([col, rng.integers(-(1 << 30), 1 << 30, size=e_cap - E).astype(np.int32)])
    results = []
    for rows, rp_h, cl_h in ((N, rowptr, col), (n_cap, rp, cl)):
        x = torch.full((rows, 3), float("nan"), dtype=torch.float32, device=DEV)
        ei = torch.zeros((2, len(cl_h)), dtype=torch.int64, device=DEV)
        ei._hex_csr = ops.GraphStructure.from_csr(rows, len(cl_h), torch.from_numpy(rp_h).to(DEV), torch.from_numpy(cl_h).to(DEV),
                                                  torch.ones(rows, dtype=torch.float32, device=DEV))
        out = torch.full((rows,), float("nan"), dtype=torch.float32, device=DEV)
        out.view(torch.int32)[N:] = torch.arange(rows - N, dtype=torch.int32, device=DEV) | 0x7fc00000      # NaNs with a payload each
        before = out.clone()
        ptr = torch.from_numpy(off.astype(np.int32)).to(DEV)
        scores, value, tables, wins = playout_values(x, ei, ptr, 100, seed=9, is_maker=maker, max_nodes=130, tables=True, out=out)
        assert scores is out
        assert torch.equal(out.view(torch.int32)[N:], before.view(torch.int32)[N:]), "rows behind ptr[b] were written"
        results.append((scores[:N].clone(), value, tables[:N].clone(), wins))
    exact, cap = results
    adjs = [po.dense_adjacency(n, g) for g, n in zip(graphs, sizes)]
    _check(exact, _oracle(("cap",), adjs, maker, 100, 9, 0), "exact-size call")
    assert np.array_equal(_bits(exact[0]), _bits(cap[0])) and np.array_equal(_bits(exact[1]), _bits(cap[1]))
    assert torch.equal(exact[2], cap[2]) and torch.equal(exact[3], cap[3])


# ---- 3. the limit ----------------------------------------------------------------------------------------------------------------

def test_graph_above_the_limit_gets_nan_and_the_status_bit():
    from gnn_hex_amd.playouts import playout_values
    sizes = [30, 641, 17]
    built = [_graph(n, tag=3) for n in sizes]
    x, ei, ptr = _batch([b[0] for b in built], sizes, True)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    scores, value, tables, wins = playout_values(x, ei, ptr, 64, seed=4, is_maker=True, max_nodes=640, tables=True, status=status)
    assert int(status) == 1
    s, v = scores.cpu().numpy(), value.cpu().numpy()
    assert np.isnan(s[30:671]).all() and np.isnan(v[1]) and int(wins[1]) == -1 and bool((tables[30:671] == -1).all())
    for g, (lo, hi) in ((0, (0, 30)), (2, (671, 688))):
        w = po.playout_graph(built[g][1], True, 64, seed=4, counter=0, g=g)
        assert np.array_equal(s[lo:hi].view(np.int32), w[0].view(np.int32)), "graph %d beside the oversized one" % g
        assert v[g].view(np.int32) == w[1].view(np.int32) and int(wins[g]) == w[3]
        assert np.array_equal(tables[lo:hi].cpu().numpy(), w[2])
    # a size hint above the limit is clamped to it: the same result, and nothing else sets the bit
    status.zero_()
    again = playout_values(x, ei, ptr, 64, seed=4, is_maker=True, max_nodes=2000, status=status)
    assert int(status) == 1 and np.array_equal(_bits(again[0])[:30], _bits(scores)[:30])
    status.zero_()
    playout_values(x[:30], ei[:, ei[0] < 30], ptr[:2], 64, seed=4, is_maker=True, status=status)
    assert int(status) == 0


# ---- 4. counter discipline -------------------------------------------------------------------------------------------------------

def test_counter_discipline_eager_and_replayed():
    from gnn_hex_amd import ops
    from gnn_hex_amd.graphs import GraphedStep
    from gnn_hex_amd.playouts import MonteCarloPlayer
    sizes = [27, 40, 2, 66]
    built = [_graph(n, tag=4) for n in sizes]
    adjs = [b[1] for b in built]
    x, ei, ptr = _batch([b[0] for b in built], sizes, False)        # the side comes from x[0, 2]: no hints on these tensors
    player = MonteCarloPlayer(32, seed=6)
    first = player(x, ei, None, ptr).clone()
    second = player(x, ei, None, ptr, advantages_only=True).clone()
    assert player.counter() == 2 and not torch.equal(first, second)
    player.set_counter(0)
    assert torch.equal(player(x, ei, None, ptr), first) and torch.equal(player(x, ei, None, ptr), second)
    for c, got in ((0, first), (1, second)):
        assert np.array_equal(_bits(got), _oracle(("ctr",), adjs, False, 32, 6, c)[0].view(np.int32)), "call %d" % c
    # graph_indices instead of ptr
    batch_vec = torch.repeat_interleave(torch.arange(len(sizes), device=DEV), torch.tensor(sizes, device=DEV))
    player.set_counter(1)
    assert torch.equal(player(x, ei, batch_vec), second)
    # a captured call advances once per replay and draws that replay's numbers (hints and a CSR attached, as the env builder
    # does: nothing is read back inside the capture)
    xh, eh, ptr32 = ops.attach_hints(x.clone(), False, max(sizes)), ei.clone(), ptr.to(torch.int32)
    eh._hex_csr = ops.GraphStructure(eh, xh.shape[0])
    player.set_counter(0)
    step = GraphedStep(lambda: player(xh, eh, None, ptr32), warmup=1)
    assert player.counter() == 1                                     # the warm-up ran, the capture did not
    for k in range(3):
        out = step.replay()
        torch.cuda.synchronize()
        assert player.counter() == 2 + k
        assert np.array_equal(_bits(out), _oracle(("ctr",), adjs, False, 32, 6, 1 + k)[0].view(np.int32)), "replay %d" % k
    player.status()


# ---- 5. arena games ---------------------------------------------------------------------------------------------------------------

def _host_game(hexref, size, g, opening, first, players):
    """Game ``g`` of a batch replayed on the host: the opening, then the oracle player of the side to move (its call counter is
    the number of its earlier plies in the batch: every ply of a side calls its player once), dead/captured removal on."""
    game = hexref.RefGame(size)
    game.maker_turn = first == "m"
    moves, t = [], 0
    while game.who_won() is None:
        if t == 0:
            v = opening
        else:
            R, seed = players[0 if game.maker_turn else 1]
            adj, bm = po.game_adjacency(game)
            v = int(bm[po.pick(po.playout_graph(adj, game.maker_turn, R, seed=seed, counter=t // 2, g=g)[0])])
        game.make_move(v, True)
        moves.append(v)
        t += 1
    return moves, game.who_won()


@pytest.mark.parametrize("first", ["m", "b"])
def test_arena_games_equal_the_host_replay(hexref, first):
    from gnn_hex_amd.arena import DeviceArena
    from gnn_hex_amd.playouts import MonteCarloPlayer
    k, openings = 6, [2, 8, 14, 20, 26, 5]
    results = {}
    for graph in (False, True):
        maker, breaker = MonteCarloPlayer(64, seed=1), MonteCarloPlayer(8, seed=2)
        arena = DeviceArena(5, k, graph=graph)
        if graph:
            arena.play(maker, breaker, first=first, openings=openings)      # captures: the warm-up plies consume counts
            assert maker.counter() > 0 and breaker.counter() > 0
        maker.set_counter(0)
        breaker.set_counter(0)
        results[graph] = res = arena.play(maker, breaker, first=first, openings=openings)
        assert maker.counter() == breaker.counter() == -(-res.plies // arena.chunk) * arena.chunk // 2
        maker.status()
        breaker.status()
    eager, graphed = results[False], results[True]
    assert np.array_equal(eager.moves, graphed.moves) and np.array_equal(eager.winner, graphed.winner)
    assert np.array_equal(eager.length, graphed.length)
    for g in range(k):
        moves, won = _host_game(hexref, 5, g, openings[g], first, ((64, 1), (8, 2)))
        assert eager.moves[g, :len(moves)].tolist() == moves, "game %d" % g
        assert (eager.moves[g, len(moves):] == -1).all() and int(eager.length[g]) == len(moves)
        assert int(eager.winner[g]) == (0 if won == "m" else 1)


# ---- 6. drop-in surfaces ------------------------------------------------------------------------------------------------------------

def test_elo_handler_takes_the_player():
    from gnn_hex_amd.arena import Elo_handler
    from gnn_hex_amd.playouts import MonteCarloPlayer
    e = Elo_handler(5)
    e.add_player("mc64", model=MonteCarloPlayer(64), uses_empty_model=False)
    e.add_player("random", model="random", simple=True, set_rating=0, rating_fixed=True, uses_empty_model=False)
    stats = e.play_some_games("mc64", "random", 4, 0)
    assert set(stats) == {"mc64", "random"} and stats["mc64"] + stats["random"] == 4
    stats = e.play_some_games("random", "mc64", 4, 0)
    assert stats["mc64"] + stats["random"] == 4


def test_env_manager_loop_and_board_values():
    from gnn_hex_amd.multi_env_manager import Env_manager
    from gnn_hex_amd.playouts import MonteCarloPlayer
    from gnn_hex_amd.positions import board_values
    size, k = 7, 4
    mgr = Env_manager(k, size)
    player = MonteCarloPlayer(64, seed=3)
    obs = mgr.observe()
    for ply in range(24):
        b = obs.to_batch()
        q = player(b.x, b.edge_index, b.batch, b.ptr, advantages_only=True)
        assert q.shape == (b.x.shape[0],) and bool(torch.isfinite(q).all())
        vert, rank, expl = mgr.select_actions(q, obs)
        legal = mgr.get_valid_actions()
        for i, v in enumerate(vert.tolist()):
            assert v in legal[i].tolist(), "ply %d env %d: vertex %d is not free" % (ply, i, v)
        # the scores back on the board: every live node's score on its cell, the fill elsewhere, the pick = the arg-max cell
        board, best = board_values(q, obs, size)
        board, bm, qh = board.cpu().numpy(), obs.backmap.cpu().numpy(), q.cpu().numpy()
        for g in range(k):
            want = np.full(size * size, -5.0, dtype=np.float32)
            lo, hi = obs.node_off[g] + 2, obs.node_off[g + 1]
            want[bm[lo:hi] - 2] = qh[lo:hi]
            assert np.array_equal(board[g].view(np.int32), want.view(np.int32)), "ply %d env %d" % (ply, g)
        assert (best.cpu().numpy() + 2 == vert.cpu().numpy()).all()
        obs, rewards, dones, infos = mgr.step(vert)                         # raises for an illegal action
    assert player.counter() == 24
    player.status()
