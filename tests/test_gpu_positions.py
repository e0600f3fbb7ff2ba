"""GPU: position set-up and board-indexed evaluation (hexgnn_env_setup, hexgnn_board_values, Env_manager.set_positions,
gnn_hex_amd/positions.py) against the C env oracle and the CPU model oracle.  Stone lists are drawn on the oracle; the device
state must equal the oracle's bit for bit (boards, side, move count, response sets) on every W instantiation; errors are the
kernel's own refusals; snapshots equal a second manager stepped ply by ply; board values equal torch indexing; the long-range
task runs end to end against oracle.model_ref."""
import ctypes as C

import numpy as np
import pytest
import torch

from positions_oracle import OracleGame, assert_env_equals, random_stone_list

pytestmark = pytest.mark.gpu

W_SIZES = [5, 8, 12, 14, 16]          # 27, 66, 146, 198, 258 vertices: W = 1, 2, 3, 4 and the generic instantiation
WINNER = {None: -1, "m": 0, "b": 1}


def _setup_raw(mgr, lists, from_start=1, maker_turn_start=1, maker_turn_after=-1, snapshots=False, L=None):
    """hexgnn_env_setup on the manager's handle: (result [k, 5], applied [k], snapshot tensors or None) as host arrays."""
    from gnn_hex_amd import _lib, ops
    arr, cnt = mgr._pack_stones(lists)
    if L is not None and L > arr.shape[1]:
        arr = np.concatenate([arr, np.zeros((arr.shape[0], L - arr.shape[1]), np.int32)], 1)
    k, L = arr.shape
    dev, nv, W = mgr.device, mgr._nv, mgr._words
    st, ct = torch.from_numpy(np.ascontiguousarray(arr)).to(dev), torch.from_numpy(cnt).to(dev)
    result = torch.full((k, 5), -9, dtype=torch.int32, device=dev)
    applied = torch.full((k,), -9, dtype=torch.int32, device=dev)
    call = _lib.SetupCall(struct_bytes=C.sizeof(_lib.SetupCall), max_stones=L, from_start=from_start,
                          maker_turn_start=maker_turn_start, maker_turn_after=maker_turn_after, stones=st.data_ptr(),
                          count=ct.data_ptr(), result=result.data_ptr(), applied=applied.data_ptr())
    snap = None
    if snapshots:
        snap = dict(adj=torch.zeros((k, L, nv, W), dtype=torch.int64, device=dev),
                    alive=torch.zeros((k, L, nv), dtype=torch.uint8, device=dev),
                    side=torch.full((k, L), 7, dtype=torch.uint8, device=dev),
                    sizes=torch.full((k, L, 2), -9, dtype=torch.int32, device=dev))
        call.adj_out, call.alive_out = snap["adj"].data_ptr(), snap["alive"].data_ptr()
        call.side_out, call.sizes_out = snap["side"].data_ptr(), snap["sizes"].data_ptr()
    _lib.check(_lib.lib().hexgnn_env_setup(mgr._h, C.byref(call), ops._stream()), "hexgnn_env_setup")
    mgr._touch += 1
    mgr.last_obs = None
    res = result.cpu().numpy()
    mgr._sizes = res[:, 2:4].astype(np.int64)
    return res, applied.cpu().numpy(), snap


def _assert_obs_equals_oracle(obs, games):
    """The batched observation against RefGame.observe() per env: x, edge_index, backmap, the offsets and the CSR."""
    from gnn_hex_amd import ops
    from gnn_hex_amd.data import Batch
    robs = [g.observe() for g in games]
    offs = np.cumsum([0] + [o[0].shape[0] for o in robs])
    assert obs.node_off == offs.tolist()
    b = Batch.from_data_list(obs)
    assert np.array_equal(b.x.cpu().numpy(), np.concatenate([o[0] for o in robs], 0))
    assert np.array_equal(b.edge_index.cpu().numpy(), np.concatenate([o[1] + int(off) for o, off in zip(robs, offs[:-1])], 1))
    assert np.array_equal(obs.backmap.cpu().numpy(), np.concatenate([o[2] for o in robs]))
    gs, gs2 = b.edge_index._hex_csr, ops.GraphStructure(b.edge_index, b.x.shape[0])
    torch.cuda.synchronize()
    assert torch.equal(gs.rowptr, gs2.rowptr) and torch.equal(gs.col[:gs.e], gs2.col[:gs2.e])
    assert torch.equal(gs.invdeg[:gs.n], gs2.invdeg[:gs2.n])


def _check_against_oracle(tag, mgr, res, applied, ogs, lists):
    st = mgr._state()
    undecided = 0
    for i, (og, lst) in enumerate(zip(ogs, lists)):
        assert res[i, 4] == 0 and applied[i] == len(lst), "%s env %d: error %d at stone %d" % (tag, i, res[i, 4], applied[i])
        assert res[i, 0] == WINNER[og.game.who_won()] and res[i, 1] == og.moves, "%s env %d" % (tag, i)
        assert int(st["total_moves"][i]) == og.moves
        if og.game.who_won() is None:      # the residual graph of a decided game is unspecified (include/hexgnn.h)
            undecided += 1
            assert_env_equals(st, i, og, tag)
            assert (res[i, 2], res[i, 3]) == (og.game.num_vertices(), 2 * og.game.num_edges()), "%s env %d: sizes" % (tag, i)
    return undecided


def _stone_case(hexref, size, k=8):
    """The seeded random stone lists of one board size, drawn on the oracle: (L, rng, oracle games after them, lists).  List
    lengths 0, 1 and up to L; a list stops when the position is decided."""
    L = 8 if size == 5 else 24
    rng = np.random.default_rng(100 + size)
    lengths = [0, 1, L, L] + [int(v) for v in rng.integers(2, L + 1, k - 4)]
    ogs = [OracleGame(hexref, size, maker_turn=False) for _ in range(k)]
    lists = [random_stone_list(og, rng, n) for og, n in zip(ogs, lengths)]
    assert len(lists[0]) == 0 and len(lists[1]) == 1 and max(len(l) for l in lists) == L
    colours = {c for l in lists for _, c, _ in l}
    assert colours == {"m", "b", "turn"} and {r for l in lists for _, _, r in l} == {False, True}
    assert sum(og.game.who_won() is None for og in ogs) >= k // 2
    assert any(int(og.moves) not in (0, len(l)) for og, l in zip(ogs, lists)), "forced stones must not count as moves"
    return L, rng, ogs, lists


@pytest.mark.parametrize("size", W_SIZES)
def test_stone_lists_bit_exact_on_every_instantiation(hexref, size):
    from gnn_hex_amd.multi_env_manager import Env_manager
    k = 8
    L, rng, ogs, lists = _stone_case(hexref, size, k)
    mgr = Env_manager(k, size)
    assert mgr._words == {5: 1, 8: 2, 12: 3, 14: 4, 16: 5}[size]
    res, applied, _ = _setup_raw(mgr, lists, from_start=1, maker_turn_start=0, maker_turn_after=-1)
    undecided = _check_against_oracle("from start", mgr, res, applied, ogs, lists)
    assert undecided >= k // 2
    # ... and again on top of what the envs hold (a decided env gets no further stone)
    more = [random_stone_list(og, rng, int(rng.integers(1, L + 1))) if og.game.who_won() is None else [] for og in ogs]
    res, applied, _ = _setup_raw(mgr, more, from_start=0, maker_turn_after=-1)
    undecided = _check_against_oracle("on top", mgr, res, applied, ogs, more)
    assert undecided >= 2
    # through the public call, which starts with the maker to move (the lists were drawn with the breaker first, so a "turn"
    # stone now plays for the other side): the longest prefix that is legal and undecided on the oracle, everyone with the
    # breaker to move afterwards
    ogs2, lists2 = [], []
    for lst, extra in zip(lists, more):
        og, keep = OracleGame(hexref, size), []
        for s in lst + extra:
            try:
                decided = og.apply(*s) is not None
            except ValueError:                             # removed as dead / captured in this line of play: stop in front of it
                break
            if decided:
                og = OracleGame(hexref, size)              # drop the deciding stone: replay the prefix
                for t in keep:
                    og.apply(*t)
                break
            keep.append(s)
        og.game.maker_turn = False
        ogs2.append(og)
        lists2.append(keep)
    obs = mgr.set_positions(lists2, onturn="b")
    assert mgr.global_onturn == "b" and len(obs) == k and obs.is_maker is False
    st = mgr._state()
    for i, og in enumerate(ogs2):
        assert_env_equals(st, i, og, "set_positions")
        assert mgr.envs[i].total_num_moves == og.moves == sum(c == "turn" for _, c, _ in lists2[i])
    assert mgr._sizes.tolist() == [[og.game.num_vertices(), 2 * og.game.num_edges()] for og in ogs2]
    _assert_obs_equals_oracle(obs, [og.game for og in ogs2])
    # the packed form gives the same boards
    arr, cnt = mgr._pack_stones(lists2)
    mgr.set_positions(arr, onturn="b", counts=cnt)
    st2 = mgr._state()
    for key in st:
        assert np.array_equal(st[key], st2[key]), key


@pytest.mark.parametrize("size", [5, 8, 12, 14, 16, 25])
def test_long_range_positions_equal_the_oracle(hexref, size):
    from gnn_hex_amd.multi_env_manager import Env_manager
    from gnn_hex_amd.positions import long_range_stones
    mgr = Env_manager(2, size)
    for defender in ("m", "b"):
        pair = long_range_stones(size, defender)
        ogs = []
        for stones in pair:
            og = OracleGame(hexref, size)
            for s in stones:
                assert og.apply(*s) is None
            og.game.maker_turn = defender == "m"
            ogs.append(og)
        obs = mgr.set_positions(pair, onturn=defender)
        assert mgr.global_onturn == defender and obs.is_maker == (defender == "m")
        st = mgr._state()
        for i, og in enumerate(ogs):
            assert_env_equals(st, i, og, "long range %s" % defender)
            assert og.moves == 0
        assert obs.node_off == [0, size * size + 2 - (4 * size - 6), 2 * (size * size + 2) - (8 * size - 10)]
        _assert_obs_equals_oracle(obs, [og.game for og in ogs])


def _captured_victim(hexref, size, rng):
    """A stone list with removal after which some vertex that was never played is gone: (list, that vertex)."""
    for _ in range(200):
        og, lst, played = OracleGame(hexref, size, maker_turn=False), [], set()
        for _ in range(size * size):
            acts = og.game.get_actions()
            v = int(acts[rng.integers(len(acts))])
            lst.append((v, "turn", True))
            played.add(v)
            if og.apply(v, "turn", True) is not None:
                break
            gone = set(range(2, size * size + 2)) - set(og.game.get_actions().tolist()) - played
            if gone:
                return lst, min(gone)
    raise AssertionError("no playout removed a dead or captured vertex")


def _decided_list(hexref, size, rng, maker_turn=False):
    og, lst = OracleGame(hexref, size, maker_turn=maker_turn), []
    while True:
        acts = og.game.get_actions()
        v = int(acts[rng.integers(len(acts))])
        lst.append((v, "turn", True))
        if og.apply(v, "turn", True) is not None:
            return lst, og


def _error_case(hexref, size=5):
    """Eight stone lists for envs that start with the BREAKER to move (maker_turn_start = 0): the expected error, the expected
    `applied` entry, and the oracle's side of the lists that are legal."""
    nv = size * size + 2
    rng = np.random.default_rng(5)
    good = [(8, "m", False), (14, "b", True), (9, "turn", True)]
    cap_list, victim = _captured_victim(hexref, size, rng)
    dec_list, dec_og = _decided_list(hexref, size, rng)
    spare = next(v for v in range(2, nv) if v not in {s[0] for s in dec_list})
    lists = [good,
             [(5, "m", False), (6, "b", False), (5, "b", False)],           # a repeated cell
             [(7, "turn", True), (1, "m", False)],                          # a terminal
             [(nv + 3, "b", False)],                                        # a vertex >= nv
             cap_list + [(victim, "m", False)],                             # removed as dead / captured earlier in the list
             dec_list + [(spare, "turn", True)],                            # behind the deciding stone
             dec_list,                                                      # the deciding stone last: a winner, no error
             good]
    want_err = [0, 1, 1, 1, 1, 2, 0, 0]
    want_idx = [3, 2, 1, 0, len(cap_list), len(dec_list), len(dec_list), 3]
    og_good = OracleGame(hexref, size, maker_turn=False)
    for s in good:
        assert og_good.apply(*s) is None
    return lists, want_err, want_idx, good, og_good, dec_list, dec_og, spare


def test_errors_are_refused_by_the_kernel_and_reset_the_env(hexref):
    """Every refusal here is the kernel's own check of the stone before the vertex is used: nothing faults."""
    from gnn_hex_amd.multi_env_manager import Env_manager
    size = 5
    nv = size * size + 2
    lists, want_err, want_idx, good, og_good, dec_list, dec_og, spare = _error_case(hexref, size)
    k = len(lists)
    mgr = Env_manager(k, size)
    for from_start in (1, 0):
        if not from_start:
            mgr.reset()                                                     # the lists again, on top of start positions
            _setup_raw(mgr, [[]] * k, from_start=1, maker_turn_start=0)
        res, applied, snap = _setup_raw(mgr, lists, from_start=from_start, maker_turn_start=0, snapshots=True)
        assert res[:, 4].tolist() == want_err and applied.tolist() == want_idx
        assert res[6, 0] == WINNER[dec_og.game.who_won()] and res[6, 1] == dec_og.moves == len(dec_list)
        st = mgr._state()
        for i in (0, 7):                                                    # envs without an error are unaffected
            assert_env_equals(st, i, og_good, "good env")
            assert res[i, 0] == -1 and (res[i, 2], res[i, 3]) == (og_good.game.num_vertices(), 2 * og_good.game.num_edges())
        start = OracleGame(hexref, size, maker_turn=False)
        for i in (1, 2, 3, 4, 5):                                           # envs with an error are at the start position
            assert_env_equals(st, i, start, "error env")
            assert res[i, 0] == -1 and res[i, 1] == 0 and (res[i, 2], res[i, 3]) == (nv, 2 * start.game.num_edges())
        sizes = snap["sizes"].cpu().numpy()
        for i in range(k):                                                  # slots from the offending stone on hold no position
            assert (sizes[i, want_idx[i]:] == 0).all()
            held = want_idx[i] - (1 if i in (5, 6) else 0)                  # (the deciding stone's slot holds none either)
            assert (sizes[i, :held, 0] > 0).all() and (sizes[i, held:want_idx[i]] == 0).all()
    # the public call names env and stone, and leaves every env with the side asked for
    with pytest.raises(ValueError, match=r"env 1, stone 2 \(vertex 5\)"):
        mgr.set_positions(lists, onturn="b")
    assert mgr.global_onturn == "b" and (mgr._state()["maker_turn"] == 0).all()
    dec_m, _ = _decided_list(hexref, size, np.random.default_rng(6), maker_turn=True)      # set_positions starts with the maker
    spare_m = next(v for v in range(2, nv) if v not in {s[0] for s in dec_m})
    with pytest.raises(ValueError, match=r"env 1, stone %d \(vertex %d\) follows" % (len(dec_m), spare_m)):
        mgr.set_positions([good, dec_m + [(spare_m, "b", False)]] + [[]] * (k - 2), onturn="m")
    with pytest.raises(ValueError, match="env 3: the position is decided"):
        mgr.set_positions([good, [], [], dec_m] + [[]] * (k - 4), onturn="m")
    obs = mgr.set_positions([good] * k, onturn="m")                         # and works again afterwards
    assert len(obs) == k and (mgr._state()["maker_turn"] == 1).all()


def _playout(hexref, size, k, plies):
    """Per env up to ``plies`` random moves (maker first, dead/captured removal), drawn on the oracle: each move is the first
    of a shuffle of the legal ones that leaves the game undecided; where every move decides it (with removal a Hex-5 game
    rarely lasts ten plies) the list ends with that deciding move.  Returns (moves per env, winner per env or None)."""
    rng = np.random.default_rng(1000 * size)
    out, winners = [], []
    for i in range(k):
        game, row = hexref.RefGame(size), []
        for t in range(plies):
            for v in rng.permutation(game.get_actions()):
                trial = game.copy()
                trial.make_move(int(v), remove_dead_and_captured=True)
                if trial.who_won() is None:
                    break
            game.make_move(int(v), remove_dead_and_captured=True)
            row.append(int(v))
            if game.who_won() is not None:
                break
        out.append(row)
        winners.append(game.who_won())
    return out, winners


@pytest.mark.parametrize("size", [5, 8])
def test_snapshots_equal_a_manager_stepped_ply_by_ply(hexref, size):
    """Slot j of every env equals the state after j + 1 calls of Env_manager.step on a second manager, bit for bit, for as long
    as the env's game lasts.  Env_manager.step restarts a finished game where the set-up has no auto reset, so a list ends with
    its deciding move: that slot holds no position, the stepped manager reports the same winner and length there, and plays on
    alone."""
    from gnn_hex_amd.multi_env_manager import Env_manager
    k, plies = 6, 10
    moves, winners = _playout(hexref, size, k, plies)
    assert any(w is None for w in winners) or size == 5
    a, b = Env_manager(k, size), Env_manager(k, size)
    lists = [[(v, "turn", True) for v in row] for row in moves]
    res, applied, snap = _setup_raw(a, lists, from_start=1, maker_turn_start=1, snapshots=True, L=plies)
    assert (res[:, 4] == 0).all() and applied.tolist() == [len(r) for r in moves] == res[:, 1].tolist()
    assert res[:, 0].tolist() == [WINNER[w] for w in winners]
    adj = snap["adj"].cpu().numpy().view(np.uint64)
    alive, side, sizes = snap["alive"].cpu().numpy(), snap["side"].cpu().numpy(), snap["sizes"].cpu().numpy()
    b.reset()
    compared = 0
    for t in range(plies):
        valid = b.get_valid_actions()
        acts = [moves[i][t] if t < len(moves[i]) else int(valid[i][0]) for i in range(k)]
        _, _, dones, infos = b.step(acts)
        st = b._state()
        for i in range(k):
            last = len(moves[i]) - 1
            if t < last or (t == last and winners[i] is None):
                assert np.array_equal(adj[i, t], st["adj"][i]) and np.array_equal(alive[i, t], st["alive"][i]), (i, t)
                assert side[i, t] == st["maker_turn"][i] and sizes[i, t].tolist() == b._sizes[i].tolist(), (i, t)
                assert not dones[i]
                compared += 1
            else:
                assert (sizes[i, t] == 0).all(), (i, t)
                if t == last:                           # the deciding move: no position, the same verdict
                    m = infos[i]["episode_metrics"]
                    assert dones[i] and m["length"] == res[i, 1] and (m["return"] == 1) == (res[i, 0] == 0), (i, t)
    assert compared >= k * plies // 2
    sa, sb = a._state(), b._state()
    for i in range(k):
        if winners[i] is None:
            for key in sa:
                assert np.array_equal(sa[key][i], sb[key][i]), (key, i)


def test_replay_games_reproduces_an_arena_match(hexref):
    from gnn_hex_amd.arena import DeviceArena
    from gnn_hex_amd.positions import replay_games
    gen = torch.Generator(device="cuda").manual_seed(3)
    match = DeviceArena(5, 6, graph=False).play("random", "random", first="b", generator=gen)
    rp = replay_games(5, match.moves, first="b")
    assert rp.winner.tolist() == match.winner.tolist() and rp.length.tolist() == match.length.tolist()
    assert rp.plies == match.plies == int(match.length.max())
    with pytest.raises(ValueError, match="no game holds a position"):
        rp.positions_at(match.plies - 1)
    for ply in sorted({0, 3, int(match.length.min()) - 1, match.plies - 2} & set(range(match.plies - 1))):
        obs, games = rp.positions_at(ply)
        # a game holds a position after its move `ply` when it had that move and was not decided by it
        assert games.tolist() == [g for g in range(6) if match.length[g] > ply + 1]
        assert obs.is_maker == (ply % 2 == 0)               # the breaker moved first
        ogs = []
        for g in games:
            og = OracleGame(hexref, 5, maker_turn=False)
            for v in match.moves[g, :ply + 1]:
                assert og.apply(int(v), "turn", True) is None
            ogs.append(og.game)
        assert len(obs) == len(ogs)
        if ogs:
            assert all(g.maker_turn == obs.is_maker for g in ogs)
            _assert_obs_equals_oracle(obs, ogs)
    with pytest.raises(ValueError, match="game 0, ply 1: illegal move"):
        replay_games(5, [[4, 4, -1], [5, 6, 7]])
    with pytest.raises(ValueError):
        replay_games(5, [[4, -1, 6]])


# ---- Q back on the board --------------------------------------------------------------------------------------------------

def _board_batch():
    """A Hex-5 + Hex-7 mixed batch, cells of a 7 x 7 board: (ptr, backmap, q).  Graph 2 has only its terminals, graph 3 a tied
    maximum, graph 4 holds NaN rows, graph 5 nothing but NaN, graph 6 one non-terminal row, graph 7 an empty 7 x 7 board."""
    rng = np.random.default_rng(11)
    cells = [(25, 14), (49, 30), (25, 0), (49, 40), (49, 33), (25, 9), (49, 1), (49, 49)]
    bms = [np.concatenate([[0, 1], 2 + np.sort(rng.choice(c, n, replace=False))]) for c, n in cells]
    ptr = np.concatenate([[0], np.cumsum([len(b) for b in bms])])
    backmap = np.concatenate(bms).astype(np.int64)
    q = (rng.random(ptr[-1]) * 4 - 2).astype(np.float32)
    q[ptr[:-1]] = 50.0                                      # a terminal row never wins and is never written
    q[ptr[3] + 2 + 7] = q[ptr[3] + 2 + 31] = 3.5            # the tie: the first index wins
    q[ptr[4] + 2 + 3] = q[ptr[4] + 2 + 20] = np.nan
    q[ptr[5] + 2:ptr[6]] = np.nan
    return ptr, backmap, q


@pytest.mark.parametrize("fill", [-5.0, 0.1])
def test_board_values_equal_torch_indexing(fill):
    from gnn_hex_amd import _lib, ops
    ptr, backmap, q = _board_batch()
    b, n = len(ptr) - 1, 7
    gptr = torch.from_numpy(ptr.astype(np.int32)).cuda()
    qd, bm = torch.from_numpy(q).cuda(), torch.from_numpy(backmap).cuda()
    board = torch.full((b, n * n), 77.0, device="cuda")
    best = torch.full((b,), -7, dtype=torch.int32, device="cuda")
    _lib.check(_lib.lib().hexgnn_board_values(b, n, gptr.data_ptr(), qd.data_ptr(), bm.data_ptr(), fill, board.data_ptr(),
                                              best.data_ptr(), ops._stream()), "hexgnn_board_values")
    # GREEDY of hexgnn_sample_actions on the same q: the comparison the NaN rows follow
    vert = torch.empty(b, dtype=torch.int32, device="cuda")
    rank = torch.empty(b, dtype=torch.int32, device="cuda")
    _lib.check(_lib.lib().hexgnn_sample_actions(b, gptr.data_ptr(), qd.data_ptr(), bm.data_ptr(), 0, 1.0, None, vert.data_ptr(),
                                                rank.data_ptr(), None, ops._stream()), "hexgnn_sample_actions")
    board, best, vert = board.cpu(), best.cpu().tolist(), vert.cpu().tolist()
    want = torch.full((b, n * n), np.float32(fill).item())
    qt, bt = torch.from_numpy(q), torch.from_numpy(backmap)
    for g in range(b):
        r0, r1 = int(ptr[g]) + 2, int(ptr[g + 1])
        want[g, bt[r0:r1] - 2] = qt[r0:r1]
        occupied = np.setdiff1d(np.arange(n * n), backmap[r0:r1] - 2)
        assert (board[g, occupied] == np.float32(fill)).all(), "fill is exact"
        if g not in (2, 4, 5):
            assert best[g] == int(bt[r0 + int(torch.argmax(qt[r0:r1]))]) - 2, g
            assert best[g] == int(torch.argmax(board[g])) or fill > qt[r0:r1].max()
        assert best[g] == (vert[g] - 2 if vert[g] >= 0 else -1), "graph %d: hexgnn_sample_actions' GREEDY pick" % g
    assert torch.equal(torch.nan_to_num(board, nan=123.0), torch.nan_to_num(want, nan=123.0))
    assert torch.isnan(board).sum() == 2 + 9
    assert best[2] == -1 and best[5] == -1 and best[3] == int(backmap[ptr[3] + 2 + 7]) - 2
    assert best[4] >= 0 and not np.isnan(q[ptr[4]:ptr[5]][np.nonzero(backmap[ptr[4]:ptr[5]] - 2 == best[4])[0][0]])
    # best may be left out
    board2 = torch.empty((b, n * n), device="cuda")
    _lib.check(_lib.lib().hexgnn_board_values(b, n, gptr.data_ptr(), qd.data_ptr(), bm.data_ptr(), fill, board2.data_ptr(),
                                              None, ops._stream()), "hexgnn_board_values")
    assert torch.equal(torch.nan_to_num(board2.cpu(), nan=123.0), torch.nan_to_num(board, nan=123.0))


def test_board_values_of_an_observation():
    from gnn_hex_amd.multi_env_manager import Env_manager
    from gnn_hex_amd.positions import board_values
    mgr = Env_manager(5, 6)
    rng = np.random.default_rng(2)
    obs = mgr.reset()
    for _ in range(7):
        obs, *_ = mgr.step([int(v[rng.integers(len(v))]) for v in mgr.get_valid_actions()])
    q = torch.randn(obs.x.shape[0], 1, device="cuda")
    board, best = board_values(q, obs, 6)
    assert board.shape == (5, 36) and board.is_cuda and best.dtype == torch.int32
    bm, qc = obs.backmap.cpu(), q.cpu().reshape(-1)
    for g in range(5):
        n0, n1 = obs.node_off[g] + 2, obs.node_off[g + 1]
        want = torch.full((36,), -5.0)
        want[bm[n0:n1] - 2] = qc[n0:n1]
        assert torch.equal(board[g].cpu(), want)
        assert int(best[g]) == int(torch.argmax(want)) == int(bm[n0 + int(torch.argmax(qc[n0:n1]))]) - 2
    vert, _, _ = mgr.select_actions(q, obs)
    assert (vert.cpu() - 2).tolist() == best.cpu().tolist()


# ---- end to end: the long-range task against the CPU model oracle ----------------------------------------------------------

E2E_SIZES = (5, 6, 7, 8, 12)
E2E_SEED = 1          # chosen on the CPU: with these weights the oracle's top-two gap is <= 1e-3 in 4 of the 20 cases (cap: 5)


def test_long_range_task_end_to_end_against_the_model_oracle(hexref):
    """Board values within the project's 1e-4 of oracle.model_ref on RefGame.observe(); arg-max cells equal wherever the oracle's
    top-two gap exceeds 1e-3 (the positions are symmetric: tied cells are common with random weights)."""
    from helpers import make_pair
    from gnn_hex_amd.multi_env_manager import Env_manager
    from gnn_hex_amd.positions import evaluate, long_range_stones
    hip, ref = make_pair(4, 24, seed=E2E_SEED)
    cases = skipped = 0
    worst = 0.0
    for size in E2E_SIZES:
        mgr = Env_manager(2, size)
        for defender in ("m", "b"):
            pair = long_range_stones(size, defender)
            obs = mgr.set_positions(pair, onturn=defender)
            board, best = evaluate(hip, obs, size)
            board, best = board.cpu(), best.cpu().tolist()
            assert board.shape == (2, size * size)
            for i, stones in enumerate(pair):
                og = OracleGame(hexref, size)
                for s in stones:
                    og.apply(*s)
                og.game.maker_turn = defender == "m"
                x, ei, bm = og.game.observe()
                n = x.shape[0]
                with torch.no_grad():
                    q = ref(torch.from_numpy(x), torch.from_numpy(ei), torch.zeros(n, dtype=torch.long), torch.tensor([0, n]))
                q = q.reshape(-1)
                want = torch.full((size * size,), -5.0)
                want[torch.from_numpy(bm[2:]) - 2] = q[2:]
                err = (board[i] - want).abs().max().item()
                worst = max(worst, err)
                assert err < 1e-4, "Hex-%d defender %s position %d: |board - oracle| %.3g" % (size, defender, i, err)
                assert (board[i][want == -5.0] == -5.0).all()
                top = torch.sort(q[2:].double()).values[-2:]
                cases += 1
                if float(top[1] - top[0]) > 1e-3:
                    assert best[i] == int(torch.argmax(want)), "Hex-%d defender %s position %d" % (size, defender, i)
                else:
                    skipped += 1
                assert best[i] == int(torch.argmax(board[i]))
    print("long-range end to end: %d cases, %d under the gap rule, worst |board - oracle| %.3g" % (cases, skipped, worst))
    assert cases == 20 and 4 * skipped <= cases, "%d of %d cases skipped by the gap rule" % (skipped, cases)
