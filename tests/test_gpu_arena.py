"""GPU: match play on the device -- the sampling kernel against a float64 CDF, the ply kernel against hexgnn_select_actions +
hexgnn_env_step on a twin handle, whole matches replayed move by move on the C env oracle with the float64 model oracle judging
every model-chosen move, and the properties of the loop (HIP graph = eager, chunking, cached graphs, the random player,
Elo_handler = its two DeviceArena.play calls, Env_manager.select_actions unchanged without a temperature)."""
import copy
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GREEDY, UNIFORM, SOFTMAX = 0, 1, 2
TOL = 1e-4        # fp32 sums of at most 625 positive terms, few-ulp expf and divide: (n + 4) 2^-24 ~ 3.8e-5 on a prefix, the same on
                  # the total, 7.5e-5 on their ratio
DRAWS = 4096


# ---- the sampling kernel alone -----------------------------------------------------------------------------------------

SIZES = [2, 3, 4, 66, 67, 130, 627, 67, 130]       # nodes per graph; graph 7: all values equal, graph 8: a tied maximum


def _sample_batch():
    rng = np.random.default_rng(7)
    ptr = np.concatenate([[0], np.cumsum(SIZES)])
    q = (rng.random(ptr[-1]) * 10 - 5).astype(np.float32)
    q[ptr[7]:ptr[8]] = 1.25
    a, b = ptr[8] + 2 + 40, ptr[8] + 2 + 90
    q[a] = q[b] = 4.9990234375                       # above every other value of the graph, twice
    assert q[ptr[8]:ptr[9]].max() == q[a] and (q[ptr[8]:ptr[9]] == q[a]).sum() == 2
    backmap = rng.permutation(ptr[-1]).astype(np.int64)
    return ptr, q, backmap


def _sample(ptr, q, backmap, mode, temperature, u, reps=1):
    """hexgnn_sample_actions over ``reps`` copies of the batch (copy r draws with u[r]): (rank [reps, b], vertex, status)."""
    from gnn_hex_amd import _lib, ops
    b, n = len(ptr) - 1, int(ptr[-1])
    gptr = (np.arange(reps)[:, None] * n + ptr[None, :-1]).reshape(-1)
    gptr = torch.from_numpy(np.concatenate([gptr, [reps * n]]).astype(np.int32)).cuda()
    qd = torch.from_numpy(q).cuda().repeat(reps) if q is not None else None
    bm = torch.from_numpy(backmap).cuda().repeat(reps)
    ud = torch.from_numpy(np.repeat(np.asarray(u, dtype=np.float32), b)).cuda() if u is not None else None
    vert = torch.full((reps * b,), -7, dtype=torch.int32, device="cuda")
    rank = torch.full((reps * b,), -7, dtype=torch.int32, device="cuda")
    status = torch.full((1,), 99, dtype=torch.int32, device="cuda")
    _lib.check(_lib.lib().hexgnn_sample_actions(reps * b, gptr.data_ptr(), qd.data_ptr() if qd is not None else None, bm.data_ptr(),
                                                mode, temperature, ud.data_ptr() if ud is not None else None, vert.data_ptr(),
                                                rank.data_ptr(), status.data_ptr(), ops._stream()), "hexgnn_sample_actions")
    return rank.cpu().numpy().reshape(reps, b), vert.cpu().numpy().reshape(reps, b), int(status.item())


@pytest.mark.parametrize("temperature", [1e-4, 0.1, 1.0, 10.0])
def test_softmax_draws_follow_the_float64_cdf(temperature):
    ptr, q, backmap = _sample_batch()
    u = (np.arange(DRAWS) + 0.5) / DRAWS
    rank, vert, status = _sample(ptr, q, backmap, SOFTMAX, temperature, u, reps=DRAWS)
    assert status == 0
    t64 = float(np.float32(temperature))              # the temperature the kernel received
    u32 = u.astype(np.float32).astype(np.float64)     # (i + 0.5) / 4096 is exact in fp32
    assert np.array_equal(u32, u)
    worst, worst_count = 0.0, 0.0
    for g, n in enumerate(SIZES):
        r = rank[:, g]
        if n == 2:
            assert (r == -1).all() and (vert[:, g] == -1).all()
            continue
        assert (vert[:, g] == backmap[ptr[g] + r]).all()
        if n == 3:
            assert (r == 2).all()
            continue
        assert (r >= 2).all() and (r < n).all()
        q64 = q[ptr[g] + 2:ptr[g + 1]].astype(np.float64)
        w = np.exp((q64 - q64.max()) / t64)
        p = w / w.sum()
        c = np.concatenate([[0.0], np.cumsum(p)])
        j = r - 2
        lo, hi = c[j] - u, u - c[j + 1]                # both must be <= TOL
        worst = max(worst, lo.max(), hi.max())
        assert (lo <= TOL).all() and (hi <= TOL).all(), "graph %d T %g: draw outside its CDF cell by %.3g / %.3g" % (g, temperature, lo.max(), hi.max())
        counts = np.bincount(j, minlength=n - 2)
        dev = np.abs(counts - DRAWS * p).max()
        worst_count = max(worst_count, dev)
        assert dev <= 2 + DRAWS * TOL, "graph %d T %g: pick counts off by %.3g" % (g, temperature, dev)
        top = np.sort(q64)[-2:]
        if temperature == 1e-4 and top[1] - top[0] > 0.01:
            assert (j == int(np.argmax(q64))).all(), "graph %d: T = 1e-4 must play the argmax" % g
    print("T %g: worst distance outside the CDF cell %.3g (tol %g), worst count deviation %.3g (bound %.3g)"
          % (temperature, worst, TOL, worst_count, 2 + DRAWS * TOL))
    if temperature == 1e-4:
        gaps = [np.diff(np.sort(q[ptr[g] + 2:ptr[g + 1]].astype(np.float64))[-2:])[0] for g in (3, 4, 5)]
        assert max(gaps) > 0.01, "no graph with a clear maximum: the argmax claim was not exercised"
        # the tied maximum: the first of the two for u below 1/2, the second above (each holds half of the mass)
        j = rank[:, 8] - 2
        assert set(j.tolist()) == {40, 90} and (j[:DRAWS // 2 - 1] == 40).all() and (j[DRAWS // 2 + 1:] == 90).all()


def test_softmax_reports_a_nan():
    ptr, q, backmap = _sample_batch()
    q = q.copy()
    q[ptr[5] + 17] = np.nan
    rank, vert, status = _sample(ptr, q, backmap, SOFTMAX, 1.0, [0.3, 0.9], reps=2)
    assert status & 1
    assert (rank[:, 5] == 2).all() and (vert[:, 5] == backmap[ptr[5] + 2]).all()
    clean = _sample(ptr, _sample_batch()[1], backmap, SOFTMAX, 1.0, [0.3, 0.9], reps=2)
    assert clean[2] == 0
    others = [g for g in range(len(SIZES)) if g != 5]
    assert np.array_equal(rank[:, others], clean[0][:, others])


def test_greedy_and_uniform_equal_select_actions():
    from gnn_hex_amd import _lib, ops
    ptr, q, backmap = _sample_batch()
    b = len(SIZES)
    rng = np.random.default_rng(3)
    u = rng.random((b, 2)).astype(np.float32)
    u[6, 1] = np.float32(1.0) - np.float32(2.0 ** -24)          # the largest fp32 below 1: floor(u * 625) must stay in range
    gptr = torch.from_numpy(ptr.astype(np.int32)).cuda()
    qd, bm, ud = torch.from_numpy(q).cuda(), torch.from_numpy(backmap).cuda(), torch.from_numpy(u).cuda()
    L = _lib.lib()
    for mode, eps in ((GREEDY, 0.0), (UNIFORM, 1.0)):
        want_v = torch.empty(b, dtype=torch.int32, device="cuda")
        want_r = torch.empty(b, dtype=torch.int32, device="cuda")
        _lib.check(L.hexgnn_select_actions(b, gptr.data_ptr(), qd.data_ptr(), bm.data_ptr(), eps, ud.data_ptr() if eps else None,
                                           want_v.data_ptr(), want_r.data_ptr(), None, ops._stream()))
        got_v = torch.empty(b, dtype=torch.int32, device="cuda")
        got_r = torch.empty(b, dtype=torch.int32, device="cuda")
        u1 = ud[:, 1].contiguous()
        _lib.check(L.hexgnn_sample_actions(b, gptr.data_ptr(), qd.data_ptr() if mode == GREEDY else None, bm.data_ptr(), mode, 1.0,
                                           u1.data_ptr() if mode == UNIFORM else None, got_v.data_ptr(), got_r.data_ptr(), None,
                                           ops._stream()))
        assert torch.equal(got_r, want_r) and torch.equal(got_v, want_v), mode
        assert int(got_r[0]) == -1 and int(got_r[1]) == 2
    assert int(got_r[6]) == 626                                   # 2 + 624: the clamp


# ---- the ply kernel alone ------------------------------------------------------------------------------------------------

def _import_positions(hexref, mgr, size, k, maker):
    """Put k random mid-game oracle positions (all with the same side to move) into the manager's envs."""
    games = [hexref.random_position(size, 100 * size + g, maker) for g in range(k)]
    st = mgr._state_tensors()
    adj = np.stack([g.dump()[0] for g in games]).view(np.int64)
    alive = np.stack([g.dump()[1] for g in games])
    st["adj"].copy_(torch.from_numpy(adj))
    st["alive"].copy_(torch.from_numpy(alive))
    st["mt"].fill_(int(maker))
    st["tm"].copy_(torch.tensor([g.total_num_moves for g in games], dtype=torch.int32))
    st["rm"].fill_(-1)
    st["rb"].fill_(-1)
    st["sizes"] = np.array([[g.num_vertices(), 2 * g.num_edges()] for g in games], dtype=np.int64)
    st["onturn"] = "m" if maker else "b"
    mgr._restore_state_tensors(st)
    return games


@pytest.mark.parametrize("maker", [True, False], ids=["maker", "breaker"])
@pytest.mark.parametrize("size", [5, 7, 11, 13, 14, 16])     # W = 1, 1, 2, 3, 4 and the generic instantiation
def test_ply_kernel_equals_select_and_step_on_a_twin(hexref, size, maker):
    from gnn_hex_amd import _lib, ops
    from gnn_hex_amd.multi_env_manager import Env_manager
    L = _lib.lib()
    k = 64
    a, b = Env_manager(k, size), Env_manager(k, size)
    a.record_snapshots = b.record_snapshots = False
    _import_positions(hexref, a, size, k, maker)
    game = torch.tensor([[-1, 0, 0, 0]], dtype=torch.int32, device="cuda").repeat(k, 1)
    forced = torch.full((k,), -1, dtype=torch.int32, device="cuda")
    log = torch.zeros(k, dtype=torch.int32, device="cuda")
    res_a = torch.zeros((k, 5), dtype=torch.int32, device="cuda")
    res_b = torch.zeros((k, 5), dtype=torch.int32, device="cuda")
    live = torch.full((1,), 77, dtype=torch.int32, device="cuda")
    gen = torch.Generator(device="cuda").manual_seed(size)
    side = maker
    finished = rested = 0
    for ply in range(30):
        st = a._state_tensors()
        b._restore_state_tensors(st)                            # the twin starts every ply from the arena handle's state
        obs_a, obs_b = a.observe(), b.observe()
        assert torch.equal(obs_a.backmap, obs_b.backmap)
        q = torch.rand(obs_a.x.shape[0], device="cuda", generator=gen) * 10 - 5
        vert, rank, _ = b.select_actions(q, obs_b)
        before = a._state()
        rec0 = game.cpu().numpy()
        was_live = (rec0[:, 0] < 0) & (rec0[:, 3] == 0)
        acts = vert.clone()
        bad_game = 10
        if ply == 0:                                           # forced entries: ten legal ones and a dead vertex
            valid = a.get_valid_actions()
            f = np.full(k, -1, dtype=np.int32)
            for g in range(10):
                f[g] = int(valid[g][-1])
            dead = np.nonzero(before["alive"][bad_game] == 0)[0]
            f[bad_game] = int(dead[0]) if len(dead) else size * size + 2 + 5        # a removed vertex, else one off the board
            forced.copy_(torch.from_numpy(f))
            acts = torch.where(forced >= 0, forced, vert)
        gptr = torch.tensor(obs_a.node_off, dtype=torch.int32, device="cuda")
        _lib.check(L.hexgnn_arena_ply(a._h, gptr.data_ptr(), q.data_ptr(), obs_a.backmap.data_ptr(), GREEDY, 1.0, None,
                                      forced.data_ptr(), int(not side), game.data_ptr(), log.data_ptr(), res_a.data_ptr(),
                                      live.data_ptr(), ops._stream()), "hexgnn_arena_ply")
        _lib.check(L.hexgnn_env_step(b._h, acts.data_ptr(), 1, 1, int(not side), res_b.data_ptr(), ops._stream()), "hexgnn_env_step")
        sa, sb = a._state(), b._state()
        ra, rb, rec, lg = res_a.cpu().numpy(), res_b.cpu().numpy(), game.cpu().numpy(), log.cpu().numpy()
        assert (forced.cpu().numpy() == -1).all(), "forced entries must be cleared once used"
        for g in range(k):
            if was_live[g]:
                for key in ("adj", "alive", "maker_turn", "total_moves", "resp_maker", "resp_breaker"):
                    assert np.array_equal(sa[key][g], sb[key][g]), (ply, g, key)
                assert ra[g].tolist() == rb[g].tolist(), (ply, g)
                assert lg[g] == int(acts[g])
                if ply == 0 and g == bad_game:
                    assert ra[g, 4] == 1 and rec[g].tolist() == [-1, 0, 0, 1]
                    for key in ("adj", "alive", "maker_turn", "total_moves"):
                        assert np.array_equal(sa[key][g], before[key][g]), key     # an illegal move leaves the env untouched
                    continue
                assert ra[g, 4] == 0 and rec[g, 2] == rec0[g, 2] + 1 and rec[g, 3] == 0
                if ra[g, 0] >= 0:
                    finished += 1
                    assert rec[g, 0] == ra[g, 0] and rec[g, 1] == ra[g, 1] and sa["total_moves"][g] == 0
                else:
                    assert rec[g, 0] == -1 and rec[g, 1] == 0
            else:                                               # a decided game rests: only the side flag flips
                rested += 1
                assert rec[g].tolist() == rec0[g].tolist() and lg[g] == -1
                for key in ("adj", "alive", "total_moves", "resp_maker", "resp_breaker"):
                    assert np.array_equal(sa[key][g], before[key][g]), (ply, g, key)
                assert sa["maker_turn"][g] == 1 - before["maker_turn"][g]
                assert ra[g].tolist() == [-1, 0, int(sa["alive"][g].sum()), int(obs_a.edge_off[g + 1] - obs_a.edge_off[g]), 0]
        undecided = int(((rec[:, 0] < 0) & (rec[:, 3] == 0)).sum())
        assert int(live.item()) == undecided
        a._sizes = ra[:, 2:4].astype(np.int64)                  # what hexgnn_env_offsets would hand to the next observation
        a.global_onturn = "b" if a.global_onturn == "m" else "m"
        side = not side
        if undecided == 0:
            break
    assert rested > 0
    if size <= 7:
        assert finished > 0, "no game finished: the finishing branch was not exercised"


# ---- whole matches against the oracles, teacher-forced -------------------------------------------------------------------

def _pair(layers, seed, norm=False):
    from helpers import make_pair, norm_model_hip, norm_model_ref, sharpen_
    if norm:
        ref = norm_model_ref("modern_two_headed", layers, 35, seed)
        return norm_model_hip("modern_two_headed", ref, layers, 35).eval(), ref
    hip, ref = make_pair(layers, 35, seed=seed)
    return sharpen_(hip).eval(), sharpen_(ref)


def _replay_leg(hexref, size, res, first, openings, refs64):
    """Replay one leg's move log on RefGame, game by game and ply by ply, with the float64 oracle of the mover judging every
    model-chosen move on the batch the device saw (finished games rest at the start position).  Returns (checked plies, plies
    whose float64 top-2 gap is below 2e-4, the gaps)."""
    k = len(res.winner)
    games = [hexref.RefGame(size) for _ in range(k)]
    done = [False] * k
    maker = first == "m"
    checked = tight = 0
    gaps = []
    for ply in range(res.plies):
        for g in games:
            g.maker_turn = maker
        movers = [g for g in range(k) if not done[g]]
        assert movers, "the log is longer than its longest game"
        if ply > 0:
            obs = [games[g].observe() if not done[g] else hexref.RefGame(size).observe() for g in range(k)]
            xs = []
            for g, (x, ei, bm) in enumerate(obs):
                x = x.copy()
                x[:, 2] = 1.0 if maker else 0.0
                xs.append(x)
            offs = np.concatenate([[0], np.cumsum([x.shape[0] for x in xs])])
            x64 = torch.from_numpy(np.concatenate(xs)).double()
            ei = torch.from_numpy(np.concatenate([o[1] + off for o, off in zip(obs, offs[:-1])], 1))
            batch = torch.from_numpy(np.repeat(np.arange(k), np.diff(offs)))
            with torch.no_grad():
                q64 = refs64[0 if maker else 1](x64, ei, batch, torch.from_numpy(offs), advantages_only=True).reshape(-1).numpy()
        for g in range(k):
            v = int(res.moves[g, ply])
            if done[g]:
                assert v == -1, "game %d: a move is logged after its end" % g
                continue
            assert v in games[g].get_actions().tolist(), "game %d ply %d: illegal move %d" % (g, ply, v)
            if ply == 0:
                assert v == openings[g]
            else:
                bm = obs[g][2]
                pick = int(np.nonzero(bm == v)[0][0])
                qa = q64[offs[g] + 2:offs[g + 1]]
                assert qa[pick - 2] >= qa.max() - 2e-4, \
                    "game %d ply %d: picked q64 %.6f, max %.6f" % (g, ply, qa[pick - 2], qa.max())
                checked += 1
                if len(qa) > 1:
                    top = np.sort(qa)[-2:]
                    gaps.append(top[1] - top[0])
                    tight += top[1] - top[0] < 2e-4
            games[g].make_move(v, remove_dead_and_captured=True)
            w = games[g].who_won()
            if w is not None:
                done[g] = True
                assert int(res.winner[g]) == (0 if w == "m" else 1), "game %d: winner" % g
                assert int(res.length[g]) == games[g].total_num_moves == ply + 1, "game %d: length" % g
        maker = not maker
    assert all(done), "a game's log ends before the game does"
    return checked, tight, gaps


def _match_against_oracle(hexref, size, per_leg, layers, norm=False):
    from gnn_hex_amd.arena import DeviceArena, Elo_handler
    (hip_a, ref_a), (hip_b, ref_b) = _pair(layers, 21, norm), _pair(layers, 22, norm)
    refs64 = (copy.deepcopy(ref_a).double(), copy.deepcopy(ref_b).double())
    random.seed(size)
    openings = Elo_handler(size)._match_plan(2 * per_leg, False)[1]
    arena = DeviceArena(size, per_leg)
    checked = tight = 0
    gaps, wins = [], 0
    for leg, first in enumerate(("m", "b")):
        res = arena.play(hip_a, hip_b, first=first, openings=openings[leg], temperature=0.0)
        assert set(res.winner.tolist()) <= {0, 1} and res.moves.shape == (per_leg, res.plies)
        wins += res.maker_wins + res.breaker_wins
        c, t, gp = _replay_leg(hexref, size, res, first, openings[leg], refs64)
        checked, tight, gaps = checked + c, tight + t, gaps + gp
    assert wins == 2 * per_leg
    print("Hex-%d%s: %d model-chosen plies checked, %d with a float64 top-2 gap below 2e-4 (%.1f %%), median gap %.3g"
          % (size, " norm" if norm else "", checked, tight, 100.0 * tight / checked, float(np.median(gaps))))
    assert tight <= 0.15 * checked, "too many near-ties: the 2e-4 tolerance would decide the test"


@pytest.mark.parametrize("size,per_leg", [(5, 15), (7, 28)])
def test_matches_replayed_on_the_oracles(hexref, size, per_leg):
    _match_against_oracle(hexref, size, per_leg, layers=10)


def test_match_on_hex13_layer_major(hexref):
    _match_against_oracle(hexref, 13, 4, layers=3)


def test_match_with_a_norm_model(hexref):
    _match_against_oracle(hexref, 5, 15, layers=4, norm=True)


# ---- properties of the loop ------------------------------------------------------------------------------------------------

def _same(a, b):
    return (np.array_equal(a.winner, b.winner) and np.array_equal(a.length, b.length) and a.plies == b.plies
            and np.array_equal(a.moves, b.moves))


@pytest.fixture(scope="module")
def models():
    return _pair(10, 31)[0], _pair(10, 32)[0]


def test_graph_equals_eager_and_chunks_agree(models):
    from gnn_hex_amd.arena import DeviceArena
    ma, mb = models
    k = 12
    openings = [2 + 2 * i for i in range(k)]
    arenas = dict(graph8=DeviceArena(5, k, graph=True, chunk=8), eager8=DeviceArena(5, k, graph=False, chunk=8),
                  graph2=DeviceArena(5, k, graph=True, chunk=2))
    for temperature in (0.0, 0.5):
        for first in ("m", "b"):
            results = {}
            for name, arena in arenas.items():
                gen = torch.Generator(device="cuda").manual_seed(5)
                results[name] = arena.play(ma, mb, first=first, openings=openings, temperature=temperature, generator=gen)
            ref = results["eager8"]
            assert set(ref.winner.tolist()) <= {0, 1} and (ref.length >= 1).all()           # every game ends
            assert (ref.moves[:, 0] == openings).all()
            for name in ("graph8", "graph2"):
                assert _same(results[name], ref), (name, temperature, first)
            # a second play replays the cached graph
            if temperature == 0.0:
                assert _same(arenas["graph8"].play(ma, mb, first=first, openings=openings), ref)
                assert len(arenas["graph8"]._graphs) == (1 if first == "m" else 2)
    # another seed, other draws (results: temperature 0.5, first "b", seed 5)
    other = arenas["graph8"].play(ma, mb, first="b", openings=openings, temperature=0.5,
                                  generator=torch.Generator(device="cuda").manual_seed(6))
    assert not np.array_equal(other.moves, results["graph8"].moves)


def test_random_player_needs_no_forward(models):
    from gnn_hex_amd.arena import DeviceArena
    ma, _ = models
    calls = [0]
    inner = ma.forward

    def counting(*args, **kw):
        calls[0] += 1
        return inner(*args, **kw)

    ma.forward = counting
    try:
        arena = DeviceArena(5, 10, graph=False, chunk=2)
        gen = torch.Generator(device="cuda").manual_seed(1)
        res = arena.play("random", ma, first="m", generator=gen)
        executed = -(-res.plies // 2) * 2
        assert calls[0] == executed // 2, "the model moves at every second ply only"
        calls[0] = 0
        res2 = arena.play("random", "random", first="b", generator=gen)
        assert calls[0] == 0
    finally:
        del ma.forward
    for r in (res, res2):
        assert set(r.winner.tolist()) <= {0, 1} and r.maker_wins + r.breaker_wins == 10
    # the random player's moves are legal and its games differ from each other
    assert len({tuple(m) for m in res2.moves.tolist()}) > 1


def test_bad_arguments_and_cached_norm_refusal(models):
    from argparse import Namespace
    from gnn_hex_amd.arena import DeviceArena
    from gnn_hex_amd.models import get_pre_defined
    ma, mb = models
    with pytest.raises(ValueError):
        DeviceArena(5, 4, chunk=3)
    arena = DeviceArena(5, 4, graph=False)
    with pytest.raises(ValueError):
        arena.play(ma, mb, first="x")
    with pytest.raises(ValueError):
        arena.play(ma, mb, openings=[2, 3])
    with pytest.raises(ValueError, match="vertex id"):
        arena.play(ma, mb, openings=[2, 0, 3, 4])                    # vertex 0 is a terminal
    with pytest.raises(ValueError, match="illegal move 100 in game 1 at ply 0"):
        arena.play(ma, mb, openings=[2, 100, 3, 4])                  # not on the board: the device reports it
    args = Namespace(num_layers=3, hidden_channels=16, norm=True, noisy_dqn=False, noisy_sigma0=0.5, num_head_layers=2)
    cached = get_pre_defined("two_headed", args).cuda()
    with pytest.raises(NotImplementedError, match="CachedGraphNorm"):
        arena.play(cached, mb)


def test_elo_handler_plays_its_two_arena_legs(models):
    from gnn_hex_amd.arena import DeviceArena, Elo_handler
    ma, mb = models
    e = Elo_handler(5)
    e.add_player("a", model=ma, set_rating=1000, uses_empty_model=False)
    e.add_player("b", model=mb, set_rating=1000, uses_empty_model=False)
    e.add_player("rnd", model="random", simple=True, set_rating=0, rating_fixed=True, uses_empty_model=False)
    for asked in (None, 12):
        random.seed(9)
        stats = e.play_some_games("a", "b", asked, 0)
        random.seed(9)
        per_leg, openings = e._match_plan(asked, False)
        assert per_leg == (15 if asked is None else 6)
        arena = DeviceArena(5, per_leg)
        legs = [arena.play(ma, mb, first=f, openings=o) for f, o in zip(("m", "b"), openings)]
        assert stats == {"a": sum(r.maker_wins for r in legs), "b": sum(r.breaker_wins for r in legs)}
        assert stats["a"] + stats["b"] == 2 * per_leg
    stats = e.play_some_games("a", "rnd", 8, 0, random_first_move=True)
    assert stats["a"] + stats["rnd"] == 8
    e.score_some_statistics([stats])
    assert e.get_rating("rnd") == 0 and e.get_rating("a") != 1000


def test_select_actions_without_temperature_is_unchanged():
    """Env_manager.select_actions(q) keeps its tensors bit for bit; with a temperature it is hexgnn_sample_actions."""
    from gnn_hex_amd import _lib, ops
    from gnn_hex_amd.multi_env_manager import Env_manager
    mgr = Env_manager(20, 7)
    obs = mgr.reset()
    rng = np.random.default_rng(2)
    for _ in range(5):
        obs, *_ = mgr.step([int(v[rng.integers(len(v))]) for v in mgr.get_valid_actions()])
    q = torch.randn(obs.x.shape[0], device="cuda", generator=torch.Generator(device="cuda").manual_seed(0))
    gptr = torch.tensor(obs.node_off, dtype=torch.int32, device="cuda")
    L = _lib.lib()
    for eps in (0.0, 0.4):
        vert, rank, expl = mgr.select_actions(q, obs, eps=eps, generator=torch.Generator(device="cuda").manual_seed(3))
        u = torch.rand((20, 2), dtype=torch.float32, device="cuda", generator=torch.Generator(device="cuda").manual_seed(3))
        wv = torch.empty(20, dtype=torch.int32, device="cuda")
        wr = torch.empty(20, dtype=torch.int32, device="cuda")
        we = torch.empty(20, dtype=torch.uint8, device="cuda")
        _lib.check(L.hexgnn_select_actions(20, gptr.data_ptr(), q.data_ptr(), obs.backmap.data_ptr(), eps,
                                           u.data_ptr() if eps > 0 else None, wv.data_ptr(), wr.data_ptr(), we.data_ptr(),
                                           ops._stream()))
        assert torch.equal(vert, wv) and torch.equal(rank, wr) and torch.equal(expl, we.bool())
        assert vert.dtype == torch.int32 and expl.dtype == torch.bool
    greedy = mgr.select_actions(q, obs)
    cold = mgr.select_actions(q, obs, temperature=0.0)
    assert torch.equal(cold[0], greedy[0]) and torch.equal(cold[1], greedy[1]) and not cold[2].any()
    warm = mgr.select_actions(q, obs, temperature=2.0, generator=torch.Generator(device="cuda").manual_seed(4))
    u = torch.rand(20, dtype=torch.float32, device="cuda", generator=torch.Generator(device="cuda").manual_seed(4))
    wv = torch.empty(20, dtype=torch.int32, device="cuda")
    wr = torch.empty(20, dtype=torch.int32, device="cuda")
    _lib.check(L.hexgnn_sample_actions(20, gptr.data_ptr(), q.data_ptr(), obs.backmap.data_ptr(), SOFTMAX, 2.0, u.data_ptr(),
                                       wv.data_ptr(), wr.data_ptr(), None, ops._stream()))
    assert torch.equal(warm[0], wv) and torch.equal(warm[1], wr) and int(mgr.sample_status.item()) == 0
    assert not torch.equal(warm[1], greedy[1])
    with pytest.raises(ValueError):
        mgr.select_actions(q, obs, eps=0.1, temperature=1.0)
    mgr.step(warm[0])                                             # sampled moves are legal
