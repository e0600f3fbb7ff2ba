"""GPU: tree reuse between plies (search_advance_kernel of search.hip, ``TreeSearch.advance``, ``SearchPlayer(reuse_tree=True)``,
``SearchSelfPlay(reuse_tree=True)``) against the host restatements of tests/search_reuse_oracle.py, on the rigs of
tests/test_gpu_search.py and tests/test_gpu_search_round.py.
(1) the kernel against the numpy compaction: every live word, the counters and ``carried`` bit for bit (P and W as raw bits), with
    all five cases of the rule in one launch, on one, two and four lane trips of edges, on a tree of more than 64 kept nodes, with
    ``remap`` full of garbage, and a second advance straight behind the first;
(2) continuation: search, advance, play the move in the root env, search on -- the advanced oracle tree follows the device's
    trace teacher-forced with the tolerances of the existing tests and ends with the same tree; one leaf and rounds, three plies;
(3) root noise on carried trees: every game once, the expanded roots before the first simulation;
(4) the players: the arena with a reusing search player, search self-play with reuse, against oracle trees advanced by the
    logged moves;
(5) the entry point's and ``TreeSearch.advance``'s argument checks on real buffers."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

import search_oracle as so
import search_reuse_oracle as reuse
import selfplay_oracle as spo
import test_gpu_search as tgs
import test_gpu_search_round as tgr
from test_search_deep_host import peaked, start_positions

pytestmark = pytest.mark.gpu

DEV = "cuda"
GUARD = 4096
POISON = tgr.POISON


# ---- plumbing ----------------------------------------------------------------------------------------------------------------
def _garbage_remap(sr, seed):
    """``remap`` and ``carried`` of the search replaced by guarded tensors; remap full of garbage of both signs, small
    non-negative values (which a missing initialisation would take for marks) included."""
    G, Cn = sr.num_games, sr.max_sims + 1
    big = torch.full((G * Cn + GUARD,), POISON, dtype=torch.int32, device=DEV)
    gen = torch.Generator(device="cpu").manual_seed(seed)
    junk = torch.randint(-3, 4, (G * Cn,), generator=gen, dtype=torch.int32)
    junk[::7] = 0x7fffffff
    big[:G * Cn] = junk.to(DEV)
    sr._remap = big[:G * Cn].view(G, Cn)
    car = torch.full((G + GUARD,), POISON, dtype=torch.int32, device=DEV)
    sr._carried = car[:G]
    return big, car


def _advance_and_compare(rig, moves, max_carry, seed=1):
    """One ``advance`` of the rig's search against ``compact`` on the tree it had; the rig's oracle trees advance too (their
    root positions stay: nothing is searched afterwards) and must equal the device's as the existing tests compare them."""
    sr, G = rig.search, rig.G
    big, car = _garbage_remap(sr, seed)
    before = sr.tree()
    status = int(sr._status.item())
    got = sr.advance(torch.tensor(moves, dtype=torch.int32, device=DEV), max_carry)
    assert got.data_ptr() == sr._carried.data_ptr()
    carried = got.cpu().numpy()
    after = sr.tree()
    want, want_carried, kept = reuse.compact(before, moves, max_carry)
    assert carried.tolist() == want_carried.tolist(), "carried %s, the compaction says %s" % (carried, want_carried)
    reuse.assert_same_live_words(after, want, before=before)
    assert after["cnt"][:, 0].tolist() == kept.tolist()
    for g in range(G):
        if carried[g] == 0:                              # a fresh tree is what hexgnn_search_reset makes: all C slots
            assert (after["ns"][g] == 0).all() and (after["ne"][g] == 0).all() and tuple(after["cnt"][g]) == (1, 0)
    assert (big[G * (sr.max_sims + 1):] == POISON).all(), "the guard behind remap was written"
    assert (car[G:] == POISON).all(), "the guard behind carried was written"
    assert (rig.big[sr.workspace_bytes:] == 0xA5).all(), "the guard behind the workspace was written"
    assert int(sr._status.item()) == status, "advance touched the status word"
    for g, (tree, mv) in enumerate(zip(rig.trees, moves)):
        assert reuse.advance(tree, mv, max_carry=max_carry, play=False) == carried[g], "game %d" % g
    rig.compare_trees()
    return carried, kept


def _best_moves(rig):
    return [tree.best() for tree in rig.trees]


# ---- (1) the kernel against the numpy compaction -------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [5, 9, 14])
def test_all_cases_of_the_rule_in_one_launch(hexref, size):
    """G = 5, 40 simulations of the synthetic evaluator (game 0 rests after 12, so that its subtree fits under a max_carry
    that game 4's exceeds): game 0 the most visited root move, game 1 a root move without a child, game 2 no move, game 3 a
    vertex that is no root edge, game 4 a subtree one above max_carry.  Then a second advance straight behind the first."""
    G, sims = 5, 40
    rig = tgs.Rig(hexref, size, G, sims)
    for s in range(sims):
        rig.sim(s, tgs._synthetic(size), active=[int(s < 12), 1, 1, 1, 1], check_env=False)
    roots = [t.nodes[0] for t in rig.trees]
    best = [so.first_max(r.N) for r in roots]
    ns = [rig.trees[g].nodes[int(roots[g].child[best[g]])].Ns if roots[g].child[best[g]] >= 0 else 0 for g in range(G)]
    max_carry = ns[4] - 2
    assert ns[4] >= 3 and 1 <= ns[0] - 1 <= max_carry, "the set-up: Ns of the best children %s" % ns
    absent = [v for v in range(2, size * size + 2) if v not in roots[3].moves]
    moves = [int(roots[0].moves[best[0]]), int(roots[1].moves[np.nonzero(roots[1].child < 0)[0][0]]), -1,
             absent[0] if absent else 1, int(roots[4].moves[best[4]])]
    carried, kept = _advance_and_compare(rig, moves, max_carry, seed=size)
    assert carried.tolist() == [ns[0], 0, 0, 0, 0] and kept[0] >= 2
    # the opponent's reply straight behind the own move: game 0 goes on, the fresh ones stay fresh whatever they are told
    root = rig.trees[0].nodes[0]
    reply = int(root.moves[so.first_max(root.N)])
    carried2, _ = _advance_and_compare(rig, [reply, moves[1], 7, -1, moves[4]], sims, seed=size + 100)
    assert carried2[1:].tolist() == [0, 0, 0, 0]
    rig.finish()


def test_a_tree_of_more_than_64_kept_nodes(hexref):
    """Hex-14 start positions, 150 simulations of the peaked evaluator: one long line, so along it nearly the whole tree is kept
    and every node moves down by one slot (game 0, and game 2 for a second trip), off it nothing is (game 1: the old slots are
    cleared).  Then once more along the line."""
    size, G, sims = 14, 3, 150
    rig = tgs.Rig(hexref, size, G, sims, games=start_positions(hexref, size, G))
    for s in range(sims):
        rig.sim(s, peaked(size), check_env=False)
    used = rig.search.tree()["cnt"][:, 0].copy()
    roots = [t.nodes[0] for t in rig.trees]
    line = _best_moves(rig)
    off = int(roots[1].moves[np.nonzero(roots[1].moves != line[1])[0][3]])
    carried, kept = _advance_and_compare(rig, [line[0], off, line[2]], sims, seed=14)
    print("Hex-14 peaked: slots in use %s, kept %s, carried %s" % (used, kept, carried))
    assert kept[0] > 64 and kept[2] > 64 and kept[1] < 3 and carried[0] > 64 and carried[1] <= 1
    assert kept[0] >= used[0] - 8, "along the line nearly everything is kept"
    t = rig.search.tree()
    assert (t["ns"][1, 1:used[1]] == 0).all() and (t["ne"][1, 1:used[1]] == 0).all()
    line = _best_moves(rig)
    carried2, kept2 = _advance_and_compare(rig, [line[0], -1, line[2]], sims, seed=15)
    print("Hex-14 peaked, second advance: kept %s, carried %s" % (kept2, carried2))
    assert kept2[0] > 64 and kept2[2] > 64 and carried2[1] == 0
    rig.finish()


# ---- (2) continuation ----------------------------------------------------------------------------------------------------------
def _openings(hexref, size, G):
    """The start position with one maker stone on a different cell per game: breaker to move everywhere."""
    out = []
    for g in range(G):
        game = hexref.RefGame(size)
        game.maker_turn = True
        game.make_move(2 + (7 * g + 3) % (size * size), True)
        out.append(game)
    return out


def _play_in_root_env(rig, moves):
    """The env's own step on the root env; the rig's positions follow the oracle trees', which ``advance`` moved on."""
    rig.mgr.step(torch.tensor(moves, dtype=torch.int32, device=DEV))
    rig.games = [t.root_game for t in rig.trees]
    got = tgs._export(rig.mgr._h, rig.G, rig.nv, rig.W)
    for g, game in enumerate(rig.games):
        assert game.who_won() is None, "game %d is decided: the set-up is meant to stay clear of that" % g
        tgs._same_env(got, g, game, "game %d after its move" % g)
    rig.root_before = got


def _policy_value():
    from gnn_hex_amd.search import PolicyValueEvaluator
    from gnn_hex_amd.torch_script_models import SAGE_torch_script
    torch.manual_seed(5)
    return PolicyValueEvaluator(SAGE_torch_script(32, 3, 2, 2).to(DEV).eval())


@pytest.mark.parametrize("K", [1, 4])
@pytest.mark.parametrize("how", ["synthetic", "traced"])
def test_the_search_goes_on_from_the_carried_tree(hexref, K, how):
    """Four searches of 24 simulations with three plies between them: the oracle follows every descent teacher-forced, then both
    trees advance by the most visited move and the root env plays it with its own step.  ``synthetic``: the kernel-level loop
    of the rigs with the synthetic evaluator, whose peaked priors carry subtrees of 4 .. 19 simulations (the oracle alone says
    so on the CPU), the leaf env compared with the replay of every path FROM THE NEW ROOT; ``traced``: ``TreeSearch.simulate``
    with a policy / value network, replayed from its trace (its flat priors carry little more than a leaf).  The device tree
    equals the oracle's after every search and every advance; no descent is SKIPPED, status stays 0, and the in-flight counts of
    the round workspace are zero after every advance."""
    # (Hex-7: two maker stones cannot yet decide the game, captured cells included, so no game ends within the three plies)
    size, G, sims, cap = 7, 4, 24, 120
    games = _openings(hexref, size, G)
    rig = tgs.Rig(hexref, size, G, cap, games=games) if K == 1 else tgr.RoundRig(hexref, size, G, K, cap, vl=2, games=games)
    rig.mgr.global_onturn = "b"
    sr = rig.search
    ev = _policy_value() if how == "traced" else None
    total = np.zeros(G, dtype=np.int64)
    for ply in range(4):
        if how == "traced":
            trace = []
            sr.simulate(rig.mgr._h, ev, sims, trace=trace)
            assert all((r["leaf"][:, :r.get("round_leaves"), 0] != so.SKIPPED).all() if K > 1 else (r["leaf"][:, 0] != so.SKIPPED).all()
                       for r in trace)
            (tgs._replay_trace if K == 1 else tgr._replay_rounds)(rig, trace)
        elif K == 1:
            for s in range(sims):
                rig.sim(ply * sims + s, tgs._synthetic(size), check_env=(s % 4 == 0))
                assert (sr.leaf[:, 0] != so.SKIPPED).all()
        else:
            for r, n in enumerate(tgr._rounds(sims, K)):
                rig.round(ply * sims + r, tgs._synthetic(size), round_leaves=n, check_env=(r % 2 == 0))
                assert (sr.leaf[:, :n, 0] != so.SKIPPED).all()
        rig.compare_trees()
        rig.compare_root()
        if ply == 3:
            break
        moves = _best_moves(rig)
        carried = sr.advance(torch.tensor(moves, dtype=torch.int32, device=DEV), cap - sims).cpu().numpy()
        want = [reuse.advance(t, mv, max_carry=cap - sims) for t, mv in zip(rig.trees, moves)]
        # (the most visited move has a child, and an expanded leaf has Ns = 1: something is always carried)
        assert carried.tolist() == want and (carried >= 1).all(), "carried %s, oracle %s" % (carried, want)
        total += carried
        rig.compare_trees()
        if K > 1:
            assert (sr.tree()["inflight"] == 0).all(), "ply %d: in-flight counts after the advance" % ply
        _play_in_root_env(rig, moves)
    applied = sr.applied().cpu().numpy()
    assert np.array_equal(applied, [t.applied for t in rig.trees]) and (applied >= sims).all() and (applied <= cap).all()
    print("K=%d %s: carried over three plies %s, applied at the end %s" % (K, how, total, applied))
    if how == "synthetic":
        assert (total >= 3 * 4).all() and (applied > sims).all(), "the synthetic evaluator carries at least 4 simulations a ply"
    out = rig.finish()
    assert out[0] > G * sims * 3
    sr.status()


# ---- (3) root noise on carried trees -------------------------------------------------------------------------------------------
def test_root_noise_reaches_every_root_once(hexref):
    """After an advance game 0 and 1 have an expanded root, game 2 and 3 a fresh one; game 1 and 3 rest.  simulate(root_noise=)
    noises game 0's carried priors (before the first simulation: the root's P is the carried P under the noise, whatever the
    simulations do) and game 2's new ones (behind it), from one draw, and leaves the resting games alone."""
    from gnn_hex_amd.search import UniformEvaluator
    size, G, A, eps, alpha = 5, 4, 25, 0.25, 0.3
    rig = tgs.Rig(hexref, size, G, 64, games=_openings(hexref, size, G))
    rig.mgr.global_onturn = "b"
    sr, ev = rig.search, UniformEvaluator()
    sr.simulate(rig.mgr._h, ev, 16)
    t0 = sr.tree()
    best = sr.root(rig.mgr.observe(), boards=True)[3].cpu().numpy()
    moves = [int(best[0]), int(best[1]), -1, -1]
    carried = sr.advance(torch.tensor(moves, dtype=torch.int32, device=DEV)).cpu().numpy()
    assert (carried[:2] >= 1).all() and (carried[2:] == 0).all()
    rig.mgr.step(torch.tensor([int(best[0]), int(best[1]), int(best[2]), int(best[3])], dtype=torch.int32, device=DEV))
    t1 = sr.tree()
    active = torch.tensor([1, 0, 1, 0], dtype=torch.int32, device=DEV)
    gen = torch.Generator(device=DEV).manual_seed(11)
    sr.simulate(rig.mgr._h, ev, 3, active=active, root_noise=(eps, alpha), generator=gen)
    gen = torch.Generator(device=DEV).manual_seed(11)
    noise = torch._standard_gamma(torch.full((G, A), alpha, dtype=torch.float32, device=DEV), generator=gen).cpu().numpy()
    t2 = sr.tree()
    ne = t2["ne"][:, 0]
    assert t2["cnt"][:, 1].tolist() == [carried[0] - 1 + 3, carried[1] - 1, 3, 0]
    want0 = spo.root_noise64(t1["P"][0, 0, :ne[0]], noise[0, :ne[0]], eps)
    assert float((np.abs(t2["P"][0, 0, :ne[0]].astype(np.float64) - want0) / want0).max()) <= 1e-6
    want2 = spo.root_noise64(np.full(ne[2], 1.0 / ne[2]), noise[2, :ne[2]], eps)
    assert float((np.abs(t2["P"][2, 0, :ne[2]].astype(np.float64) - want2) / want2).max()) <= 1e-6
    assert t2["P"][1, 0, :ne[1]].tobytes() == t1["P"][1, 0, :ne[1]].tobytes() and t2["ns"][3, 0] == 0
    # fresh trees (after reset) take today's single call: the same bits as add_root_noise behind the first simulation
    sr.reset()
    gen = torch.Generator(device=DEV).manual_seed(12)
    sr.simulate(rig.mgr._h, ev, 2, active=active, root_noise=(eps, alpha), generator=gen)
    a = sr.tree()
    sr.reset()
    sr.simulate(rig.mgr._h, ev, 1, active=active)
    gen = torch.Generator(device=DEV).manual_seed(12)
    sr.add_root_noise(eps, alpha, active=active, generator=gen)
    sr.simulate(rig.mgr._h, ev, 1, active=active)
    b = sr.tree()
    for name in ("ns", "ne", "cnt", "P", "W", "N", "child"):
        assert a[name].tobytes() == b[name].tobytes(), name
    assert t0["cnt"][:, 1].tolist() == [16] * G
    sr.status()


# ---- (4) the players -----------------------------------------------------------------------------------------------------------
class Tracing:
    """An evaluator that keeps what ``TreeSearch.simulate(trace=)`` would: host copies of every simulation's record."""

    def __init__(self, inner):
        self.inner, self.trace = inner, []

    def evaluate(self, search):
        logits, offsets, skip, value = self.inner.evaluate(search)
        self.trace.append(dict(path=search.path.cpu().numpy(), leaf=search.leaf.cpu().numpy(), logits=logits.cpu().numpy(),
                               offsets=offsets.cpu().numpy(), skip=skip, value=value.cpu().numpy() if value is not None else None))
        return logits, offsets, skip, value


def _evaluator(which):
    from gnn_hex_amd.search import UniformEvaluator
    return Tracing(UniformEvaluator() if which == "uniform" else _policy_value())


def _replay(trees, trace):
    tgs._replay_trace(types.SimpleNamespace(trees=trees), trace)


@pytest.mark.parametrize("which", ["uniform", "policy_value"])
def test_the_arena_plays_a_reusing_search_player(hexref, which):
    """Hex-5, 4 games, 12 simulations: the player is told of every ply by the arena alone; the scores it returned on each of its
    plies are the root counts of oracle trees that were advanced by the logged moves (its own and the random opponent's) and
    followed its simulations teacher-forced; ``carried`` of every advance is the oracle's."""
    from gnn_hex_amd.arena import DeviceArena
    from gnn_hex_amd.search import SearchPlayer
    size, G, sims = 5, 4, 12
    ev = _evaluator(which)
    plies, carried = [], []

    class Watched(SearchPlayer):
        def search_scores(self, env_handle, obs, active):
            start = len(ev.trace)
            scores = super().search_scores(env_handle, obs, active)
            plies.append(dict(trace=ev.trace[start:], scores=scores.cpu().numpy(), off=obs.node_off.cpu().numpy(),
                              active=active.cpu().numpy()))
            return scores

    player = Watched(ev, sims, reuse_tree=True)
    player.on_carried = lambda c: carried.append(c.cpu().numpy().copy())
    arena = DeviceArena(size, G, graph=False)
    gen = torch.Generator(device=DEV).manual_seed(3)
    res = arena.play(player, "random", first="m", generator=gen)
    player.status()
    assert player._search.max_sims == player.capacity == 4 * sims
    assert len(carried) == len(plies) * 2 == arena.chunk * -(-res.plies // arena.chunk), "one advance per ply, the opponent's too"
    trees = [so.Tree(hexref.RefGame(size), max_sims=player.capacity) for _ in range(G)]
    some, searched = 0, 0
    for t in range(res.plies):
        if t % 2 == 0:                                    # the player's ply
            rec = plies[t // 2]
            assert len(rec["trace"]) == sims
            alive = [int(t < res.length[g]) for g in range(G)]
            assert rec["active"].tolist() == alive
            _replay(trees, rec["trace"])
            for g in range(G):
                r0, r1 = rec["off"][g], rec["off"][g + 1]
                if not alive[g]:
                    assert trees[g].nodes == [None] and (rec["scores"][r0:r1] == 0).all()
                    continue
                moves, n = trees[g].root_counts()
                assert np.array_equal(rec["scores"][r0 + 2:r1], n.astype(np.float32)), "ply %d game %d" % (t, g)
                assert res.moves[g, t] == trees[g].best(), "ply %d game %d: the move played is the most visited" % (t, g)
                searched += 1
        want = [reuse.advance(trees[g], int(res.moves[g, t]), max_carry=player.capacity - sims) for g in range(G)]
        assert carried[t].tolist() == want, "ply %d: carried %s, oracle %s" % (t, carried[t], want)
        some += sum(c > 0 for c in want)
    assert some > 0 and searched >= G * 3
    print("%s: %d advances carried a subtree over %d plies; mean carried / sims per ply %.2f; %d of %d steps ambiguous" % (
        which, some, res.plies, np.mean([c.mean() for c in carried[:res.plies]]) / sims, sum(t.ambiguous for t in trees),
        sum(t.steps for t in trees)))
    for g in range(G):                                    # legal, complete games
        game = hexref.RefGame(size)
        for ply in range(int(res.length[g])):
            assert game.who_won() is None
            game.make_move(int(res.moves[g, ply]), True)
        assert game.who_won() == ("m" if res.winner[g] == 0 else "b")


@pytest.mark.parametrize("which", ["uniform", "policy_value"])
def test_selfplay_with_reuse_records_the_carried_visit_distributions(hexref, which):
    """A SearchSelfPlay(reuse_tree=True) match, greedy and without noise: pending == played (``play`` refuses anything else),
    and every sample's policy row is N / T of the oracle's carried tree, bit for bit."""
    from gnn_hex_amd.search_selfplay import SearchSampleBuffer, SearchSelfPlay
    size, G, sims, A = 5, 4, 12, 25
    ev = _evaluator(which)
    buf = SearchSampleBuffer(G * A, size, DEV)
    sp = SearchSelfPlay(size, G, ev, sims, buf, root_noise=None, proportional_plies=0, reuse_tree=True)
    carried = []
    sp.on_carried = lambda c: carried.append(c.cpu().numpy().copy())
    res, samples = sp.play("m")
    assert samples == int(res.length.sum()) == len(buf) and sp.search.max_sims == sp.capacity == 4 * sims
    assert len(ev.trace) == sims * res.plies == sims * len(carried)
    policy, meta = buf.policy[:samples].cpu().numpy(), buf.meta[:samples].cpu().numpy()
    slot_of = {(int(g), int(p)): i for i, (g, p) in enumerate(meta)}
    assert len(slot_of) == samples
    trees = [so.Tree(hexref.RefGame(size), max_sims=sp.capacity) for _ in range(G)]
    beyond = 0
    for t in range(res.plies):
        _replay(trees, ev.trace[t * sims:(t + 1) * sims])
        for g in range(G):
            if t >= res.length[g]:
                assert (g, t) not in slot_of and trees[g].nodes == [None]
                continue
            moves, n = trees[g].root_counts()
            beyond += n.sum() > sims - 1                  # a fresh tree's T is sims - 1: its first simulation expands the root
            want = spo.visit_policy(moves, n, A)
            assert policy[slot_of[(g, t)]].tobytes() == want.tobytes(), "game %d ply %d: the visit distribution" % (g, t)
            assert res.moves[g, t] == trees[g].best()
        want = [reuse.advance(trees[g], int(res.moves[g, t]), max_carry=sp.capacity - sims) for g in range(G)]
        assert carried[t].tolist() == want, "ply %d: carried %s, oracle %s" % (t, carried[t], want)
    assert beyond > 0, "no sample ever counted more visits than a fresh tree's: nothing was carried"
    print("%s self-play: mean carried / sims per ply %.2f" % (which, np.mean([c.mean() for c in carried]) / sims))


# ---- (5) argument checks -------------------------------------------------------------------------------------------------------
def test_advance_refusals_on_real_buffers(hexref):
    from gnn_hex_amd import _lib
    rig = tgs.Rig(hexref, 3, 2, 8)
    sr, L = rig.search, _lib.lib()
    for s in range(4):
        rig.sim(s, tgs._synthetic(3), check_env=False)
    before = rig.big.clone()
    moves = torch.tensor([2, 3], dtype=torch.int32, device=DEV)
    remap = torch.zeros((2, 9), dtype=torch.int32, device=DEV)
    carried = torch.full((2,), -9, dtype=torch.int32, device=DEV)

    def call(max_carry=8, **kw):
        c = _lib.SearchAdvanceCall(struct_bytes=C.sizeof(_lib.SearchAdvanceCall), call=sr._call(), moves=moves.data_ptr(),
                                   max_carry=max_carry, remap=remap.data_ptr(), carried=carried.data_ptr())
        for k, v in kw.items():
            setattr(c.call if k in ("workspace", "workspace_bytes", "status", "num_games", "hex_size", "max_sims") else c, k, v)
        return c

    for kw in (dict(struct_bytes=8), dict(workspace=None), dict(status=None), dict(workspace_bytes=sr.workspace_bytes - 1),
               dict(moves=None), dict(remap=None), dict(carried=None), dict(max_carry=-1), dict(max_carry=9), dict(max_sims=0)):
        assert L.hexgnn_search_advance(C.byref(call(**kw)), None) == -1, kw
    assert L.hexgnn_search_advance(C.byref(call(hex_size=26, moves=None)), None) == -2
    assert L.hexgnn_search_advance(C.byref(call(num_games=0, moves=None)), None) == 0
    torch.cuda.synchronize()
    assert torch.equal(rig.big, before) and (carried == -9).all(), "a refused call wrote something"
    for bad in (moves.to(torch.int64), moves[:1], torch.zeros(4, dtype=torch.int32, device=DEV)[::2], moves.cpu(), [2, 3]):
        with pytest.raises(ValueError, match="moves"):
            sr.advance(bad)
    for bad in (-1, 9, 2.5):
        with pytest.raises(ValueError, match="max_carry"):
            sr.advance(moves, bad)
    assert torch.equal(rig.big, before)
    rig.finish()
