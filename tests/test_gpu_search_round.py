"""GPU: search rounds of several leaves per game under virtual loss (search_round_descend_kernel of env.hip,
search_round_backup_kernel of search.hip, ``TreeSearch(leaves=, virtual_loss=)``) against the host oracle of
tests/search_round_oracle.py, teacher-forced as tests/test_gpu_search.py does it for the one-leaf search: the oracle follows the
K recorded paths of every game, is fed the same synthetic logits and values, checks every selection step against the float64
scores under the in-flight counts, and must end with the same tree -- N, Ns, W, children and slot counters bit for bit, P to 1e-6
-- while leaf-env game g * K + k must equal the RefGame replay of path (g, k) bit for bit.  Then K = 1 through the new entry
points against the one-leaf entry points, the limits, the one-leaf calls on a workspace of the new size, and the python level."""
import ctypes as C

import numpy as np
import pytest
import torch

import search_oracle as so
import search_round_oracle as ro
import selfplay_oracle as spo
import test_gpu_search as tgs

pytestmark = pytest.mark.gpu

DEV = "cuda"
GUARD = 4096
POISON = -1515870811            # 0xA5A5A5A5 as int32


def _guarded(t):
    """``t``'s storage replaced by the head of a poisoned tensor: ``(view, whole)``."""
    big = torch.full((t.numel() + GUARD,), POISON, dtype=torch.int32, device=DEV)
    big[:t.numel()] = 0
    return big[:t.numel()].view(t.shape), big


class RoundRig:
    """A root env with oracle positions, a TreeSearch(leaves=K) whose workspace, path, leaf record and result are each followed
    by a poisoned guard, and one oracle tree per game."""

    def __init__(self, hexref, size, G, K, max_sims, vl=1, c_puct=1.5, temperature=1.0, games=None):
        from gnn_hex_amd.multi_env_manager import Env_manager
        from gnn_hex_amd.search import TreeSearch
        self.size, self.G, self.K, self.nv = size, G, K, size * size + 2
        self.games = games if games is not None else tgs._roots(hexref, size, G)
        self.mgr = Env_manager(G, size)
        self.mgr.record_snapshots = False
        tgs._import(self.mgr, self.games)
        self.search = s = TreeSearch(size, G, max_sims, c_puct, temperature, leaves=K, virtual_loss=vl)
        assert s.num_leaves == G * K and tuple(s.path.shape) == (G, K, max_sims + 1) and tuple(s.result.shape) == (G * K, 5)
        self.big = torch.full((s.workspace_bytes + GUARD,), 0xA5, dtype=torch.uint8, device=DEV)
        s.workspace = self.big[:s.workspace_bytes]
        self.guards = {}
        for name in ("path", "leaf", "result"):
            view, whole = _guarded(getattr(s, name))
            setattr(s, name, view)
            self.guards[name] = whole
        s.reset()
        assert (s.tree()["inflight"] == 0).all(), "hexgnn_search_reset left the poisoned in-flight section as it was"
        self.trees = [ro.RoundTree(g, c_puct, temperature, max_sims, K, vl) for g in self.games]
        self.W = self.mgr._words
        self.root_before = tgs._export(self.mgr._h, G, self.nv, self.W)
        self.offsets = torch.arange(G * K + 1, dtype=torch.int32, device=DEV) * self.nv

    def round(self, r, evaluator, active=None, round_leaves=None, check_env=True):
        """One round through the kernel-level loop: descend, read the K paths back, teacher-force the oracle (which asks
        ``evaluator(g)`` for the synthetic logits / values), compare the leaf env, upload the same evaluations, back up."""
        sr, G, K, nv = self.search, self.G, self.K, self.nv
        act = torch.tensor(active, dtype=torch.int32, device=DEV) if active is not None else None
        sr.descend(self.mgr._h, act, round_leaves)
        path, rec, result = sr.path.cpu().numpy(), sr.leaf.cpu().numpy(), sr.result.cpu().numpy()
        leaf_env = tgs._export(sr.leaf_handle, G * K, nv, self.W) if check_env else None
        logits = np.zeros(G * K * nv, dtype=np.float32)
        value = np.zeros(G * K, dtype=np.float32)
        for g, tree in enumerate(self.trees):
            forced = [path[g, k, :max(int(rec[g, k, 2]), 0)] for k in range(K)]
            out = tree.round(evaluate=evaluator(g), forced=forced, kinds=rec[g, :, 0], round_leaves=round_leaves,
                             active=active is None or bool(active[g]))
            for k, d in enumerate(out):
                i = g * K + k
                what = "Hex-%d game %d round %d descent %d (%s)" % (self.size, g, r, k, ro.KIND_NAMES[d["kind"]])
                assert rec[g, k, 0] == d["kind"] and rec[g, k, 2] == len(d["path"]), what
                if d["kind"] == ro.TERMINAL:
                    assert rec[g, k, 3] == d["terminal"], "%s: terminal value %d, oracle %g" % (what, rec[g, k, 3], d["terminal"])
                if d["kind"] == ro.LEAF:
                    lg, v = d["eval"]
                    assert rec[g, k, 4] == len(lg), "%s: %d legal moves, oracle %d" % (what, rec[g, k, 4], len(lg))
                    logits[i * nv + 2:i * nv + 2 + len(lg)] = lg
                    value[i] = v
                    assert rec[g, k, 1] == int(d["game"].maker_turn), what
                if check_env:
                    leaf = d["game"]                  # the position reached for a LEAF, the root's for every other kind
                    tgs._same_env(leaf_env, i, leaf, what)
                    assert tuple(result[i]) == (-1, leaf.total_num_moves, leaf.num_vertices(), 2 * leaf.num_edges(), 0), what
        sr.backup(torch.from_numpy(logits).to(DEV), self.offsets, 2, torch.from_numpy(value).to(DEV))

    def compare_trees(self):
        tgs.Rig.compare_trees(self)

    def compare_root(self):
        tgs.Rig.compare_root(self)

    def finish(self, want_status=0):
        after = tgs._export(self.mgr._h, self.G, self.nv, self.W)
        for a, b in zip(self.root_before, after):
            assert np.array_equal(a, b), "the root env was written"
        assert (self.big[self.search.workspace_bytes:] == 0xA5).all(), "the guard behind the workspace was written"
        for name, whole in self.guards.items():
            assert (whole[getattr(self.search, name).numel():] == POISON).all(), "the guard behind %s was written" % name
        assert (self.search.tree()["inflight"] == 0).all(), "in-flight counts survive the backup"
        assert all(t.inflight_total() == 0 for t in self.trees)
        assert int(self.search._status.item()) == want_status
        steps = sum(t.steps for t in self.trees)
        ambiguous = sum(t.ambiguous for t in self.trees)
        kinds = sum(t.kinds for t in self.trees)
        print("Hex-%d G=%d K=%d: %d steps, %d ambiguous; kinds leaf/terminal/skipped/collision %s" % (self.size, self.G, self.K,
                                                                                                    steps, ambiguous, kinds))
        return steps, ambiguous, kinds


def _rounds(sims, K):
    left = sims
    while left > 0:
        yield min(K, left)
        left -= min(K, left)


# ---- 6: the tree and the leaf env against the round oracle ----------------------------------------------------------------
CASES = [(2, 3, 8, 40), (3, 1, 2, 40), (5, 70, 4, 40), (5, 3, 3, 2), (8, 3, 3, 40), (9, 3, 5, 40), (12, 3, 4, 40)]


@pytest.mark.parametrize("size,G,K,sims", CASES)
def test_rounds_follow_the_oracle(hexref, size, G, K, sims):
    rig = RoundRig(hexref, size, G, K, sims, vl=3 if size == 8 else 1)
    for r, n in enumerate(_rounds(sims, K)):
        # two of the cases: uniform logits from round 1 on, so every new node starts with exact ties
        rig.round(r, tgs._synthetic(size, uniform=(size in (9, 12) and r >= 1)), round_leaves=n, check_env=(G <= 3 or r % 4 == 0))
    rig.compare_trees()
    rig.compare_root()
    steps, ambiguous, kinds = rig.finish()
    assert ambiguous <= 0.01 * max(steps, 1)
    assert kinds.sum() == G * K * len(list(_rounds(sims, K)))
    applied = rig.search.applied().cpu().numpy()
    assert np.array_equal(applied, [t.applied for t in rig.trees])
    if sims == 2:                                     # round_leaves = 2 below K = 3: a LEAF, a COLLISION and a SKIPPED per game
        assert tuple(kinds) == (G, 0, G, G) and (applied == 1).all()
    else:
        assert kinds[ro.COLLISION] >= G * (K - 1) and kinds[ro.LEAF] >= G and steps >= G * K
    if size == 2:
        assert kinds[ro.TERMINAL] > 40, "Hex-2 trees stop growing: most descents end on a terminal"


# ---- 7: K = 1 through the new entry points is the one-leaf search, bit for bit ----------------------------------------------
@pytest.mark.parametrize("size,vl", [(5, 1), (5, 3), (9, 1), (9, 3)])
def test_one_leaf_round_calls_give_the_one_leaf_bits(hexref, size, vl):
    from gnn_hex_amd import _lib, ops
    from gnn_hex_amd.multi_env_manager import Env_manager
    from gnn_hex_amd.search import TreeSearch, tree_layout
    G, sims, nv = 3, 20, size * size + 2
    mgr = Env_manager(G, size)
    mgr.record_snapshots = False
    tgs._import(mgr, tgs._roots(hexref, size, G))
    L = _lib.lib()
    old, new = TreeSearch(size, G, sims), TreeSearch(size, G, sims)
    need = int(L.hexgnn_search_round_workspace_bytes(G, size, sims, 1))
    _, tree_bytes, old_bytes = tree_layout(G, size, sims)
    assert need > old_bytes == old.workspace_bytes
    big = torch.full((need + GUARD,), 0xA5, dtype=torch.uint8, device=DEV)
    big[:need] = 0                                    # as the one-leaf search's: slots no simulation reaches compare equal
    new.workspace, new.workspace_bytes = big[:need], need
    new.reset()

    def round_call(**kw):
        return _lib.SearchRoundCall(struct_bytes=C.sizeof(_lib.SearchRoundCall), call=new._call(**kw), leaves=1, round_leaves=1,
                                    virtual_loss=vl)

    rng = np.random.default_rng(size * 10 + vl)
    offsets = torch.arange(G + 1, dtype=torch.int32, device=DEV) * nv
    for s in range(sims):
        old.descend(mgr._h)
        _lib.check(L.hexgnn_search_round_descend(mgr._h, new.leaf_handle, C.byref(round_call()), ops._stream()), "round descend")
        for name in ("path", "leaf", "result"):
            assert torch.equal(getattr(old, name), getattr(new, name)), "simulation %d: %s" % (s, name)
        assert (new.leaf[:, 0] != ro.COLLISION).all()
        a, b = tgs._export(old.leaf_handle, G, nv, mgr._words), tgs._export(new.leaf_handle, G, nv, mgr._words)
        assert all(np.array_equal(x, y) for x, y in zip(a, b)), "simulation %d: the leaf envs differ" % s
        logits = torch.from_numpy((rng.integers(-512, 512, G * nv) / 128.0).astype(np.float32)).to(DEV)
        value = torch.from_numpy((rng.integers(-256, 256, G) / 256.0).astype(np.float32)).to(DEV)
        old.backup(logits, offsets, 2, value)
        call = round_call(skip=2, logits=logits.data_ptr(), offsets=offsets.data_ptr(), value=value.data_ptr())
        _lib.check(L.hexgnn_search_round_backup(C.byref(call), ops._stream()), "round backup")
        assert torch.equal(old.workspace[:tree_bytes], new.workspace[:tree_bytes]), "simulation %d: the trees differ" % s
    lay, _, _ = tree_layout(G, size, sims, 1)
    off, _, shape = lay["inflight"]
    assert (new.workspace[off:off + 4 * int(np.prod(shape))] == 0).all()
    assert (big[need:] == 0xA5).all() and int(old._status.item()) == int(new._status.item()) == 0
    assert int(new.applied().sum()) == G * sims


# ---- 8: limits ------------------------------------------------------------------------------------------------------------
def test_rounds_stop_at_max_sims(hexref):
    from gnn_hex_amd.search import tree_layout
    rig = RoundRig(hexref, 5, 3, 4, 10)
    sr = rig.search
    for r in range(3):
        rig.round(r, tgs._synthetic(5))
        assert (sr.applied().cpu().numpy() <= 10).all()
    assert int(sr._status.item()) == 0 and [t.applied for t in rig.trees] == [9, 9, 9]
    rig.round(3, tgs._synthetic(5))                   # one more fits; the rest of the round is SKIPPED with bit 1
    assert (sr.leaf.cpu().numpy()[:, 1:, 0] == so.SKIPPED).all() and (sr.applied().cpu().numpy() == 10).all()
    assert int(sr._status.item()) == 1
    _, tree_bytes, _ = tree_layout(3, 5, 10)
    before = rig.big[:sr.workspace_bytes].clone()
    rig.round(4, tgs._synthetic(5))                   # the oracle refuses a recording that is not SKIPPED
    assert (sr.leaf.cpu().numpy()[:, :, 0] == so.SKIPPED).all()
    assert torch.equal(rig.big[:tree_bytes], before[:tree_bytes]), "a round past max_sims changed the tree"
    rig.compare_trees()
    rig.finish(want_status=1)
    with pytest.raises(Exception, match="max_sims"):
        sr.status()


def test_a_resting_game_changes_no_word(hexref):
    rig = RoundRig(hexref, 5, 3, 4, 24)
    for r in range(2):
        rig.round(r, tgs._synthetic(3))
    before = rig.search.tree()
    for r in range(2, 5):
        rig.round(r, tgs._synthetic(3), active=[1, 0, 1])
    after = rig.search.tree()
    for name in before:
        assert before[name][1].tobytes() == after[name][1].tobytes(), "the resting game's %s changed" % name
    assert [t.applied for t in rig.trees] == [17, 5, 17]
    rig.compare_trees()
    rig.compare_root()
    rig.finish()


def test_a_non_finite_value_drops_one_simulation_of_the_round(hexref):
    rig = RoundRig(hexref, 5, 3, 4, 24)
    done = {}

    def spoiled(r):
        """The synthetic evaluator, but in round 2 the third leaf the oracle asks about for game 1 has an infinite value and
        in round 3 the second one of game 2 a NaN logit."""
        def per_game(g):
            clean = so.synthetic_evaluator(g, seed=9)
            asked = [0]

            def evaluate(game, moves):
                logits, value = clean(game, moves)
                asked[0] += 1
                if (g, r, asked[0]) == (1, 2, 3):
                    value = np.float32(np.inf)
                    done[1] = r
                if (g, r, asked[0]) == (2, 3, 2):
                    logits[len(logits) // 2] = np.nan
                    done[2] = r
                return logits, value
            return evaluate
        return per_game

    for r in range(5):
        rig.round(r, spoiled(r))
        assert int(rig.search._status.item()) == (2 if done else 0)
        assert (rig.search.tree()["inflight"] == 0).all(), "a dropped simulation keeps its in-flight counts"
    assert sorted(done) == [1, 2]
    assert [t.applied for t in rig.trees] == [17, 16, 16]            # its siblings are applied
    rig.compare_trees()
    rig.compare_root()
    rig.finish(want_status=2)


def test_too_few_logits_drop_one_simulation_of_the_round(hexref):
    rig = RoundRig(hexref, 5, 3, 4, 24)
    sr, G, K, nv = rig.search, 3, 4, rig.nv
    zeros = torch.zeros(G * K * nv + nv, dtype=torch.float32, device=DEV)
    value = torch.zeros(G * K, dtype=torch.float32, device=DEV)
    for r in range(2):
        sr.descend(rig.mgr._h)
        sr.backup(zeros, rig.offsets, 2, value)
    assert (sr.applied().cpu().numpy() == 5).all() and int(sr._status.item()) == 0
    sr.descend(rig.mgr._h)
    rec = sr.leaf.cpu().numpy()
    assert (rec[:, :, 0] == so.LEAF).all()
    off = rig.offsets.cpu().numpy().copy()
    i = 1 * K + 2                                     # leaf (1, 2): one logit fewer than it has legal moves
    off[i + 1] = off[i] + 2 + rec[1, 2, 4] - 1        # (the leaves behind it keep their rows: more than enough zeros)
    assert off[i + 2] - off[i + 1] - 2 >= nv - 2 and off[-1] <= zeros.numel()
    sr.backup(zeros, torch.from_numpy(off.astype(np.int32)).to(DEV), 2, value)
    assert sr.applied().cpu().numpy().tolist() == [9, 8, 9] and int(sr._status.item()) == 4
    t = sr.tree()
    assert (t["inflight"] == 0).all() and t["cnt"][:, 0].tolist() == [9, 8, 9]
    sr._status.zero_()
    rig.trees = []                                    # no oracle followed this
    rig.finish()


def test_round_refusals_on_real_handles(hexref):
    from gnn_hex_amd import _lib
    from gnn_hex_amd.multi_env_manager import Env_manager
    rig = RoundRig(hexref, 3, 2, 4, 8)
    sr, L = rig.search, _lib.lib()
    other_size, other_count, root_sized = Env_manager(8, 4), Env_manager(3, 3), Env_manager(2, 3)
    for root, leaf in ((other_size._h, sr.leaf_handle), (rig.mgr._h, other_size._h), (other_count._h, sr.leaf_handle),
                       (rig.mgr._h, root_sized._h), (rig.mgr._h, other_count._h)):        # a leaf handle of G, not G * K, games
        assert L.hexgnn_search_round_descend(root, leaf, C.byref(sr._round_call()), None) == -1
    for kw in (dict(c_puct=-1.0), dict(c_puct=float("nan")), dict(path=None), dict(leaf=None), dict(result=None)):
        call = sr._round_call()
        for k, v in kw.items():
            setattr(call.call, k, v)
        assert L.hexgnn_search_round_descend(rig.mgr._h, sr.leaf_handle, C.byref(call), None) == -1, kw
    for kw in (dict(leaves=0), dict(leaves=65), dict(leaves=2), dict(virtual_loss=0), dict(virtual_loss=1025), dict(round_leaves=-1),
               dict(round_leaves=5)):
        call = sr._round_call()
        for k, v in kw.items():
            setattr(call, k, v)
        assert L.hexgnn_search_round_descend(rig.mgr._h, sr.leaf_handle, C.byref(call), None) == -1, kw
    call = sr._round_call()
    call.call.workspace_bytes -= 1
    assert L.hexgnn_search_round_descend(rig.mgr._h, sr.leaf_handle, C.byref(call), None) == -1
    rig.finish()


# ---- 9: the one-leaf calls on a workspace of the new size -------------------------------------------------------------------
def test_one_leaf_calls_on_a_round_workspace(hexref):
    """hexgnn_search_descend / _backup / _root / _root_noise / _record on a workspace of hexgnn_search_round_workspace_bytes
    behave as on the one-leaf workspace: the one-leaf rig's checks against search_oracle and selfplay_oracle."""
    import test_gpu_search_selfplay as tss
    from gnn_hex_amd import _lib
    size, G, sims = 5, 3, 12
    rig = tgs.Rig(hexref, size, G, sims)
    sr = rig.search
    need = int(_lib.lib().hexgnn_search_round_workspace_bytes(G, size, sims, 4))
    assert need > sr.workspace_bytes
    rig.big = torch.full((need + GUARD,), 0xA5, dtype=torch.uint8, device=DEV)
    sr.workspace, sr.workspace_bytes = rig.big[:need], need
    sr.reset()
    for s in range(sims):
        rig.sim(s, tgs._synthetic(size))
    rig.compare_trees()
    rig.compare_root()
    # root noise against selfplay_oracle.root_noise64
    t0 = sr.tree()
    save = rig.big[:need].clone()
    noise = torch.rand((G, size * size), dtype=torch.float32, device=DEV) + 0.01
    sr.apply_root_noise(0.25, noise, None)
    t1, nz = sr.tree(), noise.cpu().numpy()
    for name in ("ns", "ne", "cnt", "W", "N", "child", "vertex"):
        assert np.array_equal(t0[name], t1[name]), name
    for g in range(G):
        ne = int(t0["ne"][g, 0])
        want = spo.root_noise64(t0["P"][g, 0, :ne], nz[g, :ne], 0.25)
        assert float((np.abs(t1["P"][g, 0, :ne].astype(np.float64) - want) / want).max()) <= 1e-6
    rig.big[:need].copy_(save)
    # record: one greedy call, against the device tree and the oracle's best move
    buf = tss.poisoned_buffer(G * size * size, size)
    pick = torch.full((G,), -5, dtype=torch.int32, device=DEV)
    tss.set_head(buf, 3)
    before = tss.ring(buf)
    buf.record(rig.mgr._h, sr, 0, 0, None, pick, None)
    assert tss.check_record(rig, buf, before, 3, 0, 0, np.zeros(G, np.float32), [1] * G, pick.cpu().numpy()) == G
    rig.finish()


# ---- 10: the python level ---------------------------------------------------------------------------------------------------
def _replay_rounds(rig, trace):
    """Teacher-force the round oracle with a TreeSearch.simulate trace: the device's own logits and values."""
    K = rig.K
    for r, rec in enumerate(trace):
        for g, tree in enumerate(rig.trees):
            kinds = rec["leaf"][g, :, 0]
            forced = [rec["path"][g, k, :max(int(rec["leaf"][g, k, 2]), 0)] for k in range(K)]
            evals = [None] * K
            for k in range(K):
                if kinds[k] == ro.LEAF:
                    i = g * K + k
                    a, b = int(rec["offsets"][i]) + rec["skip"], int(rec["offsets"][i + 1])
                    logits = rec["logits"][a:b]
                    value = rec["value"][i] if rec["value"] is not None else np.float32(min(max(logits.max(), -1.0), 1.0))
                    evals[k] = (logits, value)
            tree.round(forced=forced, kinds=kinds, evals=evals, round_leaves=rec["round_leaves"])


@pytest.mark.parametrize("which", ["uniform", "q", "policy_value"])
def test_simulate_with_leaves_replays_through_the_oracle(hexref, which):
    from gnn_hex_amd.search import PolicyValueEvaluator, QEvaluator, UniformEvaluator
    from gnn_hex_amd.torch_script_models import SAGE_torch_script
    if which == "uniform":
        ev = UniformEvaluator()
    elif which == "q":
        ev = QEvaluator(tgs._gnn_s(3))
    else:
        torch.manual_seed(5)
        ev = PolicyValueEvaluator(SAGE_torch_script(32, 3, 2, 2).to(DEV).eval())
    size, G, K, sims = 5, 8, 4, 18
    rig = RoundRig(hexref, size, G, K, sims)
    trace = []
    rig.search.simulate(rig.mgr._h, ev, sims, trace=trace)
    assert [r["round_leaves"] for r in trace] == [4, 4, 4, 4, 2]
    _replay_rounds(rig, trace)
    rig.compare_trees()
    rig.compare_root()
    steps, ambiguous, kinds = rig.finish()
    applied = rig.search.applied().cpu().numpy()
    assert np.array_equal(applied, [t.applied for t in rig.trees]) and (applied <= sims - (K - 1)).all() and (applied > K).all()
    assert steps > G * K and kinds[ro.SKIPPED] == 2 * G
    rig.search.status()


def test_arena_plays_a_search_player_with_leaves(hexref):
    from gnn_hex_amd.arena import DeviceArena
    from gnn_hex_amd.search import SearchPlayer, UniformEvaluator
    player = SearchPlayer(UniformEvaluator(), 16, leaves=4, virtual_loss=2)
    arena = DeviceArena(5, 6, graph=False)
    res = arena.play(player, "random", first="m")
    player.status()
    assert player._search.leaves == 4 and player._search.virtual_loss == 2 and player._search.num_leaves == 24
    assert set(res.winner.tolist()) <= {0, 1} and (res.length >= 5).all()
    for g in range(6):                          # the recorded moves are legal and end the game where the record says
        game = hexref.RefGame(5)
        for ply in range(int(res.length[g])):
            assert game.who_won() is None
            game.make_move(int(res.moves[g, ply]), True)
        assert game.who_won() == ("m" if res.winner[g] == 0 else "b")
        assert (res.moves[g, int(res.length[g]):] == -1).all()
        # move 0 through the round oracle: the same vertex
        tree = ro.RoundTree(hexref.RefGame(5), c_puct=1.5, leaves=4, virtual_loss=2)
        tree.search(lambda gm, moves: (np.zeros(len(gm.get_actions()), np.float32), np.float32(0)), 16)
        assert tree.best() == res.moves[g, 0]


@pytest.mark.parametrize("size", [3, 5])
def test_selfplay_with_leaves_records_the_visit_distributions(hexref, size):
    """A SearchSelfPlay(leaves=4) match: every recorded visit distribution sums to 1, and the first ply's equals N / (applied - 1)
    of the start position's tree replayed by the round oracle (the root's expansion is a simulation without a root visit)."""
    from gnn_hex_amd.search import UniformEvaluator
    from gnn_hex_amd.search_selfplay import SearchSampleBuffer, SearchSelfPlay
    G, sims, A = 4, 14, size * size
    buf = SearchSampleBuffer(G * A, size, DEV)
    sp = SearchSelfPlay(size, G, UniformEvaluator(), sims, buf, root_noise=None, proportional_plies=0, leaves=4, virtual_loss=1)
    res, samples = sp.play("m")
    assert samples == int(res.length.sum()) == len(buf) and sp.search.leaves == 4
    policy, meta = buf.policy[:samples].cpu().numpy(), buf.meta[:samples].cpu().numpy()
    assert np.abs(policy.astype(np.float64).sum(1) - 1).max() <= 1e-6
    tree = ro.RoundTree(hexref.RefGame(size), c_puct=1.5, leaves=4, virtual_loss=1, max_sims=sims)
    tree.search(lambda gm, moves: (np.zeros(len(gm.get_actions()), np.float32), np.float32(0)), sims)
    moves, N = tree.root_counts()
    assert N.sum() == tree.applied - 1
    want = spo.visit_policy(moves, N, A)
    first = np.nonzero(meta[:, 1] == 0)[0]
    assert len(first) == G
    for slot in first:
        assert policy[slot].tobytes() == want.tobytes(), "game %d: the first ply's visit distribution" % meta[slot, 0]
    for g in range(G):                          # legal, complete games; greedy plies: move 0 is the oracle's most visited
        game = hexref.RefGame(size)
        for ply in range(int(res.length[g])):
            assert game.who_won() is None
            game.make_move(int(res.moves[g, ply]), True)
        assert game.who_won() == ("m" if res.winner[g] == 0 else "b") and res.moves[g, 0] == tree.best()
