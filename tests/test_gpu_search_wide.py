"""GPU: the tree search where the other search tests do not go -- boards of four and more adjacency words, paths and trees beyond
one 64-lane trip, the accepted round limits -- against the same host oracles, teacher-forced through the same rigs
(test_gpu_search.Rig, test_gpu_search_round.RoundRig): N, Ns, W, children, vertices and counters bit for bit, P to 1e-6, the leaf env
equal to the RefGame replay of every path, guards intact, in-flight counts zero after every backup.
(a) (b) the one-leaf search and rounds on Hex-14 (W = 4: the last fixed instantiation; A = 196), Hex-16 (W = 5: the run-time word
    count; A = 256, exactly four lane trips) and Hex-25 (W = 10, A = 625: ten 64-vertex chunks in the leaf's move compaction);
(c) (d) the peaked evaluator on Hex-14 / 16 start positions: paths of 65 steps and more (the second trip of every loop over a
    path: the ``inside`` check, the N / W / Ns backup, the in-flight increment and clear) and more than 64 node slots (the reset's
    second trip, on a poisoned workspace).  tests/test_search_deep_host.py proves by the oracle alone that these inputs get
    there; here the DEVICE's records must show it;
(e) HEXGNN_SEARCH_MAX_LEAVES descents per round, at virtual loss 1 and HEXGNN_SEARCH_MAX_VIRTUAL_LOSS;
(f) TreeSearch.simulate and the evaluators on Hex-14, replayed through the oracles from its trace."""
import numpy as np
import pytest
import torch

import search_oracle as so
import search_round_oracle as ro
import test_gpu_search as tgs
import test_gpu_search_round as tgr
from test_search_deep_host import DEEP, DEEP_ONE_LEAF, DEEP_ROUNDS, LIMIT_ROUNDS, peaked, start_positions

pytestmark = pytest.mark.gpu

DEV = "cuda"


def worst_prior_error(rig):
    """The largest relative error of a device prior against the oracle's float64 softmax, over every expanded node."""
    t, worst = rig.search.tree(), 0.0
    for g, tree in enumerate(rig.trees):
        for i, nd in enumerate(tree.nodes):
            if nd is not None:
                ne = len(nd.moves)
                worst = max(worst, float((np.abs(t["P"][g, i, :ne].astype(np.float64) - nd.P) / nd.P).max()))
    return worst


def finish_one_leaf(rig, what):
    print("%s: largest relative prior error %.3g" % (what, worst_prior_error(rig)))
    rig.compare_trees()
    rig.compare_root()
    steps, ambiguous = rig.finish()
    assert ambiguous <= 0.01 * max(steps, 1)
    return steps


def finish_rounds(rig, what, rounds):
    """The checks behind test_gpu_search_round.test_rounds_follow_the_oracle's loop."""
    print("%s: largest relative prior error %.3g" % (what, worst_prior_error(rig)))
    rig.compare_trees()
    rig.compare_root()
    steps, ambiguous, kinds = rig.finish()
    assert ambiguous <= 0.01 * max(steps, 1)
    assert kinds.sum() == rig.G * rig.K * rounds
    applied = rig.search.applied().cpu().numpy()
    assert np.array_equal(applied, [t.applied for t in rig.trees])
    assert kinds[ro.COLLISION] >= rig.G * (rig.K - 1) and kinds[ro.LEAF] >= rig.G and steps >= rig.G * rig.K
    return kinds


# ---- (a) the one-leaf search on four and more words ----------------------------------------------------------------------
@pytest.mark.parametrize("size,G,sims", [(14, 3, 40), (16, 3, 40), (25, 2, 24)])
def test_wide_tree_and_leaf_env_follow_the_oracle(hexref, size, G, sims):
    rig = tgs.Rig(hexref, size, G, sims)
    assert rig.W == (size * size + 2 + 63) // 64
    for s in range(sims):
        rig.sim(s, tgs._synthetic(size))
    steps = finish_one_leaf(rig, "Hex-%d one leaf" % size)
    assert rig.kinds[so.LEAF] >= G and steps >= G * (sims - 1)


# ---- (b) rounds on the same boards -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("size,G,K,sims", [(14, 3, 4, 40), (16, 3, 5, 40), (25, 2, 4, 24)])
def test_wide_rounds_follow_the_oracle(hexref, size, G, K, sims):
    rig = tgr.RoundRig(hexref, size, G, K, sims)
    rounds = list(tgr._rounds(sims, K))
    for r, n in enumerate(rounds):
        rig.round(r, tgs._synthetic(size), round_leaves=n)
    finish_rounds(rig, "Hex-%d K=%d" % (size, K), len(rounds))


# ---- (c) paths and trees beyond one lane trip: the one-leaf search -----------------------------------------------------------
def test_deep_one_leaf_search(hexref):
    size, G, sims = DEEP_ONE_LEAF
    rig = tgs.Rig(hexref, size, G, sims, games=start_positions(hexref, size, G))
    deep = np.zeros((G, 3), dtype=np.int64)              # per game and kind: the device's descents of >= DEEP steps
    for s in range(sims):
        rig.sim(s, peaked(size))                         # (the leaf env on every simulation)
        rec = rig.search.leaf.cpu().numpy()
        for g in range(G):
            deep[g, rec[g, 0]] += rec[g, 2] >= DEEP
    print("Hex-%d one leaf, %d sims: device descents of >= %d steps leaf/terminal %d/%d" % (size, sims, DEEP, deep[:, so.LEAF].sum(),
                                                                                          deep[:, so.TERMINAL].sum()))
    assert (deep[:, so.LEAF] >= 1).all(), "a game without a LEAF of %d steps: %s" % (DEEP, deep)
    assert deep[:, so.TERMINAL].sum() >= 1
    assert (rig.search.tree()["cnt"][:, 0] > 64).all(), "a game within 64 node slots"
    finish_one_leaf(rig, "Hex-%d one leaf, peaked" % size)


# ---- (d) paths and trees beyond one lane trip: rounds ------------------------------------------------------------------------
@pytest.mark.parametrize("size,G,K,vl,sims", DEEP_ROUNDS)
def test_deep_rounds(hexref, size, G, K, vl, sims):
    rig = tgr.RoundRig(hexref, size, G, K, sims, vl=vl, games=start_positions(hexref, size, G))
    deep = np.zeros((G, 4), dtype=np.int64)
    rounds = list(tgr._rounds(sims, K))
    for r, n in enumerate(rounds):
        rig.round(r, peaked(size), round_leaves=n)       # (the leaf env on every round)
        rec = rig.search.leaf.cpu().numpy()
        for g in range(G):
            for k in range(K):
                deep[g, rec[g, k, 0]] += rec[g, k, 2] >= DEEP
        if r % 16 == 0:
            assert (rig.search.tree()["inflight"] == 0).all(), "round %d: in-flight counts survive the backup" % r
    print("Hex-%d K=%d vl=%d, %d sims: device descents of >= %d steps leaf/terminal/collision %d/%d/%d" % (
        size, K, vl, sims, DEEP, deep[:, ro.LEAF].sum(), deep[:, ro.TERMINAL].sum(), deep[:, ro.COLLISION].sum()))
    assert (deep[:, ro.LEAF] >= 1).all(), "a game without a LEAF of %d steps: %s" % (DEEP, deep)
    assert deep[:, ro.TERMINAL].sum() >= 1
    if size == 14:
        assert deep[:, ro.COLLISION].sum() >= 1
    assert (rig.search.tree()["cnt"][:, 0] > 64).all(), "a game within 64 node slots"
    finish_rounds(rig, "Hex-%d K=%d vl=%d, peaked" % (size, K, vl), len(rounds))


# ---- (e) the accepted limits -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size,G,K,sims,vl", LIMIT_ROUNDS)
def test_rounds_at_the_accepted_limits(hexref, size, G, K, sims, vl):
    from gnn_hex_amd import _lib
    assert K == _lib.SEARCH_MAX_LEAVES and vl in (1, _lib.SEARCH_MAX_VIRTUAL_LOSS)
    rig = tgr.RoundRig(hexref, size, G, K, sims, vl=vl)
    rounds = list(tgr._rounds(sims, K))
    assert rounds == [K] * 4
    for r, n in enumerate(rounds):
        rig.round(r, tgs._synthetic(size), round_leaves=n)
    kinds = finish_rounds(rig, "Hex-%d K=%d vl=%d" % (size, K, vl), len(rounds))
    assert kinds[ro.LEAF] >= 1 and kinds[ro.TERMINAL] >= 1 and kinds[ro.COLLISION] >= 1 and kinds[ro.SKIPPED] == 0


# ---- (f) the python level on Hex-14 ------------------------------------------------------------------------------------------
def _evaluator(which):
    from gnn_hex_amd.search import PolicyValueEvaluator, UniformEvaluator
    from gnn_hex_amd.torch_script_models import SAGE_torch_script
    if which == "uniform":
        return UniformEvaluator()
    torch.manual_seed(5)
    return PolicyValueEvaluator(SAGE_torch_script(32, 3, 2, 2).to(DEV).eval())


@pytest.mark.parametrize("which", ["uniform", "policy_value"])
@pytest.mark.parametrize("leaves", [1, 4])
def test_simulate_on_hex14_replays_through_the_oracle(hexref, which, leaves):
    size, G, sims = 14, 4, 18
    ev = _evaluator(which)
    if leaves == 1:
        rig, trace = tgs._traced(hexref, ev, size, G, sims)
        assert all(t.applied == sims for t in rig.trees)
    else:
        rig = tgr.RoundRig(hexref, size, G, leaves, sims)
        trace = []
        rig.search.simulate(rig.mgr._h, ev, sims, trace=trace)
        assert [r["round_leaves"] for r in trace] == [4, 4, 4, 4, 2]
        tgr._replay_rounds(rig, trace)
        rig.compare_trees()
        rig.compare_root()
        steps, ambiguous, kinds = rig.finish()
        applied = rig.search.applied().cpu().numpy()
        assert np.array_equal(applied, [t.applied for t in rig.trees]) and (applied <= sims - (leaves - 1)).all() and (applied > leaves).all()
        assert steps > G * leaves and kinds[ro.SKIPPED] == 2 * G
    rig.search.status()
