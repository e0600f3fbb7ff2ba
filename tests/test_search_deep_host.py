"""CPU: the inputs of tests/test_gpu_search_wide.py's deep and limit cases reach the regions they are there for, BY THE REFERENCE
ALONE, so that the GPU tests cannot pass vacuously.  The oracles of tests/search_oracle.py and tests/search_round_oracle.py run
free with ``select32=True`` (the fp32 restatement of the device's arithmetic) under the peaked evaluator on start positions of
Hex-14 / 16 (boards below do not reach 65 plies: their games end at depth 31-57), and must give: per game a LEAF whose path has
at least 65 steps -- a second trip of every ``for (d = lane; d < len; d += 64)`` loop over a path -- and more than 64 node slots;
per case a TERMINAL that deep; in the Hex-14 round case a COLLISION that deep; at most 1 % ambiguous steps.  The K = 64 cases
must hold every kind.  Nothing here touches a GPU."""
import numpy as np
import pytest

import search_oracle as so
import search_round_oracle as ro

DEEP = 65                                   # path steps: one more than a 64-lane trip
DEEP_ONE_LEAF = (14, 3, 120)                # size, G, max_sims
DEEP_ROUNDS = [(14, 3, 2, 1, 200), (16, 3, 3, 2, 300)]          # size, G, K, virtual loss, simulations asked for
LIMIT_ROUNDS = [(5, 3, 64, 256, 1), (5, 3, 64, 256, 1024)]      # size, G, K, max_sims, virtual loss: four full rounds


def start_positions(hexref, size, G):
    """The start position G times, sides alternating by game."""
    out = []
    for g in range(G):
        game = hexref.RefGame(size)
        game.maker_turn = g % 2 == 0
        out.append(game)
    return out


def peaked(seed):
    """Per game the peaked evaluator, seeded as the suite seeds the synthetic one: by the board size."""
    return lambda g: so.peaked_evaluator(g, seed=seed)


def deep_counts(records):
    """``records``: (kind, path length) of one game's descents -> the number of descents of >= DEEP steps per kind."""
    out = np.zeros(4, dtype=np.int64)
    for kind, ln in records:
        out[kind] += ln >= DEEP
    return out


def test_deep_one_leaf_inputs(hexref):
    size, G, sims = DEEP_ONE_LEAF
    total, steps, ambiguous = np.zeros(4, dtype=np.int64), 0, 0
    for g, game in enumerate(start_positions(hexref, size, G)):
        tree = so.Tree(game, c_puct=1.5, max_sims=sims)
        records = []
        for _ in range(sims):
            kind, _, moves = tree.simulate(peaked(size)(g), select32=True)
            records.append((kind, len(moves)))
        deep = deep_counts(records)
        assert deep[so.LEAF] >= 1, "game %d: no LEAF of %d steps" % (g, DEEP)
        assert len(tree.nodes) > 64, "game %d: %d node slots" % (g, len(tree.nodes))
        total += deep
        steps += tree.steps
        ambiguous += tree.ambiguous
    print("Hex-%d one leaf, %d sims: descents of >= %d steps leaf/terminal %d/%d; %d ambiguous of %d steps" % (
        size, sims, DEEP, total[so.LEAF], total[so.TERMINAL], ambiguous, steps))
    assert total[so.TERMINAL] >= 1
    assert ambiguous <= 0.01 * steps


@pytest.mark.parametrize("size,G,K,vl,sims", DEEP_ROUNDS)
def test_deep_round_inputs(hexref, size, G, K, vl, sims):
    total, steps, ambiguous = np.zeros(4, dtype=np.int64), 0, 0
    for g, game in enumerate(start_positions(hexref, size, G)):
        tree = ro.RoundTree(game, c_puct=1.5, max_sims=sims, leaves=K, virtual_loss=vl)
        records, left = [], sims
        while left > 0:
            n = min(K, left)
            records += [(d["kind"], len(d["path"])) for d in tree.round(peaked(size)(g), round_leaves=n, select32=True)]
            left -= n
        deep = deep_counts(records)
        assert deep[ro.LEAF] >= 1, "game %d: no LEAF of %d steps" % (g, DEEP)
        assert len(tree.nodes) > 64, "game %d: %d node slots" % (g, len(tree.nodes))
        assert tree.inflight_total() == 0 and tree.status == 0
        total += deep
        steps += tree.steps
        ambiguous += tree.ambiguous
    print("Hex-%d K=%d vl=%d, %d sims: descents of >= %d steps leaf/terminal/collision %d/%d/%d; %d ambiguous of %d steps" % (
        size, K, vl, sims, DEEP, total[ro.LEAF], total[ro.TERMINAL], total[ro.COLLISION], ambiguous, steps))
    assert total[ro.TERMINAL] >= 1
    if size == 14:
        assert total[ro.COLLISION] >= 1
    assert ambiguous <= 0.01 * steps


@pytest.mark.parametrize("size,G,K,sims,vl", LIMIT_ROUNDS)
def test_limit_round_inputs(hexref, size, G, K, sims, vl):
    """HEXGNN_SEARCH_MAX_LEAVES descents per round at virtual loss 1 and HEXGNN_SEARCH_MAX_VIRTUAL_LOSS, the synthetic
    evaluator on the GPU suite's root positions: every kind but SKIPPED occurs."""
    kinds, steps, ambiguous = np.zeros(4, dtype=np.int64), 0, 0
    for g in range(G):
        game = hexref.RefGame(size) if g == 0 else hexref.random_position(size, 900 * size + g, g % 2 == 0)
        tree = ro.RoundTree(game, c_puct=1.5, max_sims=sims, leaves=K, virtual_loss=vl)
        tree.search(so.synthetic_evaluator(g, seed=size), sims, select32=True)
        assert tree.kinds.sum() == sims and tree.kinds[ro.SKIPPED] == 0 and tree.inflight_total() == 0 and tree.status == 0
        kinds += tree.kinds
        steps += tree.steps
        ambiguous += tree.ambiguous
    print("Hex-%d K=%d vl=%d: kinds leaf/terminal/skipped/collision %s; %d ambiguous of %d steps" % (size, K, vl, kinds, ambiguous, steps))
    assert kinds[ro.LEAF] >= 1 and kinds[ro.TERMINAL] >= 1 and kinds[ro.COLLISION] >= 1
    assert ambiguous <= 0.01 * steps
