"""CPU: tree reuse between plies (include/hexgnn.h: hexgnn_search_advance; tests/search_reuse_oracle.py) on the host.
(a) the invariants of an advanced tree on free-running oracle trees, one-leaf and rounds, (b) every fresh-tree case of the rule,
(c) the two host restatements -- the node-list one and the numpy compaction -- agree with each other, (d) the entry point's
declaration, its ctypes mirror and its argument checks in the documented order, (e) the python layer's refusals that need no
device.  Nothing here touches a GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

import search_oracle as so
import search_reuse_oracle as reuse
import search_round_oracle as ro

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EUNSUPPORTED = -1, -2


def _grown(hexref, size, gid, sims, max_sims, leaves=1, peaked=False):
    game = hexref.random_position(size, 700 * size + gid, gid % 2 == 0) if gid else hexref.RefGame(size)
    ev = so.peaked_evaluator(gid, seed=size) if peaked else so.synthetic_evaluator(gid, seed=size)
    if leaves > 1:
        tree = ro.RoundTree(game, max_sims=max_sims, leaves=leaves, virtual_loss=2)
        tree.search(ev, sims)
    else:
        tree = so.Tree(game, max_sims=max_sims)
        for _ in range(sims):
            tree.simulate(ev)
    return tree, ev


def _check_invariants(tree):
    root = tree.nodes[0]
    assert root is not None
    parents = {}
    for n, nd in enumerate(tree.nodes):
        for ch in nd.child[nd.child >= 0]:
            assert n < ch < len(tree.nodes), "child %d of node %d" % (ch, n)
            assert ch not in parents, "node %d has two parents" % ch
            parents[int(ch)] = n
        assert nd.Ns == 1 + nd.N.sum()
    assert sorted(parents) == list(range(1, len(tree.nodes))), "every node but the root hangs on exactly one edge"
    assert len(tree.nodes) <= root.Ns and root.Ns - 1 == root.N.sum() == tree.applied


@pytest.mark.parametrize("leaves", [1, 4])
def test_an_advanced_tree_keeps_the_invariants(hexref, leaves):
    """(a) child > parent, kept <= Ns', Ns' - 1 == sum N(root edges) == applied, along three plies of the most visited move."""
    advanced = 0
    for size, gid, sims in ((5, 0, 40), (5, 1, 40), (7, 2, 60), (9, 3, 40)):
        tree, ev = _grown(hexref, size, gid, sims, 400, leaves)
        for ply in range(3):
            if tree.root_game.who_won() is not None or tree.nodes[0] is None:
                break
            root = tree.nodes[0]
            e = so.first_max(root.N)
            c = int(root.child[e])
            want_ns = tree.nodes[c].Ns if c >= 0 else 0
            below = [nd for nd in tree.nodes]                    # the objects, to see which ones survive
            carried = reuse.advance(tree, int(root.moves[e]))
            assert carried == want_ns
            if carried == 0:
                assert tree.nodes == [None] and tree.applied == 0
                break
            _check_invariants(tree)
            assert tree.nodes[0] is below[c] and all(any(nd is b for b in below) for nd in tree.nodes)
            # the survivors keep their relative (expansion) order
            order = [next(i for i, b in enumerate(below) if b is nd) for nd in tree.nodes]
            assert order == sorted(order) and order[0] == c
            advanced += 1
            if leaves > 1:
                tree.search(ev, 24)
            else:
                for _ in range(24):
                    tree.simulate(ev)
            _check_invariants(tree)
    assert advanced >= 8


@pytest.mark.parametrize("leaves", [1, 4])
def test_the_next_simulations_fit_behind_max_carry(hexref, leaves):
    """(a) with max_carry = max_sims - s, advancing and then simulating s times never SKIPs; one more does."""
    max_sims, s = 48, 16
    tree, ev = _grown(hexref, 5, 1, 40, max_sims, leaves)
    root = tree.nodes[0]
    by_count = np.argsort(-root.N, kind="stable")
    heavy = next(int(e) for e in by_count if root.child[e] >= 0 and tree.nodes[int(root.child[e])].Ns - 1 <= max_sims - s)
    carried = reuse.advance(tree, int(root.moves[heavy]), max_carry=max_sims - s)
    assert 1 <= carried <= max_sims - s + 1 and tree.applied == carried - 1
    if leaves > 1:
        for n in (4, 4, 4, 4):
            out = tree.round(ev, round_leaves=n)
            assert all(d["kind"] != so.SKIPPED for d in out)
        assert tree.status == 0 and tree.applied <= max_sims
    else:
        for _ in range(s):
            assert tree.simulate(ev)[0] != so.SKIPPED
        assert tree.applied == carried - 1 + s <= max_sims
        for _ in range(max_sims - tree.applied):
            assert tree.simulate(ev)[0] != so.SKIPPED
        assert tree.simulate(ev)[0] == so.SKIPPED
    assert len(tree.nodes) <= tree.applied + 1


def test_every_fresh_tree_case(hexref):
    """(b) unexpanded root, negative move, a vertex that is no root edge, an edge without a child, a subtree above max_carry."""
    def grown():
        return _grown(hexref, 5, 2, 30, 64)[0]

    tree = so.Tree(hexref.RefGame(5), max_sims=64)
    assert reuse.advance(tree, 5) == 0 and tree.nodes == [None] and tree.applied == 0
    assert tree.root_game.total_num_moves == 1, "the position moves on whatever becomes of the tree"
    tree = grown()
    assert reuse.advance(tree, -1) == 0 and tree.nodes == [None] and tree.applied == 0
    tree = grown()
    root = tree.nodes[0]
    absent = next(v for v in range(2, 27) if v not in root.moves)
    assert reuse.advance(tree, absent, play=False) == 0 and tree.nodes == [None]
    tree = grown()
    root = tree.nodes[0]
    childless = int(root.moves[np.nonzero(root.child < 0)[0][0]])
    assert reuse.advance(tree, childless) == 0 and tree.nodes == [None] and tree.applied == 0
    tree = grown()
    root = tree.nodes[0]
    e = so.first_max(root.N)
    ns_c = tree.nodes[int(root.child[e])].Ns
    assert ns_c >= 3
    assert reuse.advance(tree, int(root.moves[e]), max_carry=ns_c - 2) == 0 and tree.nodes == [None]
    tree = grown()
    assert reuse.advance(tree, int(tree.nodes[0].moves[e]), max_carry=ns_c - 1) == ns_c     # the bound is inclusive
    # a fresh tree searches on like a new one
    tree = grown()
    reuse.advance(tree, -1)
    ev = so.synthetic_evaluator(2, seed=5)
    for _ in range(8):
        tree.simulate(ev)
    assert tree.applied == 8 and tree.nodes[0].Ns == 8


def test_the_numpy_compaction_agrees_with_the_node_list(hexref):
    """(c) ``compact`` on the arrays of five oracle trees against ``advance`` on the trees themselves: every live word, the
    counters and carried -- with a peaked line (one long chain: nearly everything is kept and moves down by one slot), a move
    off that line, and the fresh cases in the same call."""
    max_sims = 96
    trees = [_grown(hexref, 7, g, 80 if g == 4 else 64, max_sims, peaked=(g in (0, 1, 4)))[0] for g in range(5)]
    t = reuse.tree_dict(trees, max_sims, 49)
    roots = [tr.nodes[0] for tr in trees]
    best = [so.first_max(r.N) for r in roots]
    off_line = int(np.argsort(-roots[1].N, kind="stable")[1])
    moves = [int(roots[0].moves[best[0]]), int(roots[1].moves[off_line]), -1,
             next(v for v in range(2, 51) if v not in roots[3].moves), int(roots[4].moves[best[4]])]
    ns4 = trees[4].nodes[int(roots[4].child[best[4]])].Ns
    carry = ns4 - 2                                          # game 4's subtree is one above it
    assert trees[0].nodes[int(roots[0].child[best[0]])].Ns - 1 <= carry, "the peaked line must fit"
    out, carried, kept = reuse.compact(t, moves, carry)
    want = [reuse.advance(tr, mv, max_carry=carry, play=False) for tr, mv in zip(trees, moves)]
    assert carried.tolist() == want and want[2] == want[3] == want[4] == 0 and want[0] > 40
    assert kept[0] > 30 and kept[1] < 3              # (the line reaches the end of a Hex-7 game: terminals add no node)
    reuse.assert_same_live_words(out, reuse.tree_dict(trees, max_sims, 49), before=t)
    for g in (2, 3, 4):
        assert (out["ns"][g] == 0).all() and (out["ne"][g] == 0).all() and tuple(out["cnt"][g]) == (1, 0)
    # and a second step straight behind the first
    root = trees[0].nodes[0]
    mv = int(root.moves[so.first_max(root.N)])
    out2, carried2, _ = reuse.compact(out, [mv, -1, -1, -1, -1], max_sims)
    assert carried2[0] == reuse.advance(trees[0], mv, play=False)
    for tr in trees[1:]:
        reuse.advance(tr, -1)
    reuse.assert_same_live_words(out2, reuse.tree_dict(trees, max_sims, 49), before=out)


# ---- (d) declaration, mirror, refusals --------------------------------------------------------------------------------------
def test_advance_is_declared_exported_and_mirrored():
    from gnn_hex_amd import _lib
    header = open(os.path.join(ROOT, "include", "hexgnn.h")).read()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    assert re.search(r"\bint\s+hexgnn_search_advance\s*\(\s*const\s+hexgnn_search_advance_call\s*\*\s*\w+\s*,\s*hexgnn_stream_t\s+\w+\s*\)",
                     header)
    assert hasattr(raw, "hexgnn_search_advance") and "hexgnn_search_advance" in _lib.exported_symbols()
    m = re.search(r"typedef\s+struct\s+hexgnn_search_advance_call\s*\{(.*?)\}\s*hexgnn_search_advance_call\s*;", header, re.S)
    decls = [d.strip() for d in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(";") if d.strip()]
    names = [re.search(r"(\w+)\s*$", d).group(1) for d in decls]
    assert names == [n for n, _ in _lib.SearchAdvanceCall._fields_] == ["struct_bytes", "call", "moves", "max_carry", "remap", "carried"]
    assert [t for _, t in _lib.SearchAdvanceCall._fields_] == [ctypes.c_size_t, _lib.SearchCall, ctypes.c_void_p, ctypes.c_int,
                                                              ctypes.c_void_p, ctypes.c_void_p]
    assert ["*" in d for d in decls] == [False, False, True, False, True, True]
    assert _lib.lib().hexgnn_abi_version() == 8


def _advance_call(_lib, p, max_carry=4, struct_bytes=None, **kw):
    L = _lib.lib()
    call = _lib.SearchCall(struct_bytes=ctypes.sizeof(_lib.SearchCall), num_games=2, hex_size=5, max_sims=8, skip=2, c_puct=1.5,
                           temperature=1.0, fill=0.0, workspace=p, workspace_bytes=L.hexgnn_search_workspace_bytes(2, 5, 8),
                           status=p, active=None, path=None, leaf=None, result=None, logits=None, offsets=None, value=None,
                           gptr=None, scores=None, counts=None, q=None, best=None)
    fields = dict(moves=p, remap=p, carried=p)
    for k, v in kw.items():
        if k in fields:
            fields[k] = v
        else:
            setattr(call, k, v)
    return _lib.SearchAdvanceCall(struct_bytes=ctypes.sizeof(_lib.SearchAdvanceCall) if struct_bytes is None else struct_bytes,
                                  call=call, max_carry=max_carry, **fields)


def test_advance_refusals_that_need_no_device():
    """Every refusal comes from the host checks, before anything is launched, in the header's order: an earlier failure wins
    over a later one (EUNSUPPORTED for Hex-26 shows through only when everything before it is in order)."""
    from gnn_hex_amd import _lib
    L = _lib.lib()
    buf = (ctypes.c_char * 4096)()
    p = ctypes.addressof(buf)

    def fn(c):
        return L.hexgnn_search_advance(ctypes.byref(c) if c is not None else None, None)

    assert fn(None) == EINVAL
    assert fn(_advance_call(_lib, p, struct_bytes=ctypes.sizeof(_lib.SearchAdvanceCall) - 8)) == EINVAL
    assert fn(_advance_call(_lib, p, struct_bytes=ctypes.sizeof(_lib.SearchRoundCall))) == EINVAL
    c = _advance_call(_lib, p)
    c.call.struct_bytes -= 8
    assert fn(c) == EINVAL
    for kw in (dict(num_games=-1), dict(hex_size=1), dict(max_sims=0), dict(max_sims=65536)):
        assert fn(_advance_call(_lib, p, **kw)) == EINVAL, kw
    assert fn(_advance_call(_lib, p, hex_size=26)) == EUNSUPPORTED
    assert fn(_advance_call(_lib, p, hex_size=26, num_games=-1)) == EINVAL
    # the board size is judged before the pointers of the outer descriptor and before max_carry
    assert fn(_advance_call(_lib, p, hex_size=26, moves=None, max_carry=-1)) == EUNSUPPORTED
    # no games: nothing to do, whatever the pointers are
    assert fn(_advance_call(_lib, p, num_games=0, workspace=None, status=None, moves=None, remap=None, carried=None,
                            max_carry=-1)) == 0
    for kw in (dict(workspace=None), dict(status=None)):
        assert fn(_advance_call(_lib, p, **kw)) == EINVAL, kw
    c = _advance_call(_lib, p)
    c.call.workspace_bytes -= 1
    assert fn(c) == EINVAL
    for kw in (dict(moves=None), dict(remap=None), dict(carried=None)):
        assert fn(_advance_call(_lib, p, **kw)) == EINVAL, kw
    for bad in (-1, 9, 1 << 30):
        assert fn(_advance_call(_lib, p, max_carry=bad)) == EINVAL, bad


# ---- (e) the python layer ---------------------------------------------------------------------------------------------------
def test_reuse_arguments_of_the_players():
    from gnn_hex_amd import _lib
    from gnn_hex_amd.search import SearchPlayer, UniformEvaluator, check_reuse_arguments
    assert check_reuse_arguments(12, False, None) == 12
    assert check_reuse_arguments(12, True, None) == 48 and check_reuse_arguments(12, True, 12) == 12
    assert check_reuse_arguments(40000, True, None) == _lib.SEARCH_MAX_SIMS
    for bad in (11, 0, -3, 12.5, _lib.SEARCH_MAX_SIMS + 1):
        with pytest.raises(ValueError, match="capacity"):
            check_reuse_arguments(12, True, bad)
    with pytest.raises(ValueError, match="reuse_tree"):
        check_reuse_arguments(12, False, 48)
    ev = UniformEvaluator()
    p = SearchPlayer(ev, 12)
    assert (p.reuse_tree, p.capacity) == (False, 12)
    p.begin_match()                                           # no search yet, no reuse: nothing happens, nothing is needed
    p.observe_moves(None)
    q = SearchPlayer(ev, 12, reuse_tree=True)
    assert (q.reuse_tree, q.capacity) == (True, 48) and SearchPlayer(ev, 12, reuse_tree=True, capacity=20).capacity == 20
    q.begin_match()
    q.observe_moves(None)                                     # before its first search there is no tree to move on
    with pytest.raises(ValueError, match="capacity"):
        SearchPlayer(ev, 12, reuse_tree=True, capacity=11)
    with pytest.raises(ValueError, match="reuse_tree"):
        SearchPlayer(ev, 12, capacity=48)


def test_the_arena_finds_the_players_that_follow_a_match():
    from gnn_hex_amd.arena import _observers
    from gnn_hex_amd.search import SearchPlayer, UniformEvaluator
    a, b = SearchPlayer(UniformEvaluator(), 8, reuse_tree=True), SearchPlayer(UniformEvaluator(), 8)
    assert _observers(((a, False), ("random", False))) == [a]
    assert _observers(((a, False), (a, False))) == [a], "a player on both sides is told once"
    assert _observers(((a, False), (b, False))) == [a, b]
    assert _observers((("random", False), (object(), False))) == []
