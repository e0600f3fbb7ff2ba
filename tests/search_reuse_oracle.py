"""Tree reuse between plies (include/hexgnn.h: hexgnn_search_advance) restated on the host, twice, both from the rule and neither
from the kernel (shared by tests/test_search_reuse_host.py and tests/test_gpu_search_reuse.py):

``compact``   the compaction on the dict of arrays that ``TreeSearch.tree()`` returns: the kept set by a breadth-first walk over
              ``child`` from the new root, sorted, the new arrays gathered from the old ones.
``advance``   the same step on a ``search_oracle.Tree`` / ``search_round_oracle.RoundTree``: the node list re-rooted in expansion
              order, ``applied`` set, the root position moved on.

The rule per game.  e = the root edge whose vertex is the move, c = child(0, e).  FRESH (one unexpanded root, counters (1, 0),
carried 0) when the root is unexpanded, the move is negative, no root edge carries it, the edge has no child, or Ns(c) - 1 >
max_carry.  Otherwise the nodes reachable from c move to the slots 0, 1, .. in ascending order of their old slots, child entries
rewritten, the slots from ``kept`` up to the old count get Ns = edges = 0, the counters become (kept, Ns(c) - 1), carried = Ns(c).
Only live words are specified: slots below the count in use, edges below a node's edge count."""
import numpy as np

EDGE_ARRAYS = ("P", "W", "N", "child", "vertex")


def _reachable(children_of, c):
    seen, queue = {c}, [c]
    while queue:
        n = queue.pop()
        for ch in children_of(n):
            if ch >= 0 and ch not in seen:
                seen.add(ch)
                queue.append(ch)
    return sorted(seen)


def compact(t, moves, max_carry):
    """``(tree dict after hexgnn_search_advance, carried [G], kept [G])`` of the tree dict ``t`` (``TreeSearch.tree()``'s
    arrays by name; not modified).  Words the rule leaves unspecified keep their old contents here; ``live_words`` lists the
    ones that count."""
    out = {k: v.copy() for k, v in t.items()}
    G = t["ns"].shape[0]
    carried, kept_n = np.zeros(G, np.int32), np.ones(G, np.int32)
    for g in range(G):
        used, mv = int(t["cnt"][g, 0]), int(moves[g])
        c = -1
        if t["ns"][g, 0] > 0 and mv >= 0:
            ne0 = int(t["ne"][g, 0])
            hit = np.nonzero(t["vertex"][g, 0, :ne0] == mv)[0]
            if len(hit):
                c = int(t["child"][g, 0, hit[0]])
        if c >= 0 and int(t["ns"][g, c]) - 1 > max_carry:
            c = -1
        if c < 0:
            out["ns"][g] = 0
            out["ne"][g] = 0
            out["cnt"][g] = (1, 0)
            continue
        keep = _reachable(lambda n: t["child"][g, n, :int(t["ne"][g, n])].tolist(), c)
        new = {old: i for i, old in enumerate(keep)}
        for i, old in enumerate(keep):
            ne = int(t["ne"][g, old])
            out["ns"][g, i], out["ne"][g, i] = t["ns"][g, old], ne
            for name in EDGE_ARRAYS:
                out[name][g, i, :ne] = t[name][g, old, :ne]
            out["child"][g, i, :ne] = [new[ch] if ch >= 0 else ch for ch in t["child"][g, old, :ne].tolist()]
        out["ns"][g, len(keep):used] = 0
        out["ne"][g, len(keep):used] = 0
        out["cnt"][g] = (len(keep), int(t["ns"][g, c]) - 1)
        carried[g], kept_n[g] = t["ns"][g, c], len(keep)
    return out, carried, kept_n


def live_words(t, before=None):
    """The specified words of a tree dict as ``{(name, game, slot): bytes}``: the counters, Ns / edge counts of every slot below
    the count in use (and below ``before``'s count, where they must read 0 after an advance), the live edges of the slots in
    use.  P and W as raw bits."""
    out = {}
    G = t["ns"].shape[0]
    for g in range(G):
        used = int(t["cnt"][g, 0])
        out[("cnt", g, 0)] = t["cnt"][g].tobytes()
        top = max(used, int(before["cnt"][g, 0])) if before is not None else used
        out[("ns", g, 0)] = t["ns"][g, :top].tobytes()
        out[("ne", g, 0)] = t["ne"][g, :top].tobytes()
        for n in range(used):
            if t["ns"][g, n] <= 0:
                continue
            ne = int(t["ne"][g, n])
            for name in EDGE_ARRAYS:
                out[(name, g, n)] = t[name][g, n, :ne].tobytes()
    return out


def assert_same_live_words(got, want, before=None):
    a, b = live_words(got, before), live_words(want, before)
    assert sorted(a) == sorted(b), "the live slots differ: %s" % sorted(set(a) ^ set(b))[:8]
    for key in sorted(a):
        assert a[key] == b[key], "%s of game %d, slot %d differs" % key


def advance(tree, move, max_carry=None, play=True):
    """``hexgnn_search_advance`` on one oracle tree: returns ``carried``.  ``play``: the root position moves on by ``move``
    (when it is a vertex; a caller whose game ended or restarted sets ``tree.root_game`` itself)."""
    root = tree.nodes[0]
    c = -1
    if root is not None and move >= 0:
        hit = np.nonzero(root.moves == move)[0]
        if len(hit):
            c = int(root.child[hit[0]])
    if c >= 0 and max_carry is not None and tree.nodes[c].Ns - 1 > max_carry:
        c = -1
    if play and move >= 0:
        game = tree.root_game.copy()
        game.make_move(int(move), True)
        tree.root_game = game
    if c < 0:
        tree.nodes, tree.applied = [None], 0
        return 0
    keep = _reachable(lambda n: tree.nodes[n].child.tolist(), c)
    new = {old: i for i, old in enumerate(keep)}
    nodes = [tree.nodes[old] for old in keep]
    for nd in nodes:
        nd.child = np.array([new[int(ch)] if ch >= 0 else -1 for ch in nd.child], dtype=np.int64)
    tree.nodes, tree.applied = nodes, nodes[0].Ns - 1
    return nodes[0].Ns


def tree_dict(trees, max_sims, slots):
    """Oracle trees as the dict of arrays ``TreeSearch.tree()`` would hold (P in fp32; slots past the tree zeroed)."""
    G, C = len(trees), max_sims + 1
    t = dict(ns=np.zeros((G, C), np.int32), ne=np.zeros((G, C), np.int32), cnt=np.zeros((G, 2), np.int32),
             P=np.zeros((G, C, slots), np.float32), W=np.zeros((G, C, slots), np.float32), N=np.zeros((G, C, slots), np.int32),
             child=np.full((G, C, slots), -1, np.int32), vertex=np.zeros((G, C, slots), np.uint16))
    for g, tree in enumerate(trees):
        t["cnt"][g] = (len(tree.nodes), tree.applied)
        for n, nd in enumerate(tree.nodes):
            if nd is None:
                continue
            ne = len(nd.moves)
            t["ns"][g, n], t["ne"][g, n] = nd.Ns, ne
            t["P"][g, n, :ne], t["W"][g, n, :ne], t["N"][g, n, :ne] = nd.P, nd.W, nd.N
            t["child"][g, n, :ne], t["vertex"][g, n, :ne] = nd.child, nd.moves
    return t
