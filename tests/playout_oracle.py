"""The playout rule of include/hexgnn.h (hexgnn_playout_values) restated in numpy (shared by tests/test_playout_host.py and
tests/test_gpu_playouts.py): the hash, the selection sampling, the reachability test, the all-moves-as-first tables and the fp32
scores.  Written from the rule, vectorised over the playouts of one graph; it shares no code with the kernel."""
import numpy as np

M32 = np.uint64(0xFFFFFFFF)


def h32(x):
    """The hash on uint64 arrays (or ints) that hold 32-bit values."""
    x = np.asarray(x, dtype=np.uint64) & M32
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x7feb352d)) & M32
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x846ca68b)) & M32
    x = x ^ (x >> np.uint64(16))
    return x


def graph_base(seed, counter, g):
    """base of graph ``g`` of a batch: the low 32 bits of ``counter`` count."""
    c = int(counter) & 0xFFFFFFFF
    return h32(int(h32((int(seed) + 0x9e3779b9 * c) & 0xFFFFFFFF)) + int(g))


def mover_sets(n, playouts, base):
    """bool [R, n]: the rows the side to move owns in every playout (rows 0 and 1, the terminals, are never owned)."""
    m = n - 2
    R = int(playouts)
    key = h32(np.uint64(int(base)) + np.arange(R, dtype=np.uint64))
    own = np.zeros((R, n), dtype=bool)
    left = np.full(R, (m + 1) // 2, dtype=np.int64)
    for i in range(m):
        r = h32(key + np.uint64(i))
        take = ((r * np.uint64(m - i)) >> np.uint64(32)).astype(np.int64) < left
        own[:, i + 2] = take
        left -= take
    return own


def connected(adj, allowed):
    """bool [R]: is row 1 reachable from row 0 through edges whose two ends are allowed?  ``adj`` bool [n, n] symmetric,
    ``allowed`` bool [R, n]."""
    A = adj.astype(np.float32)
    allowed = allowed.copy()
    allowed[:, :2] = True
    reach = np.zeros(allowed.shape, dtype=bool)
    reach[:, 0] = True
    for _ in range(adj.shape[0]):
        new = ((reach.astype(np.float32) @ A) > 0) & allowed & ~reach
        if not new.any():
            break
        reach |= new
    return reach[:, 1]


def dense_adjacency(n, edges):
    """bool [n, n] from an int array [2, E] of local row indices (made symmetric)."""
    adj = np.zeros((n, n), dtype=bool)
    if edges.size:
        adj[edges[0], edges[1]] = True
        adj[edges[1], edges[0]] = True
    return adj


def playout_graph(adj, maker_to_move, playouts, seed=0, counter=0, g=0):
    """One graph: ``(scores f32 [n], value f32, tables i32 [n, 2], wins int)`` as the kernel defines them."""
    n = adj.shape[0]
    R = int(playouts)
    own = mover_sets(n, R, graph_base(seed, counter, g))
    free = np.ones(n, dtype=bool)
    free[:2] = False
    makers = own if maker_to_move else (~own & free[None, :])
    maker_wins = connected(adj, makers)
    mover_wins = maker_wins if maker_to_move else ~maker_wins
    wins = int(mover_wins.sum())
    tables = np.zeros((n, 2), dtype=np.int32)
    tables[:, 0] = own.sum(0)
    tables[:, 1] = (own & mover_wins[:, None]).sum(0)
    scores = (2 * tables[:, 1] - tables[:, 0]).astype(np.float32) / np.maximum(tables[:, 0], 1).astype(np.float32)
    value = np.float32(2 * wins - R) / np.float32(R)
    scores[:2] = value
    return scores.astype(np.float32), np.float32(value), tables, wins


def playout_batch(adjs, maker_to_move, playouts, seed=0, counter=0):
    """A batch (list of adjacency matrices): concatenated scores and tables, value [b], wins [b]."""
    out = [playout_graph(a, maker_to_move, playouts, seed, counter, g) for g, a in enumerate(adjs)]
    return (np.concatenate([o[0] for o in out]), np.array([o[1] for o in out], dtype=np.float32),
            np.concatenate([o[2] for o in out]), np.array([o[3] for o in out], dtype=np.int32))


def game_adjacency(game):
    """``(adj bool [n, n], backmap [n])`` of a RefGame's current reduced graph (rows 0, 1 = the terminals)."""
    x, ei, bm = game.observe()
    return dense_adjacency(x.shape[0], ei), bm


def pick(scores):
    """The first maximum over the non-terminal rows (the greedy pick of hexgnn_select_actions); -1 without one."""
    return int(np.argmax(scores[2:])) + 2 if scores.shape[0] > 2 else -1
