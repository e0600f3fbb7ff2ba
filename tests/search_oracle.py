"""The PUCT search rule of include/hexgnn.h (hexgnn_search_*) restated on the host in float64 on ``oracle.env_ref.RefGame``
(shared by tests/test_search_host.py and tests/test_gpu_search.py).  A tree, one per game; written from the rule, it shares no
code with the kernels.  Two modes: FREE running (the oracle selects by the float64 first maximum) and TEACHER FORCED (it follows
a recorded path, is fed the recorded logits and values, and checks every selection step of the recording).

What is exact and what is not.  N and Ns are integers.  W is an fp32 field of the rule -- ``W(e) += v`` in fp32, one addition per
visit in visit order -- so the oracle adds in fp32 too and W is comparable bit for bit for ANY values (with the synthetic
evaluator's multiples of 1 / 256 every sum is exact anyway).  P and the selection scores are float64 here and fp32 there.

The tolerance of a teacher-forced selection step at a node with A edges and visit count Ns, eps = 2^-24 (half an fp32 ulp,
relative): the device's prior is w_j / S with w_j = expf(..) (a few eps), S a sum of A terms (at most A eps relative, all
terms positive) and one division (eps); the exploration term multiplies it by c_puct (eps), by sqrtf(Ns) (2 eps: the square
root and the product) and divides by 1 + N (eps); Q is one division (eps) and the score one addition (eps).  That is at most
A + 16 roundings of relative size eps on terms bounded by |Q| <= 1 and c_puct * P * sqrt(Ns) / (1 + N) <= c_puct * sqrt(Ns), so
one fp32 score is within (A + 16) eps (1 + c_puct sqrt(Ns)) of its float64 value, and the edge the device picked -- the maximum of
ITS scores -- lies no further below the float64 maximum than twice that:
    tol = 2 (A + 16) 2^-24 (1 + c_puct sqrt(Ns)).
A step whose recorded edge is not the float64 first maximum (but within tol) counts as AMBIGUOUS."""
import numpy as np

from playout_oracle import h32

LEAF, TERMINAL, SKIPPED = 0, 1, 2
EPS = 2.0 ** -24


def step_tolerance(num_edges, ns, c_puct):
    return 2.0 * (num_edges + 16) * EPS * (1.0 + c_puct * np.sqrt(float(ns)))


def softmax64(logits, temperature):
    z = np.asarray(logits, dtype=np.float64) / float(temperature)
    w = np.exp(z - z.max())
    return w / w.sum()


class Node:
    def __init__(self, moves, prior):
        self.moves = np.asarray(moves, dtype=np.int64)
        self.P = np.asarray(prior, dtype=np.float64)
        self.N = np.zeros(len(moves), dtype=np.int64)
        self.W = np.zeros(len(moves), dtype=np.float32)
        self.child = np.full(len(moves), -1, dtype=np.int64)
        self.Ns = 1


def scores64(node, c_puct):
    q = np.where(node.N > 0, node.W.astype(np.float64) / np.maximum(node.N, 1), 0.0)
    return q + c_puct * node.P * np.sqrt(float(node.Ns)) / (1.0 + node.N)


def scores32(node, c_puct):
    """The device's arithmetic restated in numpy fp32, every operation rounded on its own, in the header's order."""
    f = np.float32
    n = node.N.astype(f)
    q = np.where(node.N > 0, node.W / np.maximum(n, f(1)), f(0)).astype(f)
    u = ((f(c_puct) * node.P.astype(f)) * np.sqrt(f(node.Ns))) / (f(1) + n)
    return (q + u).astype(f)


def first_max(values):
    """First index of the maximum; a NaN is never picked; -1 when nothing compares."""
    best, arg = -np.inf, -1
    for i, v in enumerate(values):
        if v > best or (arg < 0 and v == best):
            best, arg = v, i
    return arg


class Tree:
    """The search tree of one game.  ``nodes[0]`` is the root (None until expanded); node numbers follow the expansion order,
    which is the device's slot order."""

    def __init__(self, root_game, c_puct=1.5, temperature=1.0, max_sims=None):
        self.root_game, self.c_puct, self.temperature, self.max_sims = root_game, float(c_puct), float(temperature), max_sims
        self.nodes = [None]
        self.applied = 0
        self.steps = self.ambiguous = 0
        self.slots = root_game.size ** 2

    # ---- one simulation -------------------------------------------------------------------------------
    def _walk(self, forced=None, select32=False):
        """From the root to a leaf / terminal: ``(game there, [(node, edge)], kind, terminal value)``.  ``forced``: the recorded
        edges to follow (each checked against the float64 scores), None: the float64 first maximum (``select32``: fp32)."""
        game = self.root_game.copy()
        node, path = 0, []
        while True:
            nd = self.nodes[node]
            if nd is None:
                return game, path, LEAF, 0.0
            s = scores64(nd, self.c_puct)
            arg = first_max(s)
            if forced is not None:
                assert len(path) < len(forced), "the recording stops at an expanded node %d" % node
                fnode, e = divmod(int(forced[len(path)]), self.slots)
                assert fnode == node, "step %d leaves node %d, the oracle stands on %d" % (len(path), fnode, node)
                assert 0 <= e < len(nd.moves)
                tol = step_tolerance(len(nd.moves), nd.Ns, self.c_puct)
                assert s[e] >= s[arg] - tol, "edge %d scores %.9g, the maximum %.9g, tol %.3g" % (e, s[e], s[arg], tol)
                self.steps += 1
                self.ambiguous += e != arg
            elif select32:
                e = first_max(scores32(nd, self.c_puct))
                self.steps += 1
                self.ambiguous += e != arg
            else:
                e = arg
            path.append((node, e))
            game.make_move(int(nd.moves[e]), True)
            won = game.who_won()
            if won is not None:                       # the side to move there: +1 if it has won, -1 if it has lost
                return game, path, TERMINAL, 1.0 if won == game.onturn else -1.0
            if nd.child[e] < 0:
                return game, path, LEAF, 0.0
            node = int(nd.child[e])

    def simulate(self, evaluate=None, forced=None, kind=None, logits=None, value=None, select32=False):
        """One simulation.  Free: ``evaluate(game, moves)`` -> (logits over the leaf's legal moves, value).  Teacher forced:
        ``forced`` = the recorded flat edges (node * size^2 + edge), ``kind`` the recorded kind, ``logits`` / ``value`` the
        recorded evaluation of a LEAF (None: ``evaluate`` is asked; ``last_eval`` keeps what was used).  Returns ``(kind, the leaf position, the moves of the path)``; a SKIPPED recording
        changes nothing."""
        if forced is not None and kind == SKIPPED:
            assert len(forced) == 0
            return SKIPPED, self.root_game.copy(), []
        if self.max_sims is not None and self.applied >= self.max_sims:
            assert forced is None, "the recording runs a simulation past max_sims"
            return SKIPPED, self.root_game.copy(), []
        game, path, k, v = self._walk(forced, select32)
        moves = [int(self.nodes[n].moves[e]) for n, e in path]
        if forced is not None:
            assert len(path) == len(forced) and k == kind, "kind %d after %d steps, recorded %d after %d" % (k, len(path), kind,
                                                                                                          len(forced))
        self.last_terminal = v if k == TERMINAL else 0.0
        if k == LEAF:
            acts = game.get_actions()
            if logits is None:
                logits, value = evaluate(game, moves)
            logits = np.asarray(logits)
            self.last_eval = (logits, value)
            assert len(logits) == len(acts), "%d logits for %d legal moves" % (len(logits), len(acts))
            if not (np.isfinite(logits).all() and np.isfinite(value)):
                return SKIPPED, game, moves                    # dropped: no expansion, no backup (the leaf was reached, though)
            new = Node(acts, softmax64(logits, self.temperature))
            if path:
                n, e = path[-1]
                self.nodes[n].child[e] = len(self.nodes)
                self.nodes.append(new)
            else:
                self.nodes[0] = new
            v = value
        v = np.float32(v)
        for n, e in reversed(path):
            nd = self.nodes[n]
            v = np.float32(-v)
            nd.N[e] += 1
            nd.W[e] = np.float32(nd.W[e] + v)
            nd.Ns += 1
        self.applied += 1
        return k, (game if k == LEAF else self.root_game.copy()), moves

    # ---- read-out -------------------------------------------------------------------------------------
    def root_counts(self):
        r = self.nodes[0]
        return (r.moves, r.N) if r is not None else (np.zeros(0, np.int64), np.zeros(0, np.int64))

    def best(self):
        r = self.nodes[0]
        return int(r.moves[first_max(r.N)]) if r is not None and len(r.moves) else -1

    def root_value(self):
        r = self.nodes[0]
        return float(r.W.astype(np.float64).sum() / (r.Ns - 1)) if r is not None and r.Ns > 1 else 0.0


# ---- the synthetic evaluator ----------------------------------------------------------------------------
def path_key(game_id, moves, seed=0):
    """lowbias32 of (seed, game id, the moves of the path in order)."""
    key = int(h32((int(seed) * 0x9e3779b9 + int(game_id)) & 0xFFFFFFFF))
    for v in moves:
        key = int(h32((key + int(v)) & 0xFFFFFFFF))
    return key


def synthetic(game_id, moves, num_actions, seed=0, uniform=False):
    """``(logits f32 [num_actions], value f32)``: logits multiples of 1 / 128 in [-4, 4) (``uniform``: all 0), the value a
    multiple of 1 / 256 in [-1, 1): every sum of such values over up to 2^15 visits is exact in fp32."""
    key = path_key(game_id, moves, seed)
    j = np.arange(num_actions, dtype=np.uint64)
    logits = ((h32(np.uint64(key) + np.uint64(1) + j) % np.uint64(1024)).astype(np.int64) - 512) / 128.0
    value = (int(h32(key ^ 0x5bd1e995)) % 512 - 256) / 256.0
    if uniform:
        logits = np.zeros(num_actions)
    return logits.astype(np.float32), np.float32(value)


def synthetic_evaluator(game_id, seed=0, uniform=False):
    return lambda game, moves: synthetic(game_id, moves, len(game.get_actions()), seed, uniform)


def peaked(game_id, moves, num_actions, seed=0):
    """The synthetic evaluation with +24 on logit ``path_key(game_id, moves, seed ^ 0x55) % num_actions`` (a multiple of 1 / 128
    below 32: exact in fp32) and the value divided by 32 (a multiple of 1 / 8192 in [-1 / 32, 1 / 32): every W sum stays exact).
    A prior this peaked under values this small makes PUCT follow one line and lengthen it by a ply per simulation: the tree
    is a chain with side branches, as deep as the game is long."""
    logits, value = synthetic(game_id, moves, num_actions, seed)
    logits[path_key(game_id, moves, seed ^ 0x55) % num_actions] += np.float32(24.0)
    return logits, np.float32(value / np.float32(32.0))


def peaked_evaluator(game_id, seed=0):
    return lambda game, moves: peaked(game_id, moves, len(game.get_actions()), seed)


# ---- positions ------------------------------------------------------------------------------------------
def response_tables(game):
    """(resp_maker, resp_breaker) int16 [nv] of a RefGame, -1 = none."""
    rm = np.array([-1 if game.get_response(v, True) is None else game.get_response(v, True) for v in range(game.nv)], np.int16)
    rb = np.array([-1 if game.get_response(v, False) is None else game.get_response(v, False) for v in range(game.nv)], np.int16)
    return rm, rb


def win_in_one_positions(env_ref, size, count=60):
    """Of ``random_position(size, 77 * size + g, g % 2 == 0)``, g < count: those with at least one winning and one losing move,
    as ``(g, game, winning vertices)``."""
    out = []
    for g in range(count):
        game = env_ref.random_position(size, 77 * size + g, g % 2 == 0)
        wins = []
        acts = game.get_actions()
        for v in acts:
            c = game.copy()
            c.make_move(int(v), True)
            if c.who_won() == game.onturn:
                wins.append(int(v))
        if wins and len(wins) < len(acts):
            out.append((g, game, wins))
    return out
