"""The rule of a search ROUND -- K descents per game under a virtual loss, one backup (include/hexgnn.h: hexgnn_search_round_*) --
restated on the host on top of tests/search_oracle.py (shared by tests/test_search_round_host.py and
tests/test_gpu_search_round.py).  ``RoundTree`` extends ``search_oracle.Tree`` with the in-flight counts I(e), the COLLISION kind
and ``round()``; written from the rule, it shares no code with the kernels.  Modes as there: FREE running in float64 (or by the
fp32 restatement, ``select32``) and TEACHER FORCED (it follows K recorded paths, is fed the recorded evaluations and checks every
selection step of the recording).

The rule in short.  Selection at a node under the in-flight counts, vl the integer virtual loss:
    Iv = vl I;  N' = N + Iv;  W' = W - Iv;  Ns' = Ns + vl sum_e I(e);  Q = N' > 0 ? W' / N' : 0;
    score = Q + c_puct P sqrt(Ns') / (1 + N'),  first maximum in edge order.
Descent k ends as LEAF (edge without child, I(e) == 0; or the unexpanded root, first time in the round), COLLISION (edge without
child on which an earlier descent of the round waits; or the unexpanded root again), TERMINAL, or SKIPPED (the game rests, k >=
round_leaves, or applied + the LEAF / TERMINAL descents of the round so far >= max_sims).  Then I(e) += 1 along its path unless
SKIPPED.  The backup expands / backs up LEAFs and TERMINALs in k order exactly as one simulation of ``search_oracle.Tree`` and
sets every I on the K paths to 0.

What is exact and what is not: as in search_oracle.  N, Ns and I are integers, W is an fp32 field added to in fp32 in visit order;
P and the scores are float64 here and fp32 on the device.

The tolerance of a teacher-forced selection step.  search_oracle derives (A + 16) roundings of relative size eps = 2^-24 for
one fp32 score at a node with A edges: the prior (expf, the sum of A terms, one division), the exploration term (c_puct, the
square root and its product, the division by 1 + N), Q's division and the final addition.  A round adds ONE rounding: W' = W -
(float) Iv is one fp32 subtraction ((float) Iv, N' and Ns' are exact: integers far below 2^24), so A + 17.  The terms stay
bounded as before: every backed-up value lies in [-1, 1], so |W| <= N and |W'| = |W - Iv| <= N + Iv = N', hence |Q| <= 1, and
c_puct P sqrt(Ns') / (1 + N') <= c_puct sqrt(Ns').  One fp32 score is therefore within (A + 17) eps (1 + c_puct sqrt(Ns')) of its
float64 value and the edge the device picked lies no further below the float64 maximum than twice that:
    tol = 2 (A + 17) 2^-24 (1 + c_puct sqrt(Ns')),  Ns' the in-flight-adjusted count.
A step whose recorded edge is not the float64 first maximum (but within tol) counts as AMBIGUOUS."""
import numpy as np

import search_oracle as so
from search_oracle import LEAF, SKIPPED, TERMINAL, first_max  # noqa: F401  (re-exported for the tests)

COLLISION = 3
KIND_NAMES = {LEAF: "LEAF", TERMINAL: "TERMINAL", SKIPPED: "SKIPPED", COLLISION: "COLLISION"}


def round_step_tolerance(num_edges, ns_adjusted, c_puct):
    return 2.0 * (num_edges + 17) * so.EPS * (1.0 + c_puct * np.sqrt(float(ns_adjusted)))


def inflight(nd):
    """The in-flight counts of a node (created on first use: search_oracle.Node knows nothing of them)."""
    if not hasattr(nd, "I"):
        nd.I = np.zeros(len(nd.moves), dtype=np.int64)
    return nd.I


def round_scores64(nd, c_puct, vl):
    iv = vl * inflight(nd)
    n = nd.N + iv
    w = nd.W.astype(np.float64) - iv
    ns = nd.Ns + vl * int(inflight(nd).sum())
    q = np.where(n > 0, w / np.maximum(n, 1), 0.0)
    return q + c_puct * nd.P * np.sqrt(float(ns)) / (1.0 + n), ns


def round_scores32(nd, c_puct, vl):
    """The device's arithmetic restated in numpy fp32, every operation rounded on its own, in the header's order."""
    f = np.float32
    iv = vl * inflight(nd)
    n = nd.N + iv
    w = (nd.W - iv.astype(f)).astype(f)
    ns = nd.Ns + vl * int(inflight(nd).sum())
    nf = n.astype(f)
    q = np.where(n > 0, w / np.maximum(nf, f(1)), f(0)).astype(f)
    u = ((f(c_puct) * nd.P.astype(f)) * np.sqrt(f(ns))) / (f(1) + nf)
    return (q + u).astype(f)


class RoundTree(so.Tree):
    """``search_oracle.Tree`` with rounds of ``leaves`` descents under ``virtual_loss``.  ``status`` collects the bits the
    device would OR into its status word (1: a descent past max_sims, 2: a non-finite evaluation dropped a simulation);
    ``kinds`` counts the descents of every kind."""

    def __init__(self, root_game, c_puct=1.5, temperature=1.0, max_sims=None, leaves=1, virtual_loss=1):
        super().__init__(root_game, c_puct, temperature, max_sims)
        self.leaves, self.vl = int(leaves), int(virtual_loss)
        self.status = 0
        self.kinds = np.zeros(4, dtype=np.int64)

    # ---- one descent ----------------------------------------------------------------------------------
    def _walk_round(self, root_waits, forced=None, select32=False):
        game = self.root_game.copy()
        node, path = 0, []
        while True:
            nd = self.nodes[node]
            if nd is None:                             # only the root is ever met unexpanded
                return game, path, (COLLISION if root_waits else LEAF), 0.0
            s, ns = round_scores64(nd, self.c_puct, self.vl)
            arg = first_max(s)
            if forced is not None:
                assert len(path) < len(forced), "the recording stops at an expanded node %d" % node
                fnode, e = divmod(int(forced[len(path)]), self.slots)
                assert fnode == node, "step %d leaves node %d, the oracle stands on %d" % (len(path), fnode, node)
                assert 0 <= e < len(nd.moves)
                tol = round_step_tolerance(len(nd.moves), ns, self.c_puct)
                assert s[e] >= s[arg] - tol, "edge %d scores %.9g, the maximum %.9g, tol %.3g" % (e, s[e], s[arg], tol)
                self.steps += 1
                self.ambiguous += e != arg
            elif select32:
                e = first_max(round_scores32(nd, self.c_puct, self.vl))
                tol = round_step_tolerance(len(nd.moves), ns, self.c_puct)
                assert s[e] >= s[arg] - tol, "fp32 pick %d scores %.9g, the maximum %.9g, tol %.3g" % (e, s[e], s[arg], tol)
                self.steps += 1
                self.ambiguous += e != arg
            else:
                e = arg
            path.append((node, e))
            game.make_move(int(nd.moves[e]), True)
            won = game.who_won()
            if won is not None:
                return game, path, TERMINAL, 1.0 if won == game.onturn else -1.0
            if nd.child[e] < 0:
                return game, path, (COLLISION if inflight(nd)[e] > 0 else LEAF), 0.0
            node = int(nd.child[e])

    # ---- one round ------------------------------------------------------------------------------------
    def round(self, evaluate=None, forced=None, kinds=None, evals=None, round_leaves=None, active=True, select32=False):
        """One round.  Free: ``evaluate(game, moves)`` -> (logits over the leaf's legal moves, value).  Teacher forced:
        ``forced[k]`` = the recorded flat edges of descent k, ``kinds[k]`` its recorded kind, ``evals[k]`` = (logits, value)
        of a recorded LEAF or None (``evaluate`` is then asked).  Returns per descent ``dict(kind, game, moves, path, terminal,
        eval, applied)``: ``game`` the position the leaf env must hold (the root's for every kind but LEAF), ``eval`` the
        (logits, value) a LEAF was given, ``applied`` whether the backup applied it."""
        K = self.leaves
        n_round = K if round_leaves is None else int(round_leaves)
        assert 0 <= n_round <= K
        out, sims, root_waits = [], 0, False
        for k in range(K):
            rec = dict(kind=SKIPPED, game=self.root_game.copy(), moves=[], path=[], terminal=0.0, eval=None, applied=False)
            out.append(rec)
            skip = not active or k >= n_round
            if not skip and self.max_sims is not None and self.applied + sims >= self.max_sims:
                skip = True
                self.status |= 1
            if skip:
                if forced is not None:
                    assert kinds[k] == SKIPPED and len(forced[k]) == 0, "descent %d: recorded %s, the oracle skips" % (
                        k, KIND_NAMES.get(int(kinds[k]), kinds[k]))
                self.kinds[SKIPPED] += 1
                continue
            if forced is not None:
                assert kinds[k] != SKIPPED, "descent %d is recorded as SKIPPED, the oracle walks" % k
            game, path, kind, tval = self._walk_round(root_waits, None if forced is None else forced[k], select32)
            if forced is not None:
                assert len(path) == len(forced[k]) and kind == kinds[k], "descent %d: %s after %d steps, recorded %s after %d" % (
                    k, KIND_NAMES[kind], len(path), KIND_NAMES.get(int(kinds[k]), kinds[k]), len(forced[k]))
            rec.update(kind=kind, path=path, moves=[int(self.nodes[n].moves[e]) for n, e in path], terminal=tval)
            if kind == LEAF:
                rec["game"] = game
            sims += kind in (LEAF, TERMINAL)
            root_waits |= kind == LEAF and not path
            for n, e in path:                          # LEAF, TERMINAL and COLLISION alike
                inflight(self.nodes[n])[e] += 1
            self.kinds[kind] += 1
        # the backup, in k order
        for k, rec in enumerate(out):
            if rec["kind"] == LEAF:
                acts = rec["game"].get_actions()
                given = evals[k] if evals is not None and evals[k] is not None else evaluate(rec["game"], rec["moves"])
                logits, value = np.asarray(given[0]), given[1]
                rec["eval"] = (logits, value)
                assert len(logits) == len(acts), "%d logits for %d legal moves" % (len(logits), len(acts))
                if not (np.isfinite(logits).all() and np.isfinite(value)):
                    self.status |= 2                   # dropped: no expansion, no backup
                    continue
                new = so.Node(acts, so.softmax64(logits, self.temperature))
                if rec["path"]:
                    n, e = rec["path"][-1]
                    assert self.nodes[n].child[e] < 0, "two LEAFs of one round on one edge"
                    self.nodes[n].child[e] = len(self.nodes)
                    self.nodes.append(new)
                else:
                    assert self.nodes[0] is None
                    self.nodes[0] = new
                v = np.float32(value)
            elif rec["kind"] == TERMINAL:
                v = np.float32(rec["terminal"])
            else:
                continue
            for n, e in reversed(rec["path"]):
                nd = self.nodes[n]
                v = np.float32(-v)
                nd.N[e] += 1
                nd.W[e] = np.float32(nd.W[e] + v)
                nd.Ns += 1
            self.applied += 1
            rec["applied"] = True
        for rec in out:                                # set, not decremented
            for n, e in rec["path"]:
                inflight(self.nodes[n])[e] = 0
        return out

    def inflight_total(self):
        return sum(int(inflight(nd).sum()) for nd in self.nodes if nd is not None)

    def search(self, evaluate, sims, select32=False):
        """``TreeSearch.simulate(sims)``: ceil(sims / K) rounds of min(K, sims left) descents."""
        left = int(sims)
        while left > 0:
            n = min(self.leaves, left)
            self.round(evaluate, round_leaves=n, select32=select32)
            left -= n


def flat_paths(tree, descents):
    """The recording a device would leave of ``RoundTree.round``'s descents: ``(forced, kinds)``."""
    return [[n * tree.slots + e for n, e in d["path"]] for d in descents], [d["kind"] for d in descents]
