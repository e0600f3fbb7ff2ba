"""CPU: a search round of several leaves per game under virtual loss (include/hexgnn.h: hexgnn_search_round_*;
gnn_hex_amd/search.py ``TreeSearch(leaves=, virtual_loss=)``) on the host.  (1) the round oracle of tests/search_round_oracle.py
with K = 1 is search_oracle.Tree, (2) its fp32 restatement of the selection under in-flight counts agrees with float64,
(3) the properties of a round, (4) a win in one with K = 4, (5) declarations, mirrors, layout and every host refusal.  Nothing
here touches a GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

import search_oracle as so
import search_round_oracle as ro
from test_search_host import _synthetic_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EUNSUPPORTED = -1, -2


# ---- 1: K = 1 is the one-leaf search ----------------------------------------------------------------------------------
@pytest.mark.parametrize("vl", [1, 3])
def test_one_leaf_rounds_build_the_one_leaf_tree(hexref, vl):
    for size, gid, game, sims in _synthetic_cases(hexref):
        ev = so.synthetic_evaluator(gid, seed=size)
        a, b = so.Tree(game, c_puct=1.5), ro.RoundTree(game, c_puct=1.5, leaves=1, virtual_loss=vl)
        for _ in range(sims):
            a.simulate(ev)
        b.search(ev, sims)
        assert b.applied == a.applied == sims and len(a.nodes) == len(b.nodes) and b.kinds[ro.COLLISION] == 0
        for x, y in zip(a.nodes, b.nodes):             # the same nodes in the same slots
            assert np.array_equal(x.moves, y.moves) and np.array_equal(x.child, y.child)
            assert np.array_equal(x.N, y.N) and x.Ns == y.Ns and x.W.tobytes() == y.W.tobytes() and np.array_equal(x.P, y.P)


# ---- 2: the fp32 selection under in-flight counts against float64 -----------------------------------------------------
def test_fp32_round_selection_agrees_with_float64(hexref):
    """The check that the synthetic inputs keep the reference within the project's cap: at most 1 % of the selection steps of the
    fp32 restatement differ from the float64 first maximum, every one of them within the step tolerance (asserted in the walk)."""
    total = 0
    for K, vl in ((2, 1), (4, 1), (4, 3), (8, 1)):
        steps = ambiguous = 0
        for uniform in (False, True):
            for size, gid, game, sims in _synthetic_cases(hexref):
                tree = ro.RoundTree(game, c_puct=1.5, leaves=K, virtual_loss=vl)
                tree.search(so.synthetic_evaluator(gid, seed=size, uniform=uniform), sims, select32=True)
                steps += tree.steps
                ambiguous += tree.ambiguous
                assert tree.inflight_total() == 0
        print("K=%d vl=%d: %d ambiguous of %d steps" % (K, vl, ambiguous, steps))
        assert steps > 1500 and ambiguous <= 0.01 * steps
        total += steps
    assert total > 6000


def test_round_step_tolerance_formula():
    assert ro.round_step_tolerance(64, 1, 1.5) == 2 * 81 * 2.0 ** -24 * 2.5
    assert ro.round_step_tolerance(4, 16, 0.0) == 2 * 21 * 2.0 ** -24
    assert ro.round_step_tolerance(25, 9, 1.5) > so.step_tolerance(25, 9, 1.5)


# ---- 3: the properties of a round ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("size,K,vl", [(2, 8, 1), (2, 3, 2), (3, 2, 1), (3, 4, 1), (5, 4, 1), (5, 8, 3), (5, 3, 1)])
def test_properties_of_a_round(hexref, size, K, vl):
    for gid in range(3):
        game = hexref.RefGame(size) if gid == 0 or size == 2 else hexref.random_position(size, 900 * size + gid, gid % 2 == 0)
        tree = ro.RoundTree(game, c_puct=1.5, leaves=K, virtual_loss=vl)
        ev = so.synthetic_evaluator(gid, seed=size)
        applied = 0
        for r in range(12):
            was_open = tree.nodes[0] is None
            out = tree.round(ev)
            kinds = [d["kind"] for d in out]
            if was_open:                               # an unexpanded root: 1 LEAF and K - 1 COLLISIONs, all with empty paths
                assert kinds == [ro.LEAF] + [ro.COLLISION] * (K - 1) and all(d["path"] == [] for d in out)
            for i in range(K):
                for j in range(i):                     # pairwise different, unless a TERMINAL or a COLLISION is involved
                    if {kinds[i], kinds[j]} <= {ro.LEAF}:
                        assert out[i]["path"] != out[j]["path"]
                if kinds[i] == ro.COLLISION and out[i]["path"]:        # a collision waits on an earlier LEAF's edge
                    assert any(kinds[j] == ro.LEAF and out[j]["path"] == out[i]["path"] for j in range(i))
            assert tree.inflight_total() == 0
            applied += sum(d["applied"] for d in out)
            assert sum(d["applied"] for d in out) == sum(k in (ro.LEAF, ro.TERMINAL) for k in kinds)
            root = tree.nodes[0]
            assert tree.applied == applied and root.Ns - 1 == root.N.sum() == applied - 1
        # (the expansion of the root is a simulation without a root visit: Ns(root) - 1 = sum N = applied - 1)
        assert tree.kinds.sum() == 12 * K and tree.kinds[ro.SKIPPED] == 0 and tree.status == 0
        if size == 2:
            assert tree.kinds[ro.TERMINAL] > 0 and tree.kinds[ro.COLLISION] >= K - 1


def test_round_limits_and_drops(hexref):
    game = hexref.random_position(5, 4502, True)
    ev = so.synthetic_evaluator(1, seed=2)
    # max_sims = 10, K = 4: never more than 10 applied, the rest SKIPPED with bit 1
    tree = ro.RoundTree(game, max_sims=10, leaves=4)
    for r in range(3):
        tree.round(ev)
    assert tree.applied <= 10 and tree.applied == 1 + 4 + 4
    out = tree.round(ev)
    assert [d["kind"] for d in out] == [ro.LEAF, ro.SKIPPED, ro.SKIPPED, ro.SKIPPED] and tree.applied == 10 and tree.status == 1
    before = [(nd.N.copy(), nd.W.copy(), nd.Ns) for nd in tree.nodes]
    out = tree.round(ev)
    assert all(d["kind"] == ro.SKIPPED for d in out) and len(tree.nodes) == len(before)
    assert all(np.array_equal(nd.N, b[0]) and nd.W.tobytes() == b[1].tobytes() and nd.Ns == b[2] for nd, b in zip(tree.nodes, before))
    # round_leaves below K, a resting game
    tree = ro.RoundTree(game, leaves=4)
    tree.round(ev)
    assert [d["kind"] for d in tree.round(ev, round_leaves=2)] == [ro.LEAF, ro.LEAF, ro.SKIPPED, ro.SKIPPED] and tree.status == 0
    assert all(d["kind"] == ro.SKIPPED for d in tree.round(ev, active=False)) and tree.applied == 3
    # a non-finite value among the K leaves drops that simulation only
    def spoiled(gm, moves):
        logits, value = ev(gm, moves)
        return logits, (np.float32(np.nan) if len(moves) == 1 and moves[0] == spoil else value)
    tree = ro.RoundTree(game, leaves=4)
    tree.round(ev)
    probe = ro.RoundTree(game, leaves=4)
    probe.round(ev)
    spoil = probe.round(ev)[2]["moves"][0]
    out = tree.round(spoiled)
    assert [d["applied"] for d in out] == [True, True, False, True] and tree.status == 2 and tree.inflight_total() == 0
    assert tree.applied == 4 and len(tree.nodes) == 4


# ---- 4: a win in one ------------------------------------------------------------------------------------------------------
WIN_SIMS = lambda acts: 2 * acts + 8     # noqa: E731  fixed after the float64 oracle solved every listed position with it


def test_round_oracle_finds_a_win_in_one(hexref):
    """Uniform priors, value 0, c_puct 1.5, K = 4, virtual loss 1, 2 A + 8 simulations asked for: the most visited root move
    wins at once in all 55 positions of test_search_host's list."""
    total = 0
    for size in (3, 4, 5):
        for g, game, wins in so.win_in_one_positions(hexref, size):
            tree = ro.RoundTree(game, c_puct=1.5, leaves=4, virtual_loss=1)
            tree.search(lambda gm, moves: (np.zeros(len(gm.get_actions()), np.float32), np.float32(0)),
                        WIN_SIMS(len(game.get_actions())))
            assert tree.best() in wins, "Hex-%d position %d: picked %d, winning %s" % (size, g, tree.best(), wins)
            total += 1
    assert total == 55


# ---- 5: declarations, mirror, layout, refusals ------------------------------------------------------------------------------
def test_round_calls_are_declared_exported_and_mirrored():
    from gnn_hex_amd import _lib
    header = open(os.path.join(ROOT, "include", "hexgnn.h")).read()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    call = r"const\s+hexgnn_search_round_call\s*\*\s*\w+\s*,\s*hexgnn_stream_t\s+\w+"
    entry = {"hexgnn_search_round_backup": call,
             "hexgnn_search_round_descend": r"const\s+hexgnn_env\s*\*\s*\w+\s*,\s*hexgnn_env\s*\*\s*\w+\s*,\s*" + call}
    for name, args in entry.items():
        assert re.search(r"\bint\s+%s\s*\(\s*%s\s*\)" % (name, args), header), name
        assert hasattr(raw, name) and name in _lib.exported_symbols()
    assert re.search(r"\bsize_t\s+hexgnn_search_round_workspace_bytes\s*\(\s*int\s+\w+\s*,\s*int\s+\w+\s*,\s*int\s+\w+\s*,\s*int\s+\w+\s*\)",
                     header)
    assert hasattr(raw, "hexgnn_search_round_workspace_bytes") and "hexgnn_search_round_workspace_bytes" in _lib.exported_symbols()
    m = re.search(r"typedef\s+struct\s+hexgnn_search_round_call\s*\{(.*?)\}\s*hexgnn_search_round_call\s*;", header, re.S)
    names = [re.search(r"(\w+)\s*$", d.strip()).group(1) for d in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(";") if d.strip()]
    assert names == [n for n, _ in _lib.SearchRoundCall._fields_] == ["struct_bytes", "call", "leaves", "round_leaves", "virtual_loss"]
    assert [t for _, t in _lib.SearchRoundCall._fields_] == [ctypes.c_size_t, _lib.SearchCall, ctypes.c_int, ctypes.c_int, ctypes.c_int]
    for name, val in (("COLLISION", _lib.SEARCH_COLLISION), ("MAX_LEAVES", _lib.SEARCH_MAX_LEAVES),
                      ("MAX_VIRTUAL_LOSS", _lib.SEARCH_MAX_VIRTUAL_LOSS)):
        assert int(re.search(r"#define\s+HEXGNN_SEARCH_%s\s+(\d+)" % name, header).group(1)) == val
    assert _lib.SEARCH_COLLISION == ro.COLLISION == 3 and _lib.SEARCH_MAX_LEAVES == 64


def test_round_workspace_bytes_and_the_python_layout():
    from gnn_hex_amd import _lib
    from gnn_hex_amd.search import tree_layout
    L = _lib.lib()
    for G, size, sims, K in ((1, 2, 1, 1), (3, 5, 40, 4), (70, 8, 2, 3), (128, 11, 64, 16), (2, 12, 7, 64), (1, 25, 3, 2), (3, 2, 40, 8)):
        old, tree, old_total = tree_layout(G, size, sims)
        lay, tree2, total = tree_layout(G, size, sims, K)
        assert L.hexgnn_search_round_workspace_bytes(G, size, sims, K) == total, (G, size, sims, K)
        assert tree2 == tree and all(lay[name] == old[name] for name in old), "the one-leaf sections keep their offsets"
        assert list(lay)[-2:] == ["inflight", "round_moves"] and lay["inflight"][0] == old_total
        assert lay["inflight"][1:] == (np.int32, (G, sims + 1, size * size)) and lay["round_moves"][1:] == (np.uint16, (G, K, size * size))
        assert all(off % 256 == 0 for off, _, _ in lay.values()) and total > old_total
    for bad in ((-1, 5, 4, 2), (1, 1, 4, 2), (1, 26, 4, 2), (1, 5, 0, 2), (1, 5, 65536, 2), (1, 5, 4, 0), (1, 5, 4, 65), (0, 5, 4, 2)):
        assert L.hexgnn_search_round_workspace_bytes(*bad) == 0, bad


def _round_call(_lib, p, leaves=4, round_leaves=4, virtual_loss=1, struct_bytes=None, **kw):
    L = _lib.lib()
    call = _lib.SearchCall(struct_bytes=ctypes.sizeof(_lib.SearchCall), num_games=2, hex_size=5, max_sims=8, skip=2, c_puct=1.5,
                           temperature=1.0, fill=0.0, workspace=p, workspace_bytes=L.hexgnn_search_round_workspace_bytes(2, 5, 8, 4),
                           status=p, active=None, path=p, leaf=p, result=p, logits=p, offsets=p, value=p, gptr=p, scores=p,
                           counts=None, q=None, best=None)
    for k, v in kw.items():
        setattr(call, k, v)
    return _lib.SearchRoundCall(struct_bytes=ctypes.sizeof(_lib.SearchRoundCall) if struct_bytes is None else struct_bytes,
                                call=call, leaves=leaves, round_leaves=round_leaves, virtual_loss=virtual_loss)


def test_round_refusals_that_need_no_device():
    """Every refusal comes from the host checks, before anything is launched, in the header's order (the checks behind the
    handles' board sizes need real handles: tests/test_gpu_search_round.py)."""
    from gnn_hex_amd import _lib
    L = _lib.lib()
    buf = (ctypes.c_char * 4096)()
    p = ctypes.addressof(buf)
    fake = ctypes.c_void_p(p)
    entries = {"backup": lambda c: L.hexgnn_search_round_backup(c, None),
               "descend": lambda c: L.hexgnn_search_round_descend(fake, ctypes.c_void_p(p + 64), c, None)}
    for name, fn in entries.items():
        assert fn(None) == EINVAL, name
        assert fn(ctypes.byref(_round_call(_lib, p, struct_bytes=ctypes.sizeof(_lib.SearchRoundCall) - 8))) == EINVAL, name
        assert fn(ctypes.byref(_round_call(_lib, p, struct_bytes=ctypes.sizeof(_lib.SearchCall)))) == EINVAL, name
        # the checks of the one-leaf calls on `call`, in their order
        c = _round_call(_lib, p)
        c.call.struct_bytes -= 8
        assert fn(ctypes.byref(c)) == EINVAL, name
        for kw in (dict(num_games=-1), dict(hex_size=1), dict(max_sims=0), dict(max_sims=65536)):
            assert fn(ctypes.byref(_round_call(_lib, p, **kw))) == EINVAL, (name, kw)
        assert fn(ctypes.byref(_round_call(_lib, p, hex_size=26))) == EUNSUPPORTED, name
        assert fn(ctypes.byref(_round_call(_lib, p, hex_size=26, max_sims=0))) == EINVAL, name
        assert fn(ctypes.byref(_round_call(_lib, None, leaves=0, num_games=0, status=None, path=None, leaf=None, logits=None))) == 0
        for kw in (dict(workspace=None), dict(status=None)):
            assert fn(ctypes.byref(_round_call(_lib, p, **kw))) == EINVAL, (name, kw)
    # descend: the handles come first of its own checks (nothing of them is read before)
    c = ctypes.byref(_round_call(_lib, p))
    assert L.hexgnn_search_round_descend(None, fake, c, None) == EINVAL
    assert L.hexgnn_search_round_descend(fake, None, c, None) == EINVAL
    assert L.hexgnn_search_round_descend(fake, fake, c, None) == EINVAL
    # backup: everything behind the common checks
    bk = entries["backup"]
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        assert bk(ctypes.byref(_round_call(_lib, p, temperature=bad))) == EINVAL, bad
    for bad in (1, 3, -2):
        assert bk(ctypes.byref(_round_call(_lib, p, skip=bad))) == EINVAL, bad
    for bad in (0, -1, 65, 1 << 20):
        assert bk(ctypes.byref(_round_call(_lib, p, leaves=bad, round_leaves=0))) == EINVAL, bad
    for bad in (0, -1, 1025):
        assert bk(ctypes.byref(_round_call(_lib, p, virtual_loss=bad))) == EINVAL, bad
    for bad in (-1, 5):
        assert bk(ctypes.byref(_round_call(_lib, p, round_leaves=bad))) == EINVAL, bad
    for name in ("path", "leaf", "logits", "offsets"):
        assert bk(ctypes.byref(_round_call(_lib, p, **{name: None}))) == EINVAL, name
    need = L.hexgnn_search_round_workspace_bytes(2, 5, 8, 4)
    assert bk(ctypes.byref(_round_call(_lib, p, workspace_bytes=need - 1))) == EINVAL
    assert bk(ctypes.byref(_round_call(_lib, p, workspace_bytes=L.hexgnn_search_workspace_bytes(2, 5, 8)))) == EINVAL
    # a workspace sized for fewer leaves than the call names
    assert bk(ctypes.byref(_round_call(_lib, p, leaves=64, workspace_bytes=need))) == EINVAL


def test_python_arguments_without_a_device():
    from gnn_hex_amd import search
    from gnn_hex_amd.search_selfplay import SearchSelfPlay
    ev = search.UniformEvaluator()
    for kw in (dict(leaves=0), dict(leaves=65), dict(leaves=2.5), dict(virtual_loss=0), dict(virtual_loss=1025), dict(virtual_loss=1.5)):
        with pytest.raises(ValueError):
            search.TreeSearch(5, 2, 8, device="cpu", **kw)
        with pytest.raises(ValueError):
            search.SearchPlayer(ev, 80, **kw)
        with pytest.raises(ValueError):
            SearchSelfPlay(5, 2, ev, 80, None, **kw)
    with pytest.raises(ValueError, match="sims > leaves"):
        search.SearchPlayer(ev, 4, leaves=4)
    with pytest.raises(ValueError, match="sims > leaves"):
        SearchSelfPlay(5, 2, ev, 8, None, leaves=8)
    pl = search.SearchPlayer(ev, 16, leaves=4, virtual_loss=3)
    assert (pl.sims, pl.leaves, pl.virtual_loss) == (16, 4, 3)
    assert (search.SearchPlayer(ev, 1).leaves, search.SearchPlayer(ev, 1).virtual_loss) == (1, 1)
