"""CPU: the PUCT search rule (include/hexgnn.h: hexgnn_search_*; gnn_hex_amd/search.py) on the host.
(a) the oracle of tests/search_oracle.py finds a win in one, (b) an fp32 restatement of the selection agrees with float64 on the
synthetic evaluator, (c) the entry points' declarations, the ctypes mirror, the workspace layout and the argument checks in their
documented order, (d) the python objects' refusals.  Nothing here touches a GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

import search_oracle as so

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EUNSUPPORTED = -1, -2


def test_oracle_finds_a_win_in_one(hexref):
    """(a) uniform priors, value 0, c_puct 1.5, A + 2 simulations: the most visited root move wins at once, in all 55 positions
    with at least one winning and one other move among 60 random positions per size 3, 4, 5."""
    total = 0
    for size in (3, 4, 5):
        for g, game, wins in so.win_in_one_positions(hexref, size):
            tree = so.Tree(game, c_puct=1.5)
            acts = len(game.get_actions())
            for _ in range(acts + 2):
                tree.simulate(lambda gm, moves: (np.zeros(len(gm.get_actions()), np.float32), np.float32(0)))
            assert tree.best() in wins, "Hex-%d position %d: picked %d, winning %s" % (size, g, tree.best(), wins)
            moves, counts = tree.root_counts()
            assert counts.sum() == acts + 1 and tree.nodes[0].Ns == acts + 2
            total += 1
    assert total == 55


def _synthetic_cases(hexref):
    start = hexref.RefGame(3)
    yield 3, 0, start, 40
    for size, sims in ((5, 64), (8, 48), (9, 40)):
        for g in range(4):
            yield size, g + 1, hexref.random_position(size, 500 * size + g, g % 2 == 0), sims


def test_fp32_selection_agrees_with_float64(hexref):
    """(b) the fp32 arithmetic of the header, restated in numpy, against the float64 first maximum on the synthetic evaluator:
    at most 1 % of the selection steps differ (a prototype gave none), and a differing step is within the step tolerance."""
    steps = ambiguous = 0
    for uniform in (False, True):
        for size, gid, game, sims in _synthetic_cases(hexref):
            tree = so.Tree(game, c_puct=1.5)
            ev = so.synthetic_evaluator(gid, seed=size, uniform=uniform)
            for _ in range(sims):
                tree.simulate(ev, select32=True)
            # the fp32 walk can be replayed teacher-forced: every step within the tolerance
            steps += tree.steps
            ambiguous += tree.ambiguous
            for nd in tree.nodes:
                assert nd is None or (nd.Ns == 1 + nd.N.sum() and abs(nd.P.sum() - 1) < 1e-12)
    print("fp32 vs float64 selection: %d ambiguous of %d steps" % (ambiguous, steps))
    assert steps > 1500 and ambiguous <= 0.01 * steps


def test_teacher_forcing_checks_a_recording(hexref):
    """The teacher-forced mode follows a free run's own recording without complaint and refuses a wrong edge."""
    game = hexref.random_position(5, 2501, True)
    free, forced = so.Tree(game), so.Tree(game)
    ev = so.synthetic_evaluator(7)
    for s in range(30):
        kind, leaf, moves = free.simulate(ev)
        # rebuild the flat path of that simulation from the moves
        node, flat = 0, []
        for v in moves:
            nd = forced.nodes[node]
            e = int(np.nonzero(nd.moves == v)[0][0])
            flat.append(node * 25 + e)
            node = int(nd.child[e])
        logits, value = so.synthetic(7, moves, len(leaf.get_actions())) if kind == so.LEAF else (None, None)
        k2, leaf2, moves2 = forced.simulate(forced=flat, kind=kind, logits=logits, value=value)
        assert k2 == kind and moves2 == moves
    assert forced.ambiguous == 0 and forced.steps > 30 and free.steps == 0
    for a, b in zip(free.nodes, forced.nodes):
        assert (a.N == b.N).all() and a.W.tobytes() == b.W.tobytes() and a.Ns == b.Ns
    # a wrong edge at the root: far below the maximum
    root = forced.nodes[0]
    worst = int(np.argmin(so.scores64(root, 1.5)))
    with pytest.raises(AssertionError):
        forced.simulate(forced=[worst], kind=so.LEAF, logits=np.zeros(24, np.float32), value=np.float32(0))


def test_step_tolerance_formula():
    assert so.step_tolerance(64, 1, 1.5) == 2 * 80 * 2.0 ** -24 * 2.5
    assert so.step_tolerance(4, 16, 0.0) == 2 * 20 * 2.0 ** -24


# ---- (c) declarations, mirror, layout, refusals ----------------------------------------------------------
ENTRY = {"hexgnn_search_reset": r"const\s+hexgnn_search_call\s*\*\s*\w+\s*,\s*hexgnn_stream_t\s+\w+",
         "hexgnn_search_backup": r"const\s+hexgnn_search_call\s*\*\s*\w+\s*,\s*hexgnn_stream_t\s+\w+",
         "hexgnn_search_root": r"const\s+hexgnn_search_call\s*\*\s*\w+\s*,\s*hexgnn_stream_t\s+\w+",
         "hexgnn_search_descend": r"const\s+hexgnn_env\s*\*\s*\w+\s*,\s*hexgnn_env\s*\*\s*\w+\s*,\s*const\s+hexgnn_search_call\s*\*\s*\w+"
                                  r"\s*,\s*hexgnn_stream_t\s+\w+"}


def test_search_calls_are_declared_exported_and_mirrored():
    from gnn_hex_amd import _lib
    header = open(os.path.join(ROOT, "include", "hexgnn.h")).read()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name, args in ENTRY.items():
        assert re.search(r"\bint\s+%s\s*\(\s*%s\s*\)" % (name, args), header), name
        assert hasattr(raw, name) and name in _lib.exported_symbols()
    assert re.search(r"\bsize_t\s+hexgnn_search_workspace_bytes\s*\(\s*int\s+\w+\s*,\s*int\s+\w+\s*,\s*int\s+\w+\s*\)", header)
    assert hasattr(raw, "hexgnn_search_workspace_bytes") and "hexgnn_search_workspace_bytes" in _lib.exported_symbols()
    assert _lib.lib().hexgnn_abi_version() == 8
    m = re.search(r"typedef\s+struct\s+hexgnn_search_call\s*\{(.*?)\}\s*hexgnn_search_call\s*;", header, re.S)
    kinds = {"size_t": ctypes.c_size_t, "int": ctypes.c_int, "float": ctypes.c_float, "void": None}
    want = []
    for decl in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(";"):
        decl = decl.strip()
        if not decl:
            continue
        head = re.match(r"(?:const\s+)?(\w+)", decl)
        for item in decl[head.end():].split(","):
            name = re.search(r"(\w+)\s*$", item).group(1)
            want.append((name, ctypes.c_void_p if "*" in item else kinds[head.group(1)]))
    assert [(n, t) for n, t in _lib.SearchCall._fields_] == want
    assert [n for n, _ in want] == ["struct_bytes", "num_games", "hex_size", "max_sims", "skip", "c_puct", "temperature", "fill",
                                    "workspace", "workspace_bytes", "status", "active", "path", "leaf", "result", "logits",
                                    "offsets", "value", "gptr", "scores", "counts", "q", "best"]
    for name, val in (("MAX_SIMS", _lib.SEARCH_MAX_SIMS), ("REC", _lib.SEARCH_REC), ("LEAF", _lib.SEARCH_LEAF),
                      ("TERMINAL", _lib.SEARCH_TERMINAL), ("SKIPPED", _lib.SEARCH_SKIPPED)):
        assert int(re.search(r"#define\s+HEXGNN_SEARCH_%s\s+(\d+)" % name, header).group(1)) == val
    assert (_lib.SEARCH_LEAF, _lib.SEARCH_TERMINAL, _lib.SEARCH_SKIPPED) == (so.LEAF, so.TERMINAL, so.SKIPPED)


def test_workspace_bytes_and_the_python_layout():
    from gnn_hex_amd import _lib
    from gnn_hex_amd.search import tree_layout
    L = _lib.lib()
    for G, size, sims in ((1, 2, 1), (3, 5, 40), (70, 8, 2), (128, 11, 64), (2, 12, 7), (1, 25, 3)):
        lay, tree, total = tree_layout(G, size, sims)
        assert L.hexgnn_search_workspace_bytes(G, size, sims) == total, (G, size, sims)
        assert 0 < tree < total and all(off % 256 == 0 for off, _, _ in lay.values())
        assert lay["score"][0] == tree and list(lay)[:8] == ["ns", "ne", "cnt", "P", "W", "N", "child", "vertex"]
    assert L.hexgnn_search_workspace_bytes(0, 5, 4) == tree_layout(0, 5, 4)[2] == 0          # no games: nothing to hold
    for bad in ((-1, 5, 4), (1, 1, 4), (1, 26, 4), (1, 5, 0), (1, 5, 65536)):
        assert L.hexgnn_search_workspace_bytes(*bad) == 0, bad


def _call(_lib, p, **kw):
    need = _lib.lib().hexgnn_search_workspace_bytes(2, 5, 8)
    call = _lib.SearchCall(struct_bytes=ctypes.sizeof(_lib.SearchCall), num_games=2, hex_size=5, max_sims=8, skip=2, c_puct=1.5,
                           temperature=1.0, fill=0.0, workspace=p, workspace_bytes=need, status=p, active=None, path=p, leaf=p,
                           result=p, logits=p, offsets=p, value=p, gptr=p, scores=p, counts=None, q=None, best=None)
    for k, v in kw.items():
        setattr(call, k, v)
    return call


def test_search_refusals_that_need_no_device():
    """Every refusal comes from the host checks, before anything is launched, in the header's order."""
    from gnn_hex_amd import _lib
    L = _lib.lib()
    buf = (ctypes.c_char * 4096)()
    p = ctypes.addressof(buf)
    fake = ctypes.c_void_p(p)
    entries = {"reset": lambda c: L.hexgnn_search_reset(c, None), "backup": lambda c: L.hexgnn_search_backup(c, None),
               "root": lambda c: L.hexgnn_search_root(c, None),
               "descend": lambda c: L.hexgnn_search_descend(fake, ctypes.c_void_p(p + 64), c, None)}
    for name, fn in entries.items():
        assert fn(None) == EINVAL, name
        assert fn(ctypes.byref(_call(_lib, p, struct_bytes=ctypes.sizeof(_lib.SearchCall) - 8))) == EINVAL, name
        assert fn(ctypes.byref(_call(_lib, p, struct_bytes=0))) == EINVAL, name
        for kw in (dict(num_games=-1), dict(hex_size=1), dict(max_sims=0), dict(max_sims=65536)):
            assert fn(ctypes.byref(_call(_lib, p, **kw))) == EINVAL, (name, kw)
        assert fn(ctypes.byref(_call(_lib, p, hex_size=26))) == EUNSUPPORTED, name
        assert fn(ctypes.byref(_call(_lib, p, hex_size=26, max_sims=0))) == EINVAL, name           # the order of the checks
        assert fn(ctypes.byref(_call(_lib, None, num_games=0, status=None, path=None, leaf=None, logits=None, gptr=None))) == 0
        assert fn(ctypes.byref(_call(_lib, p, num_games=0, hex_size=26))) == EUNSUPPORTED, name
        for kw in (dict(workspace=None), dict(status=None), dict(workspace_bytes=_call(_lib, p).workspace_bytes - 1)):
            assert fn(ctypes.byref(_call(_lib, p, **kw))) == EINVAL, (name, kw)
    # descend: the handles come first of its own checks (nothing of them is read before)
    c = ctypes.byref(_call(_lib, p))
    assert L.hexgnn_search_descend(None, fake, c, None) == EINVAL
    assert L.hexgnn_search_descend(fake, None, c, None) == EINVAL
    assert L.hexgnn_search_descend(fake, fake, c, None) == EINVAL
    # backup
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        assert L.hexgnn_search_backup(ctypes.byref(_call(_lib, p, temperature=bad)), None) == EINVAL, bad
    for bad in (1, 3, -2):
        assert L.hexgnn_search_backup(ctypes.byref(_call(_lib, p, skip=bad)), None) == EINVAL, bad
    for name in ("path", "leaf", "logits", "offsets"):
        assert L.hexgnn_search_backup(ctypes.byref(_call(_lib, p, **{name: None})), None) == EINVAL, name
    assert L.hexgnn_search_backup(ctypes.byref(_call(_lib, p, temperature=0.0, workspace=None)), None) == EINVAL
    # root
    for name in ("gptr", "scores"):
        assert L.hexgnn_search_root(ctypes.byref(_call(_lib, p, **{name: None})), None) == EINVAL, name


# ---- (d) python objects ------------------------------------------------------------------------------------
def test_python_objects_without_a_device():
    from gnn_hex_amd import search
    from gnn_hex_amd.arena import DeviceArena, _is_search
    with pytest.raises(TypeError):
        search.SearchPlayer(object(), 8)
    with pytest.raises(ValueError):
        search.SearchPlayer(search.UniformEvaluator(), 0)
    pl = search.SearchPlayer(search.UniformEvaluator(), 8, c_puct=2.0, prior_temperature=0.5)
    assert (pl.sims, pl.c_puct, pl.prior_temperature) == (8, 2.0, 0.5) and _is_search(pl) and not _is_search("random")
    assert DeviceArena._check_player(pl) is False
    pl.status()
    with pytest.raises(NotImplementedError):
        search.PolicyValueEvaluator(object())
    with pytest.raises(NotImplementedError):
        search.QEvaluator(lambda *a, **k: None, value="mean")
    with pytest.raises(TypeError):
        search.QEvaluator("random")
