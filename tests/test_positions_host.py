"""CPU: the host side of position set-up (include/hexgnn.h: hexgnn_env_setup, hexgnn_board_values; gnn_hex_amd/positions.py).
The long-range task's stone lists are legal and undecided on the C env oracle for every board size and both colours and give the
graph sizes the reference's construction gives; the call descriptor agrees with its ctypes mirror field for field; the entry points
refuse bad arguments before anything is launched; the stone packing and the wrapper's colour parsing.  Nothing here touches a
GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

from positions_oracle import OracleGame

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1

# num_vertices() / num_edges() after the positive position, from the reference's construction run on the oracle
POSITIVE_SIZES = {(5, "m"): (11, 25), (5, "b"): (11, 14), (11, "m"): (83, 250), (11, "b"): (83, 206),
                  (16, "m"): (198, 630), (16, "b"): (198, 531), (25, "m"): (531, 1755), (25, "b"): (531, 1494)}


@pytest.mark.parametrize("defender", ["m", "b"])
@pytest.mark.parametrize("n", list(range(5, 26)))
def test_long_range_stones_on_the_oracle(hexref, n, defender):
    from gnn_hex_amd.positions import long_range_stones
    negative, positive = long_range_stones(n, defender)
    assert len(negative) == 4 * n - 6 and len(positive) == 4 * n - 4
    assert positive[:len(negative)] == negative
    attacker = "b" if defender == "m" else "m"
    for stones in (negative, positive):
        assert len({v for v, _, _ in stones}) == len(stones)
        assert all(2 <= v < n * n + 2 and c in ("m", "b") and rem is False for v, c, rem in stones)
        og = OracleGame(hexref, n)
        for j, (v, c, rem) in enumerate(stones):
            won = og.apply(v, c, rem)                       # raises for an illegal stone
            assert won is None, "stone %d decides the game" % j
        assert og.game.who_won() is None and og.moves == 0
        assert og.game.num_vertices() == n * n + 2 - len(stones)
    assert sum(c == defender for _, c, _ in negative) == n and sum(c == attacker for _, c, _ in negative) == 3 * n - 6
    # the cells: the defender's line, the attacker's border pairs and border line, the two stones of the positive position
    cell = (lambda r, c: r * n + c + 2) if defender == "m" else (lambda r, c: c * n + r + 2)
    assert {v for v, c, _ in negative if c == defender} == {cell(1, i) for i in range(n)}
    assert {v for v, c, _ in negative if c == attacker} == ({cell(i, 0) for i in range(2, n)} | {cell(i, n - 1) for i in range(2, n)}
                                                            | {cell(0, i) for i in range(1, n - 1)})
    assert positive[len(negative):] == [(cell(0, n - 1), attacker, False), (cell(2 + (n - 2) // 2, n // 2), defender, False)]
    assert og.game.num_vertices() == n * n + 2 - (4 * n - 4)
    if (n, defender) in POSITIVE_SIZES:
        assert (og.game.num_vertices(), og.game.num_edges()) == POSITIVE_SIZES[(n, defender)]
    # board cell 0, the move the task asks for, is still free in the positive position
    assert 2 in og.game.get_actions().tolist()


def test_refuses_small_boards_and_unknown_colours():
    from gnn_hex_amd.positions import long_range_stones
    with pytest.raises(ValueError):
        long_range_stones(2, "m")
    with pytest.raises(ValueError):
        long_range_stones(7, "turn")


def test_stone_packing_and_colour_parsing():
    from gnn_hex_amd import _lib
    from gnn_hex_amd.positions import stone
    header = open(os.path.join(ROOT, "include", "hexgnn.h")).read()
    m = re.search(r"#define\s+HEXGNN_STONE\(v,\s*colour,\s*remove_dc\)\s+\(\(v\)\s*\|\s*\(\(colour\)\s*<<\s*(\d+)\)\s*\|\s*"
                  r"\(\(remove_dc\)\s*<<\s*(\d+)\)\)", header)
    assert m and (int(m.group(1)), int(m.group(2))) == (16, 18)
    assert stone(2, "b") == 2 and stone(626, "m") == 626 | (1 << 16) and stone(40, "turn", True) == 40 | (2 << 16) | (1 << 18)
    assert stone(7, 1, 1) == stone(7, "m", True) and stone(7, 0) == stone(7, "b", False) and stone(7, 2) == stone(7, "turn")
    assert _lib.STONE_COLOURS == {"b": 0, "m": 1, "turn": 2}
    for bad in ("x", "M", 3, -1, None):
        with pytest.raises(ValueError):
            stone(5, bad)
    for bad in (-1, 65536, 1 << 20):
        with pytest.raises(ValueError):
            stone(bad, "m")


def test_setup_call_is_declared_exported_and_mirrored():
    from gnn_hex_amd import _lib
    header = open(os.path.join(ROOT, "include", "hexgnn.h")).read()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    assert re.search(r"\bint\s+hexgnn_env_setup\s*\(\s*hexgnn_env\s*\*\s*\w+\s*,\s*const\s+hexgnn_setup_call\s*\*", header)
    assert re.search(r"\bint\s+hexgnn_board_values\s*\(\s*int\s+b\s*,\s*int\s+hex_size\s*,\s*const\s+int\s*\*\s*gptr", header)
    for name in ("hexgnn_env_setup", "hexgnn_board_values"):
        assert hasattr(raw, name) and name in _lib.exported_symbols()
    assert _lib.lib().hexgnn_abi_version() == 8
    m = re.search(r"typedef\s+struct\s+hexgnn_setup_call\s*\{(.*?)\}\s*hexgnn_setup_call\s*;", header, re.S)
    kinds = {"size_t": ctypes.c_size_t, "int": ctypes.c_int}
    want = []
    for decl in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(";"):
        decl = decl.strip()
        if not decl:
            continue
        head = re.match(r"(?:const\s+)?(\w+)", decl)
        for item in decl[head.end():].split(","):
            name = re.search(r"(\w+)\s*$", item).group(1)
            want.append((name, ctypes.c_void_p if "*" in item else kinds[head.group(1)]))
    assert [(n, t) for n, t in _lib.SetupCall._fields_] == want
    assert [n for n, _ in want] == ["struct_bytes", "max_stones", "from_start", "maker_turn_start", "maker_turn_after", "stones",
                                    "count", "result", "applied", "adj_out", "alive_out", "side_out", "sizes_out"]
    about = header[header.index("position set-up and board-indexed evaluation"):header.index("hexgnn_setup_call {")]
    assert "no test depends on a time" in about and "shannon_node_switching_game.py:80-116" in about


def _full_call(_lib, p, snapshots):
    call = _lib.SetupCall(struct_bytes=ctypes.sizeof(_lib.SetupCall), max_stones=4, from_start=1, maker_turn_start=1,
                          maker_turn_after=-1, stones=p, count=p, result=p, applied=p)
    for name in ("adj_out", "alive_out", "side_out", "sizes_out")[:snapshots]:
        setattr(call, name, p)
    return call


def test_setup_refusals_that_need_no_device():
    from gnn_hex_amd import _lib
    L = _lib.lib()
    buf = (ctypes.c_char * 4096)()
    p = ctypes.addressof(buf)
    assert L.hexgnn_env_setup(None, ctypes.byref(_full_call(_lib, p, 0)), None) == EINVAL      # no env handle
    assert L.hexgnn_env_setup(p, None, None) == EINVAL                                         # no descriptor
    call = _full_call(_lib, p, 4)
    call.struct_bytes = ctypes.sizeof(_lib.SetupCall) - 8
    assert L.hexgnn_env_setup(p, ctypes.byref(call), None) == EINVAL      # another ABI's descriptor: checked before the handle is read
    assert L.hexgnn_env_setup(None, ctypes.byref(call), None) == EINVAL
    for name in ("stones", "count", "result", "applied"):                  # a missing required pointer
        call = _full_call(_lib, p, 0)
        setattr(call, name, None)
        assert L.hexgnn_env_setup(p, ctypes.byref(call), None) == EINVAL, name
    for bad in (0, -3):
        call = _full_call(_lib, p, 0)
        call.max_stones = bad
        assert L.hexgnn_env_setup(p, ctypes.byref(call), None) == EINVAL
    for bad in (-2, 2):
        call = _full_call(_lib, p, 0)
        call.maker_turn_after = bad
        assert L.hexgnn_env_setup(p, ctypes.byref(call), None) == EINVAL
    for given in (1, 2, 3):                                                # the snapshot outputs: all four or none
        assert L.hexgnn_env_setup(p, ctypes.byref(_full_call(_lib, p, given)), None) == EINVAL, given
    for leave_out in ("adj_out", "alive_out", "side_out", "sizes_out"):
        call = _full_call(_lib, p, 4)
        setattr(call, leave_out, None)
        assert L.hexgnn_env_setup(p, ctypes.byref(call), None) == EINVAL, leave_out


def test_board_values_refusals_that_need_no_device():
    from gnn_hex_amd import _lib
    L = _lib.lib()
    buf = (ctypes.c_char * 4096)()
    p = ctypes.addressof(buf)
    assert L.hexgnn_board_values(-1, 5, p, p, p, -5.0, p, p, None) == EINVAL
    assert L.hexgnn_board_values(2, 0, p, p, p, -5.0, p, p, None) == EINVAL
    assert L.hexgnn_board_values(2, 26, p, p, p, -5.0, p, p, None) == EINVAL
    for missing in range(4):                       # gptr, q, backmap, board; best may be NULL
        args = [p, p, p, p]
        args[missing] = None
        assert L.hexgnn_board_values(2, 5, args[0], args[1], args[2], -5.0, args[3], None, None) == EINVAL, missing
    assert L.hexgnn_board_values(0, 5, None, None, None, -5.0, None, None, None) == 0      # nothing to do


def test_wrapper_argument_checks_without_a_device():
    """Env_manager._pack_stones is pure host code: run it on an object that holds no env handle."""
    from gnn_hex_amd import _lib
    from gnn_hex_amd.multi_env_manager import Env_manager
    mgr = Env_manager.__new__(Env_manager)
    mgr.num_envs, mgr._h, mgr._base = 3, None, None
    arr, cnt = mgr._pack_stones([[(2, "m"), (3, "b", True)], [], [(9, "turn", True)]])
    assert arr.dtype == np.int32 and arr.shape == (3, 2) and cnt.tolist() == [2, 0, 1]
    assert arr.tolist() == [[_lib.stone(2, "m"), _lib.stone(3, "b", True)], [0, 0], [_lib.stone(9, "turn", True), 0]]
    arr, cnt = mgr._pack_stones([[], [], []])
    assert arr.shape == (3, 1) and cnt.tolist() == [0, 0, 0]              # L >= 1 for the kernel
    packed = np.array([[5, 6], [7, 0], [0, 0]], dtype=np.int32)
    arr, cnt = mgr._pack_stones(packed, [2, 1, 0])
    assert np.array_equal(arr, packed) and cnt.tolist() == [2, 1, 0] and cnt.dtype == np.int32
    assert mgr._pack_stones(packed)[1].tolist() == [2, 2, 2]
    for bad in ([[(2, "m")]], [[(2, "x")], [], []], [[(2,)], [], []]):
        with pytest.raises((ValueError, TypeError)):
            mgr._pack_stones(bad)
    with pytest.raises(ValueError):
        mgr._pack_stones(packed, [3, 0, 0])
    with pytest.raises(ValueError):
        mgr._pack_stones(packed[:2])
    with pytest.raises(ValueError):
        mgr._pack_stones([[], [], []], [0, 0, 0])
