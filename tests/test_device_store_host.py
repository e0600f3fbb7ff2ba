"""CPU: the host side of the device-side transition assembly and replay store (include/hexgnn.h: hexgnn_transitions_assemble,
hexgnn_replay_store_dev; gnn_hex_amd.multi_env_manager.DeviceTransitionFeed).  The symbols are declared and exported, the two call
descriptors agree with their ctypes mirrors field for field, both entry points refuse bad arguments before anything is launched
(every call here is wrong in exactly one way: a fully valid one would launch), and the reward-factor table the device multiplies
by is the host expression's bits."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1


def _header():
    return open(os.path.join(ROOT, "include", "hexgnn.h")).read()


def test_new_symbols_are_declared_and_exported():
    from gnn_hex_amd import _lib
    header = _header()
    L = _lib.lib()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name, struct in (("hexgnn_transitions_assemble", "hexgnn_transitions_call"), ("hexgnn_replay_store_dev", "hexgnn_store_call")):
        assert re.search(r"\bint\s+%s\s*\(\s*const\s+%s\s*\*" % (name, struct), header), name
        assert hasattr(raw, name) and name in _lib.exported_symbols()
    assert L.hexgnn_abi_version() == 8 and re.search(r"#define\s+HEXGNN_ABI_VERSION\s+8\b", header)
    # the header names the reference code the new entry points replace
    assert "graph_game/multi_env_manager.py:113-165" in header[header.index("rollout -> replay without the host"):]


@pytest.mark.parametrize("struct,cls", [("hexgnn_transitions_call", "TransitionsCall"), ("hexgnn_store_call", "StoreCall")])
def test_call_descriptors_agree_with_their_ctypes_mirrors(struct, cls):
    from gnn_hex_amd import _lib
    m = re.search(r"typedef\s+struct\s+%s\s*\{(.*?)\}\s*%s\s*;" % (struct, struct), _header(), re.S)
    assert m, struct
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
    got = [(n, t) for n, t in getattr(_lib, cls)._fields_]
    assert got == want


def _host_ptr(keep, nbytes=4096):
    buf = (ctypes.c_char * nbytes)()
    keep.append(buf)
    return ctypes.addressof(buf)


def _valid_assemble(keep):
    from gnn_hex_amd import _lib
    n_steps = (ctypes.c_int * 2)(1, 3)
    keep.append(n_steps)
    c = _lib.TransitionsCall(struct_bytes=ctypes.sizeof(_lib.TransitionsCall), H=21, P=5, k=6, n_count=2, prune_exploratories=1,
                             side0_maker=0, list_len=96, coef_stride=6, n_steps=ctypes.cast(n_steps, ctypes.c_void_p))
    for name in "result rank expl coef src_step env action reward next_step done count".split():
        setattr(c, name, _host_ptr(keep))
    return c


def _valid_store(keep):
    from gnn_hex_amd import _lib
    c = _lib.StoreCall(struct_bytes=ctypes.sizeof(_lib.StoreCall), capacity=100, nv=27, words=1, list_len=96, side=1, edge_limit=200,
                       H=21, P=5, k=6, start_nodes=27, start_edges=132)
    for name, kind in _lib.StoreCall._fields_:
        if kind is ctypes.c_void_p and name != "env_done":
            setattr(c, name, _host_ptr(keep))
    return c


def test_assemble_refuses_bad_arguments_before_touching_the_device():
    from gnn_hex_amd import _lib
    L = _lib.lib()
    keep = []
    assert L.hexgnn_transitions_assemble(None, None) == EINVAL
    bad = [("struct_bytes", 8), ("H", 0), ("H", -3), ("P", -1), ("P", 21), ("k", 0), ("k", -1), ("n_count", 0), ("n_count", 9),
           ("list_len", 0), ("list_len", -5), ("coef_stride", 0), ("coef_stride", 4)]          # 4 < 2 * max(n_steps)
    bad += [(name, None) for name in "n_steps result rank expl coef src_step env action reward next_step done count".split()]
    for field, value in bad:
        c = _valid_assemble(keep)
        setattr(c, field, value)
        assert L.hexgnn_transitions_assemble(ctypes.byref(c), None) == EINVAL, (field, value)
    c = _valid_assemble(keep)
    zero = (ctypes.c_int * 2)(1, 0)                       # a window length below 1
    c.n_steps = ctypes.cast(zero, ctypes.c_void_p)
    assert L.hexgnn_transitions_assemble(ctypes.byref(c), None) == EINVAL


def test_store_refuses_bad_arguments_before_touching_the_device():
    from gnn_hex_amd import _lib
    L = _lib.lib()
    keep = []
    assert L.hexgnn_replay_store_dev(None, None) == EINVAL
    bad = [("struct_bytes", 0), ("capacity", 0), ("capacity", 95), ("nv", 0), ("nv", -2), ("words", 2), ("list_len", 0),
           ("list_len", -1), ("side", 2), ("side", -1), ("edge_limit", -1), ("H", 0), ("P", -1), ("P", 21), ("k", 0),
           ("start_nodes", 0), ("start_nodes", 28), ("start_edges", -1)]                        # capacity 95 < list_len 96
    bad += [(name, None) for name, kind in _lib.StoreCall._fields_ if kind is ctypes.c_void_p and name != "env_done"]
    for field, value in bad:
        c = _valid_store(keep)
        setattr(c, field, value)
        assert L.hexgnn_replay_store_dev(ctypes.byref(c), None) == EINVAL, (field, value)


@pytest.mark.parametrize("gamma", [1, 0.97, 0.5])
def test_coef_table_is_the_host_expression(gamma):
    """Env_manager.assemble_transitions: coef = ((-(jj % 2)) * 2 + 1) * (float(gamma) ** (jj // 2)) over jj = arange(2 n_step)."""
    from gnn_hex_amd.multi_env_manager import transition_coef
    for n_steps in ([1], [2], [1, 3], [3, 1, 2]):
        table = transition_coef(gamma, n_steps)
        assert table.dtype == np.float64 and table.shape == (len(n_steps), 2 * max(n_steps))
        for ni, n_step in enumerate(n_steps):
            jj = np.arange(2 * n_step)
            want = ((-(jj % 2)) * 2 + 1) * (float(gamma) ** (jj // 2))
            assert table[ni, :2 * n_step].tobytes() == want.astype(np.float64).tobytes()
            assert not table[ni, 2 * n_step:].any()
