"""CPU: the entry points of the replay draw that is sized on the device (hexgnn_replay_offsets, hexgnn_per_sample_dev) refuse bad
arguments before anything is launched, and the header, the library and the ctypes table agree on them -- name, and number of
parameters.  (The backward over such a draw -- the n_live field of hexgnn_qnet_call -- is in test_qnet_call_host.py.)"""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("hexgnn_replay_offsets", "hexgnn_per_sample_dev")


def _host_ptr():
    """An address that passes a NULL check and is never dereferenced by an argument check."""
    buf = (ctypes.c_char * 256)()
    return buf, ctypes.addressof(buf)


def test_header_library_and_ctypes_table_agree_on_the_new_entry_points():
    from gnn_hex_amd import _lib
    header = open(os.path.join(ROOT, "include", "hexgnn.h")).read()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    _lib.lib()
    for name in NEW:
        m = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % name, header, re.S)
        assert m, "%s is not declared in include/hexgnn.h" % name
        params = [p for p in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",") if p.strip()]
        assert hasattr(raw, name), "libhexgnn.so does not export %s" % name
        assert name in _lib._SIGS and name in _lib.exported_symbols()
        res, args = _lib._SIGS[name]
        assert res is ctypes.c_int and len(args) == len(params), (name, len(args), len(params))
        # pointer parameters are void pointers in the table, the rest plain ints (size_t for the workspace size)
        for p, a in zip(params, args):
            if "*" in p or "hexgnn_stream_t" in p:
                assert a is ctypes.c_void_p, (name, p)
            elif "size_t" in p:
                assert a is ctypes.c_size_t, (name, p)
            else:
                assert a is ctypes.c_int, (name, p)
    # the plain form is still there, unchanged in length
    assert len(_lib._SIGS["hexgnn_per_sample_dev"][1]) == len(_lib._SIGS["hexgnn_per_sample"][1])


def test_replay_offsets_refuses_bad_arguments():
    from gnn_hex_amd import _lib
    L = _lib.lib()
    keep, p = _host_ptr()
    f = L.hexgnn_replay_offsets
    assert f(-1, p, 0, 128, p, p, p, p, None) == -1              # k < 0
    assert f(4, None, 0, 128, p, p, p, p, None) == -1            # no slots
    assert f(4, p, 0, 128, None, p, p, p, None) == -1            # no sizes
    assert f(4, p, 0, 128, p, None, p, p, None) == -1            # no node_off
    assert f(4, p, 0, 128, p, p, None, p, None) == -1            # no edge_off
    assert f(4, p, 0, 0, p, p, p, p, None) == -1                 # no slots in the ring
    del keep


def test_per_sample_dev_refuses_bad_arguments():
    from gnn_hex_amd import _lib
    L = _lib.lib()
    keep, p = _host_ptr()
    f = L.hexgnn_per_sample_dev
    assert f(64, None, 8, p, p, p, p, p, p, None) == -1          # no fill level
    assert f(64, p, 8, None, p, p, p, p, p, None) == -1          # no beta
    assert f(48, p, 8, p, p, p, p, p, p, None) == -1             # capacity not a power of two
    assert f(64, p, 0, p, p, p, p, p, p, None) == -1             # empty draw
    assert f(64, p, 8, p, None, p, p, p, p, None) == -1          # no uniforms
    assert f(64, p, 8, p, p, None, p, p, p, None) == -1 and f(64, p, 8, p, p, p, None, p, p, None) == -1
    assert f(64, p, 8, p, p, p, p, None, p, None) == -1 and f(64, p, 8, p, p, p, p, p, None, None) == -1
    del keep
