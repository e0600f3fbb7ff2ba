"""CPU: the layer-major stack's descriptor (hexgnn_sage_stack_call, include/hexgnn.h) and its ctypes mirror agree field for field,
and the two entry points that read it refuse bad descriptors with the codes the positional entry points they replaced gave --
before anything is launched.  Device pointers are addresses no argument check dereferences; the HOST arrays the checks do read
(per-layer pointers) are real."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EUNSUPPORTED, EWORKSPACE = -1, -2, -3
LINEAR_LAST, DY_IN_PLACE = 1, 2
N, HIDDEN, LAYERS = 640, 110, 3
GONE = ("hexgnn_sage_stack_forward_blocks", "hexgnn_sage_stack_forward_groups", "hexgnn_sage_stack_backward_tap",
        "hexgnn_sage_stack_backward_blocks", "hexgnn_sage_stack_backward_groups", "hexgnn_sage_norm_stack_forward_live")

_ONE = 16                                                 # passes a NULL check, is never dereferenced
_LAYER_PTRS = (ctypes.c_void_p * 8)(*[_ONE] * 8)          # a HOST array of per-layer device pointers, every entry set
_TABLE = (ctypes.c_int * 600)()                           # stands in for the device table: a rejected call never reads it
PTRS = ctypes.addressof(_LAYER_PTRS)
HOST_ARRAYS = ("wl", "bl", "wr", "nw", "nb", "d_wl", "d_bl", "d_wr", "d_nw", "d_nb")


def _ints(vals):
    return (ctypes.c_int * len(vals))(*vals)


def _descriptor(norm=False, **over):
    """A stack over 640 rows, width 110 in and out, three layers, that passes every argument check of both entry points: the
    plain stack (no table, no tap), or the norm stack (``norm``); then ``over``."""
    from gnn_hex_amd import _lib
    f = {name: (PTRS if name in HOST_ARRAYS else _ONE) for name, kind in _lib.SageStackCall._fields_ if kind is ctypes.c_void_p}
    f.update(struct_bytes=ctypes.sizeof(_lib.SageStackCall), n=N, c_in=HIDDEN, hidden=HIDDEN, num_layers=LAYERS, x_stride=112,
             need_backward=1, flags=0, workspace_bytes=1 << 34, block_starts=None, num_blocks=0, group_starts=None, num_groups=0,
             eps=1e-5, norm_ws_bytes=1 << 20, n_live=None, tap_layer=-1, tap_out=None)
    if not norm:
        f.update(nw=None, nb=None, d_nw=None, d_nb=None)
    f.update(over)
    return _lib.SageStackCall(**f)


def _forward(norm=False, **over):
    from gnn_hex_amd import _lib
    return _lib.lib().hexgnn_sage_stack_call_forward(_descriptor(norm, **over), None)


def _backward(norm=False, **over):
    from gnn_hex_amd import _lib
    return _lib.lib().hexgnn_sage_stack_call_backward(_descriptor(norm, **over), None)


def test_header_struct_and_ctypes_structure_agree():
    """Names, order, kinds (pointer -> c_void_p, size_t -> c_size_t, int -> c_int, float -> c_float), and with them every
    field's offset and size."""
    from gnn_hex_amd import _lib
    header = open(os.path.join(ROOT, "include", "hexgnn.h")).read()
    m = re.search(r"typedef\s+struct\s+hexgnn_sage_stack_call\s*\{(.*?)\}\s*hexgnn_sage_stack_call\s*;", header, re.S)
    assert m, "hexgnn_sage_stack_call is not declared in include/hexgnn.h"
    kinds = {"int": ctypes.c_int, "size_t": ctypes.c_size_t, "float": ctypes.c_float}
    fields = []
    for decl in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(";"):
        decl = decl.strip()
        if not decl:
            continue
        base = re.match(r"(?:const\s+)?(\w+)", decl).group(1)
        assert base in ("int", "size_t", "float", "void"), decl
        for item in decl[re.match(r"(?:const\s+)?\w+", decl).end():].split(","):
            name = re.search(r"(\w+)\s*$", item).group(1)
            fields.append((name, ctypes.c_void_p if "*" in item else kinds[base]))
    assert fields == list(_lib.SageStackCall._fields_)
    assert fields[0] == ("struct_bytes", ctypes.c_size_t) and len(fields) == 43

    class FromHeader(ctypes.Structure):
        _fields_ = fields
    for name, _ in fields:
        h, c = getattr(FromHeader, name), getattr(_lib.SageStackCall, name)
        assert (h.offset, h.size) == (c.offset, c.size), name
    assert _lib.SAGE_STACK_CALL_BYTES == ctypes.sizeof(_lib.SageStackCall) == ctypes.sizeof(FromHeader)
    # both entry points take the descriptor by pointer
    for name in ("hexgnn_sage_stack_call_forward", "hexgnn_sage_stack_call_backward"):
        assert re.search(r"\bint\s+%s\s*\(\s*const\s+hexgnn_sage_stack_call\s*\*" % name, header), name
        assert _lib._SIGS[name] == (ctypes.c_int, [ctypes.POINTER(_lib.SageStackCall), ctypes.c_void_p])
    for gone in GONE:
        assert gone not in _lib._SIGS and not re.search(r"\b%s\b" % gone, header), gone
        assert not hasattr(ctypes.CDLL(_lib.LIB_PATH), gone), gone
    for kept in ("hexgnn_sage_stack_forward", "hexgnn_sage_stack_backward", "hexgnn_sage_norm_stack_forward",
                 "hexgnn_sage_norm_stack_backward"):
        assert kept in _lib._SIGS and re.search(r"\bint\s+%s\s*\(" % kept, header), kept
    assert _lib.ABI_VERSION == 8 and re.search(r"#define\s+HEXGNN_ABI_VERSION\s+8\b", header)


def test_struct_bytes_is_checked_first():
    from gnn_hex_amd import _lib
    L = _lib.lib()
    size = ctypes.sizeof(_lib.SageStackCall)
    for wrong in (0, size - 8, size + 8):
        empty = _lib.SageStackCall(wrong)              # nothing else set: any later check would have to read a NULL
        for d in (empty, _descriptor(struct_bytes=wrong), _descriptor(True, struct_bytes=wrong)):
            assert L.hexgnn_sage_stack_call_forward(d, None) == EINVAL
            assert L.hexgnn_sage_stack_call_backward(d, None) == EINVAL
    assert L.hexgnn_sage_stack_call_forward(None, None) == EINVAL and L.hexgnn_sage_stack_call_backward(None, None) == EINVAL
    # the right size is not refused for that reason: the answers are those of later checks (feature count, workspace size)
    for norm in (False, True):
        assert _forward(norm, c_in=9, x_stride=9) == EUNSUPPORTED and _backward(norm, c_in=9, x_stride=9) == EUNSUPPORTED
        assert _backward(norm, workspace_bytes=16) == EWORKSPACE


def test_forward_refuses_bad_arguments():
    assert _forward(n=-1) == EINVAL
    assert _forward(flags=DY_IN_PLACE) == EINVAL and _forward(flags=4) == EINVAL          # (the backward's flag, an unknown one)
    assert _forward(num_layers=0) == EUNSUPPORTED and _forward(hidden=257) == EUNSUPPORTED    # (the plan's answers, as before)
    assert _forward(wpack=None) == EINVAL
    assert _forward(wl=None) == EINVAL and _forward(bl=None, wr=None) == EINVAL           # some of the three arrays, not all
    for field in ("rowptr", "col", "invdeg", "x", "acts", "saved"):
        assert _forward(**{field: None}) == EINVAL, field
    assert _forward(x_stride=110) == EINVAL and _forward(c_in=3, x_stride=2) == EINVAL    # padded layout; raw rows
    # a table: [ceil(n / 128), 512] blocks, with a pointer
    assert _forward(block_starts=ctypes.addressof(_TABLE), num_blocks=4) == EINVAL
    assert _forward(block_starts=ctypes.addressof(_TABLE), num_blocks=513) == EINVAL
    assert _forward(block_starts=None, num_blocks=5) == EINVAL
    # hidden 129..256 (the plain kernels): the arrays are wanted
    assert _forward(c_in=3, hidden=144, x_stride=3, wl=None, bl=None, wr=None) == EINVAL
    assert _forward(c_in=3, hidden=144, x_stride=3, acts=None) == EINVAL


def test_backward_refuses_bad_arguments():
    from gnn_hex_amd import _lib
    need = _lib.lib().hexgnn_sage_stack_backward_workspace_bytes(N, HIDDEN, HIDDEN, LAYERS)
    assert need > 0
    assert _backward(workspace_bytes=need - 1) == EWORKSPACE and _backward(workspace=None) == EWORKSPACE
    assert _backward(n=-1) == EINVAL and _backward(flags=4) == EINVAL
    assert _backward(flags=DY_IN_PLACE | LINEAR_LAST) == EINVAL
    assert _backward(flags=DY_IN_PLACE | LINEAR_LAST, workspace=None) == EINVAL           # (before the workspace is looked at)
    assert _backward(hidden=257) == EUNSUPPORTED
    for field in ("d_wl", "d_bl", "d_wr", "wpack", "saved", "rowptr_t", "col_t", "invdeg", "x", "acts", "dy"):
        assert _backward(**{field: None}, workspace_bytes=need) == EINVAL, field
        assert _backward(**{field: None}, workspace_bytes=need - 1) == EWORKSPACE, field  # (the workspace comes first)
    holes = (ctypes.c_void_p * 8)(_ONE, _ONE, None, *[_ONE] * 5)                           # layer 2 has no gradient buffer
    for field in ("d_wl", "d_bl", "d_wr"):
        assert _backward(**{field: ctypes.addressof(holes)}) == EINVAL, field
    # dy in place: it must BE the top layer's slab of the workspace (this one is not); nothing is launched before the test
    assert _backward(flags=DY_IN_PLACE) == EINVAL
    assert _backward(flags=DY_IN_PLACE, workspace_bytes=need - 1) == EWORKSPACE
    # the tap: a layer below the top one, checked before the first launch
    for layer in (-1, LAYERS - 1, LAYERS):
        assert _backward(tap_out=_ONE, tap_layer=layer) == EINVAL, layer
    assert _backward(block_starts=ctypes.addressof(_TABLE), num_blocks=4) == EINVAL
    assert _backward(block_starts=None, num_blocks=5) == EINVAL
    wide = dict(c_in=3, hidden=144, x_stride=3)                                          # hidden 129..256 (the plain kernels)
    assert _backward(**wide, d_wl=None) == EINVAL and _backward(**wide, dy=None) == EINVAL


def test_norm_stack_refuses_bad_arguments():
    from gnn_hex_amd import _lib
    L = _lib.lib()
    live = _ONE
    assert _forward(True, n_live=live, need_backward=1) == EINVAL                         # a live row count is forward-only
    assert _forward(True, n_live=live, need_backward=1, c_in=9, x_stride=9) == EINVAL     # (before the plan)
    assert _forward(True, n=-1) == EINVAL and _forward(True, hidden=144, c_in=3, x_stride=3) == EUNSUPPORTED
    for field in ("wl", "bl", "wr", "nw", "nb", "wpack", "stats", "norm_ws", "rowptr", "col", "invdeg", "x", "acts", "pre", "saved"):
        assert _forward(True, **{field: None}) == EINVAL, field
    assert _forward(True, x_stride=110) == EINVAL
    holes = (ctypes.c_void_p * 8)(_ONE, None, *[_ONE] * 6)
    assert _forward(True, nw=ctypes.addressof(holes)) == EINVAL and _forward(True, nb=ctypes.addressof(holes)) == EINVAL
    need = L.hexgnn_sage_norm_stack_backward_workspace_bytes(N, HIDDEN, HIDDEN, LAYERS)
    assert need > L.hexgnn_sage_stack_backward_workspace_bytes(N, HIDDEN, HIDDEN, LAYERS)
    assert _backward(True, workspace_bytes=need - 1) == EWORKSPACE and _backward(True, workspace=None) == EWORKSPACE
    assert _backward(True, n=-1) == EINVAL and _backward(True, hidden=144, c_in=3, x_stride=3) == EUNSUPPORTED
    for field in ("d_wl", "d_bl", "d_wr", "d_nw", "d_nb", "nw", "wpack", "saved", "stats", "norm_ws", "rowptr_t", "col_t", "invdeg",
                  "x", "acts", "pre", "dy"):
        assert _backward(True, **{field: None}, workspace_bytes=need) == EINVAL, field
    for field in ("d_wl", "d_nw", "d_nb", "nw"):
        assert _backward(True, **{field: ctypes.addressof(holes)}, workspace_bytes=need) == EINVAL, field
    # what no entry point could express before ABI 8: the norm stack takes no table, no groups, no tap and no flags
    table, groups = ctypes.addressof(_TABLE), _ints([0, 5])
    for call in (_forward, _backward):
        assert call(True, block_starts=table, num_blocks=5) == EINVAL
        assert call(True, block_starts=table, num_blocks=5, group_starts=ctypes.addressof(groups), num_groups=1) == EINVAL
        assert call(True, group_starts=ctypes.addressof(groups)) == EINVAL and call(True, num_groups=1) == EINVAL
        assert call(True, flags=LINEAR_LAST) == EINVAL
        assert call(True, flags=LINEAR_LAST, workspace=None, c_in=9, x_stride=9) == EINVAL   # (before the plan and the workspace)
    assert _backward(True, tap_out=_ONE, tap_layer=0) == EINVAL and _backward(True, flags=DY_IN_PLACE) == EINVAL
    # the positional adapters without their norm arrays do not turn into the plain stack
    one = ctypes.c_void_p(_ONE)
    assert L.hexgnn_sage_norm_stack_forward(N, HIDDEN, HIDDEN, LAYERS, one, one, one, one, 112, PTRS, PTRS, PTRS, None, None, 1e-5,
                                            one, one, one, one, one, one, 1 << 20, 1, None) == EINVAL
    assert L.hexgnn_sage_norm_stack_backward(N, HIDDEN, HIDDEN, LAYERS, one, one, one, one, 112, one, one, one, one, one, None,
                                             1e-5, one, None, PTRS, PTRS, PTRS, PTRS, PTRS, one, 1 << 34, one, 1 << 20,
                                             None) == EINVAL
