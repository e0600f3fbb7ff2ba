"""CPU: the fused call's descriptor (hexgnn_qnet_call, include/hexgnn.h) and its ctypes mirror agree field for field, and the two
entry points that read it refuse bad descriptors with the codes the positional entry points they replaced gave -- before anything
is launched.  Pointers are host memory that no argument check dereferences."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EUNSUPPORTED, EWORKSPACE = -1, -2, -3
DATA, SMALL, HIDDEN = 1, 2, 4


def _host_ptr():
    """An address that passes a NULL check and is never dereferenced by an argument check."""
    buf = (ctypes.c_char * 256)()
    return buf, ctypes.addressof(buf)


def _descriptor(p, **over):
    """A TD step's descriptor that passes every argument check of both entry points (4 graphs, 204 rows, 2 features, width 35,
    3 body + 2 head layers), then ``over``."""
    from gnn_hex_amd import _lib
    f = dict.fromkeys((name for name, _ in _lib.QNetCall._fields_), p)
    f.update(struct_bytes=ctypes.sizeof(_lib.QNetCall), n=204, b=4, c_in=2, hidden=35, total_layers=5, body_layers=3, mode=0,
             math=0, x_stride=2, need_backward=1, acts_layer=-1, workspace_bytes=1 << 30, td_loss_fn=0, out_v=None, d_out_v=None)
    f.update(over)
    return _lib.QNetCall(**f)


def test_header_struct_and_ctypes_structure_agree():
    """Names, order and kinds: pointer -> c_void_p, size_t -> c_size_t, int -> c_int."""
    from gnn_hex_amd import _lib
    header = open(os.path.join(ROOT, "include", "hexgnn.h")).read()
    m = re.search(r"typedef\s+struct\s+hexgnn_qnet_call\s*\{(.*?)\}\s*hexgnn_qnet_call\s*;", header, re.S)
    assert m, "hexgnn_qnet_call is not declared in include/hexgnn.h"
    fields = []
    for decl in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(";"):
        decl = decl.strip()
        if not decl:
            continue
        base = re.match(r"(?:const\s+)?(\w+)", decl).group(1)
        assert base in ("int", "size_t", "float", "void", "int64_t"), decl
        for item in decl[re.match(r"(?:const\s+)?\w+", decl).end():].split(","):
            name = re.search(r"(\w+)\s*$", item).group(1)
            if "*" in item:
                fields.append((name, ctypes.c_void_p))
            else:
                assert base in ("int", "size_t"), decl
                fields.append((name, ctypes.c_size_t if base == "size_t" else ctypes.c_int))
    assert fields == list(_lib.QNetCall._fields_)
    assert fields[0] == ("struct_bytes", ctypes.c_size_t) and len(fields) == 50
    assert _lib.QNET_CALL_BYTES == ctypes.sizeof(_lib.QNetCall)
    # both entry points take the descriptor by pointer
    for name, rest in (("hexgnn_qnet_call_forward", [ctypes.c_int]), ("hexgnn_qnet_call_backward", [ctypes.c_int] * 3)):
        assert re.search(r"\bint\s+%s\s*\(\s*const\s+hexgnn_qnet_call\s*\*" % name, header), name
        assert _lib._SIGS[name] == (ctypes.c_int, [ctypes.POINTER(_lib.QNetCall)] + rest + [ctypes.c_void_p])
    for gone in ("hexgnn_qnet_forward_td", "hexgnn_qnet_step_td", "hexgnn_qnet_backward_flat", "hexgnn_qnet_backward_flat_td",
                 "hexgnn_qnet_backward_flat_td_live"):
        assert gone not in _lib._SIGS and not re.search(r"\bint\s+%s\s*\(" % gone, header), gone
        assert not hasattr(ctypes.CDLL(_lib.LIB_PATH), gone), gone


def test_struct_bytes_is_checked_first():
    from gnn_hex_amd import _lib
    L = _lib.lib()
    keep, p = _host_ptr()
    size = ctypes.sizeof(_lib.QNetCall)
    for wrong in (0, size - 8, size + 8):
        empty = _lib.QNetCall(wrong)              # nothing else set: any later check would have to read a NULL
        full = _descriptor(p, struct_bytes=wrong)
        for d in (empty, full):
            assert L.hexgnn_qnet_call_forward(d, 0, None) == EINVAL and L.hexgnn_qnet_call_forward(d, 1, None) == EINVAL
            assert L.hexgnn_qnet_call_backward(d, DATA | SMALL | HIDDEN, 1, 5, None) == EINVAL
    # the right size is not refused for that reason: the answers are those of later checks (feature count, workspace size)
    d = _descriptor(p, c_in=9, x_stride=9)
    assert L.hexgnn_qnet_call_forward(d, 0, None) == EUNSUPPORTED and L.hexgnn_qnet_call_forward(d, 1, None) == EUNSUPPORTED
    assert L.hexgnn_qnet_call_backward(_descriptor(p, workspace_bytes=16), DATA | SMALL | HIDDEN, 1, 5, None) == EWORKSPACE
    assert L.hexgnn_qnet_call_forward(None, 0, None) == EINVAL and L.hexgnn_qnet_call_backward(None, 7, 1, 5, None) == EINVAL
    del keep


def test_live_backward_refuses_bad_arguments():
    """A live row count with math 1 (f16x3) is unsupported; a missing gradient buffer or loss is a bad argument.  A missing live
    count selects the host's row count: that descriptor passes every argument check (shown with the one stage that launches
    nothing over an empty layer range, and by the workspace check -- the last before the pointers -- being reached).  Every
    pointer the checks want is given (host memory, never dereferenced): the answers come before any launch."""
    from gnn_hex_amd import _lib
    L = _lib.lib()
    keep, p = _host_ptr()
    offsets = (ctypes.c_int64 * (3 * 5 + 6))()          # (HOST: the one table the accepted call reads)
    need = L.hexgnn_qnet_backward_workspace_bytes(204, 4, 2, 35, 5)
    assert need > 0

    def call(stages=DATA | SMALL | HIDDEN, lo=1, **over):
        tot = over.get("total_layers", 5)
        d = _descriptor(p, **dict(dict(offsets=ctypes.addressof(offsets), workspace_bytes=need), **over))
        return L.hexgnn_qnet_call_backward(d, stages, lo, tot if stages & DATA else lo, None)
    assert call(math=1) == EUNSUPPORTED                          # the split-f16 GEMM takes no live count
    assert call(flat=None) == EINVAL and call(offsets=None) == EINVAL
    assert call(td_loss_part=None) == EINVAL and call(td_loss=None) == EINVAL
    assert call(math=2) == EINVAL and call(math=-1) == EINVAL
    assert call(total_layers=0) == EINVAL and call(total_layers=65) == EINVAL
    # no live count: accepted
    assert call(n_live=None, workspace_bytes=need - 1) == EWORKSPACE and call(n_live=None, workspace=None) == EWORKSPACE
    assert call(n_live=None, stages=HIDDEN) not in (EINVAL, EUNSUPPORTED, EWORKSPACE)
    assert call(stages=HIDDEN) not in (EINVAL, EUNSUPPORTED, EWORKSPACE)          # (and so is the base of the refusals above)
    assert call(n_live=None, math=1, workspace=None) == EWORKSPACE                # f16x3 by the host's count is supported
    del keep


def test_chained_forward_and_td_tail_refuse_bad_arguments():
    """The forward with the backward's data chain in its launch: exact fp32 only, and every pointer of the chain is wanted (a
    missing or short workspace answers as it does in the backward).  The TD tail wants all its buffers."""
    from gnn_hex_amd import _lib
    L = _lib.lib()
    keep, p = _host_ptr()

    def forward(chain, **over):
        return L.hexgnn_qnet_call_forward(_descriptor(p, **over), chain, None)
    assert forward(1, math=1) == EINVAL
    assert forward(1, workspace=None) == EWORKSPACE and forward(1, workspace_bytes=16) == EWORKSPACE
    assert forward(1, rowptr_t=None) == EINVAL and forward(1, col_t=None) == EINVAL
    assert forward(1, td_sel=None) == EINVAL and forward(1, body_layers=0) == EINVAL and forward(1, body_layers=6) == EINVAL
    assert forward(1, n=0) == EINVAL and forward(1, b=0) == EINVAL
    assert forward(1, total_layers=65, body_layers=3) == EUNSUPPORTED
    for chain in (0, 1):
        for field in ("td_dq", "td_target", "td_out", "td_loss_part"):
            assert forward(chain, **{field: None}) == EINVAL, (chain, field)
        assert forward(chain, td_loss_fn=2) == EINVAL and forward(chain, td_loss_fn=-1) == EINVAL
        assert forward(chain, mode=2) == EINVAL and forward(chain, need_backward=0) == EINVAL
        # (the complete tail is not what these refuse: the same descriptor gets as far as the shape checks)
        assert forward(chain, c_in=9, x_stride=9) == EUNSUPPORTED
    assert forward(0, x_stride=1) == EINVAL and forward(0, lin_w=None) == EINVAL and forward(0, math=2) == EINVAL
    del keep
