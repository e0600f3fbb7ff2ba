"""Host side of the HIP path: graph-structure build + ``torch.autograd.Function`` wrappers that hand raw
device pointers and the current HIP stream to libhexgnn.so (include/hexgnn.h).

PyTorch is plumbing here: allocator, stream, autograd bookkeeping.  All arithmetic of the hot path
runs in the hand-written kernels under gnn_hex_amd/csrc; there is no eager/PyTorch fallback.
"""
from __future__ import annotations

import ctypes as C
import os
import sys
import threading
from typing import List, Optional, Sequence

import torch

from . import _lib


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)
_USE_EDGE_PTR = os.environ.get("HEXGNN_NO_EDGE_PTR", "") in ("", "0")      # (A/B switch: ignore the collation's edge offsets)
_DEVICE_BLOCKS = os.environ.get("HEXGNN_NO_DEVICE_BLOCKS", "") in ("", "0")  # (A/B switch: no device-built row-block tables)


def _stream() -> int:
    """Raw hipStream_t of the current torch stream (the private fast accessor when this torch has it: the public
    ``torch.cuda.current_stream()`` costs ~17 us per call, three times per step)."""
    if _raw_stream is not None:
        return _raw_stream(torch.cuda.current_device())
    return torch.cuda.current_stream().cuda_stream


def _require_cuda(t: torch.Tensor, what: str) -> None:
    if not t.is_cuda:
        raise _lib.HexGnnError(
            "%s is on %s: gnn_hex_amd runs only on the MI355X HIP path (no CPU fallback)" % (what, t.device))


def attach_hints(x: torch.Tensor, is_maker=None, max_nodes=None) -> torch.Tensor:
    """Host-known metadata of a batch (side to move, largest graph) as attributes of its feature tensor, stamped with the
    tensor's version counter: an in-place edit of ``x`` afterwards invalidates them (``hints_of`` then returns nothing and
    the model falls back to the reference's device checks)."""
    if is_maker is not None:
        x._hex_is_maker = bool(is_maker)
    if max_nodes is not None:
        x._hex_max_nodes = int(max_nodes)
    x._hex_hint_version = x._version
    return x


def hints_of(x: torch.Tensor):
    """(is_maker, max_nodes) hints of ``x`` or (None, None) when absent or stale (x modified in place since)."""
    ver = getattr(x, "_hex_hint_version", None)
    if ver is not None and ver != x._version:
        return None, None
    return getattr(x, "_hex_is_maker", None), getattr(x, "_hex_max_nodes", None)


def padded_width(hidden: int) -> int:
    hp = _lib.lib().hexgnn_padded_width(int(hidden))
    if hp < 0:
        raise _lib.HexGnnError("hidden_channels=%d not supported by the compiled kernels (1..256)" % hidden)
    return hp


def _bytes(nbytes: int, device) -> torch.Tensor:
    return torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=device)


def _ptr_array(tensors: Sequence[torch.Tensor]):
    return (C.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


_STICKY = {}


def sticky_status(device) -> torch.Tensor:
    """One int32 error word per device, zero unless a kernel found broken input (bits: GraphStructure.check).  The
    one-launch CSR build and the fused kernels OR into it and never clear it, so no per-batch memset is needed; the
    first ``check()`` after an error reports it and clears the word (errors are sticky across batches until then)."""
    dev = torch.device(device)
    key = (dev.type, dev.index if dev.index is not None else torch.cuda.current_device())
    t = _STICKY.get(key)
    if t is None:
        t = torch.zeros(1, dtype=torch.int32, device=dev)
        _STICKY[key] = t
    return t


def _blocks_of(edge_index, n: int):
    """The collation's row-block table of a batch (``edge_index._hex_blocks`` = (int32 device tensor [nb + 1], nb), attached by
    ``Batch.from_data_list(..., pack=True)`` / ``data.attach_blocks``): graph-aligned blocks for the one-launch stack kernels
    (``hexgnn_sage_stack_call.block_starts``).  Anything malformed is ignored (the default 128-row blocks then)."""
    blk = getattr(edge_index, "_hex_blocks", None)
    if blk is None:
        return None
    try:
        t, nb = blk
        nb = int(nb)
    except (TypeError, ValueError):
        return None
    if not (torch.is_tensor(t) and t.dtype == torch.int32 and t.is_cuda and t.is_contiguous() and t.dim() == 1
            and t.numel() == nb + 1 and (int(n) + 127) // 128 <= nb <= min(512, max(int(n), 1))):
        return None
    return (t, nb)


def _groups_of(edge_index, n: int):
    """The collation's block table of a batch that needs more blocks than can be resident at once, with its groups
    (``edge_index._hex_block_groups`` = (int32 device tensor [nb + 1], nb, groups), ``data.attach_block_groups``): every group
    is one launch of the one-launch stack kernels (``hexgnn_sage_stack_call.group_starts``).  Returns (table, nb, groups, the
    groups as a C int array) or None; anything malformed is ignored."""
    grp = getattr(edge_index, "_hex_block_groups", None)
    if grp is None:
        return None
    try:
        t, nb, groups = grp
        nb = int(nb)
        groups = tuple(int(g) for g in groups)
    except (TypeError, ValueError):
        return None
    if not (torch.is_tensor(t) and t.dtype == torch.int32 and t.is_cuda and t.is_contiguous() and t.dim() == 1
            and t.numel() == nb + 1 and (int(n) + 127) // 128 <= nb <= min(512, max(int(n), 1))):
        return None
    if len(groups) < 2 or groups[0] != 0 or groups[-1] != nb or any(b <= a for a, b in zip(groups, groups[1:])):
        return None
    return (t, nb, groups, (C.c_int * len(groups))(*groups))


def _stack_call(gs, gp, n, c_in, hidden, layers, x, x_stride, arrays, wpack, acts, saved, need_bwd, flags=0, norm=None):
    """The ``hexgnn_sage_stack_call`` of a layer-major stack's forward over ``gs``, with the batch's grouped table, else its
    plain table, else the default blocks; the backward sets its own fields on the same object.  Everything but ``gs`` is an
    address or a number: ``gp`` = (rowptr, col, rowptr_t, col_t, invdeg) or None (taken from ``gs``), ``arrays`` = the wl / bl /
    wr pointer arrays (None each: packed by the CSR call), ``norm`` = the norm group's fields by name (the norm stack).
    The descriptor holds RAW ADDRESSES: its owner keeps what they point at."""
    if gp is None:
        gp = (gs.rowptr.data_ptr(), gs.col.data_ptr(), gs.rowptr_t.data_ptr(), gs.col_t.data_ptr(), gs.invdeg.data_ptr())
    d = _lib.SageStackCall(struct_bytes=_lib.SAGE_STACK_CALL_BYTES, n=n, c_in=c_in, hidden=hidden, num_layers=layers,
                           x_stride=x_stride, need_backward=int(need_bwd), flags=flags, rowptr=gp[0], col=gp[1], rowptr_t=gp[2],
                           col_t=gp[3], invdeg=gp[4], x=x, wl=arrays[0], bl=arrays[1], wr=arrays[2], wpack=wpack, acts=acts,
                           saved=saved, tap_layer=-1, **(norm or {}))
    if norm is None and gs.groups is not None:
        t, nb, groups, cgroups = gs.groups
        d.block_starts, d.num_blocks, d.group_starts, d.num_groups = t.data_ptr(), nb, C.addressof(cgroups), len(groups) - 1
    elif norm is None and gs.blocks:                     # (the norm stack runs a launch per layer: no table)
        d.block_starts, d.num_blocks = gs.blocks[0].data_ptr(), gs.blocks[1]
    return d


def _ptr_arrays(tensors: Sequence[torch.Tensor], k: int):
    """``tensors`` dealt into ``k`` pointer arrays (every k-th tensor each), and the arrays' addresses as a descriptor holds them."""
    arrays = [_ptr_array(tensors[i::k]) for i in range(k)]
    return arrays, [C.addressof(a) for a in arrays]


def _f32c(t: torch.Tensor) -> torch.Tensor:
    """``t`` as a contiguous fp32 tensor (``t`` itself when it is one)."""
    return t if (t.is_contiguous() and t.dtype == torch.float32) else t.float().contiguous()


class GraphStructure:
    """Target-major CSR of a batch + its transpose + 1/deg, built once per batch on the device.

    rowptr/col: in-neighbours (sources) of every node, ascending; rowptr_t/col_t: out-neighbours.
    Replaces the per-layer x[edge_index[0]] / scatter(edge_index[1]) indexing of the reference
    (GN0/models.py:276)."""

    __slots__ = ("n", "e", "rowptr", "col", "rowptr_t", "col_t", "invdeg", "status", "_ptrs", "blocks", "groups")

    def __init__(self, edge_index: torch.Tensor, num_nodes: int, gptr: Optional[torch.Tensor] = None, b: int = 0,
                 ptr64: Optional[torch.Tensor] = None):
        """``gptr`` (int32 [b+1] node ranges) selects the single-launch build for batches whose edges are grouped by
        graph in graph order (``Batch.from_data_list``, the env builder); without it the general build runs.  With
        ``ptr64`` (the batch's int64 ``ptr``) the node ranges are read from it and ``gptr`` (preallocated) receives the
        int32 copy."""
        _require_cuda(edge_index, "edge_index")
        if edge_index.dim() != 2 or edge_index.shape[0] != 2:
            raise ValueError("edge_index must be [2, E]")
        blocks = _blocks_of(edge_index, num_nodes)
        groups = _groups_of(edge_index, num_nodes) if blocks is None else None
        if edge_index.dtype != torch.int64:
            edge_index = edge_index.long()
        edge_index = edge_index.contiguous()
        dev = edge_index.device
        n, e = int(num_nodes), int(edge_index.shape[1])
        L = _lib.lib()
        self.n, self.e = n, e
        self._ptrs = None
        self.blocks = blocks
        self.groups = groups
        if gptr is not None and b > 0:
            ibuf = torch.empty(2 * (n + 1), dtype=torch.int32, device=dev)
            self.rowptr, self.rowptr_t = ibuf[:n + 1], ibuf[n + 1:2 * (n + 1)]
            self.status = sticky_status(dev)
            self.col = torch.empty(max(e, 1), dtype=torch.int32, device=dev)
            self.col_t = torch.empty(max(e, 1), dtype=torch.int32, device=dev)
            self.invdeg = torch.empty(max(n, 1), dtype=torch.float32, device=dev)
            _lib.check(L.hexgnn_csr_build_grouped(n, e, int(b), edge_index[0].data_ptr(), edge_index[1].data_ptr(),
                                                  gptr.data_ptr() if ptr64 is None else None,
                                                  ptr64.data_ptr() if ptr64 is not None else None,
                                                  gptr.data_ptr() if ptr64 is not None else None,
                                                  self.rowptr.data_ptr(), self.col.data_ptr(),
                                                  self.rowptr_t.data_ptr(), self.col_t.data_ptr(), self.invdeg.data_ptr(),
                                                  self.status.data_ptr(), _stream()), "hexgnn_csr_build_grouped")
            return
        ws_bytes = L.hexgnn_csr_workspace_bytes(n, e)
        # one int32 buffer [rowptr | rowptr_t | status | workspace]: the build zeroes it with a single memset
        ibuf = torch.empty(2 * (n + 1) + 1 + (ws_bytes + 3) // 4, dtype=torch.int32, device=dev)
        self.rowptr = ibuf[:n + 1]
        self.rowptr_t = ibuf[n + 1:2 * (n + 1)]
        self.status = ibuf[2 * (n + 1):2 * (n + 1) + 1]
        ws = ibuf[2 * (n + 1) + 1:]
        self.col = torch.empty(max(e, 1), dtype=torch.int32, device=dev)
        self.col_t = torch.empty(max(e, 1), dtype=torch.int32, device=dev)
        self.invdeg = torch.empty(max(n, 1), dtype=torch.float32, device=dev)
        src = edge_index[0]
        dst = edge_index[1]
        _lib.check(L.hexgnn_csr_build(n, e, src.data_ptr(), dst.data_ptr(), self.rowptr.data_ptr(),
                                      self.col.data_ptr(), self.rowptr_t.data_ptr(), self.col_t.data_ptr(),
                                      self.invdeg.data_ptr(), self.status.data_ptr(), ws.data_ptr(), ws_bytes,
                                      _stream()), "hexgnn_csr_build")

    @classmethod
    def grouped(cls, edge_index: torch.Tensor, num_nodes: int, b: int, ptr64: torch.Tensor, pack=None, device_blocks: bool = False):
        """The one-launch build for a collated batch (edges grouped by graph, int64 ``ptr`` on the device) with ONE int32
        allocation [rowptr | rowptr_t | col | col_t | gptr] + one for 1/deg instead of six, and the raw pointers kept in
        ``_ptrs`` = (rowptr, col, rowptr_t, col_t, invdeg, gptr, status) so that the fused calls need no ``data_ptr()``: the
        eager hot path (a ``torch.empty`` costs ~2.5 us of host time, a slice ~1 us).  Returns ``(gs, gptr)``."""
        self = _GroupedStructure.__new__(_GroupedStructure)
        dev = edge_index.device
        n, e = int(num_nodes), int(edge_index.shape[1])
        self.n, self.e = n, e
        self.blocks = _blocks_of(edge_index, n)
        self.groups = _groups_of(edge_index, n) if self.blocks is None else None
        e1 = e if e > 0 else 1
        o1, o2 = n + 1, 2 * (n + 1)
        o3, o4 = o2 + e1, o2 + 2 * e1
        ibuf = torch.empty(o4 + b + 1, dtype=torch.int32, device=dev)
        invdeg = torch.empty(n if n > 0 else 1, dtype=torch.float32, device=dev)
        status = sticky_status(dev)
        base = ibuf.data_ptr()
        src = edge_index.data_ptr()
        self._ibuf, self._offs = ibuf, (o1, o2, o3, o4)
        self.invdeg, self.status = invdeg, status
        self._ptrs = (base, base + 4 * o2, base + 4 * o1, base + 4 * o3, invdeg.data_ptr(), base + 4 * o4, status.data_ptr())
        if pack is not None:
            # + the weight pack of the network call that follows, in the same launch: pack = (c_in, hidden, layers, wl, bl, wr
            # pointer arrays, wpack address); that call is then given no weight arrays
            # (the collation's per-graph edge offsets, when the batch carries them: Batch.from_data_list attaches them)
            ep = getattr(edge_index, "_hex_edge_ptr", None) if _USE_EDGE_PTR else None
            if ep is not None and not (torch.is_tensor(ep) and ep.dtype == torch.long and ep.device == dev and ep.is_contiguous()
                                       and ep.numel() == int(b) + 1):
                ep = None
            tbl, budget = None, 0
            if device_blocks and self.blocks is None and self.groups is None and _DEVICE_BLOCKS:
                # the layer-major path of a batch that carries no block table (raw tensors: another collation): built on the device
                # in this launch, in the batch's own graph order (the host never sees the sizes)
                budget = stack_block_budget()
                if 0 < budget and (n + 127) // 128 <= budget:
                    tbl = torch.empty(budget + 1, dtype=torch.int32, device=dev)
                    self.blocks = (tbl, budget)
                else:
                    budget = 0
            _lib.check(_lib.lib().hexgnn_csr_build_grouped_pack_b(
                n, e, int(b), src, src + 8 * e, None, ptr64.data_ptr(), ep.data_ptr() if ep is not None else None,
                base + 4 * o4, base, base + 4 * o2, base + 4 * o1, base + 4 * o3, self._ptrs[4], self._ptrs[6], pack[0], pack[1],
                pack[2], pack[3], pack[4], pack[5], pack[6], tbl.data_ptr() if tbl is not None else None, budget, _stream()),
                "hexgnn_csr_build_grouped_pack_b")
            return self
        _lib.check(_lib.lib().hexgnn_csr_build_grouped(
            n, e, int(b), src, src + 8 * e, None, ptr64.data_ptr(), base + 4 * o4, base, base + 4 * o2, base + 4 * o1,
            base + 4 * o3, self._ptrs[4], self._ptrs[6], _stream()), "hexgnn_csr_build_grouped")
        return self

    @classmethod
    def from_csr(cls, n: int, e: int, rowptr, col, invdeg, rowptr_t=None, col_t=None) -> "GraphStructure":
        """Adopt an existing sorted CSR (the env builder emits one).  Without a transpose the graph is taken to be
        symmetric (board graphs are), i.e. its own transpose."""
        self = cls.__new__(cls)
        self.n, self.e = int(n), int(e)
        self.rowptr, self.col, self.invdeg = rowptr, col, invdeg
        self.rowptr_t = rowptr if rowptr_t is None else rowptr_t
        self.col_t = col if col_t is None else col_t
        self.status = sticky_status(rowptr.device)
        self._ptrs = None
        self.blocks = None
        self.groups = None
        return self

    def check(self) -> None:
        """Host-synchronising validity check (debug aid; not called on the hot path).  Batches built by the one-launch
        CSR build share the device's sticky error word: an error is reported by the first check after it, then cleared."""
        code = int(self.status.item())              # (synchronises)
        rc = _lib.lib().hexgnn_stack_status(1)      # a one-launch stack kernel that ran out of its poll budget since the last check
        if rc != 0:
            _lib.check(rc, "a one-launch SAGE stack kernel (its output rows were poisoned with NaN)")
        if code != 0:
            if self.status is _STICKY.get((self.status.device.type, self.status.device.index)):
                self.status.zero_()
            raise IndexError("invalid batch structure (status=%d): 1 = node id outside [0,n), 2 = graph larger than "
                             "128 nodes reached the fused kernel, 4 = an edge connects two graphs (or a batch passed as grouped is "
                             "not), 8 = graph above 2048 nodes in the grouped build, 16 = td_step: a selected node outside its graph.  This batch has n = %d; the word is shared "
                             "by every batch of this device since the last check(), so the error may stem from an EARLIER "
                             "batch (it is cleared now)" % (code, self.n))


class _GroupedStructure(GraphStructure):
    """GraphStructure.grouped(): the index arrays are views of ONE buffer, made when somebody asks for them."""
    __slots__ = ("_ibuf", "_offs")

    @property
    def rowptr(self):
        return self._ibuf[:self._offs[0]]

    @property
    def rowptr_t(self):
        return self._ibuf[self._offs[0]:self._offs[1]]

    @property
    def col(self):
        return self._ibuf[self._offs[1]:self._offs[2]]

    @property
    def col_t(self):
        return self._ibuf[self._offs[2]:self._offs[3]]

    @property
    def gptr(self):
        return self._ibuf[self._offs[3]:]


def graph_ptr(graph_indices: Optional[torch.Tensor], ptr: Optional[torch.Tensor], n: int, device):
    """(gptr int32 [B+1] on device, B).  Uses ``ptr`` when given (no host sync); otherwise derives it from
    the sorted ``graph_indices`` with B = max+1 -- the same host sync the reference has at
    GN0/models.py:576."""
    if ptr is not None:
        b = int(ptr.numel()) - 1
        return ptr.to(device=device, dtype=torch.int32), b
    if graph_indices is None:
        return torch.tensor([0, n], dtype=torch.int32, device=device), 1
    _require_cuda(graph_indices, "graph_indices")
    b = int(graph_indices.max()) + 1 if n > 0 else 0
    gi = graph_indices.long().contiguous()
    gptr = torch.empty(b + 1, dtype=torch.int32, device=device)
    _lib.check(_lib.lib().hexgnn_graph_ptr(n, b, gi.data_ptr(), gptr.data_ptr(), _stream()), "hexgnn_graph_ptr")
    return gptr, b


# ------------------------------------------------------------------------------------------------
# padded layout helpers
# ------------------------------------------------------------------------------------------------

def _is_padded_view(t: torch.Tensor, hidden: int, hp: int) -> bool:
    if t.dim() != 2 or t.shape[1] != hidden or t.dtype != torch.float32:
        return False
    if t.shape[0] > 0 and t.stride() != (hp, 1):
        return False
    need = (t.storage_offset() + t.shape[0] * hp) * 4
    return t.untyped_storage().nbytes() >= need and t.data_ptr() % 16 == 0


def as_padded(t: torch.Tensor, hidden: int, trust_pads: bool) -> torch.Tensor:
    """Return a [n, HP] tensor sharing memory with ``t`` when ``t`` already is a padded-layout view whose pad
    columns are known to be zero (tensors produced by this module carry ``_hexgnn_hp``), or whose pads do
    not matter (``trust_pads``: gradients, which the kernels mask); otherwise a zero-padded copy."""
    hp = padded_width(hidden)
    n = t.shape[0]
    tagged = getattr(t, "_hexgnn_hp", None) == hp
    if (tagged or trust_pads) and _is_padded_view(t, hidden, hp):
        return torch.as_strided(t, (n, hp), (hp, 1))
    _require_cuda(t, "feature matrix")
    src = t if (t.stride(1) == 1 and t.dtype == torch.float32) else t.float().contiguous()
    out = torch.empty((n, hp), dtype=torch.float32, device=t.device)
    _lib.check(_lib.lib().hexgnn_pad_rows(n, hidden, src.data_ptr(), src.stride(0) if n > 0 else hidden,
                                          out.data_ptr(), _stream()), "hexgnn_pad_rows")
    return out


def _logical(padded: torch.Tensor, hidden: int) -> torch.Tensor:
    v = padded[:, :hidden]
    v._hexgnn_hp = padded.shape[1]
    return v


# ------------------------------------------------------------------------------------------------
# GraphSAGE stack
# ------------------------------------------------------------------------------------------------

def _stack_inputs(x, c_in: int, hidden: int, params):
    """What both stacks are handed: (n, hp, the input rows, their stride, the parameters as contiguous fp32) -- raw features
    (c_in != hidden) as fp32 rows of any stride, a hidden-wide input in the padded layout."""
    n = int(x.shape[0])
    hp = padded_width(hidden)
    if c_in != hidden:
        if x.dtype != torch.float32 or x.stride(1) != 1:
            x = x.float().contiguous()
        xin, x_stride = x, (x.stride(0) if n > 0 else c_in)
    else:
        xin, x_stride = as_padded(x, hidden, trust_pads=False), hp
    return n, hp, xin, x_stride, [_f32c(p) for p in params]


def _stack_backward(ctx, grad_out, k: int, ws_bytes: int):
    """The backward of both stacks (``k`` parameters per layer): the backward fields of the forward's descriptor, one call.
    Returns (the input gradient or None, the parameter gradients)."""
    n, c_in, hidden, num_layers, hp = ctx.dims
    dev = grad_out.device
    dy = as_padded(grad_out, hidden, trust_pads=True)
    want_dx = ctx.needs_input_grad[0] and c_in == hidden
    dx = torch.empty((n, hp), dtype=torch.float32, device=dev) if want_dx else None
    grads = [torch.empty(s, dtype=torch.float32, device=dev) for s in ctx.param_shapes]
    ws = _bytes(ws_bytes, dev)
    d = ctx.desc
    garrays, ga = _ptr_arrays(grads, k)
    d.dy, d.dx, d.workspace, d.workspace_bytes = dy.data_ptr(), dx.data_ptr() if dx is not None else None, ws.data_ptr(), ws_bytes
    d.d_wl, d.d_bl, d.d_wr = ga[:3]
    if k == 5:
        d.d_nw, d.d_nb = ga[3:]
    _lib.check(_lib.lib().hexgnn_sage_stack_call_backward(d, _stream()), "hexgnn_sage_stack_call_backward")
    return (_logical(dx, hidden) if dx is not None else None), tuple(grads)


class SageStackFn(torch.autograd.Function):
    """y = relu(SAGE_L(... relu(SAGE_1(x)) ...)); CachifiedGNN.forward, GN0/models.py:261-294."""

    @staticmethod
    def forward(ctx, x, gs: GraphStructure, c_in: int, hidden: int, num_layers: int, flags: int, *params):
        L = _lib.lib()
        dev = x.device
        n, hp, xin, x_stride, params = _stack_inputs(x, c_in, hidden, params)
        arrays, pa = _ptr_arrays(params, 3)
        need_bwd = any(ctx.needs_input_grad)
        acts = torch.empty((num_layers, n, hp), dtype=torch.float32, device=dev)
        wpack = _bytes(L.hexgnn_sage_stack_pack_bytes(c_in, hidden, num_layers), dev)
        # (hidden > 128: the plain kernels materialise every layer's aggregate, with or without a backward)
        saved = _bytes(L.hexgnn_sage_stack_saved_bytes(n, c_in, hidden, num_layers), dev) if (need_bwd or hidden > 128) else None
        desc = _stack_call(gs, None, n, c_in, hidden, num_layers, xin.data_ptr(), x_stride, pa, wpack.data_ptr(), acts.data_ptr(),
                           saved.data_ptr() if saved is not None else None, need_bwd, int(flags))
        _lib.check(L.hexgnn_sage_stack_call_forward(desc, _stream()), "hexgnn_sage_stack_call_forward")
        if need_bwd:
            # the descriptor holds raw addresses; ctx keeps what they point at: gs (the graph arrays, the table, the groups' C
            # array), bufs (input rows and the forward's buffers), keep (the pointer arrays)
            ctx.desc, ctx.gs, ctx.bufs, ctx.keep = desc, gs, (xin, acts, saved, wpack), arrays
            ctx.dims = (n, c_in, hidden, num_layers, hp)
            ctx.param_shapes = [p.shape for p in params]
        return acts[num_layers - 1][:, :hidden]

    @staticmethod
    def backward(ctx, grad_out):
        gx, grads = _stack_backward(ctx, grad_out, 3, _lib.lib().hexgnn_sage_stack_backward_workspace_bytes(*ctx.dims[:4]))
        return (gx, None, None, None, None, None) + grads


SAGE_LINEAR_LAST = 1      # HEXGNN_SAGE_LINEAR_LAST: no ReLU after the last layer of the stack


def sage_stack(x: torch.Tensor, gs: GraphStructure, c_in: int, hidden: int, convs, linear_last: bool = False) -> torch.Tensor:
    """Run a stack of SAGEConv parameter holders (objects with lin_l.weight/bias, lin_r.weight): ReLU after every layer
    (CachifiedGNN.forward), except after the last one when ``linear_last`` (a bare SAGEConv.forward)."""
    _require_cuda(x, "x")
    params: List[torch.Tensor] = []
    for conv in convs:
        params += [conv.lin_l.weight, conv.lin_l.bias, conv.lin_r.weight]
    out = SageStackFn.apply(x, gs, c_in, hidden, len(convs), SAGE_LINEAR_LAST if linear_last else 0, *params)
    out._hexgnn_hp = padded_width(hidden)
    return out


def stack_block_budget(device=None) -> int:
    """Row blocks the one-launch stack kernels may use on ``device`` right now (CUs minus those reserved for kernels that run
    beside them, ``GradSync.enable_overlap``): what ``data.pack_order`` packs against."""
    if device is not None and torch.device(device).type == "cuda":
        with torch.cuda.device(device):
            return int(_lib.lib().hexgnn_stack_block_budget())
    return int(_lib.lib().hexgnn_stack_block_budget())


class live_rows:
    """``with ops.live_rows(count):`` -- inside, the whole-batch LayerNorm calls (``sage_norm_stack``, ``graph_layernorm``) take
    their row count from ``count`` (a 1-element int32 device tensor, at most the buffers' row count) instead of the tensors'
    shapes: the closed acting loop (``multi_env_manager.DeviceRollout``) hands the model capacity-sized buffers whose live
    node total exists on the device only.  Forward-only: a call that would need a backward raises."""
    _tls = threading.local()

    def __init__(self, count: Optional[torch.Tensor]):
        if count is not None and (count.dtype != torch.int32 or count.numel() != 1 or not count.is_cuda):
            raise ValueError("live_rows: a 1-element int32 device tensor")
        self.count = count

    def __enter__(self):
        self.prev = getattr(live_rows._tls, "count", None)
        live_rows._tls.count = self.count
        return self

    def __exit__(self, *exc):
        live_rows._tls.count = self.prev
        return False

    @staticmethod
    def current(*tensors) -> Optional[torch.Tensor]:
        """The count in force (called by the wrappers OUTSIDE the autograd function: there the grad mode is the caller's)."""
        c = getattr(live_rows._tls, "count", None)
        if c is not None and torch.is_grad_enabled() and any(t.requires_grad for t in tensors):
            raise RuntimeError("ops.live_rows is forward-only (acting loop): run the model under torch.no_grad()")
        return c


class SageNormStackFn(torch.autograd.Function):
    """x = relu(norm_l(SAGE_l(x))) for every layer: CachifiedGNN.forward with the LayerNorm of --norm=True (GN0/models.py:
    261-294, 935, 945) as one call per direction (``hexgnn_sage_norm_stack_*``).  params: per layer lin_l.weight, lin_l.bias,
    lin_r.weight, norm.weight, norm.bias."""

    @staticmethod
    def forward(ctx, x, gs: GraphStructure, c_in: int, hidden: int, num_layers: int, eps: float, live, *params):
        L = _lib.lib()
        dev = x.device
        n, hp, xin, x_stride, params = _stack_inputs(x, c_in, hidden, params)
        arrays, pa = _ptr_arrays(params, 5)
        # live: ops.live_rows' device-side row count (forward-only)
        need_bwd = any(ctx.needs_input_grad) and live is None
        # [pre | acts]: contraction outputs and norm + ReLU outputs of every layer
        both = torch.empty((2, num_layers, n, hp), dtype=torch.float32, device=dev)
        pre, acts = both[0], both[1]
        wpack = _bytes(L.hexgnn_sage_stack_pack_bytes(c_in, hidden, num_layers), dev)
        saved = _bytes(L.hexgnn_sage_stack_saved_bytes(n, c_in, hidden, num_layers), dev) if need_bwd else None
        stats = torch.empty((num_layers, 2), dtype=torch.float32, device=dev)
        nws_bytes = L.hexgnn_graph_layernorm_workspace_bytes(hidden)
        nws = _bytes(nws_bytes, dev)
        norm = dict(nw=pa[3], nb=pa[4], eps=float(eps), pre=pre.data_ptr(), stats=stats.data_ptr(), norm_ws=nws.data_ptr(),
                    norm_ws_bytes=nws_bytes, n_live=live.data_ptr() if live is not None else None)
        desc = _stack_call(gs, None, n, c_in, hidden, num_layers, xin.data_ptr(), x_stride, pa[:3],
                           wpack.data_ptr(), acts.data_ptr(), saved.data_ptr() if saved is not None else None, need_bwd, 0, norm)
        _lib.check(L.hexgnn_sage_stack_call_forward(desc, _stream()), "hexgnn_sage_stack_call_forward")
        if need_bwd:
            # (as in SageStackFn: ctx keeps what the descriptor's addresses point at; + the fp32 norm weights, which the
            # backward reads through `nw` and which may be copies that nothing else owns)
            ctx.desc, ctx.gs, ctx.bufs, ctx.keep = desc, gs, (xin, both, saved, wpack, stats, params[3::5]), arrays
            ctx.dims = (n, c_in, hidden, num_layers, hp)
            ctx.param_shapes = [p.shape for p in params]
        return acts[num_layers - 1][:, :hidden]

    @staticmethod
    def backward(ctx, grad_out):
        L = _lib.lib()
        nws_bytes = L.hexgnn_graph_layernorm_workspace_bytes(ctx.dims[2])
        nws = _bytes(nws_bytes, grad_out.device)
        ctx.desc.norm_ws, ctx.desc.norm_ws_bytes = nws.data_ptr(), nws_bytes
        gx, grads = _stack_backward(ctx, grad_out, 5, L.hexgnn_sage_norm_stack_backward_workspace_bytes(*ctx.dims[:4]))
        return (gx, None, None, None, None, None, None) + grads


def sage_norm_stack(x: torch.Tensor, gs: GraphStructure, c_in: int, hidden: int, convs, norms) -> torch.Tensor:
    """conv -> LayerNorm (whole batch) -> ReLU for every layer of a stack (``--norm=True``)."""
    _require_cuda(x, "x")
    eps = float(norms[0].eps)
    params: List[torch.Tensor] = []
    for conv, norm in zip(convs, norms):
        if float(norm.eps) != eps:
            raise ValueError("the norms of one stack must share eps")
        params += [conv.lin_l.weight, conv.lin_l.bias, conv.lin_r.weight, norm.weight, norm.bias]
    out = SageNormStackFn.apply(x, gs, c_in, hidden, len(convs), eps, live_rows.current(x, *params), *params)
    out._hexgnn_hp = padded_width(hidden)
    return out


class GraphLayerNormFn(torch.autograd.Function):
    """torch_geometric LayerNorm(mode="graph") without a batch vector: normalise over ALL nodes and channels of the batch,
    affine, optional fused ReLU (GN0/models.py:286-289 norm -> act).  C ABI ``hexgnn_graph_layernorm_*``."""

    @staticmethod
    def forward(ctx, x, weight, bias, eps: float, relu: bool, live=None):
        L = _lib.lib()
        hidden = int(x.shape[1])
        hp = padded_width(hidden)
        n = int(x.shape[0])
        xp = as_padded(x, hidden, trust_pads=False)
        w = _f32c(weight)
        b = _f32c(bias)
        y = torch.empty((n, hp), dtype=torch.float32, device=x.device)
        stats = torch.empty(2, dtype=torch.float32, device=x.device)
        ws_bytes = L.hexgnn_graph_layernorm_workspace_bytes(hidden)
        ws = _bytes(ws_bytes, x.device)
        _lib.check(L.hexgnn_graph_layernorm_forward_live(n, live.data_ptr() if live is not None else None, hidden,
                                                         xp.data_ptr(), w.data_ptr(), b.data_ptr(), float(eps), int(relu),
                                                         y.data_ptr(), stats.data_ptr(), ws.data_ptr(), ws_bytes, _stream()),
                   "hexgnn_graph_layernorm_forward_live")
        ctx.dims = (n, hidden, hp, float(eps), bool(relu))
        ctx.bufs = (xp, y, w, stats)
        return _logical(y, hidden)

    @staticmethod
    def backward(ctx, dy):
        L = _lib.lib()
        n, hidden, hp, eps, relu = ctx.dims
        xp, y, w, stats = ctx.bufs
        dyp = as_padded(dy, hidden, trust_pads=True)
        dx = torch.empty((n, hp), dtype=torch.float32, device=xp.device)
        dw = torch.empty(hidden, dtype=torch.float32, device=xp.device)
        db = torch.empty(hidden, dtype=torch.float32, device=xp.device)
        ws_bytes = L.hexgnn_graph_layernorm_workspace_bytes(hidden)
        ws = _bytes(ws_bytes, xp.device)
        _lib.check(L.hexgnn_graph_layernorm_backward(n, hidden, xp.data_ptr(), y.data_ptr(), w.data_ptr(), stats.data_ptr(),
                                                     dyp.data_ptr(), eps, int(relu), dx.data_ptr(), dw.data_ptr(),
                                                     db.data_ptr(), ws.data_ptr(), ws_bytes, _stream()),
                   "hexgnn_graph_layernorm_backward")
        return _logical(dx, hidden), dw, db, None, None, None


def graph_layernorm(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor, eps: float = 1e-5, relu: bool = False):
    _require_cuda(x, "x")
    out = GraphLayerNormFn.apply(x, weight, bias, eps, relu, live_rows.current(x, weight, bias))
    out._hexgnn_hp = padded_width(int(x.shape[1]))
    return out


class GraphColNormFn(torch.autograd.Function):
    """CachedGraphNorm (GN0/models.py:644-670) without a batch vector: per-channel mean / variance over ALL nodes of the
    batch, ``weight * (x - mean * mean_scale) / sqrt(var + eps) + bias``, optional fused ReLU.  ``cache`` = None: fresh
    statistics (returned as the second output, [2, hidden] = mean | var, not differentiable); ``cache`` = a [2, hidden]
    tensor: the cached statistics are constants.  C ABI ``hexgnn_graph_colnorm_*``."""

    @staticmethod
    def forward(ctx, x, weight, bias, mean_scale, eps: float, relu: bool, cache):
        L = _lib.lib()
        hidden = int(x.shape[1])
        hp = padded_width(hidden)
        n = int(x.shape[0])
        xp = as_padded(x, hidden, trust_pads=False)
        ps = [_f32c(p) for p in (weight, bias, mean_scale)]
        y = torch.empty((n, hp), dtype=torch.float32, device=x.device)
        stats = torch.zeros((2, hp), dtype=torch.float32, device=x.device)
        use_cache = cache is not None
        if use_cache:
            stats[:, :hidden] = cache.reshape(2, hidden).to(device=x.device, dtype=torch.float32)
        ws_bytes = L.hexgnn_graph_colnorm_workspace_bytes(hidden)
        ws = _bytes(ws_bytes, x.device)
        _lib.check(L.hexgnn_graph_colnorm_forward(n, hidden, xp.data_ptr(), ps[0].data_ptr(), ps[1].data_ptr(),
                                                  ps[2].data_ptr(), float(eps), int(relu), int(use_cache), y.data_ptr(),
                                                  stats.data_ptr(), ws.data_ptr(), ws_bytes, _stream()),
                   "hexgnn_graph_colnorm_forward")
        ctx.dims = (n, hidden, hp, float(eps), bool(relu), use_cache)
        ctx.bufs = (xp, y, ps[0], ps[2], stats)
        out_stats = stats[:, :hidden]
        ctx.mark_non_differentiable(out_stats)
        return _logical(y, hidden), out_stats

    @staticmethod
    def backward(ctx, dy, _dstats):
        L = _lib.lib()
        n, hidden, hp, eps, relu, use_cache = ctx.dims
        xp, y, w, ms, stats = ctx.bufs
        dyp = as_padded(dy, hidden, trust_pads=True)
        dx = torch.empty((n, hp), dtype=torch.float32, device=xp.device)
        dw = torch.empty(hidden, dtype=torch.float32, device=xp.device)
        db = torch.empty(hidden, dtype=torch.float32, device=xp.device)
        dms = torch.empty(hidden, dtype=torch.float32, device=xp.device)
        ws_bytes = L.hexgnn_graph_colnorm_workspace_bytes(hidden)
        ws = _bytes(ws_bytes, xp.device)
        _lib.check(L.hexgnn_graph_colnorm_backward(n, hidden, xp.data_ptr(), y.data_ptr(), w.data_ptr(), ms.data_ptr(),
                                                   stats.data_ptr(), dyp.data_ptr(), eps, int(relu), int(use_cache),
                                                   dx.data_ptr(), dw.data_ptr(), db.data_ptr(), dms.data_ptr(),
                                                   ws.data_ptr(), ws_bytes, _stream()), "hexgnn_graph_colnorm_backward")
        return _logical(dx, hidden), dw, db, dms, None, None, None


def graph_colnorm(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor, mean_scale: torch.Tensor, eps: float = 1e-5,
                  relu: bool = False, cache: Optional[torch.Tensor] = None):
    """-> (y [n, hidden], stats [2, hidden] = mean | var as used)."""
    _require_cuda(x, "x")
    out, stats = GraphColNormFn.apply(x, weight, bias, mean_scale, eps, relu, cache)
    out._hexgnn_hp = padded_width(int(x.shape[1]))
    return out, stats


# ------------------------------------------------------------------------------------------------
# head tail (advantage linear + pooling + value MLP + dueling combine)
# ------------------------------------------------------------------------------------------------

class HeadTailFn(torch.autograd.Function):
    """mode 0: Q [n]; mode 1: (V [b], A - mean(A) [n]); mode 2: 2*tanh(adv) [n]; mode 3: raw (value [b], advantages [n])
    of HeadNetwork.forward; mode 4: raw advantages [n] only.  GN0/models.py:368-384,567-584."""

    @staticmethod
    def forward(ctx, h, gptr, b: int, hidden: int, mode: int, lin_w, lin_b, v0_w, v0_b, v1_w, v1_b):
        L = _lib.lib()
        dev = h.device
        n = int(h.shape[0])
        hp = padded_width(hidden)
        hpad = as_padded(h, hidden, trust_pads=False)
        ps = [_f32c(p) for p in (lin_w, lin_b, v0_w, v0_b, v1_w, v1_b)]
        q = torch.empty(n, dtype=torch.float32, device=dev)
        out_v = torch.empty(b, dtype=torch.float32, device=dev) if mode in (1, 3) else None
        saved = _bytes(L.hexgnn_head_saved_bytes(n, b, hidden), dev)
        _lib.check(L.hexgnn_head_forward(
            n, b, hidden, mode, gptr.data_ptr(), hpad.data_ptr(), ps[0].data_ptr(), ps[1].data_ptr(),
            ps[2].data_ptr(), ps[3].data_ptr(), ps[4].data_ptr(), ps[5].data_ptr(), q.data_ptr(),
            out_v.data_ptr() if out_v is not None else None, saved.data_ptr(), _stream()), "hexgnn_head_forward")
        ctx.dims = (n, b, hidden, mode, hp)
        ctx.bufs = (hpad, gptr, saved, ps)
        if mode in (1, 3):
            return out_v, q
        return q

    @staticmethod
    def backward(ctx, *gouts):
        L = _lib.lib()
        n, b, hidden, mode, hp = ctx.dims
        hpad, gptr, saved, ps = ctx.bufs
        dev = hpad.device
        if mode in (1, 3):
            d_v, dq = gouts
            if d_v is None:
                d_v = torch.zeros(b, dtype=torch.float32, device=dev)
            if dq is None:
                dq = torch.zeros(n, dtype=torch.float32, device=dev)
            d_v = d_v.float().contiguous()
        else:
            (dq,) = gouts
            d_v = None
        dq = dq.float().contiguous()
        dh = torch.empty((n, hp), dtype=torch.float32, device=dev)
        g = [torch.empty_like(p) for p in ps]
        ws_bytes = L.hexgnn_head_backward_workspace_bytes(n, b, hidden)
        ws = _bytes(ws_bytes, dev)
        _lib.check(L.hexgnn_head_backward(
            n, b, hidden, mode, gptr.data_ptr(), hpad.data_ptr(), ps[0].data_ptr(), ps[2].data_ptr(),
            ps[4].data_ptr(), saved.data_ptr(), dq.data_ptr(), d_v.data_ptr() if d_v is not None else None,
            dh.data_ptr(), g[0].data_ptr(), g[1].data_ptr(), g[2].data_ptr(), g[3].data_ptr(), g[4].data_ptr(),
            g[5].data_ptr(), ws.data_ptr(), ws_bytes, _stream()), "hexgnn_head_backward")
        if mode in (2, 4):   # value path unused: no gradient for the value head (reference: grads stay None)
            g[2] = g[3] = g[4] = g[5] = None
        return (_logical(dh, hidden), None, None, None, None) + tuple(g)


class HeadLinearTailFn(torch.autograd.Function):
    """The head tail of the ``two_headed`` family: value_head_type="linear" over ("mean",) pooling (GN0/models.py:319-330,
    374-384), same modes as HeadTailFn.  C ABI ``hexgnn_head_linear_*``."""

    @staticmethod
    def forward(ctx, h, gptr, b: int, hidden: int, mode: int, lin_w, lin_b, val_w, val_b):
        L = _lib.lib()
        dev = h.device
        n = int(h.shape[0])
        hp = padded_width(hidden)
        hpad = as_padded(h, hidden, trust_pads=False)
        ps = [_f32c(p) for p in (lin_w, lin_b, val_w, val_b)]
        q = torch.empty(n, dtype=torch.float32, device=dev)
        out_v = torch.empty(b, dtype=torch.float32, device=dev) if mode in (1, 3) else None
        saved = _bytes(L.hexgnn_head_linear_saved_bytes(n, b), dev)
        _lib.check(L.hexgnn_head_linear_forward(
            n, b, hidden, mode, gptr.data_ptr(), hpad.data_ptr(), ps[0].data_ptr(), ps[1].data_ptr(), ps[2].data_ptr(),
            ps[3].data_ptr(), q.data_ptr(), out_v.data_ptr() if out_v is not None else None, saved.data_ptr(), _stream()),
            "hexgnn_head_linear_forward")
        ctx.dims = (n, b, hidden, mode, hp)
        ctx.bufs = (hpad, gptr, saved, ps)
        if mode in (1, 3):
            return out_v, q
        return q

    @staticmethod
    def backward(ctx, *gouts):
        L = _lib.lib()
        n, b, hidden, mode, hp = ctx.dims
        hpad, gptr, saved, ps = ctx.bufs
        dev = hpad.device
        if mode in (1, 3):
            d_v, dq = gouts
            if d_v is None:
                d_v = torch.zeros(b, dtype=torch.float32, device=dev)
            if dq is None:
                dq = torch.zeros(n, dtype=torch.float32, device=dev)
            d_v = d_v.float().contiguous()
        else:
            (dq,) = gouts
            d_v = None
        dq = dq.float().contiguous()
        dh = torch.empty((n, hp), dtype=torch.float32, device=dev)
        g = [torch.empty_like(p) for p in ps]
        ws_bytes = L.hexgnn_head_linear_backward_workspace_bytes(n, b, hidden)
        ws = _bytes(ws_bytes, dev)
        _lib.check(L.hexgnn_head_linear_backward(
            n, b, hidden, mode, gptr.data_ptr(), hpad.data_ptr(), ps[0].data_ptr(), ps[2].data_ptr(), saved.data_ptr(),
            dq.data_ptr(), d_v.data_ptr() if d_v is not None else None, dh.data_ptr(), g[0].data_ptr(), g[1].data_ptr(),
            g[2].data_ptr(), g[3].data_ptr(), ws.data_ptr(), ws_bytes, _stream()), "hexgnn_head_linear_backward")
        if mode in (2, 4):
            g[2] = g[3] = None
        return (_logical(dh, hidden), None, None, None, None) + tuple(g)


# ------------------------------------------------------------------------------------------------
# HexAra policy head pieces (GN0/torch_script_models.py:286-379)
# ------------------------------------------------------------------------------------------------

class SageScalarFn(torch.autograd.Function):
    """SAGEConv(H, 1), the last layer of the HexAra policy head: ``b + wr . h_i + mean_{j in N(i)} wl . h_j`` -> [n]."""

    @staticmethod
    def forward(ctx, h, gs: GraphStructure, hidden: int, wl, bl, wr):
        L = _lib.lib()
        dev = h.device
        n = int(h.shape[0])
        hpad = as_padded(h, hidden, trust_pads=False)
        ps = [_f32c(p) for p in (wl, bl, wr)]
        out = torch.empty(n, dtype=torch.float32, device=dev)
        dots = torch.empty((n, 2), dtype=torch.float32, device=dev)
        _lib.check(L.hexgnn_sage_scalar_forward(n, hidden, gs.rowptr.data_ptr(), gs.col.data_ptr(), gs.invdeg.data_ptr(),
                                                hpad.data_ptr(), ps[0].data_ptr(), ps[2].data_ptr(), ps[1].data_ptr(),
                                                out.data_ptr(), dots.data_ptr(), _stream()), "hexgnn_sage_scalar_forward")
        ctx.gs = gs
        ctx.dims = (n, hidden)
        ctx.bufs = (hpad, ps)
        return out

    @staticmethod
    def backward(ctx, dout):
        L = _lib.lib()
        n, hidden = ctx.dims
        hpad, ps = ctx.bufs
        gs = ctx.gs
        dev = hpad.device
        hp = padded_width(hidden)
        dout = dout.float().contiguous()
        dh = torch.empty((n, hp), dtype=torch.float32, device=dev)
        g = [torch.empty_like(p) for p in ps]
        ws_bytes = L.hexgnn_sage_scalar_backward_workspace_bytes(n, hidden)
        ws = _bytes(ws_bytes, dev)
        _lib.check(L.hexgnn_sage_scalar_backward(n, hidden, gs.rowptr_t.data_ptr(), gs.col_t.data_ptr(), gs.invdeg.data_ptr(),
                                                 hpad.data_ptr(), ps[0].data_ptr(), ps[2].data_ptr(), dout.data_ptr(),
                                                 dh.data_ptr(), g[0].data_ptr(), g[2].data_ptr(), g[1].data_ptr(),
                                                 ws.data_ptr(), ws_bytes, _stream()), "hexgnn_sage_scalar_backward")
        return _logical(dh, hidden), None, None, g[0], g[1], g[2]


def sage_scalar(h: torch.Tensor, gs: GraphStructure, hidden: int, conv) -> torch.Tensor:
    _require_cuda(h, "h")
    return SageScalarFn.apply(h, gs, hidden, conv.lin_l.weight, conv.lin_l.bias, conv.lin_r.weight)


class PolicyLogSoftmaxFn(torch.autograd.Function):
    """Terminal rows dropped, swap logits inserted, scatter_log_softmax per graph (torch_script_models.py:326-378).
    -> (pi [capacity], output_graph_indices [capacity], output_batch_ptr [b+1]); the caller trims to output_batch_ptr[-1]."""

    @staticmethod
    def forward(ctx, pi_raw, should_swap, x, gptr, b: int, swap_allowed: bool):
        L = _lib.lib()
        dev = pi_raw.device
        n = int(pi_raw.shape[0])
        pi_raw = pi_raw.float().contiguous()
        ss = should_swap.float().contiguous() if should_swap is not None else None
        cap = max(n - 2 * b + (b if swap_allowed else 0), 0)
        out_pi = torch.empty(cap, dtype=torch.float32, device=dev)
        out_gi = torch.empty(cap, dtype=torch.int64, device=dev)
        out_ptr = torch.empty(b + 1, dtype=torch.int64, device=dev)
        xs = x if (x.dtype == torch.float32 and x.stride(1) == 1) else x.float().contiguous()
        _lib.check(L.hexgnn_policy_log_softmax_forward(
            n, b, gptr.data_ptr(), xs.data_ptr(), xs.stride(0) if n > 0 else 3, int(swap_allowed), pi_raw.data_ptr(),
            ss.data_ptr() if ss is not None else None, out_pi.data_ptr(), out_gi.data_ptr(), out_ptr.data_ptr(), _stream()),
            "hexgnn_policy_log_softmax_forward")
        ctx.dims = (n, b, bool(swap_allowed), cap)
        ctx.bufs = (gptr, xs, out_ptr, out_pi)
        ctx.mark_non_differentiable(out_gi, out_ptr)
        return out_pi, out_gi, out_ptr

    @staticmethod
    def backward(ctx, d_pi, _dgi, _dptr):
        L = _lib.lib()
        n, b, swap_allowed, cap = ctx.dims
        gptr, xs, out_ptr, out_pi = ctx.bufs
        dev = out_pi.device
        d_pi = d_pi.float().contiguous()
        d_raw = torch.empty(n, dtype=torch.float32, device=dev)
        d_ss = torch.empty(b, dtype=torch.float32, device=dev) if swap_allowed else None
        _lib.check(L.hexgnn_policy_log_softmax_backward(
            n, b, gptr.data_ptr(), xs.data_ptr(), xs.stride(0) if n > 0 else 3, int(swap_allowed), out_ptr.data_ptr(),
            out_pi.data_ptr(), d_pi.data_ptr(), d_raw.data_ptr(), d_ss.data_ptr() if d_ss is not None else None, _stream()),
            "hexgnn_policy_log_softmax_backward")
        return d_raw, d_ss, None, None, None, None


# ------------------------------------------------------------------------------------------------
# fused per-graph path: whole network in one launch per direction (graphs <= 128 nodes, hidden <= 112)
# ------------------------------------------------------------------------------------------------

_FUSED_ENABLED = True
_MATH = 0     # 0 = exact fp32 MFMA, 1 = split precision "f16x3" (fused kernels only)


def set_math(mode) -> None:
    """Arithmetic of the fused kernels' contractions: "fp32" (exact fp32 MFMA, default) or "f16x3" (fp32 operands
    scaled by exact powers of two and split into fp16 hi+lo pairs = 22 significand bits, three f16 MFMAs per product
    block, fp32 accumulation; ~1e-6 relative)."""
    global _MATH
    _MATH = {"fp32": 0, 0: 0, "f16x3": 1, 1: 1}[mode]


def get_math() -> str:
    return "f16x3" if _MATH == 1 else "fp32"


def set_fused(enabled: bool) -> None:
    """Enable/disable the fused per-graph kernels (tests exercise both paths)."""
    global _FUSED_ENABLED
    _FUSED_ENABLED = bool(enabled)


_ONE_LAUNCH_STEP = True


def set_one_launch_step(enabled: bool) -> None:
    """``td_step``'s fused form as ONE launch for the forward, the TD loss and the backward's data chain
    (``hexgnn_qnet_call_forward`` with ``chain_backward``: a workgroup runs its graph's backward chain right behind its forward)
    instead of two.  Same bits; taken in exact fp32 without ``defer_lower``, a grad-stage hook or ``x._hex_live_rows`` (tests
    and A/B switch it)."""
    global _ONE_LAUNCH_STEP
    _ONE_LAUNCH_STEP = bool(enabled)


_GRAD_STAGE_HOOK = None


def set_grad_stage_hook(fn) -> None:
    """``fn(flat, lo, hi)`` is called INSIDE the fused backward as soon as the gradient elements ``flat[lo:hi]`` are final
    (their kernels are enqueued on the current stream) while the weight-gradient GEMM of the remaining layers is still
    to be enqueued: ``gnn_hex_amd.dist.GradSync.enable_overlap`` starts that segment's all-reduce there.
    None switches the staging off (one backward call, one reduce launch)."""
    global _GRAD_STAGE_HOOK
    _GRAD_STAGE_HOOK = fn


_SUPPORTED = {}


def qnet_fused_supported(c_in: int, hidden: int, max_nodes: int) -> bool:
    if not _FUSED_ENABLED:
        return False
    key = (c_in, hidden, max_nodes)
    ok = _SUPPORTED.get(key)
    if ok is None:
        if len(_SUPPORTED) > 4096:
            _SUPPORTED.clear()
        ok = _SUPPORTED[key] = bool(_lib.lib().hexgnn_qnet_supported(int(c_in), int(hidden), int(max_nodes)))
    return ok


# ------------------------------------------------------------------------------------------------
# the fused Q-network call: one forward (qnet_forward), one backward (qnet_backward), two autograd forms
# ------------------------------------------------------------------------------------------------
# The direct-gradient form (QNetDirectFn, the eager step an unmodified train.py issues): the parameters are NOT autograd
# inputs -- handing 57 parameter tensors to autograd and receiving 57 gradients back cost ~0.45 ms of Python + autograd per
# step (66 AccumulateGrad nodes), which left GNN-S host-bound at 0.8 M graphs/s against 2 M replayed.  The function has ONE
# differentiable input (a per-model anchor), the forward call uses pointer arrays cached per (model, head) -- re-validated by
# data_ptr every call, 57 C-level calls -- and the backward writes every gradient into ONE flat buffer
# (``hexgnn_qnet_call_backward``: base pointer + cached offset table) and assigns the views to ``p.grad`` itself
# (accumulating when a gradient is already there, like AccumulateGrad).  Not usable with ``torch.autograd.grad(loss,
# parameters)`` or hooks on parameters: the model takes the autograd form (QNetFusedFn: parameters are inputs, the same flat
# buffer's views are returned) when it finds hooks, frozen or non-leaf parameters, or after ``set_direct_grads(False)``.
# Same kernels, same bits.
_DIRECT_GRADS = True


def set_direct_grads(enabled: bool) -> None:
    global _DIRECT_GRADS
    _DIRECT_GRADS = bool(enabled)


_FREE_RC = None


def _free_refcount() -> int:
    """What ``sys.getrefcount(v)`` returns inside ``for v in views`` for an object that only the tuple ``views`` holds (3 on
    CPython 3.10: the tuple, the loop variable, the call's argument) -- measured, not assumed."""
    global _FREE_RC
    if _FREE_RC is None:
        probe = (object(),)
        for v in probe:
            _FREE_RC = sys.getrefcount(v)
    return _FREE_RC


class QNetParamCache:
    """Per (model, head): the parameter list of the fused call, its cached pointer arrays and the flat gradient layout."""
    __slots__ = ("params", "ptrs", "wl", "bl", "wr", "wlp", "tail", "flat_params", "offsets", "offsets_p", "total", "direct_ok",
                 "tot", "sizes", "cut", "grad_ring")

    def __init__(self, params, tot):
        self.params = params
        self.tot = tot
        self.ptrs = None
        self.sizes = {}          # (layered, n, b) -> buffer sizes of the fused calls (qnet_forward)
        self.grad_ring = []      # [(flat gradient buffer, its per-parameter views, stream, storage use count)]: grad_buffer()
        self.refresh()

    def grad_buffer(self, dev):
        """The flat buffer the backward writes and its per-parameter views.  A training loop drops its gradients every step
        (``zero_grad(set_to_none=True)`` / ``p.grad = None``) and the next backward allocates them again: 60 views through
        ``unflatten_dense_tensors`` cost 25 us per step -- a sixth of the host time of an eager GNN-S step.  A buffer of an
        earlier backward is handed out again when NOBODY references any of its views any more (Python reference counts: the
        ring's own tuple only), which is exactly when autograd's freshly allocated gradients would be indistinguishable
        from it; a view still held anywhere (``p.grad`` not cleared, a list of gradients kept for logging) leaves that buffer
        alone (``Tensor._use_count()`` sees the holders Python reference counts do not: ``.grad`` itself), and so does any
        other tensor on the buffer's storage (``p.grad.detach()``, ``.data``, ``.view(-1)``, a slice of the buffer: the
        storage's use count is then above the one recorded when the buffer was made).  Not inside a HIP-graph capture (those
        gradients must come from the graph's pool)."""
        if torch.cuda.is_current_stream_capturing():
            return torch.empty(self.total, dtype=torch.float32, device=dev), None
        rc = sys.getrefcount
        free_rc = _free_refcount()
        st = _stream()
        for flat, views, owner, uses in self.grad_ring:
            if owner == st and flat.device == dev:      # (same stream only: the caching allocator's rule for a freed block)
                for v in views:
                    # Python side: the tuple, the loop variable, the argument (measured once, _free_refcount); C++ side (a .grad, a
                    # saved tensor): the wrapper only
                    if rc(v) != free_rc or v._use_count() != 1:
                        break
                else:
                    if torch._C._storage_Use_Count(flat.untyped_storage()._cdata) == uses:
                        return flat, views
        flat = torch.empty(self.total, dtype=torch.float32, device=dev)
        views = tuple(torch._C._nn.unflatten_dense_tensors(flat, self.flat_params))
        if len(self.grad_ring) >= 3:
            self.grad_ring.pop(0)
        self.grad_ring.append((flat, views, st, torch._C._storage_Use_Count(flat.untyped_storage()._cdata)))
        return flat, views

    def refresh(self):
        params, tot = self.params, self.tot
        self.ptrs = list(map(torch.Tensor.data_ptr, params))
        vp = C.c_void_p * tot
        pt = self.ptrs
        self.wl, self.bl, self.wr = vp(*pt[0:3 * tot:3]), vp(*pt[1:3 * tot:3]), vp(*pt[2:3 * tot:3])
        self.wlp = (C.addressof(self.wl), C.addressof(self.bl), C.addressof(self.wr))      # (what a descriptor holds of them)
        self.tail = tuple(pt[3 * tot:])
        nconv = 3 * tot
        order = list(range(nconv)) + [nconv + 2, nconv + 3, nconv + 4, nconv + 5, nconv + 0, nconv + 1]   # parameters() order
        offs, o = [0] * len(params), 0
        for i in order:
            offs[i] = o
            o += params[i].numel()
        self.flat_params = [params[i] for i in order]
        self.offsets = (C.c_int64 * len(params))(*offs)
        self.offsets_p = C.addressof(self.offsets)
        self.total = o
        self.grad_ring = []
        self.cut = offs[3 * (1 + tot // 2)] if tot >= 3 else 0      # flat position where the staged backward splits
        # (post-accumulate-grad hooks -- optimizer-in-backward, FSDP-style reducers -- hang off AccumulateGrad, which the direct
        # path never runs: such parameters take the autograd form, like tensor hooks do)
        self.direct_ok = all(p.is_leaf and p.requires_grad and p.dtype == torch.float32 and p.is_contiguous() and p.is_cuda
                             and not p._backward_hooks and not getattr(p, "_post_accumulate_grad_hooks", None) for p in params)

    def valid(self) -> bool:
        """Pointers unchanged (parameters updated in place keep them; ``.to()`` / ``p.data = ...`` do not) and the flags
        ``direct_ok`` was derived from still hold (a parameter frozen or given a tensor hook since)."""
        ps = self.params
        return list(map(torch.Tensor.data_ptr, ps)) == self.ptrs and \
            self.direct_ok == all(p.requires_grad and not p._backward_hooks and
                                  not getattr(p, "_post_accumulate_grad_hooks", None) for p in ps)


class _QNetCall:
    """Everything one fused forward leaves behind for its backward (plain attributes: cheaper than ctx.save_for_backward).
    ``assign``: the direct form (the backward assigns ``p.grad``) rather than the autograd form (it returns the gradients);
    ``nonleaf``: a parameter of the call is computed per forward (no staging, see qnet_backward); ``live``: td_step() over
    capacity-sized buffers -- the 1-element int32 device tensor that holds the live row count (``x._hex_live_rows``).

    ``desc``: the call's ``hexgnn_qnet_call`` (``layered``: the stack's ``hexgnn_sage_stack_call``, which reads the graph arrays,
    the table and groups of ``gs``, x, ``bufs`` and ``keep``), filled by the forward; the backward sets its backward group.  It
    holds raw addresses, and these attributes keep what they point at alive for as long as it can be used: ``x``: x; ``gs`` and
    ``gptr``: the graph arrays and the status word; ``bufs``: acts | wpack | saved; ``cache``: the parameters (``cache.params``);
    ``keep``: the pointer arrays wl / bl / wr the forward was given (``cache.refresh()`` replaces the cache's own); ``td``: td_dq |
    td_out | td_loss_part | td_loss; ``live``: n_live; ``step_ws``: workspace and d_embeds of a chained forward until the backward
    takes them.  td_sel / td_target / td_weights and q / out_v are read and written by the forward launch only, which is
    enqueued before ``qnet_forward`` returns.  What the backward adds (dq, d_out_v, d_embeds, flat, workspace, ``cache.offsets``)
    lives through ``qnet_backward``, which issues every launch that reads it -- except a deferred lower half, for which
    ``pending`` holds flat, the workspace, d_embeds and the offsets table until ``finish_backward``."""
    __slots__ = ("cache", "gs", "gptr", "dims", "x", "bufs", "math", "sink", "gp", "done", "layered", "td", "pending", "versions",
                 "assign", "nonleaf", "live", "step_ws", "desc", "keep")


def qnet_forward(cache: QNetParamCache, x, gs: GraphStructure, gptr, b: int, c_in: int, hidden: int, body_layers: int,
                 head_layers: int, mode: int, need_bwd: bool, layered: bool = False, assign: bool = True):
    """Launch the fused forward with the cache's pointer arrays; returns (q, out_v, call) -- ``call`` feeds qnet_backward.
    ``gptr`` may be None when ``gs`` comes from ``GraphStructure.grouped`` (it carries the pointer), and ``gs`` may be the
    deferred grouped build's arguments (models.py): the build then runs here, with the weight pack in the same launch.

    ``layered``: the same network on the layer-major kernels (graphs above 128 nodes, hidden 113..128): body + head SAGE layers
    as ONE stack of body_layers + head_layers layers (``hexgnn_sage_stack_call_forward``; the head's gnn is just more SAGE
    layers with ReLU), then the head tail (``hexgnn_head_forward``).  Against the per-module composition (body stack, head
    stack, head tail as three autograd functions) the backward has ONE batched weight-gradient GEMM + ONE slab reduce over all
    hidden layers instead of two of each, no stack-boundary combine, and ~1 ms less Python per step.

    ``assign``: see _QNetCall; td_step()'s loss in the forward kernel's tail is taken by the direct form only."""
    L = _lib.lib()
    dev = x.device
    n = x.shape[0]
    tot = body_layers + head_layers
    if x.dtype != torch.float32 or x.stride(1) != 1:
        x = x.float().contiguous()
    x_stride = x.stride(0) if n > 0 else c_in
    key = (layered, n, b)
    sizes = cache.sizes.get(key)
    if sizes is None:
        # (hp, activations, weight pack, saved state, backward workspace): C queries once per batch shape
        hp = padded_width(hidden)
        if layered:
            al = lambda v: (max(int(v), 16) + 255) & ~255
            s_bytes = al(L.hexgnn_sage_stack_saved_bytes(n, c_in, hidden, tot))
            sizes = (hp, al(4 * tot * n * hp), al(L.hexgnn_sage_stack_pack_bytes(c_in, hidden, tot)),
                     s_bytes + al(L.hexgnn_head_saved_bytes(n, b, hidden)),
                     (s_bytes, al(L.hexgnn_sage_stack_backward_workspace_bytes(n, c_in, hidden, tot)),
                      al(L.hexgnn_head_backward_workspace_bytes(n, b, hidden))))
        else:
            sizes = (hp, (4 * tot * n * hp + 255) & ~255, (L.hexgnn_sage_stack_pack_bytes(c_in, hidden, tot) + 255) & ~255,
                     max(L.hexgnn_qnet_saved_bytes(n, b, c_in, hidden, tot), 16),
                     max(L.hexgnn_qnet_backward_workspace_bytes(n, b, c_in, hidden, tot), 16))
        if len(cache.sizes) > 64:
            cache.sizes.clear()
        cache.sizes[key] = sizes
    hp, a_bytes, w_bytes, s_bytes, bwd_bytes = sizes
    # [acts | wpack | saved] in ONE allocation (256-byte aligned parts)
    buf = torch.empty(a_bytes + w_bytes + s_bytes, dtype=torch.uint8, device=dev)
    base = buf.data_ptr()
    wpack, saved = base + a_bytes, base + a_bytes + w_bytes
    q = torch.empty(n, dtype=torch.float32, device=dev)
    out_v = torch.empty(b, dtype=torch.float32, device=dev) if mode == 1 else None
    wl, bl, wr = cache.wl, cache.bl, cache.wr
    if type(gs) is tuple:       # deferred grouped build: CSR + weight pack in one launch, now that wpack exists
        if (hidden <= 128) if layered else (_MATH == 0):        # (layered: the packed layout exists up to 128)
            gs = GraphStructure.grouped(gs[0], gs[1], gs[2], gs[3], pack=(c_in, hidden, tot, wl, bl, wr, wpack),
                                        device_blocks=layered)
            wl = bl = wr = None
        else:
            gs = GraphStructure.grouped(*gs)
    gp = gs._ptrs
    if gp is None:
        gp = (gs.rowptr.data_ptr(), gs.col.data_ptr(), gs.rowptr_t.data_ptr(), gs.col_t.data_ptr(), gs.invdeg.data_ptr(),
              gptr.data_ptr(), gs.status.data_ptr())
    t = cache.tail
    stream = _stream()
    td = live = step_ws = None
    if layered:
        desc = _stack_call(gs, gp, n, c_in, hidden, tot, x.data_ptr(), x_stride, cache.wlp if wl is not None else (None,) * 3,
                           wpack, base, saved, need_bwd)
        _lib.check(L.hexgnn_sage_stack_call_forward(desc, stream), "hexgnn_sage_stack_call_forward")
        _lib.check(L.hexgnn_head_forward(n, b, hidden, mode, gp[5], base + 4 * (tot - 1) * n * hp, t[0], t[1], t[2], t[3],
                                         t[4], t[5], q.data_ptr(), out_v.data_ptr() if out_v is not None else None,
                                         saved + bwd_bytes[0], stream), "hexgnn_head_forward")
    else:
        tda = getattr(_TD_STEP, "args", None) if assign else None
        # the differences between the three forms, as field values: the TD tail, the chained backward's workspace and d_embeds
        tdf = (None, None, None, 0, None, None, None)
        acts_layer, ws_p, demb_p = body_layers - 1, None, None
        if tda is not None and mode == 0 and need_bwd and b > 0 and n > 0 and tda[0].numel() == b:
            # td_step(): the update's loss is formed in the forward kernel's tail (one selected node per graph)
            sel, tgt, w, lfn = tda
            # one buffer: dq [n] | td [b] | loss terms [b] | loss [1]
            tb = torch.empty(n + 2 * b + 1, dtype=torch.float32, device=dev)
            tp = tb.data_ptr()
            tdf = (sel.data_ptr(), tgt.data_ptr(), w.data_ptr() if w is not None else None, lfn, tp, tp + 4 * n, tp + 4 * (n + b))
            acts_layer = -1
            live = getattr(_TD_STEP, "live", None)
            if _ONE_LAUNCH_STEP and _MATH == 0 and live is None and getattr(_TD_STEP, "whole", False):
                # the backward's data chain in the same launch: its workspace exists from here on (qnet_backward runs the rest)
                # (and the gradient of the body's output, which the model's activations hook receives in qnet_backward)
                step_ws = (torch.empty(bwd_bytes, dtype=torch.uint8, device=dev),
                           torch.empty((n, hp), dtype=torch.float32, device=dev))
                ws_p, demb_p = step_ws[0].data_ptr(), step_ws[1].data_ptr()
            td = (tb, n, b)
        wlp = cache.wlp if wl is not None else (None, None, None)
        desc = _lib.QNetCall(
            _lib.QNET_CALL_BYTES, n, b, c_in, hidden, tot, body_layers, mode, _MATH, x_stride, int(need_bwd), acts_layer,
            gp[5], gp[0], gp[1], gp[2], gp[3], gp[4], x.data_ptr(),
            wlp[0], wlp[1], wlp[2], t[0], t[1], t[2], t[3], t[4], t[5],
            wpack, base, saved, ws_p, bwd_bytes,
            q.data_ptr(), out_v.data_ptr() if out_v is not None else None, gp[6],
            tdf[0], tdf[1], tdf[2], tdf[3], tdf[4], tdf[5], tdf[6], None,
            None, None, demb_p, None, None, None)
        _lib.check(L.hexgnn_qnet_call_forward(desc, int(step_ws is not None), stream), "hexgnn_qnet_call_forward")
    call = _QNetCall()
    call.desc, call.keep = desc, (wl, bl, wr)
    call.cache, call.gs, call.gptr, call.x = cache, gs, gptr, x
    # (bwd_bytes: the fused backward's workspace bytes; layered: (stack saved, stack workspace, head workspace) bytes)
    call.dims = (n, b, c_in, hidden, tot, body_layers, mode, hp, x_stride, a_bytes, w_bytes, bwd_bytes)
    call.bufs, call.math, call.gp = buf, 0 if layered else _MATH, gp
    call.sink, call.done, call.layered, call.td, call.pending = None, False, layered, td, None
    call.assign, call.nonleaf, call.live, call.step_ws = assign, False, live, step_ws
    # the backward reads the head tail's weights LIVE (the SAGE layers' from the pack made by this forward): an in-place update
    # between the two would mix old and new weights without autograd's saved-tensor version check to notice it
    call.versions = tuple(p._version for p in cache.params[-6:]) if need_bwd else None
    return q, out_v, call


def _assign_flat_grads(cache: QNetParamCache, flat: torch.Tensor, mode: int, views=None) -> None:
    """Views of the flat gradient buffer -> ``p.grad`` (accumulating into a gradient that is already there)."""
    fp = cache.flat_params
    if views is None:
        views = torch._C._nn.unflatten_dense_tensors(flat, fp)
    skip = mode == 2          # advantages only: the value head (flat positions -6 .. -3) has no gradient
    k_lo, k_hi = len(fp) - 6, len(fp) - 2
    for k, (p, v) in enumerate(zip(fp, views)):
        if skip and k_lo <= k < k_hi:
            continue
        g = p.grad
        p.grad = v if g is None else g + v


def qnet_embeds(call: _QNetCall) -> torch.Tensor:
    """final_conv_acts of a fused forward: the body output as a [n, hidden] view of the activation slab."""
    n, b, c_in, hidden, tot, body_layers, mode, hp = call.dims[:8]
    acts = call.bufs[:4 * tot * n * hp].view(torch.float32).view(tot, n, hp)
    return acts[body_layers - 1][:, :hidden]


def qnet_backward(call: _QNetCall, dq, d_v=None, defer_lower: bool = False):
    """The fused backward of a fused forward: every parameter gradient into ONE flat buffer (the layout of
    ``model.parameters()``, so that GradSync can all-reduce it in place).  The direct form (``call.assign``) assigns the views
    to ``p.grad`` (accumulated when a gradient is already there) and returns None; called by autograd (QNetDirectFn.backward,
    on the engine's device thread) or straight from ``ops.backward(loss)`` on the caller's thread.  The autograd form returns
    the views in the call's parameter order (None for the value head in mode 2), from a fresh buffer every time.

    Staging (fused kernels only): with a stage hook installed (``set_grad_stage_hook``) or ``defer_lower``, the first stage
    runs the data chain, the small reduces and the weight gradients of the upper half of the hidden layers -- the TAIL of the
    flat buffer is then final.  The hook gets that segment (all-reduce on the collective's own stream) while the lower half's
    weight-gradient GEMM is enqueued behind it, then the head of the buffer; ``defer_lower`` leaves the lower half to
    ``finish_backward(call)`` instead (a step captured as two HIP graphs split there lets the tail's all-reduce travel while
    the second graph computes: graphs.GraphedSplitStep).  Not for non-leaf parameters (``--noisy_dqn=True``: d_sigma = d_w *
    eps with per-rank noise is not the average of the ranks' d_sigma if d_w is averaged first, and the mu / sigma gradients
    live outside the flat buffer; GradSync reduces the finished .grad tensors through its bucket)."""
    call.pending = None
    if call.versions is not None and call.versions != tuple(p._version for p in call.cache.params[-6:]):
        raise RuntimeError("a head parameter of the model was modified in place between this forward and its backward (the "
                           "fused backward reads the head tail's weights live); run the backward before optimizer.step()")
    if call.done:
        raise RuntimeError("this forward's backward already ran through ops.backward(loss) (its graph is spent, as after "
                           "loss.backward() without retain_graph)")
    L = _lib.lib()
    cache = call.cache
    n, b, c_in, hidden, tot, body_layers, mode, hp, x_stride, a_bytes, w_bytes, bwd_bytes = call.dims
    dev = call.x.device
    if mode == 1:
        d_v = torch.zeros(b, dtype=torch.float32, device=dev) if d_v is None else d_v.float().contiguous()
    else:
        d_v = None
    dq = torch.zeros(n, dtype=torch.float32, device=dev) if dq is None else _f32c(dq)
    if call.assign:
        flat, gviews = cache.grad_buffer(dev)
    else:
        flat, gviews = torch.empty(cache.total, dtype=torch.float32, device=dev), None
    base, gp, t, fb = call.bufs.data_ptr(), call.gp, cache.tail, flat.data_ptr()
    live = call.live
    if live is not None and (call.layered or call.math != 0 or call.td is None or dq.data_ptr() != call.td[0].data_ptr()
                             or defer_lower or _GRAD_STAGE_HOOK is not None):
        raise NotImplementedError("a device-side live row count (x._hex_live_rows) is taken by td_step()'s fused form in exact "
                                  "fp32 only: no layer-major path, no set_math(\"f16x3\"), no staged backward")
    if call.layered:
        s_bytes, ws_bytes, hws_bytes = bwd_bytes
        ws = torch.empty(ws_bytes + hws_bytes, dtype=torch.uint8, device=dev)
        # the head tail writes dh * [h > 0] = G of the top layer straight into its slab of the stack's workspace
        # (HEXGNN_HEAD_MASK_DH / HEXGNN_SAGE_DY_IN_PLACE: no masked copy in between)
        dh_ptr = ws.data_ptr() + 4 * (tot - 1) * n * hp
        d_emb = torch.empty((n, hp), dtype=torch.float32, device=dev) if (call.sink is not None and body_layers < tot) else None
        offs = cache.offsets
        tp = [fb + 4 * offs[3 * tot + k] for k in range(6)]          # d_lin_w, d_lin_b, d_v0_w, d_v0_b, d_v1_w, d_v1_b
        vh = mode != 2
        stream = _stream()
        h_top = base + 4 * (tot - 1) * n * hp
        _lib.check(L.hexgnn_head_backward(n, b, hidden, mode | 8, gp[5], h_top, t[0], t[2], t[4],
                                          base + a_bytes + w_bytes + s_bytes, dq.data_ptr(),
                                          d_v.data_ptr() if d_v is not None else None, dh_ptr, tp[0], tp[1],
                                          tp[2] if vh else None, tp[3] if vh else None, tp[4] if vh else None,
                                          tp[5] if vh else None, ws.data_ptr() + ws_bytes, hws_bytes, stream),
                   "hexgnn_head_backward")
        vp = C.c_void_p * tot
        d_wl = vp(*[fb + 4 * offs[3 * l] for l in range(tot)])
        d_bl = vp(*[fb + 4 * offs[3 * l + 1] for l in range(tot)])
        d_wr = vp(*[fb + 4 * offs[3 * l + 2] for l in range(tot)])
        desc = call.desc          # (the stack's hexgnn_sage_stack_call; everything set here lives until the call below returns)
        desc.flags, desc.dy, desc.workspace, desc.workspace_bytes = 2, dh_ptr, ws.data_ptr(), ws_bytes
        desc.d_wl, desc.d_bl, desc.d_wr = C.addressof(d_wl), C.addressof(d_bl), C.addressof(d_wr)
        desc.tap_layer, desc.tap_out = (body_layers - 1, d_emb.data_ptr()) if d_emb is not None else (-1, None)
        _lib.check(L.hexgnn_sage_stack_call_backward(desc, stream), "hexgnn_sage_stack_call_backward")
    else:
        ws_bytes = bwd_bytes
        td = call.td
        # the chained forward ran the data chain: the remaining stages work on its workspace
        chained = call.step_ws is not None and td is not None and dq.data_ptr() == td[0].data_ptr() \
            and not defer_lower and _GRAD_STAGE_HOOK is None
        if chained:
            ws, d_emb = call.step_ws
            call.step_ws = True          # (the chain's results are taken; tests look at this)
            if call.sink is None:
                d_emb = None
        else:
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
            d_emb = torch.empty((n, hp), dtype=torch.float32, device=dev) if call.sink is not None else None
        offsets = cache.offsets
        desc = call.desc
        desc.dq, desc.d_out_v = dq.data_ptr(), d_v.data_ptr() if d_v is not None else None
        desc.d_embeds = d_emb.data_ptr() if d_emb is not None else None
        desc.flat, desc.offsets, desc.workspace = fb, cache.offsets_p, ws.data_ptr()
        # td_step(): d loss / d Q came from the forward launch, and the reduce launch also writes the loss (mean of the graphs'
        # terms); over capacity-sized buffers the weight-gradient GEMM takes the live row count from the device
        td_bwd = td is not None and dq.data_ptr() == td[0].data_ptr()
        desc.td_loss = td[0].data_ptr() + 4 * (td[1] + 2 * td[2]) if td_bwd else None
        desc.n_live = live.data_ptr() if (td_bwd and live is not None) else None
        hook = _GRAD_STAGE_HOOK
        split = tot >= 3 and mode != 2 and not call.nonleaf and (defer_lower or hook is not None)
        mid = 1 + tot // 2 if split else 1
        _lib.check(L.hexgnn_qnet_call_backward(desc, 6 if chained else 7, mid, tot, _stream()), "hexgnn_qnet_call_backward")
        if split and defer_lower:
            call.pending = (desc, mid, flat, cache.cut, ws, d_emb, offsets)
        elif split:
            hook(flat, cache.cut, cache.total)
            _lib.check(L.hexgnn_qnet_call_backward(desc, 4, 1, mid, _stream()), "hexgnn_qnet_call_backward")
            hook(flat, 0, cache.cut)
    grads = None
    if call.assign:
        _assign_flat_grads(cache, flat, mode, gviews)
        del gviews
    else:
        # flat order -> the call's order: the head tail's (lin_w, lin_b, v0_w, v0_b, v1_w, v1_b) sit in the flat buffer as
        # (v0_w, v0_b, v1_w, v1_b, lin_w, lin_b)
        g = torch._C._nn.unflatten_dense_tensors(flat, cache.flat_params)
        nconv = 3 * tot
        grads = tuple(g[:nconv]) + tuple(g[-2:]) + ((None,) * 4 if mode == 2 else tuple(g[nconv:nconv + 4]))
    if d_emb is not None:
        call.sink(d_emb[:, :hidden])
    return grads


class QNetDirectFn(torch.autograd.Function):
    """Autograd node of the direct form: ONE differentiable input (the per-model anchor, whose gradient is never produced);
    ``fargs`` = the arguments of ``qnet_forward``, ``holder`` = a list that receives the call record.  The backward runs the
    fused backward kernels and assigns the parameter gradients (see the section comment)."""

    @staticmethod
    def forward(ctx, anchor, holder, fargs):
        ctx.set_materialize_grads(False)
        q, out_v, call = qnet_forward(*fargs)
        ctx.call = call
        holder.append(call)
        if out_v is None:
            return q
        return q, out_v

    @staticmethod
    def backward(ctx, dq, d_v=None):
        qnet_backward(ctx.call, dq, d_v)
        return None, None, None


class QNetFusedFn(torch.autograd.Function):
    """The autograd form: DuellingTwoHeaded.forward (GN0/models.py:537-584) on the fused kernels with the parameters as
    autograd inputs (frozen or hooked parameters, post-accumulate hooks, ``--noisy_dqn`` weights formed per forward,
    ``torch.autograd.grad``, ``set_direct_grads(False)``).  ``cache`` = the head's QNetParamCache, or None when the weights
    are formed per forward (a cache is then built for the call).  Outputs: mode 0 -> (Q, embeds); 1 -> (V, A-mean(A),
    embeds); 2 -> (2tanh(adv), embeds).  ``embeds`` (final_conv_acts) is returned non-differentiable; its gradient is handed
    to ``grad_sink(d_embeds)`` during backward (final_conv_grads / Grad-CAM)."""

    @staticmethod
    def forward(ctx, cache, x, gs: GraphStructure, gptr, b: int, c_in: int, hidden: int, body_layers: int, head_layers: int,
                mode: int, grad_sink, *params):
        ctx.set_materialize_grads(False)      # unused outputs (embeds, V) arrive as None instead of freshly zeroed tensors
        # a parameter that is computed per forward (FactorizedNoisyLinear's mu + sigma * eps) is no leaf: its gradient is
        # an intermediate that autograd still has to carry to mu / sigma, so it must not be all-reduced in place
        nonleaf = any(p.grad_fn is not None for p in params)
        conv = [_f32c(p) for p in params]
        if cache is None or any(p is not c for p, c in zip(conv, cache.params)):
            cache = QNetParamCache(conv, body_layers + head_layers)
        q, out_v, call = qnet_forward(cache, x, gs, gptr, b, c_in, hidden, body_layers, head_layers, mode,
                                      any(ctx.needs_input_grad), assign=False)
        call.nonleaf, call.sink = nonleaf, grad_sink
        ctx.call = call
        embeds = qnet_embeds(call)
        ctx.mark_non_differentiable(embeds)
        if mode == 1:
            return out_v, q, embeds
        return q, embeds

    @staticmethod
    def backward(ctx, *gouts):
        dq, d_v = (gouts[1], gouts[0]) if ctx.call.dims[6] == 1 else (gouts[0], None)
        return (None,) * 11 + qnet_backward(ctx.call, dq, d_v)


def finish_backward(call: "_QNetCall"):
    """Second stage of a backward started with ``defer_lower=True``: the weight-gradient GEMM + slab reduce of the lower half of
    the hidden layers (the head of the flat gradient buffer).  Returns ``(flat, cut)``: the buffer and the position where its
    two segments meet (None, 0 when nothing was deferred).  May be issued again on the same call (same result)."""
    pend = call.pending
    if pend is None:
        return None, 0
    desc, mid, flat, cut, _ws, _d_emb, _offsets = pend
    _lib.check(_lib.lib().hexgnn_qnet_call_backward(desc, 4, 1, mid, _stream()), "hexgnn_qnet_call_backward")
    return flat, cut


# d loss / d q of the TdLossFn forward that just ran on THIS thread (picked up by td_loss()); "the loss is the root of the backward
# pass" travels on the loss's own autograd node (ctx._hex_unit, set by backward()): TdLossFn.backward runs on the autograd
# engine's device thread, where neither a module global nor a thread-local of the caller is safe to read
_TD_TLS = threading.local()
_ONES = {}


def _td_args(sel, target, weights, dev):
    """sel / target / weights of a TD loss as contiguous tensors on ``dev`` (int64, fp32, fp32) of one length.  (.to() costs
    ~2 us even when nothing changes: the usual case -- device tensors of the right type -- skips it.)"""
    if sel.dtype != torch.long or sel.device != dev or not sel.is_contiguous():
        sel = sel.to(device=dev, dtype=torch.long).contiguous()
    if target.dtype != torch.float32 or target.device != dev or not target.is_contiguous():
        target = target.to(device=dev, dtype=torch.float32).contiguous()
    if weights is not None and (weights.dtype != torch.float32 or weights.device != dev or not weights.is_contiguous()):
        weights = weights.to(device=dev, dtype=torch.float32).contiguous()
    if target.numel() != sel.numel() or (weights is not None and weights.numel() != sel.numel()):
        raise ValueError("sel / target / weights must have the same length")
    return sel, target, weights


class TdLossFn(torch.autograd.Function):
    """``loss_fn(Q[sel], target)`` of the DQN update: mean of importance-weighted squared ("mse") or Huber errors over the
    selected nodes.  When Q needs a gradient the forward is ONE launch that also produces ``d loss / d Q``
    (``hexgnn_td_loss_forward_backward``); the backward then hands that buffer on when the loss is the root of the pass
    (``ops.backward(loss)``: nothing is launched at all) and runs the two-launch form's scatter with the upstream scale
    otherwise (``loss.backward()`` / a scaled loss: ``hexgnn_td_loss_backward``).  Same bits either way."""

    @staticmethod
    def forward(ctx, q, sel, target, weights, loss_fn: int):
        L = _lib.lib()
        ctx.set_materialize_grads(False)
        dev = q.device
        qf = q if q.dim() == 1 else q.reshape(-1)
        if qf.dtype != torch.float32 or not qf.is_contiguous():
            qf = qf.float().contiguous()
        sel, tgt, w = _td_args(sel, target, weights, dev)
        k, n = sel.numel(), qf.numel()
        loss = torch.empty((), dtype=torch.float32, device=dev)
        td = torch.empty(k, dtype=torch.float32, device=dev)
        dq = None
        if ctx.needs_input_grad[0]:
            dq = torch.empty(n, dtype=torch.float32, device=dev)
            _lib.check(L.hexgnn_td_loss_forward_backward(n, k, qf.data_ptr(), sel.data_ptr(), tgt.data_ptr(),
                                                         w.data_ptr() if w is not None else None, loss_fn,
                                                         loss.data_ptr(), td.data_ptr(), dq.data_ptr(), _stream()),
                       "hexgnn_td_loss_forward_backward")
        else:
            _lib.check(L.hexgnn_td_loss_forward(n, k, qf.data_ptr(), sel.data_ptr(), tgt.data_ptr(),
                                                w.data_ptr() if w is not None else None, loss_fn, loss.data_ptr(),
                                                td.data_ptr(), _stream()), "hexgnn_td_loss_forward")
        ctx.save_for_backward(sel, td, w if w is not None else td)
        ctx.dq = dq
        _TD_TLS.last = dq
        ctx.has_w, ctx.loss_fn, ctx.shape = w is not None, loss_fn, q.shape
        ctx.mark_non_differentiable(td)
        return loss, td

    @staticmethod
    def backward(ctx, gloss, _gtd):
        if gloss is None:
            return None, None, None, None, None
        if getattr(ctx, "_hex_unit", False) and ctx.dq is not None:   # the loss is the root: d loss / d q came with the forward launch
            dq, ctx.dq = ctx.dq, None
            return dq.view(ctx.shape), None, None, None, None
        sel, td, w = ctx.saved_tensors
        n = 1
        for d in ctx.shape:
            n *= int(d)
        dq = torch.empty(n, dtype=torch.float32, device=td.device)
        g = gloss.reshape(1).float().contiguous()
        _lib.check(_lib.lib().hexgnn_td_loss_backward(n, int(sel.numel()), sel.data_ptr(), td.data_ptr(),
                                                      w.data_ptr() if ctx.has_w else None, ctx.loss_fn, g.data_ptr(),
                                                      dq.data_ptr(), _stream()), "hexgnn_td_loss_backward")
        return dq.view(ctx.shape), None, None, None, None


def td_loss(q: torch.Tensor, sel: torch.Tensor, target: torch.Tensor, weights: Optional[torch.Tensor] = None,
            loss_fn: str = "mse"):
    """``(loss, td_errors)`` with ``loss = mean(weights * l(q[sel] - target))``, ``l`` = squared error ("mse", the
    reference's ``--loss_fn=mse``) or Huber with delta 1 ("huber"); ``td_errors = q[sel] - target`` (detached) feed
    ``GraphReplayBuffer.update_priorities``.  Equal to ``F.mse_loss(q[sel], target)`` / ``F.huber_loss`` when
    ``weights`` is None."""
    if q.device.type != "cuda":
        raise _lib.HexGnnError("td_loss runs only on the MI355X HIP path (no CPU fallback)")
    q = q.__dict__.get("_hex_plain", q)      # (the model's QValues wrapper: the ordinary tensor underneath, qvalues.py)
    _TD_TLS.last = None
    out = TdLossFn.apply(q, sel, target, weights, {"mse": 0, "huber": 1}[loss_fn])
    loss = out[0]
    loss._hex_td_root = True
    call = getattr(q, "_hex_call", None)
    last = getattr(_TD_TLS, "last", None)
    if call is not None and last is not None and q.dim() == 1 and q.dtype == torch.float32 and q.is_contiguous():
        # q is the fused network's own output and d loss / d q exists already: ops.backward(loss) can run the network's
        # backward directly on this thread (no autograd engine, no hop to its device thread and back: ~100 us of host time)
        loss._hex_direct = (call, last)
    _TD_TLS.last = None
    return out


class PolicyValueLossFn(torch.autograd.Function):
    """The policy/value update's loss over ``hexgnn_pv_loss`` (include/hexgnn.h): ``val_factor * sum_g (value_g - y_g) ** 2 +
    pol_factor * sum_g sum_j -t_gj * logp_j`` with ``y = (1 - q_ratio) z + q_ratio root_q`` and the targets ``t`` read from the
    sample ring's ``policy`` rows by board cell -- the reference's ``MSELoss * B + SoftCrossEntropy`` of
    rl_loop/trainer_agent_pytorch.py.  ``logp [M]`` / ``out_ptr [b + 1]``: the network's compacted log-policy; ``gptr`` int32
    ``[b + 1]`` / ``backmap``: the batch's observation; ``index`` int32 ``[b]``: the drawn slots; ``status``: int32 [1], bit 64.
    Returns ``(loss [], per_graph [b, 4])`` with ``per_graph = (ce, se, policy argmax hit, value sign hit)``; the one call
    also produces both gradients, and the backward scales them by the incoming scalar."""

    @staticmethod
    def forward(ctx, logp, value, out_ptr, gptr, backmap, policy, z, root_q, index, hex_size: int, q_ratio: float,
                val_factor: float, pol_factor: float, status):
        dev = logp.device
        _require_cuda(logp, "logp")
        lp, v = _f32c(logp.reshape(-1)), _f32c(value.reshape(-1))
        b, m, n = int(v.numel()), int(lp.numel()), int(backmap.numel())
        if out_ptr.dtype != torch.int64 or gptr.dtype != torch.int32 or index.dtype != torch.int32 or backmap.dtype != torch.int64:
            raise ValueError("out_ptr / backmap int64, gptr / index int32")
        if out_ptr.numel() != b + 1 or gptr.numel() != b + 1 or index.numel() != b:
            raise ValueError("out_ptr and gptr hold b + 1 = %d entries, index b" % (b + 1))
        if policy.dtype != torch.float32 or policy.dim() != 2 or policy.shape[1] != hex_size * hex_size or not policy.is_contiguous():
            raise ValueError("policy: the ring's contiguous float32 [capacity, %d]" % (hex_size * hex_size))
        cap = int(policy.shape[0])
        for name, t in (("z", z), ("root_q", root_q)):
            if t.dtype != torch.float32 or t.dim() != 1 or t.numel() < cap or not t.is_contiguous():
                raise ValueError("%s: the ring's contiguous float32 [capacity = %d]" % (name, cap))
        if status.dtype != torch.int32 or status.numel() < 1 or not status.is_contiguous():
            raise ValueError("status: an int32 [1] tensor")
        for name, t in (("out_ptr", out_ptr), ("gptr", gptr), ("backmap", backmap), ("index", index)):
            if not t.is_contiguous():
                raise ValueError("%s must be contiguous" % name)
        for name, t in (("value", v), ("out_ptr", out_ptr), ("gptr", gptr), ("backmap", backmap), ("policy", policy), ("z", z),
                        ("root_q", root_q), ("index", index), ("status", status)):
            if t.device != dev:
                raise ValueError("%s is on %s, logp on %s" % (name, t.device, dev))
        loss = torch.empty((), dtype=torch.float32, device=dev)
        d_logp = torch.empty(m, dtype=torch.float32, device=dev)
        d_value = torch.empty(b, dtype=torch.float32, device=dev)
        per_graph = torch.empty((b, 4), dtype=torch.float32, device=dev)
        call = _lib.PVLossCall(struct_bytes=C.sizeof(_lib.PVLossCall), b=b, n=n, m=m, hex_size=int(hex_size),
                               capacity=cap, q_ratio=float(q_ratio), val_factor=float(val_factor),
                               pol_factor=float(pol_factor), logp=lp.data_ptr(), out_ptr=out_ptr.data_ptr(),
                               gptr=gptr.data_ptr(), backmap=backmap.data_ptr(), value=v.data_ptr(), policy=policy.data_ptr(),
                               z=z.data_ptr(), root_q=root_q.data_ptr(), index=index.data_ptr(), loss=loss.data_ptr(),
                               d_logp=d_logp.data_ptr(), d_value=d_value.data_ptr(), per_graph=per_graph.data_ptr(),
                               status=status.data_ptr())
        _lib.check(_lib.lib().hexgnn_pv_loss(C.byref(call), _stream()), "hexgnn_pv_loss")
        ctx.save_for_backward(d_logp, d_value)
        ctx.shapes = (logp.shape, value.shape)
        ctx.mark_non_differentiable(per_graph)
        return loss, per_graph

    @staticmethod
    def backward(ctx, gloss, _gpg):
        d_logp, d_value = ctx.saved_tensors
        g = gloss.reshape(()).float()
        return ((d_logp * g).view(ctx.shapes[0]), (d_value * g).view(ctx.shapes[1])) + (None,) * 12


def backward(loss: torch.Tensor) -> None:
    """``loss.backward()`` for a loss returned by ``td_loss`` without the two launches autograd adds around it: the
    ``ones_like(loss)`` fill that seeds the pass, and the scaling scatter of ``d loss / d Q`` (the fused forward launch
    already produced it for a unit seed).  Any other tensor falls through to ``loss.backward()``.  Gradients are
    bit-identical to ``loss.backward()``."""
    if not getattr(loss, "_hex_td_root", False) or not loss.is_cuda:
        loss.backward()
        return
    direct = loss.__dict__.pop("_hex_direct", None) if _GRAD_STAGE_HOOK is None else None
    if direct is not None and not direct[0].done:
        call, dq = direct
        qnet_backward(call, dq, None)
        call.done = True            # like autograd without retain_graph: a second backward through this forward is an error
        return
    key = (loss.device.type, loss.device.index)
    one = _ONES.get(key)
    if one is None:
        one = torch.ones((), dtype=torch.float32, device=loss.device)
        _ONES[key] = one
    node = loss.grad_fn
    if node is not None:
        node._hex_unit = True          # (read by TdLossFn.backward on the engine's thread: this loss IS the root, seed == 1)
    try:
        torch.autograd.backward((loss,), (one,))
    finally:
        if node is not None:
            node._hex_unit = False


_TD_STEP = threading.local()      # .args = (sel, target, weights, loss_fn) while td_step() runs the model's forward


def td_step(model, x: torch.Tensor, edge_index, graph_indices=None, ptr=None, *, sel: torch.Tensor, target: torch.Tensor,
            weights: Optional[torch.Tensor] = None, loss_fn: str = "mse", defer_lower: bool = False):
    """One DQN update on a batch in its fused form: ``q = model(x, edge_index, graph_indices, ptr)``,
    ``loss, td = td_loss(q, sel, target, weights, loss_fn)``, ``backward(loss)`` -- returns ``(loss, td, q)`` with every
    parameter's ``.grad`` set, same values as those three calls (``td`` and the gradients bit-identical).

    When the update selects ONE node per graph, ``sel[g]`` a node of graph g (the action of the sampled transition: what the
    RainbowDQN step gathers, README.md:5,7) and the batch runs on the fused per-graph kernels, the loss is graph-local and the
    forward kernel forms it in its tail: no launch between the network's forward and backward, ``loss`` is written by the
    backward's reduce launch (the ``td_*`` fields of the call's ``hexgnn_qnet_call``; in exact fp32 the forward and the backward's
    data chain are one launch, ``hexgnn_qnet_call_forward`` with ``chain_backward``, see ``set_one_launch_step``).
    A ``sel[g]`` outside graph g makes ``loss`` / ``td[g]`` NaN and raises at the next ``GraphStructure.check()`` (status 16).
    Anything else (several selections per graph, graphs above 128 nodes, frozen parameters, ``--noisy_dqn``) runs the three
    calls.

    ``defer_lower=True`` returns ``(loss, td, q, call)`` with only the first stage of the staged backward issued (see
    ``qnet_backward``); ``finish_backward(call)`` issues the rest (a no-op returning (None, 0) where the step did not
    take the fused path and ran whole).

    Capacity-sized batches (``GraphReplayBuffer.sample_device``): ``x._hex_live_rows``, a 1-element int32 device tensor, says
    how many of the rows hold graphs (``ptr[-1]``); rows at or behind it are never read -- the per-graph kernels work from
    ``ptr``, the batched weight-gradient GEMM takes the count from the device (the descriptor's ``n_live``).  Only the
    fused form above in exact fp32 takes such a batch: anything else raises ``NotImplementedError``."""
    if not x.is_cuda:
        raise _lib.HexGnnError("td_step runs only on the MI355X HIP path (no CPU fallback)")
    live = getattr(x, "_hex_live_rows", None)
    if live is not None:
        if not (torch.is_tensor(live) and live.is_cuda and live.dtype == torch.int32 and live.numel() == 1):
            raise ValueError("x._hex_live_rows: a 1-element int32 device tensor")
        if _MATH != 0 or defer_lower or _GRAD_STAGE_HOOK is not None or not _FUSED_ENABLED:
            raise NotImplementedError("td_step over a capacity-sized batch (x._hex_live_rows) runs on the fused per-graph kernels "
                                      "in exact fp32 only: no set_math(\"f16x3\"), no set_fused(False), no staged backward")
    sel, target, weights = _td_args(sel, target, weights, x.device)
    lfn = {"mse": 0, "huber": 1}[loss_fn]
    _TD_STEP.args = (sel, target, weights, lfn)
    _TD_STEP.live = live
    _TD_STEP.whole = not defer_lower and _GRAD_STAGE_HOOK is None      # (the one-launch form: set_one_launch_step)
    try:
        q = model(x, edge_index, graph_indices, ptr)
    finally:
        _TD_STEP.args = None
        _TD_STEP.live = None
        _TD_STEP.whole = False
    q = q.__dict__.get("_hex_plain", q)      # (td_step hands back the ordinary tensor, not the QValues wrapper)
    call = getattr(q, "_hex_call", None)
    td = call.td if call is not None else None
    if live is not None and (td is None or call.live is None):
        raise NotImplementedError("td_step over a capacity-sized batch (x._hex_live_rows): this model / batch does not take the "
                                  "fused per-graph kernels (norm layers, a noisy head, hidden > 112, graphs above 128 nodes, "
                                  "frozen or hooked parameters, or not one selected node per graph), and every other path "
                                  "reads all rows of its buffers")
    if td is None:
        loss, tde = td_loss(q, sel, target, weights, loss_fn)
        direct = getattr(loss, "_hex_direct", None)
        if defer_lower and direct is not None and _GRAD_STAGE_HOOK is None:
            loss.__dict__.pop("_hex_direct", None)
            qnet_backward(direct[0], direct[1], None, defer_lower=True)
            direct[0].done = True
            return loss, tde, q, direct[0]
        backward(loss)
        if defer_lower:
            if call is None:
                call = _QNetCall()
            call.pending = None
            return loss, tde, q, call
        return loss, tde, q
    tb, n, b = td
    qnet_backward(call, tb[:n], None, defer_lower=defer_lower and _GRAD_STAGE_HOOK is None)
    call.done = True
    if defer_lower:
        return tb[n + 2 * b], tb[n:n + b], q, call
    return tb[n + 2 * b], tb[n:n + b], q


def greedy_nodes(q: torch.Tensor, ptr: torch.Tensor) -> torch.Tensor:
    """For every graph of a batch the global index of its best non-terminal node: ``ptr[g] + 2 + argmax(q[ptr[g]+2 :
    ptr[g+1]])`` (first maximum) -- the per-graph python argmax of GN0/RainbowDQN/evaluate_elo.py:253-266, and the
    double-DQN action selection over a sampled batch, as one launch (``hexgnn_select_actions`` without a backmap)."""
    _require_cuda(q, "q")
    b = int(ptr.numel()) - 1
    gptr = ptr.to(device=q.device, dtype=torch.int32)
    qf = q.reshape(-1)
    if qf.dtype != torch.float32 or not qf.is_contiguous():
        qf = qf.float().contiguous()
    rank = torch.empty(b, dtype=torch.int32, device=q.device)
    _lib.check(_lib.lib().hexgnn_select_actions(b, gptr.data_ptr(), qf.data_ptr(), None, 0.0, None, None, rank.data_ptr(),
                                                None, _stream()), "hexgnn_select_actions")
    return gptr[:-1].long() + rank.long()


# ------------------------------------------------------------------------------------------------
# several networks over ONE batch in one load-balanced forward launch; double-DQN targets
# ------------------------------------------------------------------------------------------------
MAX_SETS = 4          # HEXGNN_MAX_SETS


def forward_jobs(ptr: torch.Tensor, k: int) -> torch.Tensor:
    """The int32 job table ``[b * k]`` of a batch for ``k`` weight sets: job ``j`` = ``graph << 2 | set`` =
    ``(order[j // k], j % k)``, ``order`` = the graphs by descending node count, ties by ascending graph index (built on the
    device: no host sync).  The fused forward of ``multi_forward`` runs its workgroups in this order -- longest job first."""
    _require_cuda(ptr, "ptr")
    if not 1 <= int(k) <= MAX_SETS:
        raise ValueError("1..%d weight sets" % MAX_SETS)
    b = int(ptr.numel()) - 1
    gptr = ptr.to(dtype=torch.int32).contiguous()
    jobs = torch.empty(max(b, 0) * int(k), dtype=torch.int32, device=ptr.device)
    if b > 0:
        _lib.check(_lib.lib().hexgnn_qnet_forward_jobs(b, int(k), gptr.data_ptr(), jobs.data_ptr(), 0, 0, 0, None, None, None,
                                                       None, _stream()), "hexgnn_qnet_forward_jobs")
    return jobs


def _multi_plan(models, x, edge_index, graph_indices, ptr):
    """What the fused multi-set forward needs, or None when it does not apply (the callers then run every model's ordinary
    forward): fused kernels on, exact fp32 math, every model a dueling Q-network with a parameter cache (no noisy head) and the
    same (c_in, hidden, body layers, head layers), every graph within 128 nodes, hidden <= 112.  The side to move, the largest
    graph and the CSR are found exactly as ``DuellingTwoHeaded.forward`` finds them (hints of ``x``, an attached
    ``_hex_csr``, the one-launch build for a grouped batch)."""
    if not _FUSED_ENABLED or _MATH != 0:
        return None
    hint, max_nodes = hints_of(x)
    if hint is None:
        assert torch.all(x[:, 2] == x[0, 2])
        is_maker = bool(x[0, 2] == 1)
    else:
        is_maker = bool(hint)
    dev, n = x.device, x.shape[0]
    caches, dims = [], None
    for m in models:
        entry = getattr(m, "_fused_entry", None)
        if entry is None:
            return None
        ent = entry(m._modules["maker_head" if is_maker else "breaker_head"])
        c_in, h, n_body, n_head, fusable, noisy = ent[3]
        cache = ent[2]
        if not fusable or noisy or cache is None or (dims is not None and dims != (c_in, h, n_body, n_head)):
            return None
        dims = (c_in, h, n_body, n_head)
        if not cache.valid():
            cache.refresh()
        if not all(p.is_cuda and p.device == dev and p.dtype == torch.float32 and p.is_contiguous() for p in cache.params):
            return None
        caches.append(cache)
    c_in, h, n_body, n_head = dims
    x2 = x[:, :2]
    if x2.shape[1] != c_in:
        return None
    gptr = None
    if max_nodes is None:
        gptr, b = graph_ptr(graph_indices, ptr, n, dev)
        max_nodes = int((gptr[1:] - gptr[:-1]).max()) if b > 0 else 0         # host sync (no size hint given)
    if not qnet_fused_supported(c_in, h, max_nodes):
        return None
    gs = getattr(edge_index, "_hex_csr", None)
    if gs is not None and gs.n != n:
        gs = None
    if gs is None and gptr is None and getattr(edge_index, "_hex_grouped", False) and max_nodes <= 2048 and ptr is not None \
            and ptr.dtype == torch.int64 and ptr.is_cuda and ptr.is_contiguous() and int(ptr.numel()) > 1 \
            and edge_index.dtype == torch.int64 and edge_index.dim() == 2 and edge_index.is_contiguous() and edge_index.is_cuda:
        b = int(ptr.numel()) - 1
        gs = GraphStructure.grouped(edge_index, n, b, ptr)        # the one-launch build; carries its int32 node ranges
    else:
        if gptr is None:
            gptr, b = graph_ptr(graph_indices, ptr, n, dev)
        if gs is None:
            grouped = getattr(edge_index, "_hex_grouped", False) and max_nodes <= 2048 and b > 0
            gs = GraphStructure(edge_index, n, gptr, b) if grouped else GraphStructure(edge_index, n)
    return caches, x2, gs, gptr, b, c_in, h, n_body + n_head


def _multi_run(plan):
    """packs + job table (one launch, two beyond two sets), then ONE forward launch over b * k jobs.  Returns the k Q vectors
    and the int32 node ranges' address."""
    caches, x, gs, gptr, b, c_in, hidden, tot = plan
    L = _lib.lib()
    dev, n, k = x.device, x.shape[0], len(caches)
    if x.dtype != torch.float32 or x.stride(1) != 1:
        x = x.float().contiguous()
    x_stride = x.stride(0) if n > 0 else c_in
    gp = gs._ptrs
    if gp is None:
        gp = (gs.rowptr.data_ptr(), gs.col.data_ptr(), gs.rowptr_t.data_ptr(), gs.col_t.data_ptr(), gs.invdeg.data_ptr(),
              gptr.data_ptr(), gs.status.data_ptr())
    key = ("multi", n, b, k)
    sizes = caches[0].sizes.get(key)
    if sizes is None:
        w_bytes = (L.hexgnn_sage_stack_pack_bytes(c_in, hidden, tot) + 255) & ~255
        total = L.hexgnn_qnet_multi_workspace_bytes(n, b, c_in, hidden, tot, k)
        if total == 0:
            raise _lib.HexGnnError("hexgnn_qnet_multi_workspace_bytes: unsupported configuration")
        sizes = caches[0].sizes[key] = (w_bytes, total)
    w_bytes, total = sizes
    buf = torch.empty(total, dtype=torch.uint8, device=dev)       # [pack 0 | .. | pack k-1 | jobs]
    base = buf.data_ptr()
    jobs = base + k * w_bytes
    q = torch.empty((k, n), dtype=torch.float32, device=dev)
    vp = C.c_void_p
    wpack = (vp * k)(*[base + s * w_bytes for s in range(k)])
    arr = lambda name: (vp * k)(*[C.cast(getattr(c, name), vp).value for c in caches])      # noqa: E731
    stream = _stream()
    _lib.check(L.hexgnn_qnet_forward_jobs(b, k, gp[5], jobs, c_in, hidden, tot, arr("wl"), arr("bl"), arr("wr"), wpack, stream),
               "hexgnn_qnet_forward_jobs")
    tails = [(vp * 6)(*c.tail) for c in caches]
    tail = (vp * k)(*[C.cast(t, vp).value for t in tails])
    qs = (vp * k)(*[q.data_ptr() + 4 * n * s for s in range(k)])
    status = (vp * k)(*([gp[6]] * k))
    _lib.check(L.hexgnn_qnet_forward_multi(n, b, k, c_in, hidden, tot, gp[5], gp[0], gp[1], gp[4], x.data_ptr(), x_stride, jobs,
                                           wpack, tail, qs, status, stream), "hexgnn_qnet_forward_multi")
    return [q[s] for s in range(k)], gp[5]


def multi_forward(models, x: torch.Tensor, edge_index, graph_indices=None, ptr=None) -> List[torch.Tensor]:
    """Q-values of 1..4 models over ONE batch: ``[m(x, edge_index, graph_indices, ptr) for m in models]`` under
    ``torch.no_grad()``, bit for bit, from ONE forward launch whose b * k workgroups run largest graph first (a replay batch
    has graphs of very different sizes, and the launch is otherwise bound by its largest graph per CU).  The CSR is built or
    taken once (an attached ``_hex_csr`` as it is; a grouped batch takes the one-launch build); beyond it: the weight packs
    with the job table, and the forward.  Forward only: nothing is saved for a backward, ``model._fca`` /
    ``final_conv_acts`` and every ``.grad`` stay as they are.

    Where the fused form does not apply -- graphs above 128 nodes, hidden > 112, ``set_math("f16x3")``,
    ``set_fused(False)``, a noisy head, models of different shape -- every model's ordinary forward runs instead (same
    values; that path does set ``final_conv_acts``).  CPU tensors raise ``HexGnnError``."""
    models = list(models)
    if not 1 <= len(models) <= MAX_SETS:
        raise ValueError("multi_forward takes 1..%d models" % MAX_SETS)
    _require_cuda(x, "x")
    with torch.no_grad():
        plan = _multi_plan(models, x, edge_index, graph_indices, ptr)
        if plan is None:
            return [m(x, edge_index, graph_indices, ptr) for m in models]
        return _multi_run(plan)[0]


def double_dqn_targets(online, target, x: torch.Tensor, edge_index, graph_indices, ptr, reward: torch.Tensor,
                       done: torch.Tensor, gamma_n: float):
    """Double-DQN targets of an update (the RainbowDQN step): ``(y, a2)`` with ``a2 = greedy_nodes(online(next states), ptr)``
    and ``y = reward + gamma_n * target(next states)[a2] * (~done).float()``, bit for bit -- ``multi_forward([online,
    target], ...)`` plus ONE launch that forms both (no torch arithmetic in between; no host sync when ``ptr`` and the
    size hints of ``x`` are there).  Falls back to the plain sequence where ``multi_forward`` does."""
    _require_cuda(x, "x")
    with torch.no_grad():
        plan = _multi_plan([online, target], x, edge_index, graph_indices, ptr)
        b = int(ptr.numel()) - 1 if ptr is not None else -1
        # (the target launch takes float32 rewards and boolean flags, one per graph: what the torch expression is then bit-equal to)
        if plan is None or ptr is None or reward.dtype != torch.float32 or done.dtype != torch.bool \
                or tuple(reward.shape) != (b,) or tuple(done.shape) != (b,) or reward.device != x.device \
                or done.device != x.device:
            q_on = online(x, edge_index, graph_indices, ptr)
            q_tg = target(x, edge_index, graph_indices, ptr)
            if ptr is None:
                ptr = graph_ptr(graph_indices, None, x.shape[0], x.device)[0]
            a2 = greedy_nodes(q_on, ptr)
            return reward + gamma_n * q_tg[a2] * (~done).float(), a2
        (q_on, q_tg), gptr = _multi_run(plan)
        dev = x.device
        r, d = reward.contiguous(), done.contiguous().view(torch.uint8)
        y = torch.empty(b, dtype=torch.float32, device=dev)
        a2 = torch.empty(b, dtype=torch.int64, device=dev)
        _lib.check(_lib.lib().hexgnn_dqn_targets(b, gptr, q_on.data_ptr(), q_tg.data_ptr(), r.data_ptr(), d.data_ptr(),
                                                 float(gamma_n), y.data_ptr(), a2.data_ptr(), _stream()), "hexgnn_dqn_targets")
        return y, a2
