"""The positional C entry points of the layer-major stack that INTEGRATION.md shows to C callers -- hexgnn_sage_stack_forward /
_backward and hexgnn_sage_norm_stack_forward / _backward -- against ops.sage_stack / ops.sage_norm_stack on the same parameters.
Python drives the descriptor form (hexgnn_sage_stack_call); the positional forms are adapters onto the same implementation, so
both sides run the same kernels on the same arguments: every activation slab and every gradient must have the same bits, no
tolerance.

One batch of two graphs, 130 and 5 rows: two default 128-row blocks, the first graph cut across them, with edges across the cut
(a block then waits for the other, layer by layer).  Hidden 35 (three 16-column tiles, HP 48)."""
import ctypes
from types import SimpleNamespace

import pytest
import torch

pytestmark = pytest.mark.gpu

SIZES, P_EDGE, HIDDEN = (130, 5), 0.05, 35
_BATCH = []


def _batch():
    """(n, edge_index on the device): every pair of a graph is an edge, in both directions, with probability P_EDGE."""
    if not _BATCH:
        gen = torch.Generator().manual_seed(11)
        src, dst, off = [], [], 0
        for size in SIZES:
            i, j = torch.triu_indices(size, size, offset=1)
            keep = torch.rand(i.numel(), generator=gen) < P_EDGE
            i, j = i[keep] + off, j[keep] + off
            src += [i, j]
            dst += [j, i]
            off += size
        ei = torch.stack([torch.cat(src), torch.cat(dst)])
        # (host, before any launch) the first graph has edges between its rows in block 0 and its rows in block 1
        first = (ei[0] < SIZES[0]) & (ei[1] < SIZES[0])
        assert int((first & (ei[0] < 128) & (ei[1] >= 128)).sum()) > 0 and int((first & (ei[0] >= 128) & (ei[1] < 128)).sum()) > 0
        assert off == 135 and (off + 127) // 128 == 2
        _BATCH.append((off, ei.to("cuda:0")))
    return _BATCH[0]


def _bits(t):
    return t.contiguous().reshape(-1).view(torch.int32)


def _ptr_array(tensors):
    return (ctypes.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


def _rand(gen, *shape, scale=1.0, dev="cuda:0"):
    return ((torch.rand(*shape, generator=gen) * 2 - 1) * scale).to(dev)


def _layers(gen, c_in, layers, norm):
    """Leaf parameters per layer (lin_l.weight, lin_l.bias, lin_r.weight[, norm.weight, norm.bias]) and the holders ops takes."""
    params, convs, norms = [], [], []
    for l in range(layers):
        cin = c_in if l == 0 else HIDDEN
        p = [_rand(gen, HIDDEN, cin, scale=0.4), _rand(gen, HIDDEN, scale=0.2), _rand(gen, HIDDEN, cin, scale=0.4)]
        if norm:                      # perturbed from the identity (weight 1, bias 0)
            p += [1 + _rand(gen, HIDDEN, scale=0.3), _rand(gen, HIDDEN, scale=0.3)]
        p = [t.requires_grad_(True) for t in p]
        params += p
        convs.append(SimpleNamespace(lin_l=SimpleNamespace(weight=p[0], bias=p[1]), lin_r=SimpleNamespace(weight=p[2])))
        if norm:
            norms.append(SimpleNamespace(weight=p[3], bias=p[4], eps=1e-5))
    return params, convs, norms


def _padded(t, hp):
    out = torch.zeros(t.shape[0], hp, device=t.device)
    out[:, :t.shape[1]] = t
    return out


def _buf(nbytes, dev):
    return torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=dev)


def _compare(names, refs, got):
    assert len(names) == len(refs) == len(got)
    for name, r, g in zip(names, refs, got):
        assert r.shape == g.shape and not torch.isnan(r).any(), name
        assert torch.equal(_bits(r), _bits(g)), name


@pytest.mark.parametrize("c_in,layers", [(3, 3), (HIDDEN, 2)], ids=["raw3-L3", "hidden-L2"])
def test_plain_stack_adapters_give_the_bits_of_the_descriptor_path(c_in, layers):
    from gnn_hex_amd import _lib, ops
    L = _lib.lib()
    dev = torch.device("cuda:0")
    n, ei = _batch()
    hp = ops.padded_width(HIDDEN)
    gen = torch.Generator().manual_seed(3)
    params, convs, _ = _layers(gen, c_in, layers, False)
    x = _rand(gen, n, c_in).requires_grad_(c_in == HIDDEN)
    dy = _rand(gen, n, HIDDEN)
    assert getattr(ei, "_hex_blocks", None) is None and getattr(ei, "_hex_block_groups", None) is None
    gs = ops.GraphStructure(ei, n)
    assert gs.blocks is None and gs.groups is None
    y_ref = ops.sage_stack(x, gs, c_in, HIDDEN, convs)
    acts_ref = y_ref.grad_fn.bufs[1]
    assert acts_ref.shape == (layers, n, hp)
    g_ref = torch.autograd.grad(y_ref, ([x] if c_in == HIDDEN else []) + params, dy)
    torch.cuda.synchronize()
    assert L.hexgnn_stack_status(1) == 0

    # the same call through the positional entry points, on buffers of its own
    xin = _padded(x.detach(), hp) if c_in == HIDDEN else x.detach()
    x_stride = hp if c_in == HIDDEN else c_in
    ps = [p.detach() for p in params]
    acts = torch.full((layers, n, hp), float("nan"), device=dev)
    wpack = _buf(L.hexgnn_sage_stack_pack_bytes(c_in, HIDDEN, layers), dev)
    saved = _buf(L.hexgnn_sage_stack_saved_bytes(n, c_in, HIDDEN, layers), dev)
    ws_bytes = L.hexgnn_sage_stack_backward_workspace_bytes(n, c_in, HIDDEN, layers)
    ws = _buf(ws_bytes, dev)
    stream = torch.cuda.current_stream().cuda_stream
    _lib.check(L.hexgnn_sage_stack_forward(
        n, c_in, HIDDEN, layers, gs.rowptr.data_ptr(), gs.col.data_ptr(), gs.invdeg.data_ptr(), xin.data_ptr(), x_stride,
        _ptr_array(ps[0::3]), _ptr_array(ps[1::3]), _ptr_array(ps[2::3]), wpack.data_ptr(), acts.data_ptr(), saved.data_ptr(), 1, 0,
        stream), "hexgnn_sage_stack_forward")
    grads = [torch.full_like(p, float("nan")) for p in ps]
    dx = torch.full((n, hp), float("nan"), device=dev) if c_in == HIDDEN else None
    dyp = _padded(dy, hp)
    _lib.check(L.hexgnn_sage_stack_backward(
        n, c_in, HIDDEN, layers, gs.rowptr.data_ptr(), gs.col.data_ptr(), gs.rowptr_t.data_ptr(), gs.col_t.data_ptr(),
        gs.invdeg.data_ptr(), xin.data_ptr(), x_stride, acts.data_ptr(), saved.data_ptr(), wpack.data_ptr(), dyp.data_ptr(),
        dx.data_ptr() if dx is not None else None, _ptr_array(grads[0::3]), _ptr_array(grads[1::3]), _ptr_array(grads[2::3]),
        ws.data_ptr(), ws_bytes, 0, stream), "hexgnn_sage_stack_backward")
    torch.cuda.synchronize()
    assert L.hexgnn_stack_status(1) == 0

    _compare(["acts[%d]" % l for l in range(layers)], list(acts_ref), list(acts))
    _compare(["y"], [y_ref.detach()], [acts[layers - 1][:, :HIDDEN]])
    got = ([dx[:, :HIDDEN]] if dx is not None else []) + grads
    names = (["dx"] if dx is not None else []) + ["layer %d %s" % (l, k) for l in range(layers) for k in ("d_wl", "d_bl", "d_wr")]
    assert len(grads) == 3 * layers
    _compare(names, list(g_ref), got)


def test_norm_stack_adapters_give_the_bits_of_the_descriptor_path():
    from gnn_hex_amd import _lib, ops
    L = _lib.lib()
    dev = torch.device("cuda:0")
    n, ei = _batch()
    c_in, layers, eps = 3, 2, 1e-5
    hp = ops.padded_width(HIDDEN)
    gen = torch.Generator().manual_seed(4)
    params, convs, norms = _layers(gen, c_in, layers, True)
    x = _rand(gen, n, c_in)
    dy = _rand(gen, n, HIDDEN)
    gs = ops.GraphStructure(ei, n)
    y_ref = ops.sage_norm_stack(x, gs, c_in, HIDDEN, convs, norms)
    both_ref, stats_ref = y_ref.grad_fn.bufs[1], y_ref.grad_fn.bufs[4]
    assert both_ref.shape == (2, layers, n, hp) and stats_ref.shape == (layers, 2)
    g_ref = torch.autograd.grad(y_ref, params, dy)
    torch.cuda.synchronize()
    assert L.hexgnn_stack_status(1) == 0

    ps = [p.detach() for p in params]
    pre = torch.full((layers, n, hp), float("nan"), device=dev)
    acts = torch.full((layers, n, hp), float("nan"), device=dev)
    stats = torch.full((layers, 2), float("nan"), device=dev)
    wpack = _buf(L.hexgnn_sage_stack_pack_bytes(c_in, HIDDEN, layers), dev)
    saved = _buf(L.hexgnn_sage_stack_saved_bytes(n, c_in, HIDDEN, layers), dev)
    nws_bytes = L.hexgnn_graph_layernorm_workspace_bytes(HIDDEN)
    nws = _buf(nws_bytes, dev)
    ws_bytes = L.hexgnn_sage_norm_stack_backward_workspace_bytes(n, c_in, HIDDEN, layers)
    ws = _buf(ws_bytes, dev)
    stream = torch.cuda.current_stream().cuda_stream
    nw = _ptr_array(ps[3::5])
    _lib.check(L.hexgnn_sage_norm_stack_forward(
        n, c_in, HIDDEN, layers, gs.rowptr.data_ptr(), gs.col.data_ptr(), gs.invdeg.data_ptr(), x.data_ptr(), c_in,
        _ptr_array(ps[0::5]), _ptr_array(ps[1::5]), _ptr_array(ps[2::5]), nw, _ptr_array(ps[4::5]), eps, wpack.data_ptr(),
        pre.data_ptr(), acts.data_ptr(), saved.data_ptr(), stats.data_ptr(), nws.data_ptr(), nws_bytes, 1, stream),
        "hexgnn_sage_norm_stack_forward")
    grads = [torch.full_like(p, float("nan")) for p in ps]
    dyp = _padded(dy, hp)
    _lib.check(L.hexgnn_sage_norm_stack_backward(
        n, c_in, HIDDEN, layers, gs.rowptr_t.data_ptr(), gs.col_t.data_ptr(), gs.invdeg.data_ptr(), x.data_ptr(), c_in,
        pre.data_ptr(), acts.data_ptr(), saved.data_ptr(), wpack.data_ptr(), stats.data_ptr(), nw, eps, dyp.data_ptr(), None,
        _ptr_array(grads[0::5]), _ptr_array(grads[1::5]), _ptr_array(grads[2::5]), _ptr_array(grads[3::5]),
        _ptr_array(grads[4::5]), ws.data_ptr(), ws_bytes, nws.data_ptr(), nws_bytes, stream), "hexgnn_sage_norm_stack_backward")
    torch.cuda.synchronize()
    assert L.hexgnn_stack_status(1) == 0

    _compare(["pre", "acts", "stats"], [both_ref[0], both_ref[1], stats_ref], [pre, acts, stats])
    assert len(grads) == 10
    _compare(["layer %d %s" % (l, k) for l in range(layers) for k in ("d_wl", "d_bl", "d_wr", "d_nw", "d_nb")], list(g_ref), grads)


def test_norm_stack_backward_owns_its_converted_norm_weights():
    """Norm weights that are not contiguous fp32 reach the kernels as copies made in the forward, and the backward reads them
    again: the copies must live until then.  The weights here are strided views; between forward and backward the test
    allocates and fills tensors of the copies' size, which would land in their memory had it been released.  All gradients
    must have the bits of the run on contiguous weights."""
    from gnn_hex_amd import _lib, ops
    n, ei = _batch()
    c_in, layers = 3, 2
    gen = torch.Generator().manual_seed(4)
    params, convs, norms = _layers(gen, c_in, layers, True)
    x = _rand(gen, n, c_in)
    dy = _rand(gen, n, HIDDEN)
    gs = ops.GraphStructure(ei, n)
    g_ref = torch.autograd.grad(ops.sage_norm_stack(x, gs, c_in, HIDDEN, convs, norms), params, dy)

    strided = []
    for nm in norms:
        wide = torch.zeros(HIDDEN, 2, device=x.device)
        wide[:, 0] = nm.weight.detach()
        strided.append(wide[:, 0].requires_grad_(True))
        assert not strided[-1].is_contiguous()
    norms2 = [SimpleNamespace(weight=w, bias=nm.bias, eps=nm.eps) for w, nm in zip(strided, norms)]
    params2 = list(params)
    params2[3::5] = strided
    y = ops.sage_norm_stack(x, gs, c_in, HIDDEN, convs, norms2)
    junk = [torch.full((HIDDEN,), 1e3, device=x.device) for _ in range(8)]
    g = torch.autograd.grad(y, params2, dy)
    torch.cuda.synchronize()
    assert _lib.lib().hexgnn_stack_status(1) == 0 and len(junk) == 8
    _compare(["layer %d %s" % (l, k) for l in range(layers) for k in ("d_wl", "d_bl", "d_wr", "d_nw", "d_nb")], list(g_ref), list(g))
