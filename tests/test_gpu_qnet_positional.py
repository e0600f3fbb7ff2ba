"""The positional C entry points of the fused call that INTEGRATION.md shows to C callers -- hexgnn_qnet_forward,
hexgnn_qnet_backward and hexgnn_qnet_backward_staged -- against ops.qnet_forward / ops.qnet_backward on the same parameters.
Python drives the descriptor form (hexgnn_qnet_call); the positional forms are adapters onto the same implementation, so both
sides run the same kernels on the same arguments: q, out_v and every gradient must have the same bits, no tolerance.

One batch: graphs of 2, 17 and 128 nodes (rings in both directions; the 17-node graph is a 16-ring and an isolated node), 3 raw
features in rows of 4 floats, hidden 35 (three 16-column tiles, HP 48), 2 body + 2 head layers, exact fp32, modes 0, 1, 2."""
import ctypes

import pytest
import torch

from helpers import qnet_params, qnet_ref

pytestmark = pytest.mark.gpu

C_IN, X_STRIDE, HIDDEN, BODY, HEAD = 3, 4, 35, 2, 2
TOT = BODY + HEAD
DATA, SMALL, HID = 1, 2, 4


def _batch():
    src, dst, ptr, off = [], [], [0], 0
    for n, ring in ((2, 2), (17, 16), (128, 128)):
        pairs = {(i, (i + 1) % ring) for i in range(ring)}
        pairs |= {(t, s) for s, t in pairs}
        for s, t in sorted(pairs):
            src.append(off + s)
            dst.append(off + t)
        off += n
        ptr.append(off)
    gen = torch.Generator().manual_seed(5)
    x = torch.rand(off, X_STRIDE, generator=gen) * 2 - 1
    return x, torch.tensor([src, dst], dtype=torch.long), torch.tensor(ptr, dtype=torch.long)


def _bits(t):
    return t.contiguous().reshape(-1).view(torch.int32)


def _ptr_array(tensors):
    return (ctypes.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


def _grad_buffers(params, mode):
    """NaN-filled destinations, one per parameter in call order (None for the value head in mode 2), and the arguments that name
    them: the three pointer arrays and the six of the head tail."""
    grads = [torch.full_like(p, float("nan")) for p in params]
    if mode == 2:
        grads[3 * TOT + 2:] = [None] * 4
    tail = [g.data_ptr() if g is not None else None for g in grads[3 * TOT:]]
    return grads, (_ptr_array(grads[0:3 * TOT:3]), _ptr_array(grads[1:3 * TOT:3]), _ptr_array(grads[2:3 * TOT:3]), *tail)


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_positional_entry_points_give_the_bits_of_the_descriptor_path(mode):
    from gnn_hex_amd import _lib, ops
    L = _lib.lib()
    dev = torch.device("cuda:0")
    x4, ei, ptr = _batch()
    x = x4.to(dev)[:, :C_IN]
    assert x.stride(0) == X_STRIDE and x.stride(1) == 1
    ei, ptr = ei.to(dev), ptr.to(dev)
    n, b = x.shape[0], ptr.numel() - 1
    named = qnet_params(qnet_ref(C_IN, HIDDEN, BODY, HEAD, seed=2))
    names = [name for name, _ in named]
    params = [p.detach().to(device=dev, dtype=torch.float32).clone().requires_grad_(True) for _, p in named]
    gen = torch.Generator().manual_seed(7)
    dq = (torch.rand(n, generator=gen) * 2 - 1).to(dev)
    dv = (torch.rand(b, generator=gen) * 2 - 1).to(dev) if mode == 1 else None
    prev = ops.get_math()
    ops.set_math("fp32")
    try:
        cache = ops.QNetParamCache(params, TOT)
        gs = ops.GraphStructure.grouped(ei, n, b, ptr)
        q_ref, v_ref, call = ops.qnet_forward(cache, x, gs, None, b, C_IN, HIDDEN, BODY, HEAD, mode, True, assign=False)
        g_ref = ops.qnet_backward(call, dq, dv)
    finally:
        ops.set_math(prev)
    assert call.desc is not None and not call.layered
    torch.cuda.synchronize()

    # the same call through the positional entry points, on buffers of its own
    hp = ops.padded_width(HIDDEN)
    rowptr, col, rowptr_t, col_t, invdeg, gptr, status = call.gp
    acts = torch.empty(TOT * n * hp, dtype=torch.float32, device=dev)
    wpack = torch.empty(L.hexgnn_sage_stack_pack_bytes(C_IN, HIDDEN, TOT), dtype=torch.uint8, device=dev)
    saved = torch.empty(L.hexgnn_qnet_saved_bytes(n, b, C_IN, HIDDEN, TOT), dtype=torch.uint8, device=dev)
    ws_bytes = L.hexgnn_qnet_backward_workspace_bytes(n, b, C_IN, HIDDEN, TOT)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    q = torch.full((n,), float("nan"), device=dev)
    out_v = torch.full((b,), float("nan"), device=dev) if mode == 1 else None
    t = cache.tail
    stream = torch.cuda.current_stream().cuda_stream
    _lib.check(L.hexgnn_qnet_forward(
        n, b, C_IN, HIDDEN, TOT, mode, gptr, rowptr, col, invdeg, x.data_ptr(), X_STRIDE, cache.wl, cache.bl, cache.wr,
        t[0], t[1], t[2], t[3], t[4], t[5], wpack.data_ptr(), acts.data_ptr(), saved.data_ptr(), 1, BODY - 1, 0, q.data_ptr(),
        out_v.data_ptr() if out_v is not None else None, status, stream), "hexgnn_qnet_forward")

    def backward_args(dst):
        return (n, b, C_IN, HIDDEN, TOT, BODY, mode, 0, gptr, rowptr_t, col_t, invdeg, x.data_ptr(), X_STRIDE, acts.data_ptr(),
                saved.data_ptr(), wpack.data_ptr(), t[0], t[2], t[4], dq.data_ptr(), dv.data_ptr() if dv is not None else None,
                None, *dst, ws.data_ptr(), ws_bytes, status)
    g_whole, dst = _grad_buffers(params, mode)
    _lib.check(L.hexgnn_qnet_backward(*backward_args(dst), stream), "hexgnn_qnet_backward")
    # staged: data chain + small reduces + the upper hidden layers, then the lower ones
    g_staged, dst = _grad_buffers(params, mode)
    mid = 1 + TOT // 2
    _lib.check(L.hexgnn_qnet_backward_staged(*backward_args(dst), DATA | SMALL | HID, mid, TOT, stream), "staged, upper")
    _lib.check(L.hexgnn_qnet_backward_staged(*backward_args(dst), HID, 1, mid, stream), "staged, lower")
    torch.cuda.synchronize()
    assert int(gs.status.item()) == 0

    assert torch.equal(_bits(q), _bits(q_ref)) and not torch.isnan(q_ref).any()
    if mode == 1:
        assert torch.equal(_bits(out_v), _bits(v_ref))
    assert len(g_ref) == len(g_whole) == len(g_staged) == len(names) == 3 * TOT + 6
    for name, ref, whole, staged in zip(names, g_ref, g_whole, g_staged):
        if ref is None:
            assert mode == 2 and whole is None and "value_head" in name
            continue
        assert not torch.isnan(ref).any(), name
        assert torch.equal(_bits(whole), _bits(ref)), "hexgnn_qnet_backward: %s" % name
        assert torch.equal(_bits(staged), _bits(ref)), "hexgnn_qnet_backward_staged: %s" % name
