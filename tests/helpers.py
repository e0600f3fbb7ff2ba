"""Shared test helpers: synthetic batches and model pairs (HIP path + CPU oracle)."""
from argparse import Namespace

import numpy as np
import torch


def model_args(num_layers, hidden, head_layers=2):
    return Namespace(num_layers=num_layers, hidden_channels=hidden, norm=False, noisy_dqn=False,
                     noisy_sigma0=0.5, num_head_layers=head_layers)


def make_pair(num_layers, hidden, seed=0, device="cuda"):
    """(HIP model on device, CPU oracle) with identical weights (torch.manual_seed(seed))."""
    from gnn_hex_amd.models import get_pre_defined
    from oracle.model_ref import get_pre_defined_ref
    torch.manual_seed(seed)
    ref = get_pre_defined_ref("modern_two_headed", model_args(num_layers, hidden))
    hip = get_pre_defined("modern_two_headed", model_args(num_layers, hidden))
    hip.load_state_dict(ref.state_dict())
    return hip.to(device), ref


def sharpen_(model, alpha=0.8, beta=0.5, gain=2.0, vscale=0.02):
    """In-place change of a freshly initialised model into a state whose signal does NOT collapse (with the
    default init a 15-layer mean-aggregating ReLU stack over-smooths -- std(A - mean A) ~ 1e-5, advantage-linear gradients
    ~ 1e-5 -- so absolute 1e-4 gates cannot see an error there).  Every hidden SAGE layer becomes a high-pass filter,
    lin_r <- gain * lin_r, lin_l <- beta * gain * lin_l - alpha * lin_r (node minus most of its neighbourhood mean keeps
    the differences between nodes alive through the stack), and the value MLP's first layer is scaled down so that
    tanh(v) does not saturate on the sum-pooled inputs.  Measured with the oracle on GNN-L Hex-11 and GNN-S Hex-7, start
    and mid-game boards, both heads: std(A - mean A) 0.3-0.6, Q spread > 1.5, every gradient tensor's |g|max >= 1e-2.
    Works on the oracle and on the HIP mirror alike (same parameter names)."""
    with torch.no_grad():
        sd = dict(model.named_parameters())
        for k, p in sd.items():
            if k.endswith("lin_r.weight") and p.shape[1] > 2:
                p.mul_(gain)
                l = sd[k.replace("lin_r", "lin_l")]
                l.mul_(beta * gain).add_(p, alpha=-alpha)
            if "value_head.layers.0.weight" in k:
                p.mul_(vscale)
    return model


def batch_tensors(kind, sizes, maker=True):
    from oracle import env_ref
    x, ei, batch, ptr = env_ref.make_batch(kind, sizes, maker_turn=maker)
    return (torch.from_numpy(x), torch.from_numpy(ei), torch.from_numpy(batch), torch.from_numpy(ptr))


# ---- the weight-gradient GEMM's row-slice plan (hexgnn_dw_slice_plan) and the batch shapes chosen from it ----------------

def dw_plan(n, hidden_layers, math=0, stack_hidden_layers=None):
    """(slices, rows_per_slice) of one weight-gradient launch, from the library's own host query."""
    import ctypes
    from gnn_hex_amd import _lib
    s, r = ctypes.c_int(), ctypes.c_int()
    rc = _lib.lib().hexgnn_dw_slice_plan(int(n), int(hidden_layers), int(math),
                                         int(hidden_layers if stack_hidden_layers is None else stack_hidden_layers),
                                         ctypes.byref(s), ctypes.byref(r))
    assert rc == 0, rc
    return s.value, r.value


def dw_empty_slices(n, slices, rows_per_slice):
    """Slices of a plan that start at or beyond row n: they have no row, and must still deliver a zero slab."""
    return sum(1 for s in range(slices) if s * rows_per_slice >= n)


def dw_launches(num_layers, head_layers=2, staged=False, norm=False):
    """[(hidden-input layers of the launch, of its whole stack)] for the weight-gradient launches of one backward of
    modern_two_headed -- the host logic of gnn_hex_amd/ops.py and models.py restated: body + head SAGE layers run as ONE
    stack whose first layer (2 input features) has a kernel of its own; the staged backward (ops.qnet_backward with a stage
    hook) cuts the stack at layer 1 + total // 2, upper part first; --norm=True runs body and head as two stacks, the head's
    first layer being a hidden-input layer."""
    tot = num_layers + head_layers
    if norm:
        return [(num_layers - 1, num_layers - 1), (head_layers, head_layers)]
    if staged:
        mid = 1 + tot // 2
        return [(tot - mid, tot - 1), (mid - 1, tot - 1)]
    return [(tot - 1, tot - 1)]


def dw_has_empty(n, launches, math):
    return any(dw_empty_slices(n, *dw_plan(n, h, math, sh)) > 0 for h, sh in launches)


def start_board_nodes(size):
    """Nodes of a start-position graph (kind "D0") of a size x size board: the cells and the mover's two terminals."""
    return size * size + 2


# (id, num_layers, hidden, board size): the networks whose batches tests/test_gpu_dw_slices.py draws from the plan
DW_MODELS = {"L": (15, 110, 11), "S": (10, 35, 7), "h128": (4, 128, 7), "h64": (4, 64, 7)}


def dw_case_list(max_graphs=256):
    """Start-position batches placed on the edges of the slice plan: [(case id, model key, graphs, staged, norm)].
    GNN-L / GNN-S, per math mode m: the smallest and the largest graph count <= max_graphs whose plan has an empty slice, the
    counts just before and just after the smallest one that have none, the largest count with fewer than 256 nodes, and the
    count whose node total sits closest above a multiple of 1024; one empty-slice batch each for hidden 128 (NT = 8) and
    hidden 64 (NT = 4), for the staged backward of GNN-L, and for GNN-L with --norm=True.  A count picked for one math mode
    runs on every path, so a case id names every role it plays."""
    roles = {}

    def add(key, b, role, staged=False, norm=False):
        roles.setdefault((key, b, staged, norm), []).append(role)

    for key in ("L", "S"):
        layers, _, size = DW_MODELS[key]
        npg, launches = start_board_nodes(size), dw_launches(layers)
        for m in (0, 1):
            empty = [b for b in range(1, max_graphs + 1) if dw_has_empty(b * npg, launches, m)]
            assert empty, (key, m)
            first = empty[0]
            add(key, first, "m%d-first" % m)
            add(key, empty[-1], "m%d-last" % m)
            if first > 1:
                add(key, first - 1, "m%d-before" % m)
            add(key, next(b for b in range(first + 1, max_graphs + 1) if b not in empty), "m%d-after" % m)
        add(key, max(b for b in range(1, max_graphs + 1) if b * npg < 256), "tiny")
        add(key, min((b for b in range(1, max_graphs + 1) if b * npg > 1024 and (b * npg) % 1024),
                     key=lambda b: ((b * npg) % 1024, b)), "over1024")
    for key in ("h128", "h64"):
        layers, _, size = DW_MODELS[key]
        npg, launches = start_board_nodes(size), dw_launches(layers)
        # hidden 128 never takes the fused kernels (math 0 everywhere); hidden 64: empty in BOTH plans
        modes = (0,) if key == "h128" else (0, 1)
        add(key, next(b for b in range(1, max_graphs + 1) if all(dw_has_empty(b * npg, launches, m) for m in modes)), "empty")
    layers, _, size = DW_MODELS["L"]
    npg = start_board_nodes(size)
    add("L", next(b for b in range(1, max_graphs + 1)
                  if all(dw_has_empty(b * npg, dw_launches(layers, staged=True), m) for m in (0, 1))), "empty", staged=True)
    # --norm=True: the head stack (two hidden-input layers) is the launch that may use twice kDwMaxSlices = 64 slices
    head = dw_launches(layers, norm=True)[1]
    add("L", next(b for b in range(1, max_graphs + 1)
                  if dw_plan(b * npg, head[0], 0, head[1])[0] > 64 and dw_has_empty(b * npg, [head], 0)), "empty", norm=True)
    out = []
    for (key, b, staged, norm), rs in sorted(roles.items()):
        name = "%s%s%s-B%d-%s" % (key, "-staged" if staged else "", "-norm" if norm else "", b, "+".join(rs))
        out.append((name, key, b, staged, norm))
    return out


def sel_and_targets(ptr, seed=1):
    """one non-terminal node per graph, index 2 + (g*7919 mod (n_g-2)); targets ~ U(-1,1)"""
    ptr = ptr.tolist()
    sel = []
    for g in range(len(ptr) - 1):
        n_g = ptr[g + 1] - ptr[g]
        sel.append(ptr[g] + 2 + (g * 7919) % max(n_g - 2, 1))
    gen = torch.Generator().manual_seed(seed)
    tgt = torch.rand(len(sel), generator=gen) * 2 - 1
    return torch.tensor(sel, dtype=torch.long), tgt
