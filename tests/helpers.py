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


# ---- raw feature counts 1..8 on every path (tests/test_gpu_feature_counts.py) ---------------------------------------------

def feature_batch(sizes, c_in, seed, p_edge=0.08):
    """Symmetric random graphs with ``c_in`` raw features per node: ``(x [n, c_in], edge_index, batch, ptr)``, edges grouped by
    graph in graph order (what a collation produces).  Column 0 holds integers 0..8 (a degree-like count), odd columns 0/1
    flags, the other even columns U(-1, 1); no column is constant over the batch.  Every graph of two or more nodes has the
    edge 0 <-> 1, so that the neighbour mean is exercised in the 2- and 3-node graphs too; graphs above 3 nodes keep their
    last node isolated."""
    rng = np.random.default_rng(seed)
    xs, eis, bv, ptr, off = [], [], [], [0], 0
    for g, n in enumerate(sizes):
        x = np.zeros((n, c_in), np.float32)
        for k in range(c_in):
            if k == 0:
                x[:, k] = rng.integers(0, 9, n)
            elif k % 2 == 1:
                x[:, k] = rng.random(n) < 0.4
            else:
                x[:, k] = rng.random(n) * 2 - 1
        m = np.triu(rng.random((n, n)) < p_edge, 1)
        if n >= 2:
            m[0, 1] = True
        if n > 3:
            m[:, n - 1] = False
        src, dst = np.nonzero(m)
        src, dst = np.concatenate([src, dst]), np.concatenate([dst, src])
        perm = rng.permutation(len(src))
        xs.append(x)
        eis.append(np.stack([src[perm], dst[perm]]).astype(np.int64) + off)
        bv.append(np.full(n, g, np.int64))
        off += n
        ptr.append(off)
    x = np.concatenate(xs)
    assert all(np.ptp(x[:, k]) > 0 for k in range(c_in)), "a feature column is constant over the batch"
    return (torch.from_numpy(x), torch.from_numpy(np.concatenate(eis, 1)), torch.from_numpy(np.concatenate(bv)),
            torch.tensor(ptr, dtype=torch.long))


def qnet_ref(c_in, hidden, body, head, seed):
    """The oracle's Q-network with ``c_in`` raw features: DuellingTwoHeadedRef built directly (get_pre_defined_ref fixes
    in_channels = 2) with the ``modern_two_headed`` head, in the sharpened state."""
    from oracle.model_ref import DuellingTwoHeadedRef
    torch.manual_seed(seed)
    ref = DuellingTwoHeadedRef(
        gnn_kwargs=dict(in_channels=c_in, num_layers=body, hidden_channels=hidden, cached_norm=False, norm=None, act="relu"),
        head_kwargs=dict(value_head_type="mlp", value_aggr_types=("sum", "max", "min", "mean"), num_layers=head,
                         noisy_dqn=False, noise_sigma=0.5, norm=None))
    return sharpen_(ref)


def qnet_params(model):
    """[(name, parameter)] of a ``qnet_ref`` model in the order of the fused call: (wl, bl, wr) per SAGE layer, body then
    maker head, then lin_w, lin_b, v0_w, v0_b, v1_w, v1_b."""
    out = []
    for tag, convs in (("gnn", model.gnn.convs), ("maker_head.gnn", model.maker_head.gnn.convs)):
        for l, conv in enumerate(convs):
            out += [("%s.convs.%d.lin_l.weight" % (tag, l), conv.lin_l.weight), ("%s.convs.%d.lin_l.bias" % (tag, l), conv.lin_l.bias),
                    ("%s.convs.%d.lin_r.weight" % (tag, l), conv.lin_r.weight)]
    h = model.maker_head
    out += [("maker_head.linear.weight", h.linear.weight), ("maker_head.linear.bias", h.linear.bias)]
    for l in (0, 1):
        out += [("maker_head.value_head.layers.%d.weight" % l, h.value_head.layers[l].weight),
                ("maker_head.value_head.layers.%d.bias" % l, h.value_head.layers[l].bias)]
    return out


def qnet_ref_forward(model, x, ei, batch, mode):
    """DuellingTwoHeadedRef.forward (oracle/model_ref.py) without the ``x[:, :2]`` slice and the side flag (the maker head
    is evaluated): gnn -> maker_head -> 2 tanh(a), tanh(v), dueling combine.  Returns ``(q [n], out_v)``: mode 0 -> (Q, None),
    1 (``seperate``) -> (A - mean A, tanh(v) [b]), 2 (``advantages_only``) -> (2 tanh(a), None)."""
    from oracle.model_ref import scatter_ref
    embeds = model.gnn(x, ei)
    if mode == 2:
        return (2 * torch.tanh(model.maker_head(embeds, ei, batch, advantages_only=True))).reshape(-1), None
    adv, value = model.maker_head(embeds, ei, batch)
    adv, value = 2 * torch.tanh(adv), torch.tanh(value)
    b = int(batch.max()) + 1
    centred = adv - scatter_ref(adv, batch, dim_size=b, reduce="mean").index_select(0, batch)
    if mode == 1:
        return centred.reshape(-1), value.reshape(-1)
    return (value.index_select(0, batch) + centred).reshape(-1), None


def one_row_per_graph(ptr, seed=1):
    """(sel, tgt): row ptr[g] + (7919 g mod n_g) of every graph (1-node graphs included) and targets ~ U(-1, 1)."""
    p = ptr.tolist()
    sel = [p[g] + (g * 7919) % (p[g + 1] - p[g]) for g in range(len(p) - 1)]
    gen = torch.Generator().manual_seed(seed)
    return torch.tensor(sel, dtype=torch.long), torch.rand(len(sel), generator=gen) * 2 - 1


def feature_loss(q, out_v, sel, tgt, mode):
    """64 * mse(Q[sel], tgt), one selected row per graph; in mode 1 Q[sel] is put together from the two outputs
    (tanh(v) of the row's graph + the centred advantage), so that both receive a gradient."""
    pred = q[sel] + out_v if mode == 1 else q[sel]
    return 64.0 * torch.nn.functional.mse_loss(pred, tgt)


def qnet_hip_call(ref, x, ei, ptr, c_in, hidden, body, head, mode, layered, deferred, sel, tgt, gs=None, out=None):
    """One forward + backward of the oracle's network through ``ops.qnet_forward`` / ``ops.qnet_backward`` (fused kernels, or
    the layer-major ones when ``layered``; the math mode is the caller's ``ops.set_math``).  ``x`` [n, c_in] (any row stride),
    ``ei`` and the int64 ``ptr`` are device tensors.  The structure is ``gs`` when given, the deferred grouped build
    (CSR build and weight pack in one launch) when ``deferred``, else a prebuilt ``GraphStructure.grouped``; ``out``
    (a dict) receives the structure the call ran on.  Returns ``(q, out_v, grads)``, the gradients of
    ``feature_loss`` in call order (``qnet_params``; None for the value head in mode 2)."""
    from gnn_hex_amd import ops
    dev = x.device
    params = [p.detach().to(device=dev, dtype=torch.float32).clone().requires_grad_(True) for _, p in qnet_params(ref)]
    cache = ops.QNetParamCache(params, body + head)
    n, b = int(x.shape[0]), int(ptr.numel()) - 1
    if gs is None:
        gs = (ei, n, b, ptr) if deferred else ops.GraphStructure.grouped(ei, n, b, ptr)
    q, out_v, call = ops.qnet_forward(cache, x, gs, None, b, c_in, hidden, body, head, mode, True, layered=layered,
                                      assign=False)
    if out is not None:
        out["gs"] = call.gs
    ql = q.detach().clone().requires_grad_(True)
    vl = out_v.detach().clone().requires_grad_(True) if mode == 1 else None
    feature_loss(ql, vl, sel, tgt, mode).backward()
    grads = ops.qnet_backward(call, ql.grad, vl.grad if mode == 1 else None)
    torch.cuda.synchronize()
    return q, out_v, grads
