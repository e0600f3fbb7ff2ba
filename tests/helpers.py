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


def reorder_graphs(x, ei, ptr, order):
    """The collated batch with its graphs in the order ``order`` (position k holds graph order[k], as ``data.pack_order`` gives
    it): ``(x, edge_index, batch, ptr, rows)``, rows[i] = the old row of new row i; edges stay grouped by graph, each graph's
    edges in the order they had."""
    p = ptr.tolist()
    order = [int(g) for g in order]
    assert sorted(order) == list(range(len(p) - 1))
    rows = torch.cat([torch.arange(p[g], p[g + 1]) for g in order])
    new_of = torch.empty_like(rows)
    new_of[rows] = torch.arange(rows.numel())
    eg = torch.bucketize(ei[1], ptr[1:], right=True)                    # graph of every edge
    assert bool((eg == torch.bucketize(ei[0], ptr[1:], right=True)).all())
    cols = torch.cat([torch.nonzero(eg == g).reshape(-1) for g in order])
    sizes = [p[g + 1] - p[g] for g in order]
    nptr = torch.tensor([0] + list(np.cumsum(sizes)), dtype=torch.long)
    batch = torch.repeat_interleave(torch.arange(len(order)), torch.tensor(sizes))
    return x[rows], new_of[ei[:, cols]], batch, nptr, rows


# ---- graph-aligned row-block tables of the one-launch stack kernels (tests/test_gpu_block_tables.py) ---------------------------

# The smallest batch with every geometric case of a table: feature_batch(TABLE_SIZES, 2, seed=102, p_edge=TABLE_P_EDGE), 392 rows.
# head64: the 200-row graph is a 64-row head and two 68-row pieces -- three blocks, so the kernel's block_of() has a neighbour
# that is neither blk - 1 nor blk + 1; head0: block 1 = the 72-row tail of the 200-row graph + the whole 40-row graph, block 3
# starts with the LAST row of the cut 129-row graph, four whole graphs behind it; packed: data.pack_order's order and table.
TABLE_SIZES = [200, 40, 129, 1, 2, 3, 17]
TABLE_P_EDGE = 0.06
TABLE_STARTS = {"head64": [0, 64, 132, 200, 240, 304, 369, 392], "head0": [0, 128, 240, 368, 392],
                "packed": [0, 64, 132, 200, 264, 329, 392]}
TABLE_ORDER = [0, 2, 1, 6, 5, 4, 3]                                    # pack_order(TABLE_SIZES)[0]
TABLE_GROUPS = {"head64": (3, [0, 3, 6, 7]), "head0": (2, [0, 2, 4])}   # table -> (budget, block_groups(sizes, table, budget))
# wave counts of table_geometry() on that batch, and the fewest a table may have for its cases to count as covered
TABLE_WAVES = {
    "head64": dict(next_only=4, prev_only=4, both=5, far=9, remote_short=11, remote_long=11, slot3=22),
    "head0": dict(next_only=8, prev_only=5, both=0, far=0, remote_short=1, remote_long=12, slot3=13),
    "packed": dict(next_only=4, prev_only=4, both=5, far=9, remote_short=11, remote_long=11, slot3=22)}
TABLE_WAVES_MIN = {
    "head64": dict(next_only=4, prev_only=4, both=4, far=4, remote_short=4, remote_long=4, slot3=4),
    "head0": dict(next_only=4, prev_only=4, remote_long=4, slot3=4),
    "packed": dict(next_only=4, prev_only=4, both=4, far=4, remote_short=4, remote_long=4, slot3=4)}
# head0 on the same sizes at p_edge 0.04: the other side of its split into remote waves without / with a long row
TABLE_P_EDGE_SPARSE = 0.04
TABLE_WAVES_SPARSE = dict(next_only=8, prev_only=5, both=0, far=0, remote_short=12, remote_long=1, slot3=13)
TABLE_WAVES_SPARSE_MIN = dict(next_only=4, prev_only=4, remote_short=4, slot3=4)
TABLE_ELL = 16                 # neighbour slots of a row in the kernels' registers (kEll); rows above it are "long"


def table_geometry(edge_index, starts, ptr=None):
    """What the waves of a row-block table read, on the host with numpy: every block of ``starts`` cut into its eight 16-row
    waves, a row's in-neighbours taken in ascending source order (the CSR GraphStructure documents; slot k = the k-th of them).
    A wave is *remote* when a neighbour of one of its rows lies in another block.  Returns counts of waves:
      next_only / prev_only   every remote neighbour in block blk + 1 / blk - 1 (the two register fast paths of block_of());
      both                    remote neighbours in blk - 1 and blk + 1 and nowhere else;
      far                     a remote neighbour two or more blocks away (the bisection);
      remote_long / _short    remote waves with / without a row of more than 16 neighbours (a long-row wave also waits for its
                              own block);
      slot3                   a remote neighbour in a slot k < 16 with k % 4 == 3 (the tail ring's fourth landing buffer);
      idle                    waves without rows (blocks shorter than 113 rows).
    With ``ptr`` also the blocks ``mixed`` (rows of a graph that continues in another block together with whole graphs) and
    ``last_row_first`` (the block's first row is the last row of a graph that began in an earlier block)."""
    ei = np.asarray(edge_index)
    starts = np.asarray(starts, dtype=np.int64)
    n, nb = int(starts[-1]), len(starts) - 1
    assert starts[0] == 0 and np.all(np.diff(starts) > 0) and np.all(np.diff(starts) <= 128)
    assert ei.size == 0 or (ei.min() >= 0 and ei.max() < n)
    perm = np.lexsort((ei[0], ei[1]))                                  # by target row, then ascending source
    src, dst = ei[0][perm], ei[1][perm]
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(dst, minlength=n))])
    block = np.searchsorted(starts, np.arange(n), side="right") - 1     # block of every row
    out = dict(next_only=0, prev_only=0, both=0, far=0, remote_short=0, remote_long=0, slot3=0, idle=0)
    for blk in range(nb):
        for w in range(8):
            r0 = int(starts[blk]) + 16 * w
            r1 = min(r0 + 16, int(starts[blk + 1]))
            if r1 <= r0:
                out["idle"] += 1
                continue
            rel, long_row, slot3 = set(), False, False
            for row in range(r0, r1):
                nbrs = src[rowptr[row]:rowptr[row + 1]]
                long_row |= len(nbrs) > TABLE_ELL
                for k, j in enumerate(nbrs):
                    if block[j] != blk:
                        rel.add(int(block[j]) - blk)
                        slot3 |= k < TABLE_ELL and k % 4 == 3
            if not rel:
                continue
            out["remote_long" if long_row else "remote_short"] += 1
            out["slot3"] += int(slot3)
            if any(abs(d) >= 2 for d in rel):
                out["far"] += 1
            elif rel == {1}:
                out["next_only"] += 1
            elif rel == {-1}:
                out["prev_only"] += 1
            else:
                out["both"] += 1
    if ptr is not None:
        p = [int(v) for v in np.asarray(ptr)]
        cut = [any(p[g] < s < p[g + 1] for s in starts) for g in range(len(p) - 1)]     # graphs that span blocks
        mixed, last_first = [], []
        for blk in range(nb):
            b0, b1 = int(starts[blk]), int(starts[blk + 1])
            inside = [g for g in range(len(p) - 1) if p[g] < b1 and p[g + 1] > b0 and p[g + 1] > p[g]]
            if any(cut[g] for g in inside) and any(not cut[g] for g in inside):
                mixed.append(blk)
            if any(cut[g] and p[g] < b0 and p[g + 1] - 1 == b0 for g in inside):
                last_first.append(blk)
        out["mixed"], out["last_row_first"] = mixed, last_first
    return out


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


# ---- the float64 parity rule and its input conditions (tests/test_gpu_feature_counts.py, tests/test_gpu_wide_parity.py) -------

MARGIN = 2.0 ** -16      # smallest |ReLU input| / rms a weight state may have (tests/test_gpu_dw_slices.py: _well_conditioned_ref)
SEEDS = 400


class PoisonedTorch:
    """Stands in for the name ``torch`` inside gnn_hex_amd.ops while a test runs: ``empty`` fills device uint8 tensors (the
    library's scratch) with one byte before the library sees them; everything else is torch's own."""

    def __init__(self, byte):
        self.byte, self.filled = byte, 0

    def __getattr__(self, name):
        return getattr(torch, name)

    def empty(self, *args, **kwargs):
        t = torch.empty(*args, **kwargs)
        if t.dtype == torch.uint8 and t.is_cuda:
            t.fill_(self.byte)
            self.filled += 1
        return t


def rel_bound(tag, name, g, g32, g64, floor=2e-3):
    """||g - g64|| / ||g64|| <= max(3 x the fp32 oracle's own, floor); absolute 1e-6 for a vanishing tensor.  Returns the pair."""
    g, g32 = g.detach().cpu().double(), g32.double()
    assert torch.isfinite(g).all(), "%s %s: not finite" % (tag, name)
    nrm = g64.norm().item()
    if nrm < 1e-6:
        assert (g - g64).abs().max().item() < 1e-6, "%s %s" % (tag, name)
        return 0.0, 0.0
    rel, rel32 = (g - g64).norm().item() / nrm, (g32 - g64).norm().item() / nrm
    assert rel <= max(3.0 * rel32, floor), \
        "%s %s: ||g - g64|| / ||g64|| = %.3g, the fp32 oracle's own %.3g, floor %g" % (tag, name, rel, rel32, floor)
    return rel, rel32


def abs_bound(tag, name, y, y32, y64, const):
    y = y.detach().cpu().double()
    assert torch.isfinite(y).all(), "%s %s: not finite" % (tag, name)
    e, e32 = (y - y64).abs().max().item(), (y32.double() - y64).abs().max().item()
    assert e <= max(3.0 * e32, const), "%s: |%s - %s64| %.3g (fp32 oracle %.3g, constant %g)" % (tag, name, name, e, e32, const)
    return e, e32


def check_grads(tag, names, grads, g32, g64, c_in, first=(0, 2)):
    """Every gradient tensor, and every column k < c_in of the raw first layer's d_wl / d_wr (positions ``first``) against
    that column's own float64 norm.  Returns the worst (ratio, oracle32's, name) of the tensors and of the columns."""
    worst, worst_col = (0.0, 0.0, ""), (0.0, 0.0, "")
    assert len(grads) == len(g64) == len(names)
    for i, (name, g, a32, a64) in enumerate(zip(names, grads, g32, g64)):
        if a64 is None:
            assert g is None, name
            continue
        assert g is not None and tuple(g.shape) == tuple(a64.shape), name
        r = rel_bound(tag, name, g, a32, a64)
        worst = max(worst, r + (name,))
        if i in first:
            assert a64.shape[1] == c_in
            for k in range(c_in):
                cname = "%s[:, %d]" % (name, k)
                r = rel_bound(tag, cname, g[:, k], a32[:, k], a64[:, k])
                worst_col = max(worst_col, r + (cname,))
    return worst, worst_col


def column_shares(g, c_in):
    return [(g[:, k].norm() / g.norm()).item() for k in range(c_in)]


def same_bits(tag, a, b):
    """Two ``(q, out_v, grads)`` results of ``qnet_hip_call``: the same bits."""
    assert torch.equal(a[0], b[0]), "%s: Q differs" % tag
    assert (a[1] is None) == (b[1] is None) and (a[1] is None or torch.equal(a[1], b[1])), "%s: out_v differs" % tag
    for i, (ga, gb) in enumerate(zip(a[2], b[2])):
        assert (ga is None) == (gb is None) and (ga is None or torch.equal(ga, gb)), "%s: gradient %d differs" % (tag, i)


class QnetCases:
    """The Q-network cases of one batch shape and depth: ``feature_batch(sizes, c_in, seed=100 + c_in)`` with one selected row
    per graph, ``body`` + ``head`` layers, loss ``feature_loss``; per (c_in, hidden) the float64 and fp32 oracle results at the
    first weight seed that meets the four input conditions (see tests/test_gpu_feature_counts.py), once per session.
    ``p_edge``: the batch's edge probability; ``order``: the batch with its graphs in that order (``reorder_graphs``), every
    graph keeping its selected row and its target."""

    def __init__(self, sizes, body, head, p_edge=0.08, order=None):
        self.sizes, self.body, self.head = list(sizes), body, head
        self.p_edge, self.order = p_edge, None if order is None else list(order)
        self._batches, self._oracles = {}, {}

    def batch(self, c_in):
        if c_in not in self._batches:
            x, ei, batch, ptr = feature_batch(self.sizes, c_in, seed=100 + c_in, p_edge=self.p_edge)
            sel, tgt = one_row_per_graph(ptr)
            if self.order is not None:
                local = sel - ptr[:-1]
                x, ei, batch, ptr, _ = reorder_graphs(x, ei, ptr, self.order)
                sel, tgt = ptr[:-1] + local[self.order], tgt[self.order]
            self._batches[c_in] = (x, ei, batch, ptr, sel, tgt)
        return self._batches[c_in]

    def dev(self, c_in):
        x, ei, batch, ptr, sel, tgt = self.batch(c_in)
        return x.cuda(), ei.cuda(), ptr.cuda(), sel.cuda(), tgt.cuda()

    @staticmethod
    def ref_run(model, x, ei, batch, sel, tgt, mode):
        model.zero_grad(set_to_none=True)
        q, v = qnet_ref_forward(model, x, ei, batch, mode)
        feature_loss(q, v, sel, tgt, mode).backward()
        grads = [None if p.grad is None else p.grad.detach().clone() for _, p in qnet_params(model)]
        return q.detach(), None if v is None else v.detach(), grads

    @staticmethod
    def relu_margin(model, run):
        """min |ReLU input| / rms over the SAGE layers of body and maker head and the value MLP's first layer, during run()."""
        store, hooks = {}, []
        for conv in list(model.gnn.convs) + list(model.maker_head.gnn.convs):
            hooks.append(conv.register_forward_hook(lambda mod, inp, out: store.__setitem__(id(mod), out.detach())))
        hooks.append(model.maker_head.value_head.layers[0].register_forward_hook(
            lambda mod, inp, out: store.__setitem__("value", out.detach())))
        try:
            with torch.no_grad():
                run()
        finally:
            for h in hooks:
                h.remove()
        return min((t.abs().min() / t.pow(2).mean().sqrt().clamp(min=1e-300)).item() for t in store.values())

    def conditions(self, ref64, c_in, mode, search=False):
        """The four input conditions on the float64 oracle: (ok, text, q64, v64, g64).  ``search``: give up at once (ok False,
        nothing else) where the cheapest one, the ReLU margin, already fails."""
        x, ei, batch, ptr, sel, tgt = self.batch(c_in)
        x64, tgt64 = x.double(), tgt.double()
        margin = self.relu_margin(ref64, lambda: qnet_ref_forward(ref64, x64, ei, batch, mode))
        if search and margin < MARGIN:
            return False, "", None, None, None
        q64, v64, g64 = self.ref_run(ref64, x64, ei, batch, sel, tgt64, mode)
        sens = []
        with torch.no_grad():
            for k in range(c_in):
                xz = x64.clone()
                xz[:, k] = 0
                sens.append((qnet_ref_forward(ref64, xz, ei, batch, mode)[0] - q64).abs().max().item())
        shares = column_shares(g64[0], c_in) + column_shares(g64[2], c_in)
        spread = (q64.max() - q64.min()).item()
        gmax = min(g.abs().max().item() for g in g64 if g is not None)
        ok = min(sens) > 0.1 and min(shares) >= 0.02 and spread >= 0.5 and gmax >= 1e-2 and margin >= MARGIN
        text = "Q sensitivity per feature %.3g..%.3g (> 0.1), layer-0 gradient column share %.3g..%.3g (>= 0.02), Q spread " \
               "%.3g (>= 0.5), smallest |g|max %.3g (>= 1e-2), smallest |ReLU input| / rms %.3g (>= 2^-16)" \
               % (min(sens), max(sens), min(shares), max(shares), spread, gmax, margin)
        return ok, text, q64, v64, g64

    def oracle(self, c_in, hidden, mode=0):
        """fp32 and float64 oracle results of one case, once per session.  The weight seed is the first at which the conditions
        hold in all three modes (the modes share their weights)."""
        import copy
        key = (c_in, hidden)
        if key not in self._oracles:
            for seed in range(SEEDS):
                ref64 = qnet_ref(c_in, hidden, self.body, self.head, seed).double()
                if all(self.conditions(ref64, c_in, m, search=True)[0] for m in (0, 1, 2)):
                    break
            else:
                raise AssertionError("c_in %d hidden %d: no weight seed below %d meets the oracle conditions"
                                     % (c_in, hidden, SEEDS))
            self._oracles[key] = {"seed": seed}
        ent = self._oracles[key]
        if mode not in ent:
            x, ei, batch, ptr, sel, tgt = self.batch(c_in)
            ref = qnet_ref(c_in, hidden, self.body, self.head, ent["seed"])
            ref64 = copy.deepcopy(ref).double()
            ok, text, q64, v64, g64 = self.conditions(ref64, c_in, mode)
            q32, v32, g32 = self.ref_run(ref, x, ei, batch, sel, tgt, mode)
            ent[mode] = dict(ref=ref, ok=ok, text=text, q64=q64, v64=v64, g64=g64, q32=q32, v32=v32, g32=g32, seed=ent["seed"])
            print("oracle c_in %d hidden %d mode %d: weight seed %d; %s" % (c_in, hidden, mode, ent["seed"], text))
        o = ent[mode]
        assert o["ok"], "c_in %d hidden %d mode %d: %s" % (c_in, hidden, mode, o["text"])
        return o

    CONST, CONST_SPLIT = 5e-6, 8e-6        # the absolute floor under 3 x the fp32 oracle's own distance: exact fp32, f16x3

    @staticmethod
    def check(tag, o, q, out_v, grads, c_in, mode, split):
        const = QnetCases.CONST_SPLIT if split else QnetCases.CONST
        eq = abs_bound(tag, "Q", q, o["q32"], o["q64"], const)
        ev = abs_bound(tag, "out_v", out_v, o["v32"], o["v64"], const) if mode == 1 else None
        names = [k for k, _ in qnet_params(o["ref"])]
        worst, worst_col = check_grads(tag, names, list(grads), o["g32"], o["g64"], c_in)
        print("%s: |Q-Q64| %.3g (oracle32 %.3g)%s; worst gradient tensor %s rel %.3g (oracle32 %.3g); worst layer-0 column %s rel "
              "%.3g (oracle32 %.3g)" % (tag, eq[0], eq[1], "" if ev is None else "; |v-v64| %.3g (oracle32 %.3g)" % ev, worst[2],
                                        worst[0], worst[1], worst_col[2], worst_col[0], worst_col[1]))

    def run_case(self, c_in, hidden, mode, layered, x=None, deferred=False, gs=None, out=None):
        o = self.oracle(c_in, hidden, mode)
        xd, eid, ptrd, seld, tgtd = self.dev(c_in)
        res = qnet_hip_call(o["ref"], xd if x is None else x, eid, ptrd, c_in, hidden, self.body, self.head, mode, layered,
                            deferred, seld, tgtd, gs=gs, out=out)
        return o, res


# ---- a SAGE stack through autograd: the oracle's side --------------------------------------------------------------------------

def stack_model(kind, c_in, hidden, seed, layers=3):
    from oracle.model_ref import GraphSAGERef, SAGEConvRef
    torch.manual_seed(seed)
    if kind == "single":                # a bare SAGEConv(c_in, H): no ReLU behind it
        m = torch.nn.Module()
        m.convs, m.norms = torch.nn.ModuleList([SAGEConvRef(c_in, hidden)]), None
    else:
        m = GraphSAGERef(c_in, hidden, layers, norm=True if kind == "norm" else None)
    return sharpen_(m)


def stack_forward(kind, m, x, ei, store=None):
    """GraphSAGERef.forward / SAGEConvRef.forward; ``store`` receives every tensor a ReLU is applied to."""
    if kind == "single":
        return m.convs[0](x, ei)
    for l, conv in enumerate(m.convs):
        x = conv(x, ei)
        if m.norms is not None:
            x = m.norms[l](x)
        if store is not None:
            store.append(x.detach())
        x = torch.relu(x)
    return x


def stack_params(m):
    names, ps = [], []
    for l, conv in enumerate(m.convs):
        names += ["convs.%d.lin_l.weight" % l, "convs.%d.lin_l.bias" % l, "convs.%d.lin_r.weight" % l]
        ps += [conv.lin_l.weight, conv.lin_l.bias, conv.lin_r.weight]
        if m.norms is not None:
            names += ["norms.%d.weight" % l, "norms.%d.bias" % l]
            ps += [m.norms[l].weight, m.norms[l].bias]
    return names, ps


def stack_run(kind, m, x, ei, r, want_dx, scale=1.0):
    """Forward and backward of loss = scale * sum(y * r) / n: (y, parameter gradients, dx or None)."""
    m.zero_grad(set_to_none=True)
    x = x.detach().clone().requires_grad_(want_dx)
    y = stack_forward(kind, m, x, ei)
    ((y * r).sum() * scale / y.shape[0]).backward()
    return y.detach(), [p.grad.detach().clone() for p in stack_params(m)[1]], x.grad.detach().clone() if want_dx else None


# ---- the whole-batch norms under the float64 rule (tests/test_gpu_norm_parity.py) ------------------------------------------------

NORM_EPS = 1e-5
NORM_KINDS = ("layernorm", "colnorm", "colnorm-cached")
DEAD_ZERO, DEAD_CONST, DEAD_MS1 = (3, 17), 5, 7          # columns of the "dead" variant


def ref_layernorm(x, w, b, relu, pre=None):
    """torch_geometric LayerNorm(mode="graph") without a batch vector (oracle/model_ref.py: LayerNormRef), ReLU behind it."""
    xc = x - x.mean()
    y = xc / (xc.std(unbiased=False) + NORM_EPS) * w + b
    if pre is not None:
        pre.append(y.detach())
    return torch.relu(y) if relu else y


def ref_colnorm(x, w, b, ms, relu, cache=None, pre=None):
    """CachedGraphNorm without a batch vector (oracle/model_ref.py: CachedGraphNormRef): (y, [2, H] = mean | var as used)."""
    if cache is None:
        mean = x.mean(0, keepdim=True)
        out = x - mean * ms
        var = out.pow(2).mean(0, keepdim=True)
    else:
        mean, var = cache[0:1], cache[1:2]
        out = x - mean * ms
    y = w * out / (var + NORM_EPS).sqrt() + b
    if pre is not None:
        pre.append(y.detach())
    return (torch.relu(y) if relu else y), torch.cat([mean, var]).detach()


def norm_inputs(kind, n, hidden, variant, seed):
    """x = randn * 3 + 1.5 [n, hidden], weight ~ U(0.5, 1.5), bias ~ 0.3 N(0, 1), mean_scale ~ U(0.6, 1.4), R ~ U(-1, 1), cached
    statistics mean ~ 1.5 + 0.5 N(0, 1), var ~ 9 U(0.5, 1.5).  Variants: "shift" moves x to a mean of ten standard deviations;
    "dead" (colnorm) zeroes columns 3 and 17, holds column 5 at 1.5 and sets mean_scale[7] = 1; "const" holds every element
    at 1.5; "corr" adds (x - 1.5) / 3 to R, so that sum(dy * xhat) grows with the element count instead of its square root
    and the statistics' own share of dx (k (x - mu) of the LayerNorm, B o of CachedGraphNorm) is of the size of dx."""
    gen = torch.Generator().manual_seed(((seed * 1031 + n) * 257 + hidden) * 3 + NORM_KINDS.index(kind))
    x = torch.randn(n, hidden, generator=gen) * 3.0 + 1.5
    t = dict(w=torch.rand(hidden, generator=gen) + 0.5, b=torch.randn(hidden, generator=gen) * 0.3,
             ms=torch.rand(hidden, generator=gen) * 0.8 + 0.6, r=torch.rand(n, hidden, generator=gen) * 2 - 1)
    cache = torch.stack([1.5 + 0.5 * torch.randn(hidden, generator=gen), 9.0 * (torch.rand(hidden, generator=gen) + 0.5)])
    if variant == "shift":
        x, cache[0] = x + 28.5, cache[0] + 28.5
    elif variant == "dead":
        x[:, list(DEAD_ZERO)], x[:, DEAD_CONST], t["ms"][DEAD_MS1] = 0.0, 1.5, 1.0
    elif variant == "const":
        x[:] = 1.5
    elif variant == "corr":
        t["r"] = t["r"] + (x - 1.5) / 3.0
    else:
        assert variant == "plain", variant
    t["x"] = x
    if kind == "layernorm":
        del t["ms"]
    if kind == "colnorm-cached":
        t["cache"] = cache
    return t


def norm_leaves(kind):
    return ("x", "w", "b") if kind == "layernorm" else ("x", "w", "b", "ms")


def norm_fwd_bwd(kind, inp, relu, dtype=torch.float32, device=None, pre=None):
    """Forward and backward of sum(y * R): dict(y, stats, grads {x, w, b[, ms]}).  ``device``: through ops.graph_layernorm /
    ops.graph_colnorm, and ``raw_dx`` is the gradient tensor as the backward returned it; else the torch expression on the
    CPU in ``dtype``."""
    leaves = {k: inp[k].to(dtype=dtype, device=device).clone().requires_grad_(True) for k in norm_leaves(kind)}
    r = inp["r"].to(dtype=dtype, device=device)
    cache = inp["cache"].to(dtype=dtype, device=device) if kind == "colnorm-cached" else None
    raw = []
    if device is not None:
        from gnn_hex_amd import ops
        leaves["x"].register_hook(raw.append)
        if kind == "layernorm":
            y, stats = ops.graph_layernorm(leaves["x"], leaves["w"], leaves["b"], NORM_EPS, relu), None
        else:
            y, stats = ops.graph_colnorm(leaves["x"], leaves["w"], leaves["b"], leaves["ms"], NORM_EPS, relu, cache)
    elif kind == "layernorm":
        y, stats = ref_layernorm(leaves["x"], leaves["w"], leaves["b"], relu, pre), None
    else:
        y, stats = ref_colnorm(leaves["x"], leaves["w"], leaves["b"], leaves["ms"], relu, cache, pre)
    (y * r).sum().backward()
    if device is not None:
        torch.cuda.synchronize()
    return dict(y=y.detach(), stats=None if stats is None else stats.detach(), grads={k: v.grad for k, v in leaves.items()},
                raw_dx=raw[0] if raw else None)


def relu_margin_of(tensors):
    """min |t| / rms(t) over the tensors a ReLU is applied to (1 when there is none)."""
    return min([(t.abs().min() / t.pow(2).mean().sqrt().clamp(min=1e-300)).item() for t in tensors if t.numel()] + [1.0])


def norm_kernel_oracle(kind, n, hidden, variant, zero_grads=()):
    """float64 and fp32 results of one kernel case, with and without the ReLU, at the first input seed below SEEDS whose float64
    pre-ReLU tensor keeps MARGIN and whose gradient tensors (with and without the ReLU; not those of ``zero_grads``, which vanish
    identically in this variant) all reach |g|max >= 1e-2."""
    for seed in range(SEEDS):
        inp = norm_inputs(kind, n, hidden, variant, seed)
        pre = []
        r64 = {False: norm_fwd_bwd(kind, inp, False, torch.float64, pre=pre)}
        margin = relu_margin_of(pre)
        if margin < MARGIN:
            continue
        r64[True] = norm_fwd_bwd(kind, inp, True, torch.float64)
        gmax = min(g.abs().max().item() for relu in (False, True) for k, g in r64[relu]["grads"].items() if k not in zero_grads)
        if gmax >= 1e-2:
            break
    else:
        raise AssertionError("%s n %d hidden %d %s: no input seed below %d meets the oracle conditions" % (kind, n, hidden, variant, SEEDS))
    for relu in (False, True):
        for k in zero_grads:
            assert float(r64[relu]["grads"][k].abs().max()) == 0.0, k
    text = "smallest |ReLU input| / rms %.3g (>= 2^-16), smallest |g|max %.3g (>= 1e-2)" % (margin, gmax)
    print("oracle %s n %d hidden %d %s: input seed %d; %s" % (kind, n, hidden, variant, seed, text))
    r32 = {relu: norm_fwd_bwd(kind, inp, relu, torch.float32) for relu in (False, True)}
    return dict(inp=inp, seed=seed, ok=margin >= MARGIN and gmax >= 1e-2, text=text, r64=r64, r32=r32)


# ---- the norm stack (ops.sage_norm_stack) on batches of any size --------------------------------------------------------------

def stack_conditions(kind, m64, c_in, x64, ei, r64, padded, layers=3, p_edge=0.08):
    """The input conditions of a SAGE stack on its float64 oracle, with the loss scaled by the smallest power of two at which every
    gradient tensor reaches |g|max >= 1e-2 (exact in every arithmetic, no relative figure changes): (ok, text, scale, y64, g64, dx64).
    ``layers`` and ``p_edge`` say what the caller built ``m64`` and ``ei`` with: the ReLU margin is taken over exactly ``layers``
    pre-activation tensors, and the text names both where they are not the defaults."""
    pre = []
    with torch.no_grad():
        stack_forward(kind, m64, x64, ei, pre)
    assert len(pre) == (0 if kind == "single" else layers), (kind, len(pre), layers)
    margin = relu_margin_of(pre)
    if margin < MARGIN:
        return False, "smallest |ReLU input| / rms %.3g" % margin, 1.0, None, None, None
    y64, g64, dx64 = stack_run(kind, m64, x64, ei, r64, padded)
    scale, gmax = 1.0, min(g.abs().max().item() for g in g64 + ([dx64] if padded else []))
    while gmax * scale < 1e-2 and scale < 2.0 ** 12:
        scale *= 2.0
    if scale != 1.0:
        y64, g64, dx64 = stack_run(kind, m64, x64, ei, r64, padded, scale)
    sens = []
    with torch.no_grad():
        for k in range(c_in if not padded else 0):
            xz = x64.clone()
            xz[:, k] = 0
            sens.append((stack_forward(kind, m64, xz, ei) - y64).abs().max().item())
    shares = [1.0] if padded else column_shares(g64[0], c_in) + column_shares(g64[2], c_in)
    sens = sens or [1.0]
    spread = (y64.max() - y64.min()).item()
    ok = min(sens) > 0.1 and min(shares) >= 0.02 and spread >= 0.5 and gmax * scale >= 1e-2
    text = "output sensitivity per feature %.3g..%.3g (> 0.1), layer-0 gradient column share %.3g..%.3g (>= 0.02), output spread " \
           "%.3g (>= 0.5), smallest |g|max %.3g (>= 1e-2) at loss scale %g, smallest |ReLU input| / rms %.3g (>= 2^-16)" \
           % (min(sens), max(sens), min(shares), max(shares), spread, gmax * scale, scale, margin)
    if (layers, p_edge) != (3, 0.08):
        text += "; %d layers, p_edge %g" % (layers, p_edge)
    return ok, text, scale, y64, g64, dx64


def stack_oracle(kind, c_in, hidden, sizes, layers=3, p_edge=0.08, order=None):
    """A stack of ``layers`` layers on ``feature_batch(sizes, c_in, seed=100 + c_in, p_edge=p_edge)`` (``order``: its graphs in
    that order, ``reorder_graphs``; R stays with its rows), loss scale * sum(y * R) / n with R ~ U(-1, 1): the float64 and fp32
    oracle results at the first weight seed below SEEDS that meets ``stack_conditions``."""
    import copy
    x, ei, bv, ptr = feature_batch(sizes, c_in, seed=100 + c_in, p_edge=p_edge)
    gen = torch.Generator().manual_seed(7)
    r = torch.rand(x.shape[0], hidden, generator=gen) * 2 - 1
    if order is not None:
        x, ei, bv, ptr, rows = reorder_graphs(x, ei, ptr, order)
        r = r[rows]
    padded = c_in == hidden
    for seed in range(SEEDS):
        m = stack_model(kind, c_in, hidden, seed, layers)
        if kind == "norm":                  # non-trivial affine parameters (the default is weight 1, bias 0)
            with torch.no_grad():
                for nm in m.norms:
                    nm.weight.add_(torch.randn(hidden) * 0.2)
                    nm.bias.add_(torch.randn(hidden) * 0.2)
        ok, text, scale, y64, g64, dx64 = stack_conditions(kind, copy.deepcopy(m).double(), c_in, x.double(), ei, r.double(), padded,
                                                           layers, p_edge)
        if ok:
            break
    else:
        raise AssertionError("%s c_in %d hidden %d rows %d: no weight seed below %d meets the oracle conditions"
                             % (kind, c_in, hidden, x.shape[0], SEEDS))
    y32, g32, dx32 = stack_run(kind, m, x, ei, r, padded, scale)
    print("oracle %s c_in %d hidden %d rows %d: weight seed %d; %s" % (kind, c_in, hidden, x.shape[0], seed, text))
    return dict(m=m, x=x, ei=ei, ptr=ptr, r=r, scale=scale, seed=seed, ok=ok, text=text, y64=y64, g64=g64, dx64=dx64, y32=y32, g32=g32,
                dx32=dx32)


# ---- the two model families with their norms ----------------------------------------------------------------------------------------

def norm_model_ref(family, layers, hidden, seed, head_layers=2):
    """The oracle's ``modern_two_headed`` (whole-batch LayerNorm) or ``two_headed`` (CachedGraphNorm) with norm=True, sharpened,
    every norm's weight, bias and mean_scale moved by 0.2 N(0, 1)."""
    from oracle.model_ref import get_pre_defined_ref
    args = Namespace(num_layers=layers, hidden_channels=hidden, norm=True, noisy_dqn=False, noisy_sigma0=0.5, num_head_layers=head_layers)
    torch.manual_seed(seed)
    ref = sharpen_(get_pre_defined_ref(family, args))
    with torch.no_grad():
        for k, p in ref.named_parameters():
            if "norm" in k:
                p.add_(torch.randn(p.shape) * 0.2)
    return ref


def norm_model_hip(family, ref, layers, hidden, head_layers=2):
    from gnn_hex_amd.models import get_pre_defined
    args = Namespace(num_layers=layers, hidden_channels=hidden, norm=True, noisy_dqn=False, noisy_sigma0=0.5, num_head_layers=head_layers)
    hip = get_pre_defined(family, args)
    res = hip.load_state_dict(ref.state_dict())
    assert not res.missing_keys and not res.unexpected_keys
    return hip.cuda()


def model_step(model, batch, sel, tgt, **kw):
    """mse(Q[sel], tgt) forward and backward: (Q, final_conv_acts, {name: gradient or None})."""
    model.zero_grad(set_to_none=True)
    q = model(*batch, **kw)
    torch.nn.functional.mse_loss(q.reshape(-1)[sel], tgt).backward()
    return (q.detach().reshape(-1), model.final_conv_acts.detach().clone(),
            {k: (None if p.grad is None else p.grad.detach().clone()) for k, p in model.named_parameters()})


def norm_model_margin(ref64, maker, run):
    """min |ReLU input| / rms during run(): the outputs of the body's and the playing head's norms (the ReLU follows the norm; no
    ReLU follows after_embed_norm) and of the value MLP's first layer where there is one."""
    head = ref64.maker_head if maker else ref64.breaker_head
    mods = list(ref64.gnn.norms) + list(head.gnn.norms)
    if hasattr(head.value_head, "layers"):
        mods.append(head.value_head.layers[0])
    pre, hooks = [], [m.register_forward_hook(lambda mod, inp, out: pre.append(out.detach())) for m in mods]
    try:
        out = run()
    finally:
        for h in hooks:
            h.remove()
    assert len(pre) >= len(mods) - 1              # advantages_only runs no value MLP
    return relu_margin_of(pre), out


# ---- every tile count, kernel form and CSR home of the fused per-graph kernels (tests/test_gpu_fused_instantiations.py) ---------

def csr_capacity(hidden):
    """Edges of one graph the fused kernels keep in LDS at this width (hexgnn_qnet_csr_capacity)."""
    from gnn_hex_amd import _lib
    cap = _lib.lib().hexgnn_qnet_csr_capacity(int(hidden))
    assert cap > 0, (hidden, cap)
    return cap


def model_relu_margin(ref64, maker, run):
    """min |ReLU input| / rms over the SAGE layers of the body and of the playing head and the value MLP's first layer of an
    oracle model without norms, during run()."""
    store, hooks = {}, []
    head = ref64.maker_head if maker else ref64.breaker_head
    for conv in list(ref64.gnn.convs) + list(head.gnn.convs):
        hooks.append(conv.register_forward_hook(lambda mod, inp, out: store.__setitem__(id(mod), out.detach())))
    hooks.append(head.value_head.layers[0].register_forward_hook(lambda mod, inp, out: store.__setitem__("value", out.detach())))
    try:
        with torch.no_grad():
            run()
    finally:
        for h in hooks:
            h.remove()
    return min((t.abs().min() / t.pow(2).mean().sqrt()).item() for t in store.values())


def truncated_graphs(make, rows, edge_counts, seed, p_edge):
    """One batch of len(edge_counts) graphs of ``rows`` nodes each: graph g is ``make([rows], seed + g, p_edge=p_edge)`` (an
    edge list in random order) cut to exactly edge_counts[g] edges."""
    xs, eis, bv, ptr = [], [], [], [0]
    for g, k in enumerate(edge_counts):
        x, ei, _, _ = make([rows], seed=seed + g, p_edge=p_edge)
        assert ei.shape[1] >= k, "graph %d: %d edges, %d wanted" % (g, ei.shape[1], k)
        xs.append(x)
        eis.append(ei[:, :k] + ptr[-1])
        bv.append(torch.full((rows,), g, dtype=torch.long))
        ptr.append(ptr[-1] + rows)
    return torch.cat(xs), torch.cat(eis, 1), torch.cat(bv), torch.tensor(ptr, dtype=torch.long)


def graph_edge_counts(ei, ptr):
    """Edges per graph, by the graph of the edge's target row."""
    return torch.bincount(torch.bucketize(ei[1], ptr[1:], right=True), minlength=ptr.numel() - 1).tolist()


def spread_selection(ptr, seed=1):
    """(sel, tgt, w): ``one_row_per_graph``, every second graph's selection (graphs 0, 2, ..) moved to its LAST row, and weights
    ~ U(0.5, 1.5)."""
    sel, tgt = one_row_per_graph(ptr, seed)
    sel = sel.clone()
    sel[0::2] = ptr[1:][0::2] - 1
    gen = torch.Generator().manual_seed(seed + 1000)
    return sel, tgt, torch.rand(sel.numel(), generator=gen) + 0.5


class TdCases:
    """The TD step of ``modern_two_headed`` (``body`` + ``head`` layers, sharpened) on named batches: per (batch, hidden) the
    float64 and fp32 oracle results of loss = mean(w (Q[sel] - tgt)^2) at the first weight seed below SEEDS at which the float64
    oracle has no ReLU input within MARGIN of zero (relative to its tensor's rms), a Q spread >= 0.5 and |g|max >= 1e-2 in every
    gradient tensor -- once per session, from the oracle alone.  ``recorded`` {(batch key, hidden): seed} holds what that search
    found before (a float64 pass over these batches takes seconds, a search up to a minute): the conditions are evaluated at the
    recorded seed as at any other, and the search runs where there is none or where it no longer meets them."""

    def __init__(self, body, head, batches, recorded=None):
        self.body, self.head, self.batches = body, head, batches       # batches(name, hidden) -> (builder, key)
        self.recorded = dict(recorded or {})
        self._batches, self._oracles = {}, {}

    def args(self, hidden):
        return model_args(self.body, hidden, self.head)

    def ref(self, hidden, seed):
        from oracle.model_ref import get_pre_defined_ref
        torch.manual_seed(seed)
        return sharpen_(get_pre_defined_ref("modern_two_headed", self.args(hidden)))

    def hip(self, ref, hidden):
        from gnn_hex_amd.models import get_pre_defined
        hip = get_pre_defined("modern_two_headed", self.args(hidden))
        res = hip.load_state_dict(ref.state_dict())
        assert not res.missing_keys and not res.unexpected_keys
        return hip.cuda()

    def batch(self, name, hidden):
        b, key = self.batches(name, hidden)
        if key not in self._batches:
            x, ei, bv, ptr = b()
            self._batches[key] = (x, ei, bv, ptr) + spread_selection(ptr)
        return key, self._batches[key]

    @staticmethod
    def ref_run(model, x, ei, bv, ptr, sel, tgt, w):
        model.zero_grad(set_to_none=True)
        q = model(x, ei, bv, ptr)
        d = q[sel] - tgt
        loss = (w * d * d).mean()
        loss.backward()
        return dict(loss=loss.detach(), td=d.detach(), q=q.detach(),
                    grads=[None if p.grad is None else p.grad.detach().clone() for p in model.parameters()])

    def conditions(self, ref64, inputs, search=False):
        x, ei, bv, ptr, sel, tgt, w = inputs
        x64 = x.double()
        margin = model_relu_margin(ref64, bool(x[0, 2] == 1), lambda: ref64(x64, ei, bv, ptr))
        if search and margin < MARGIN:
            return False, "", None
        r64 = self.ref_run(ref64, x64, ei, bv, ptr, sel, tgt.double(), w.double())
        spread = (r64["q"].max() - r64["q"].min()).item()
        gmax = min(g.abs().max().item() for g in r64["grads"] if g is not None)
        ok = margin >= MARGIN and spread >= 0.5 and gmax >= 1e-2
        return ok, "Q spread %.3g (>= 0.5), smallest |g|max %.3g (>= 1e-2), smallest |ReLU input| / rms %.3g (>= 2^-16)" \
            % (spread, gmax, margin), r64

    def oracle(self, name, hidden):
        import copy
        key, inputs = self.batch(name, hidden)
        if (key, hidden) not in self._oracles:
            known = self.recorded.get((key, hidden))
            for seed in ([] if known is None else [known]) + list(range(SEEDS)):
                ref = self.ref(hidden, seed)
                ok, text, r64 = self.conditions(copy.deepcopy(ref).double(), inputs, search=True)
                if ok:
                    break
            else:
                raise AssertionError("%s hidden %d: no weight seed below %d meets the oracle conditions" % (key, hidden, SEEDS))
            x, ei, bv, ptr, sel, tgt, w = inputs
            print("oracle %s hidden %d: %d rows, weight seed %d; %s" % (key, hidden, x.shape[0], seed, text))
            self._oracles[(key, hidden)] = dict(ref=ref, seed=seed, ok=ok, text=text, r64=r64, inputs=inputs,
                                               r32=self.ref_run(ref, x, ei, bv, ptr, sel, tgt, w),
                                               names=[k for k, _ in ref.named_parameters()])
        o = self._oracles[(key, hidden)]
        assert o["ok"], "%s hidden %d: %s" % (key, hidden, o["text"])
        return o


# ---- the self-play acting path at the published widths (tests/test_gpu_acting_path.py) -------------------------------------------

# shape -> (board size, body layers, hidden); two head layers.  L: the published GNN-L (123-row start graphs: all eight waves own
# rows, 5 padding rows; NT 7 with two pad columns); S: GNN-S (NT 3 with pad columns, 51 rows: waves 4-7 own none); W: 146 rows, the
# layer-major kernels over a capacity-sized target with clear_tail
ACTING_SHAPES = {"L": (11, 15, 110), "S": (7, 10, 35), "W": (12, 3, 110)}
ACTING_ENVS = 6


def acting_script(hexref, size, odd, recorded=None, k=ACTING_ENVS, max_plies=400):
    """A script of legal random moves that brings ``k`` lock-stepped envs from the start position to ``k`` DIFFERENT node counts
    with at least one env auto-reset on the way, found on the C env oracle alone: per seed (``recorded`` first, then 0, 1, ..) every
    env plays ``default_rng(seed)``'s choice among its legal vertices, and the script ends at the first ply count of the wanted
    parity (even: the maker is to move) at which both properties hold.  Returns dict(seed, moves [plies][k], ref = the oracle
    manager at the end, reset [k] = which envs were reset)."""
    for seed in ([] if recorded is None else [recorded]) + list(range(64)):
        ref = hexref.RefEnvManager(k, size)
        ref.reset()
        rng = np.random.default_rng(seed)
        moves, reset = [], np.zeros(k, dtype=bool)
        for ply in range(1, max_plies + 1):
            acts = [int(v[rng.integers(len(v))]) for v in ref.get_valid_actions()]
            _, _, dones, _ = ref.step(acts)
            moves.append(acts)
            reset |= dones
            nodes = [e.num_vertices() for e in ref.envs]
            if ply % 2 == int(odd) and reset.any() and len(set(nodes)) == k and min(nodes) >= 4:
                return dict(seed=seed, moves=moves, ref=ref, reset=reset)
    raise AssertionError("Hex-%d: no move script below seed 64 gives %d different graph sizes and a reset env" % (size, k))


def oracle_batch(games):
    """The oracle's own observations of ``games`` (RefGame), collated: (x, edge_index, batch, ptr, backmap) as CPU tensors."""
    obs = [g.observe() for g in games]
    offs = np.concatenate([[0], np.cumsum([o[0].shape[0] for o in obs])]).astype(np.int64)
    return (torch.from_numpy(np.concatenate([o[0] for o in obs])),
            torch.from_numpy(np.concatenate([o[1] + off for o, off in zip(obs, offs[:-1])], 1)),
            torch.from_numpy(np.repeat(np.arange(len(obs)), np.diff(offs))), torch.from_numpy(offs),
            torch.from_numpy(np.concatenate([o[2] for o in obs])))


def graph_spreads(a, ptr):
    """max - min of ``a`` over the non-terminal rows of every graph."""
    p = [int(v) for v in ptr]
    return [(a[p[g] + 2:p[g + 1]].max() - a[p[g] + 2:p[g + 1]].min()).item() for g in range(len(p) - 1)]


def acting_oracle(body, hidden, batch, maker, recorded=None, head=2, need_margin=True):
    """Advantages (``advantages_only``: 2 tanh(a) per node) of the sharpened ``modern_two_headed`` oracle on ``batch`` in float64
    and fp32, at the first weight seed below SEEDS (``recorded`` first; the conditions are evaluated there as anywhere) at which
    the float64 oracle alone has no ReLU input within MARGIN of zero (relative to its tensor's rms) and an advantage spread of at
    least 0.5 over the non-terminal rows of every graph.  ``need_margin=False`` (a batch on which a full scan found no seed
    below SEEDS with that margin: the caller records the scan) takes the first seed that meets the spread condition and reports
    the margin it has."""
    import copy
    from oracle.model_ref import get_pre_defined_ref
    x, ei, bv, ptr = batch[:4]
    assert bool((x[:, 2] == (1.0 if maker else 0.0)).all()), "the batch's side flag"
    x64 = x.double()
    for seed in ([] if recorded is None else [recorded]) + list(range(SEEDS)):
        torch.manual_seed(seed)
        ref = sharpen_(get_pre_defined_ref("modern_two_headed", model_args(body, hidden, head)))
        ref64 = copy.deepcopy(ref).double()
        out = []
        margin = model_relu_margin(ref64, maker, lambda: out.append(ref64(x64, ei, bv, ptr, advantages_only=True).reshape(-1)))
        if need_margin and margin < MARGIN:
            continue
        spread = min(graph_spreads(out[0], ptr))
        if spread >= 0.5:
            break
    else:
        raise AssertionError("%d + %d layers, hidden %d, %d rows: no weight seed below %d meets the oracle conditions"
                             % (body, head, hidden, x.shape[0], SEEDS))
    with torch.no_grad():
        a32 = ref(x, ei, bv, ptr, advantages_only=True).reshape(-1)
    text = "smallest |ReLU input| / rms %.3g (%s), smallest advantage spread of a graph %.3g (>= 0.5)" \
           % (margin, ">= 2^-16" if need_margin else "no condition", spread)
    return dict(ref=ref, ref64=ref64, seed=seed, ok=(margin >= MARGIN or not need_margin) and spread >= 0.5, text=text, margin=margin,
                a64=out[0].detach(), a32=a32)


# ---- the stand-alone head tails (tests/test_gpu_head_tail.py) and the HexAra head kernels (tests/test_gpu_hexara_kernels.py) ----

# rows per graph of the "full" batch: both sides of the 16- and 32-row unrolled steps of the two row phases (row + 14 < r1,
# row + 30 < r1), of the per-row strides 64 and 256, and of the 1024 rows head_bwd_kernel keeps in LDS
HEAD_ROWS = [1, 2, 3, 15, 16, 17, 30, 31, 32, 33, 34, 47, 48, 49, 63, 64, 65, 66, 127, 128, 129, 255, 256, 257, 1023, 1024, 1025, 1300]
HEAD_WIDTHS = [2, 3, 16, 35, 62, 63, 64, 65, 66, 110, 127, 128]       # H / 2 = 1, 31, 32, 33, 64; odd H; padded width = H
HEAD_WIDE = 144                                                         # the same calls reach wide.hip
HEAD_MODE_WIDTHS = (35, 66, 128)                                        # all five modes run here
HEAD_NAMES = {"mlp": ["lin_w", "lin_b", "v0_w", "v0_b", "v1_w", "v1_b"], "linear": ["lin_w", "lin_b", "val_w", "val_b"]}
HEAD_TOP = 8.0                                                          # above every |N(0, 1)| draw of these batches (asserted)


def head_sizes(name):
    """Rows per graph: "full" = HEAD_ROWS in a fixed shuffled order with an empty graph in the middle and one at the end; "row1" and
    "rows1025" = one graph."""
    if name == "row1":
        return [1]
    if name == "rows1025":
        return [1025]
    assert name == "full", name
    sizes = [int(v) for v in np.random.default_rng(11).permutation(HEAD_ROWS)]
    assert sizes != sorted(sizes) and sizes != sorted(sizes, reverse=True)
    return sizes[:len(sizes) // 2] + [0] + sizes[len(sizes) // 2:] + [0]


def tie_rows(cnt, g):
    """Offsets (lo, hi) of the two rows of a graph that hold column 1's maximum in the "ties" family: opposite row parities, the
    lower one in the odd row phase for even g and in the even phase for odd g; hi is the last row of its parity."""
    if cnt < 4:
        return 0, 1
    if g % 2 == 0:
        return 1, (cnt - 1) & ~1
    return 0, cnt - 1 if (cnt - 1) % 2 == 1 else cnt - 2


def head_inputs(name, hidden, family):
    """dict(sizes, ptr, batch, b, h [n, hidden], r1 [n], r2 [b], sel): family "randn": h ~ N(0, 1); "ties": h = relu(N(0, 1)) (about
    half the entries exactly 0: min ties are the norm, as behind a ReLU layer), column 0 constant over every graph, column 1 equal
    to its maximum HEAD_TOP in exactly the two rows ``tie_rows`` of every graph with two or more rows, column 2 equal to HEAD_TOP in
    rows 1021 and 1024 of every graph above 1024 rows.  r1, r2 ~ U(-1, 1) weight the outputs in the loss; ``sel`` = one row of every
    non-empty graph (``one_row_per_graph`` on the pointer without its empty graphs)."""
    sizes = head_sizes(name)
    ptr = torch.tensor([0] + list(np.cumsum(sizes)), dtype=torch.long)
    b, n = len(sizes), int(ptr[-1])
    batch = torch.repeat_interleave(torch.arange(b), torch.tensor(sizes))
    gen = torch.Generator().manual_seed((hidden * 7919 + n) * 2 + (family == "ties"))
    h = torch.randn(n, hidden, generator=gen)
    assert float(h.abs().max()) < HEAD_TOP
    if family == "ties":
        assert hidden >= 4
        h = torch.relu(h)
        for g, cnt in enumerate(sizes):
            r0 = int(ptr[g])
            if cnt == 0:
                continue
            h[r0:r0 + cnt, 0] = 0.25 + 0.125 * (g % 5)
            if cnt >= 2:
                lo, hi = tie_rows(cnt, g)
                assert lo < hi < cnt and (lo + hi) % 2 == 1
                h[r0 + lo, 1] = h[r0 + hi, 1] = HEAD_TOP
            if cnt > 1024:
                h[r0 + 1021, 2] = h[r0 + 1024, 2] = HEAD_TOP
    else:
        assert family == "randn", family
    r1, r2 = torch.rand(n, generator=gen) * 2 - 1, torch.rand(b, generator=gen) * 2 - 1
    sel, _ = one_row_per_graph(torch.unique_consecutive(ptr))
    return dict(sizes=sizes, ptr=ptr, batch=batch, b=b, n=n, h=h, r1=r1, r2=r2, sel=sel)


def head_modules(kind, hidden, seed, vscale=0.02):
    """(advantage Linear(H, 1), value head) at torch's default init under manual_seed(seed): kind "mlp" -> MLPRef(H / 2, 1, 4 H, 1)
    with its first layer scaled by ``vscale`` (``sharpen_``: tanh(v) must not saturate on sum-pooled inputs of a thousand rows),
    "linear" -> Linear(H, 1)."""
    from oracle.model_ref import MLPRef
    torch.manual_seed(seed)
    lin = torch.nn.Linear(hidden, 1)
    if kind == "mlp":
        val = MLPRef(hidden // 2, 1, 4 * hidden, 1)
        with torch.no_grad():
            val.layers[0].weight.mul_(vscale)
    else:
        assert kind == "linear", kind
        val = torch.nn.Linear(hidden, 1)
    return lin, val


def head_params(lin, val):
    """Parameters in the order of ops.HeadTailFn / ops.HeadLinearTailFn (HEAD_NAMES)."""
    return [lin.weight, lin.bias] + [p for layer in getattr(val, "layers", [val]) for p in (layer.weight, layer.bias)]


def head_pooled(h, batch, b, val):
    """What the value head reads: [sum | max | min | mean] over every graph's rows for the MLP, the mean alone for the Linear; an
    empty graph pools to zeros, max / min send their gradient to the first row that attains them (scatter_ref)."""
    from oracle.model_ref import scatter_ref
    aggr = ("sum", "max", "min", "mean") if hasattr(val, "layers") else ("mean",)
    return torch.cat([scatter_ref(h, batch, dim_size=b, reduce=a) for a in aggr], dim=1)


def head_tail_ref(h, batch, b, mode, lin, val):
    """HeadNetwork.forward behind its SAGE layers (advantage linear, pooling, value head) and DuellingTwoHeaded's combine as one
    torch expression.  Returns (q [n], out_v [b] or None): mode 0 Q; 1 (A - mean A, tanh(v)); 2 2 tanh(a); 3 raw (a, v); 4 raw a."""
    from oracle.model_ref import scatter_ref
    a = lin(h).reshape(-1)
    if mode == 4:
        return a, None
    t = 2 * torch.tanh(a)
    if mode == 2:
        return t, None
    v = val(head_pooled(h, batch, b, val)).reshape(-1)
    if mode == 3:
        return a, v
    centred = t - scatter_ref(t, batch, dim_size=b, reduce="mean").index_select(0, batch)
    if mode == 1:
        return centred, torch.tanh(v)
    return torch.tanh(v).index_select(0, batch) + centred, None


def head_loss(q, out_v, r1, r2):
    """sum(q * R1) + sum(out_v * R2): separable, so every row and every graph has a gradient of its own."""
    loss = (q * r1).sum()
    return loss if out_v is None else loss + (out_v * r2).sum()


def head_ref_run(lin, val, h, batch, b, mode, r1, r2):
    ps = head_params(lin, val)
    for p in ps:
        p.grad = None
    h = h.detach().clone().requires_grad_(True)
    q, v = head_tail_ref(h, batch, b, mode, lin, val)
    head_loss(q, v, r1, r2).backward()
    return dict(q=q.detach(), v=None if v is None else v.detach(), dh=h.grad.detach().clone(),
                grads=[None if p.grad is None else p.grad.detach().clone() for p in ps])


def head_dev_run(kind, ps, h, gptr, b, hidden, mode, r1, r2):
    """The same step through ops.HeadTailFn / ops.HeadLinearTailFn; ``ps`` (CPU tensors in HEAD_NAMES order), h, r1, r2 on the CPU."""
    from gnn_hex_amd import ops
    leaves = [p.detach().cuda().clone().requires_grad_(True) for p in ps]
    hd = h.cuda().requires_grad_(True)
    out = (ops.HeadTailFn if kind == "mlp" else ops.HeadLinearTailFn).apply(hd, gptr, b, hidden, mode, *leaves)
    q, v = (out[1], out[0]) if mode in (1, 3) else (out, None)
    head_loss(q, v, r1.cuda(), r2.cuda()).backward()
    torch.cuda.synchronize()
    return dict(q=q.detach(), v=None if v is None else v.detach(), dh=hd.grad, grads=[p.grad for p in leaves])


def head_same_bits(tag, a, b):
    for k in ("q", "v", "dh"):
        assert (a[k] is None) == (b[k] is None) and (a[k] is None or torch.equal(a[k], b[k])), "%s: %s differs" % (tag, k)
    for i, (ga, gb) in enumerate(zip(a["grads"], b["grads"])):
        assert (ga is None) == (gb is None) and (ga is None or torch.equal(ga, gb)), "%s: gradient %d differs" % (tag, i)


class HeadCases:
    """The stand-alone head-tail cases: per (kind, batch, hidden, family) the first weight seed below SEEDS at which, in float64 on
    the CPU, every pre-activation of the value MLP's ReLU is at least MARGIN x its tensor's rms away from 0 (the Linear value head
    has no ReLU: seed 0), and per (mode, loss form) the float64 and fp32 results of the torch expression -- once per session.
    Loss forms: "dense" R1 ~ U(-1, 1) on every row; "sel" R1 non-zero on one row per graph (the shape of a TD-loss gradient)."""

    def __init__(self):
        self._inputs, self._seeds, self._oracles = {}, {}, {}

    def inputs(self, name, hidden, family):
        key = (name, hidden, family)
        if key not in self._inputs:
            self._inputs[key] = head_inputs(name, hidden, family)
        return self._inputs[key]

    def margin(self, kind, name, hidden, family, seed):
        if kind == "linear":
            return 1.0
        inp = self.inputs(name, hidden, family)
        _, val = head_modules(kind, hidden, seed)
        val = val.double()
        if "pooled64" not in inp:
            inp["pooled64"] = head_pooled(inp["h"].double(), inp["batch"], inp["b"], val)
        with torch.no_grad():
            return relu_margin_of([val.layers[0](inp["pooled64"])])

    def seed(self, kind, name, hidden, family):
        key = (kind, name, hidden, family)
        if key not in self._seeds:
            for seed in range(SEEDS):
                margin = self.margin(kind, name, hidden, family, seed)
                if margin >= MARGIN:
                    break
            else:
                raise AssertionError("%s %s hidden %d %s: no weight seed below %d keeps the value MLP's ReLU inputs clear of zero"
                                     % (kind, name, hidden, family, SEEDS))
            self._seeds[key] = (seed, margin)
        return self._seeds[key]

    def r1(self, inp, loss):
        if loss == "dense":
            return inp["r1"]
        assert loss == "sel", loss
        r1 = torch.zeros_like(inp["r1"])
        r1[inp["sel"]] = inp["r1"][inp["sel"]]
        assert int((r1 != 0).sum()) == sum(1 for s in inp["sizes"] if s > 0)
        return r1

    def oracle(self, kind, name, hidden, family, mode, loss="dense"):
        import copy
        key = (kind, name, hidden, family, mode, loss)
        if key not in self._oracles:
            seed, margin = self.seed(kind, name, hidden, family)
            inp = self.inputs(name, hidden, family)
            lin, val = head_modules(kind, hidden, seed)
            r1 = self.r1(inp, loss)
            r64 = head_ref_run(copy.deepcopy(lin).double(), copy.deepcopy(val).double(), inp["h"].double(), inp["batch"], inp["b"],
                               mode, r1.double(), inp["r2"].double())
            r32 = head_ref_run(lin, val, inp["h"], inp["batch"], inp["b"], mode, r1, inp["r2"])
            print("oracle head %s %s hidden %d %s mode %d %s: weight seed %d, smallest |ReLU input| / rms %.3g (>= 2^-16)"
                  % (kind, name, hidden, family, mode, loss, seed, margin))
            self._oracles[key] = dict(inp=inp, r1=r1, seed=seed, margin=margin, r64=r64, r32=r32,
                                      ps=[p.detach().clone() for p in head_params(lin, val)])
        o = self._oracles[key]
        assert o["margin"] >= MARGIN
        return o

    def run(self, kind, name, hidden, family, mode, loss="dense"):
        o = self.oracle(kind, name, hidden, family, mode, loss)
        inp = o["inp"]
        return o, head_dev_run(kind, o["ps"], inp["h"], inp["ptr"].to(torch.int32).cuda(), inp["b"], hidden, mode, o["r1"], inp["r2"])

    @staticmethod
    def check(tag, kind, o, res, mode):
        """The rule of tests/test_gpu_wide_parity.py's stand-alone head case: q and out_v within max(3 x the fp32 expression's own,
        5e-6) of float64, dh and every parameter gradient within max(3 x its own, 2e-3) in relative norm; no value-head gradient
        in modes 2 and 4.  Returns {name: (kernel's figure, the fp32 expression's)}."""
        r64, r32 = o["r64"], o["r32"]
        assert tuple(res["q"].shape) == tuple(r64["q"].shape)
        figs = {"q": abs_bound(tag, "q", res["q"], r32["q"], r64["q"], QnetCases.CONST)}
        assert (res["v"] is None) == (mode not in (1, 3))
        if res["v"] is not None:
            assert tuple(res["v"].shape) == tuple(r64["v"].shape)
            figs["out_v"] = abs_bound(tag, "out_v", res["v"], r32["v"], r64["v"], QnetCases.CONST)
        assert tuple(res["dh"].shape) == tuple(r64["dh"].shape)
        figs["dh"] = rel_bound(tag, "dh", res["dh"], r32["dh"], r64["dh"])
        for name, g, a32, a64 in zip(HEAD_NAMES[kind], res["grads"], r32["grads"], r64["grads"]):
            if a64 is None:
                assert mode in (2, 4) and name[0] == "v", name
                assert g is None or float(g.abs().max()) == 0.0, "%s: %s has a gradient in mode %d" % (tag, name, mode)
                continue
            assert g is not None and tuple(g.shape) == tuple(a64.shape), name
            figs[name] = rel_bound(tag, name, g, a32, a64)
        print("%s: " % tag + "; ".join("%s %.3g (fp32 %.3g)" % ((k,) + v) for k, v in figs.items()))
        return figs


def sage_scalar_ref(h, ei, wl, bl, wr):
    """SAGEConv(H, 1) as scalars: out_i = b + h_i . w_r + mean over the in-edges (j -> i) of h_j . w_l (duplicates counted, a row
    without in-edges gets 0 for the mean)."""
    from oracle.model_ref import scatter_ref
    s = h @ wl.reshape(-1)
    return bl.reshape(()) + h @ wr.reshape(-1) + scatter_ref(s.index_select(0, ei[0]), ei[1], dim_size=h.shape[0], reduce="mean")


def policy_ref(pi_raw, should_swap, x, ptr, swap_allowed):
    """The output surgery and log-softmax of SageTorchScriptRef.forward (oracle/hexara_ref.py) on given logits: the two terminal
    rows of every graph dropped; with ``swap_allowed`` the graph's swap logit appended where feature 2 is set -- probed on the
    graph's LAST row for every graph but the last one and on the FIRST row of the last graph; log-softmax per segment.
    Returns (pi [live], output_graph_indices [live], output_batch_ptr [b + 1])."""
    from oracle.hexara_ref import scatter_log_softmax_ref
    nb = ptr.numel() - 1
    pieces, seg_ids, starts = [], [], [0]
    for gi in range(nb):
        lo, hi = int(ptr[gi]), int(ptr[gi + 1])
        seg = pi_raw[lo + 2:hi]
        if swap_allowed:
            probe_row = hi - 1 if gi < nb - 1 else lo
            if bool(x[probe_row, 2] != 0):
                seg = torch.cat((seg, should_swap[gi:gi + 1]))
        pieces.append(seg)
        seg_ids.append(torch.full((seg.numel(),), gi, dtype=torch.long))
        starts.append(starts[-1] + seg.numel())
    gi = torch.cat(seg_ids)
    return scatter_log_softmax_ref(torch.cat(pieces), gi), gi, torch.tensor(starts, dtype=torch.long)


# graph rows -> 1, 2, 128, 255..258, 512, 513 and 698 entries in front of the swap slot: both sides of policy_lsm_*_kernel's stride 256
POLICY_ROWS = [3, 4, 130, 257, 258, 259, 260, 514, 515, 700]
POLICY_BATCHES = {"rows": POLICY_ROWS, "many": [3] * 300, "one": [259]}


def policy_inputs(name, last, family):
    """dict(x [n, 3], ptr, pi_raw [n], should_swap [b], r): feature 2 is set per ROW -- graph g: g % 4 == 0 on its first row only,
    1 on its last row only, 2 on no row, 3 on every row; the LAST graph on its first row only (``last`` = "first": the first-row
    rule gives a slot, the last-row rule would not) or on its last row only ("last": the other way round).  family "unit":
    logits ~ N(0, 1); "spread": U(-30, 30), where nothing but the subtracted maximum keeps exp() in range.  r ~ U(-1, 1) [n]
    weights the live outputs in the loss (its first entries)."""
    sizes = POLICY_BATCHES[name]
    ptr = torch.tensor([0] + list(np.cumsum(sizes)), dtype=torch.long)
    b, n = len(sizes), int(ptr[-1])
    gen = torch.Generator().manual_seed(n * 4 + 2 * (last == "last") + (family == "spread"))
    x = torch.zeros(n, 3)
    x[:, 0] = torch.randint(0, 9, (n,), generator=gen).float()
    for g in range(b):
        lo, hi = int(ptr[g]), int(ptr[g + 1])
        x[lo:lo + 2, 1] = 1.0
        kind = g % 4 if g < b - 1 else {"first": 0, "last": 1}[last]
        if kind == 0:
            x[lo, 2] = 1.0
        elif kind == 1:
            x[hi - 1, 2] = 1.0
        elif kind == 3:
            x[lo:hi, 2] = 1.0
    if family == "spread":
        pi_raw, ss = (torch.rand(n, generator=gen) * 2 - 1) * 30, (torch.rand(b, generator=gen) * 2 - 1) * 30
    else:
        assert family == "unit", family
        pi_raw, ss = torch.randn(n, generator=gen), torch.randn(b, generator=gen)
    return dict(x=x, ptr=ptr, b=b, n=n, pi_raw=pi_raw, should_swap=ss, r=torch.rand(n, generator=gen) * 2 - 1)


def policy_ref_run(inp, swap_allowed, dtype):
    """Forward and backward of sum(pi * r[:live]) through ``policy_ref``: dict(pi, gi, ptr, d_raw [n], d_ss [b] or None)."""
    raw = inp["pi_raw"].to(dtype).clone().requires_grad_(True)
    ss = inp["should_swap"].to(dtype).clone().requires_grad_(True)
    pi, gi, optr = policy_ref(raw, ss, inp["x"], inp["ptr"], swap_allowed)
    (pi * inp["r"][:pi.numel()].to(dtype)).sum().backward()
    d_ss = None
    if swap_allowed:
        d_ss = torch.zeros_like(ss) if ss.grad is None else ss.grad.detach().clone()
    return dict(pi=pi.detach(), gi=gi, ptr=optr, d_raw=raw.grad.detach().clone(), d_ss=d_ss)


# ---- graph-structure kernels (csr.hip): the numpy reference of a sorted CSR + transpose ------------------------------------

def csr_reference(src, dst, n):
    """(rowptr, col, rowptr_t, col_t, invdeg) of the edge list src -> dst over n nodes, numpy only: row r of (rowptr, col) holds
    the sources of the edges INTO r, ascending; (rowptr_t, col_t) the targets of the edges OUT OF r; invdeg = 1 / max(in-degree, 1)
    in float32.  Multi-edges and self loops are kept, so the sorted result is unique and every comparison is array_equal."""
    src, dst = np.asarray(src, dtype=np.int64), np.asarray(dst, dtype=np.int64)
    deg = np.bincount(dst, minlength=n).astype(np.int64)
    rowptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    col = src[np.lexsort((src, dst))]
    rowptr_t = np.concatenate([[0], np.cumsum(np.bincount(src, minlength=n))]).astype(np.int64)
    col_t = dst[np.lexsort((dst, src))]
    invdeg = np.float32(1) / np.maximum(deg, 1).astype(np.float32)
    return rowptr, col, rowptr_t, col_t, invdeg
