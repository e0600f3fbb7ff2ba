"""GPU: the replay draw whose sizes never leave the device, and the update built on it.

1. ``hexgnn_replay_offsets``: offsets of hand-picked slot lists against numpy cumsums of the host's sizes, exactly.
2. ``GraphReplayBuffer.sample_device`` against ``sample`` from equally seeded generators: same slots and weights, the live
   part of both batches bit-equal, nothing written behind the live rows.
3. ``ops.td_step`` over capacity-sized buffers (``x._hex_live_rows``) against the exact-size call and the float64 oracle, with
   the live row count placed where the weight-gradient GEMM's device-side slice plan can go wrong.
4. ``GraphedUpdate``: six captured steps against six eager ones, every parameter and both priority trees bit-equal after every
   step, with a target sync and a ``put_block`` in between.
5. The refusals.

The float64 rule of part 3 is tests/helpers.py's (``check_grads`` / ``rel_bound``): per gradient tensor ||g - g64|| / ||g64|| <=
max(3 x the fp32 oracle's own distance, 2e-3), vanishing tensors to 1e-6 absolute, the raw first layer's columns one by one.
Weight state: ``helpers.sharpen_`` at the first seed whose ReLU inputs stay clear of zero (2^-16 of the tensor's rms, float64
oracle only) on ONE start board -- what the all-start-positions case needs, where every graph is the same graph and one
pre-activation within fp32 rounding of zero flips its mask in all of them at once (tests/test_gpu_dw_slices.py).  The mid-game
batches hold different boards: a flipped mask element there is one row of one graph among hundreds of rows, far below the
floor, so they carry no condition of their own.
"""
import copy

import numpy as np
import pytest
import torch

from helpers import MARGIN, PoisonedTorch, batch_tensors, check_grads, dw_plan, model_args, sel_and_targets, sharpen_
from helpers import model_relu_margin as _relu_margin      # (min |ReLU input| / rms over the SAGE layers and the value MLP)

pytestmark = pytest.mark.gpu


# ---- a short rollout, shared ---------------------------------------------------------------------------------------------

def _play(mgr, steps, rng):
    obs0 = mgr.reset()
    states, actions, rewards, dones, expl = [], [], [], [], []
    obs = obs0
    for _ in range(steps):
        acts_rank = [int(rng.integers(2, obs.node_off[i + 1] - obs.node_off[i])) for i in range(mgr.num_envs)]
        obs2, r, d, _ = mgr.step(mgr.validate_actions(obs, acts_rank))
        states.append(obs2); actions.append(acts_rank); rewards.append(r); dones.append(d)
        expl.append(np.zeros(mgr.num_envs, dtype=bool))
        obs = obs2
    return obs0, states, actions, rewards, dones, expl


@pytest.fixture(scope="module")
def rollouts():
    """Two Hex-5 rollouts of 12 envs x 14 moves: ((maker list, breaker list), (maker block, breaker block)) each."""
    from gnn_hex_amd.multi_env_manager import Env_manager
    out = []
    for seed in (3, 4):
        rng = np.random.default_rng(seed)
        mgr = Env_manager(12, 5, gamma=0.97, n_steps=[2])
        hist = _play(mgr, 14, rng)
        out.append((mgr.get_transitions(*hist), mgr.assemble_transitions(*hist)))
    return out


def _full_buffer(rollouts, capacity=64):
    from gnn_hex_amd.replay import GraphReplayBuffer
    buf = GraphReplayBuffer(capacity, 5, prioritized=True, alpha=0.5)
    buf.put(rollouts[0][0][0])
    buf.put_block(rollouts[1][1][0])
    assert len(buf) == capacity, "the two rollouts no longer fill the ring"
    return buf


# ---- 1. offsets ------------------------------------------------------------------------------------------------------------

def test_size_mirror_and_offsets_equal_numpy_cumsums(rollouts):
    buf = _full_buffer(rollouts)
    C = buf.capacity
    mirror = buf.sizes_dev.cpu().numpy()
    assert np.array_equal(mirror[:, 0], buf.n_nodes) and np.array_equal(mirror[:, 1], buf.n_edges)
    assert buf.n_nodes.min() >= 3 and len(set(buf.n_nodes.tolist())) > 3, "graphs of several sizes"
    rng = np.random.default_rng(0)
    for k in (1, 2, 63, 64, 65, 257, 1024, 4096):
        slots = rng.integers(0, C, k).astype(np.int32)
        slots[0] = 0                                        # slot 0 ...
        slots[-1] = C - 1 if k > 1 else 0                   # ... the last slot ...
        if k > 4:
            slots[3] = slots[1]                             # ... and a duplicate
        sd = torch.from_numpy(slots).cuda()
        for shift in (0, C):
            node_off = torch.full((k + 1,), -1, dtype=torch.int32, device="cuda")
            edge_off = torch.full((k + 1,), -1, dtype=torch.int32, device="cuda")
            ptr = torch.full((k + 1,), -1, dtype=torch.int64, device="cuda")
            buf.draw_offsets(sd, shift, node_off, edge_off, ptr)
            want_n = np.concatenate([[0], np.cumsum(buf.n_nodes[slots.astype(np.int64) + shift])])
            want_e = np.concatenate([[0], np.cumsum(buf.n_edges[slots.astype(np.int64) + shift])])
            assert np.array_equal(node_off.cpu().numpy(), want_n), (k, shift)
            assert np.array_equal(edge_off.cpu().numpy(), want_e), (k, shift)
            assert np.array_equal(ptr.cpu().numpy(), want_n) and ptr.dtype == torch.int64, (k, shift)
    # the list (1-slot) form: slot 0 alone and the last slot alone
    for slot in (0, C - 1):
        sd = torch.tensor([slot], dtype=torch.int32, device="cuda")
        node_off = torch.zeros(2, dtype=torch.int32, device="cuda")
        edge_off = torch.zeros(2, dtype=torch.int32, device="cuda")
        buf.draw_offsets(sd, C, node_off, edge_off, None)
        assert node_off.tolist() == [0, int(buf.n_nodes[C + slot])] and edge_off.tolist() == [0, int(buf.n_edges[C + slot])]


# ---- 2. the draw -----------------------------------------------------------------------------------------------------------

SENTINEL = -7


def _poison(bufs):
    for half in (bufs.state, bufs.next):
        half.x.fill_(float("nan"))
        half.gs.invdeg.fill_(float("nan"))
        for t in (half.gs.rowptr, half.gs.col, half.batch_vec, half.backmap, half.edge_global, half.edge_local):
            t.fill_(SENTINEL)


@pytest.mark.parametrize("fill", ["full", "partial"])
@pytest.mark.parametrize("static", [True, False], ids=["static-buffers", "fresh-buffers"])
def test_sample_device_equals_sample_and_leaves_the_tail_alone(rollouts, fill, static):
    from gnn_hex_amd.replay import GraphReplayBuffer
    if fill == "full":
        buf = _full_buffer(rollouts)
    else:
        buf = GraphReplayBuffer(64, 5, prioritized=True, alpha=0.5)
        buf.put(rollouts[1][0][0][:31])
        buf.put(rollouts[0][0][0][:9])
        assert 0 < len(buf) < 64
    n_fill = len(buf)
    buf.update_priorities(torch.arange(8, device="cuda"), torch.linspace(0.5, 9.0, 8, device="cuda"))
    k, nv = 16, buf.nv
    g1 = torch.Generator(device="cuda").manual_seed(5)
    g2 = torch.Generator(device="cuda").manual_seed(5)
    want = buf.sample(k, beta=0.6, generator=g1)
    out = None
    if static:
        out = buf.draw_buffers(k)
        _poison(out)
    got = buf.sample_device(k, beta=0.6, generator=g2, out=out)
    torch.cuda.synchronize()
    assert torch.equal(got[0], want[0]) and got[0].dtype == torch.long and int(got[0].max()) < n_fill
    assert torch.equal(got[1], want[1]) and not torch.all(got[1] == 1.0)
    for j in (4, 5, 6):
        assert torch.equal(got[j], want[j]) and got[j].dtype == want[j].dtype, j
    e_cap = buf.edge_capacity()
    for g, w in ((got[2], want[2]), (got[3], want[3])):
        N, E = int(w.ptr[-1]), int(w.edge_index.shape[1])
        gs, ws = g.edge_index._hex_csr, w.edge_index._hex_csr
        assert tuple(g.x.shape) == (k * nv, 3) and tuple(g.edge_index.shape) == (2, k * e_cap) and gs.n == k * nv
        assert 0 < N < k * nv, "this draw should leave a tail behind the live rows"
        assert torch.equal(g.ptr, w.ptr) and g.ptr.dtype == torch.int64 and g.num_graphs == k
        assert torch.equal(g.x[:N], w.x) and torch.equal(g.batch[:N], w.batch)
        assert torch.equal(g.edge_index[:, :E], w.edge_index)
        assert torch.equal(gs.rowptr[:N + 1], ws.rowptr) and torch.equal(gs.col[:E], ws.col) and torch.equal(gs.invdeg[:N], ws.invdeg)
        live = g.x._hex_live_rows
        assert live.dtype == torch.int32 and live.numel() == 1 and live.is_cuda and int(live) == N
        assert g.x._hex_is_maker == w.x._hex_is_maker and g.x._hex_max_nodes == nv
        if static:      # nothing behind the live rows / edges was written
            assert torch.isnan(g.x[N:]).all() and torch.isnan(gs.invdeg[N:]).all()
            assert (gs.rowptr[N + 1:] == SENTINEL).all() and (gs.col[E:] == SENTINEL).all()
            assert (g.batch[N:] == SENTINEL).all() and (g.edge_index[:, E:] == SENTINEL).all()
    if static:          # a second draw into the same storage: the same tensors again, new contents
        again = buf.sample_device(k, beta=0.6, generator=g2, out=out)
        assert again[0].data_ptr() == got[0].data_ptr() and again[2].x.data_ptr() == got[2].x.data_ptr()
        want2 = buf.sample(k, beta=0.6, generator=g1)
        assert torch.equal(again[0], want2[0]) and torch.equal(again[2].x[:int(want2[2].ptr[-1])], want2[2].x)


# ---- 3. the weight gradient bounded by a device-side row count ---------------------------------------------------------

BOARD, NV, LAYERS, HEAD = 7, 51, 3, 2
CAP_GRAPHS = 32                        # the capacity row count of the big cases: 32 Hex-7 boards
_counts, _oracles, _seeds = {}, {}, {}


def _d1_count(size, g, maker):
    """Nodes of the mid-game board ("D1") number g of one size: a graph depends on (size, position in the list) only."""
    if (size, maker) not in _counts:
        ptr = batch_tensors("D1", [size] * CAP_GRAPHS, maker=maker)[3]
        _counts[(size, maker)] = (ptr[1:] - ptr[:-1]).tolist()
    return _counts[(size, maker)][g]


def _sizes_for(total, b, maker):
    """Board sizes of b mid-game graphs with exactly ``total`` nodes (reachable sums, graph by graph)."""
    reach = [{0: None}]
    for g in range(b):
        nxt = {}
        for s, _ in reach[-1].items():
            for size in (7, 6, 5, 4):
                t = s + _d1_count(size, g, maker)
                if t <= total and t not in nxt:
                    nxt[t] = (s, size)
        reach.append(nxt)
    assert total in reach[b], "no %d mid-game boards with %d nodes" % (b, total)
    sizes, s = [], total
    for g in range(b, 0, -1):
        s, size = reach[g][s]
        sizes.append(size)
    return sizes[::-1]


def _case_list():
    cap = CAP_GRAPHS * NV
    S, rps = dw_plan(cap, LAYERS + HEAD - 1)
    assert S >= 4 and rps % 32 == 0, (S, rps)
    m = 3 if 3 * rps + 1 < cap else 2
    return {
        "one-slice-plan": (4 * NV, 4, None),             # capacity below 512 rows: the plan itself has ONE slice
        "below-256": (cap, 10, 200),                      # live rows below 256 in a plan of S slices
        "below-32-per-slice": (cap, 8, 32 * S - 57),     # fewer live rows than slices x 32: trailing slices are empty
        "multiple": (cap, 32, m * rps),                  # exactly a multiple of the capacity plan's rows per slice ...
        "multiple-1": (cap, 32, m * rps - 1),            # ... one below ...
        "multiple+1": (cap, 32, m * rps + 1),            # ... and one above
        "full": (cap, CAP_GRAPHS, cap),                  # live == capacity, all start positions: the exact-size bits
    }


CASES = ("one-slice-plan", "below-256", "below-32-per-slice", "multiple", "multiple-1", "multiple+1", "full")


def _args(hidden):
    return model_args(LAYERS, hidden, HEAD)


def _ref_model(hidden, maker):
    """The sharpened fp32 oracle at the first weight seed whose ReLU inputs stay clear of zero on the start board."""
    from oracle.model_ref import get_pre_defined_ref
    if (hidden, maker) not in _seeds:
        x, ei, batch, ptr = batch_tensors("D0", [BOARD], maker=maker)
        for seed in range(200):
            torch.manual_seed(seed)
            ref = sharpen_(get_pre_defined_ref("modern_two_headed", _args(hidden)))
            ref64 = copy.deepcopy(ref).double()
            if _relu_margin(ref64, maker, lambda: ref64(x.double(), ei, batch, ptr)) >= MARGIN:
                break
        else:
            raise AssertionError("no weight seed below 200 keeps the ReLU inputs clear of zero")
        _seeds[(hidden, maker)] = ref
    return copy.deepcopy(_seeds[(hidden, maker)])


def _ref_run(model, x, ei, batch, ptr, sel, tgt, w):
    model.zero_grad(set_to_none=True)
    q = model(x, ei, batch, ptr)
    d = q[sel] - tgt
    loss = (w * d * d).mean()
    loss.backward()
    return loss.detach(), d.detach(), q.detach(), [None if p.grad is None else p.grad.detach().clone() for p in model.parameters()]


def _oracle(case, hidden, maker):
    key = (case, hidden, maker)
    if key not in _oracles:
        cap, b, total = _case_list()[case]
        if case == "full":
            x, ei, batch, ptr = batch_tensors("D0", [BOARD] * b, maker=maker)
        elif total is None:
            x, ei, batch, ptr = batch_tensors("D1", [BOARD] * b, maker=maker)
        else:
            x, ei, batch, ptr = batch_tensors("D1", _sizes_for(total, b, maker), maker=maker)
            assert int(ptr[-1]) == total
        sel, tgt = sel_and_targets(ptr)
        w = torch.rand(b, generator=torch.Generator().manual_seed(9)) + 0.5
        ref = _ref_model(hidden, maker)
        ref64 = copy.deepcopy(ref).double()
        r64 = _ref_run(ref64, x.double(), ei, batch, ptr, sel, tgt.double(), w.double())
        r32 = _ref_run(ref, x, ei, batch, ptr, sel, tgt, w)
        _oracles[key] = dict(inputs=(x, ei, batch, ptr, sel, tgt, w), state=ref.state_dict(), r64=r64, r32=r32,
                             names=[k for k, _ in ref.named_parameters()], cap=cap)
    return _oracles[key]


@pytest.mark.parametrize("maker", [True, False], ids=["maker", "breaker"])
@pytest.mark.parametrize("hidden", [35, 110])
@pytest.mark.parametrize("case", CASES)
def test_td_step_over_capacity_sized_buffers(case, hidden, maker, monkeypatch):
    from gnn_hex_amd import ops
    from gnn_hex_amd.models import get_pre_defined
    o = _oracle(case, hidden, maker)
    x, ei, batch, ptr, sel, tgt, w = o["inputs"]
    cap, N, b = o["cap"], int(ptr[-1]), len(ptr) - 1
    S, rps = dw_plan(cap, LAYERS + HEAD - 1)
    assert N <= cap and (case == "full") == (N == cap)
    if case == "one-slice-plan":
        assert S == 1 and N < 256
    if case == "below-256":
        assert S > 1 and N < 256
    if case == "below-32-per-slice":
        assert N < 32 * S
    if case.startswith("multiple"):
        assert (N - {"multiple": 0, "multiple-1": -1, "multiple+1": 1}[case]) % rps == 0 and S > 1
    assert ops.qnet_fused_supported(2, hidden, NV)

    hip = get_pre_defined("modern_two_headed", _args(hidden))
    hip.load_state_dict(o["state"])
    hip = hip.cuda()
    dev = torch.device("cuda")
    # the exact-size batch and the same batch inside capacity-sized buffers: one CSR, built once
    gs0 = ops.GraphStructure(ei.cuda(), N)
    E = gs0.e
    rowptr, col, invdeg = gs0.rowptr.clone(), gs0.col.clone(), gs0.invdeg.clone()
    assert torch.equal(gs0.rowptr_t, rowptr) and torch.equal(gs0.col_t[:E], col[:E]), "board graphs are their own transpose"
    e_cap = max(E, 1) + 64
    ptrd, seld, tgtd, wd = ptr.cuda(), sel.cuda(), tgt.cuda(), w.cuda()

    def exact():
        xd = x.cuda()
        ops.attach_hints(xd, maker, NV)
        eid = ei.cuda()
        eid._hex_csr = ops.GraphStructure.from_csr(N, E, rowptr, col, invdeg)
        return xd, eid

    def capacity():
        xc = torch.full((cap, 3), float("nan"), device=dev)
        xc[:N] = x.cuda()
        rp = torch.full((cap + 1,), E, dtype=torch.int32, device=dev)          # (in-range garbage behind the live rows)
        rp[:N + 1] = rowptr
        cc = torch.zeros(e_cap, dtype=torch.int32, device=dev)
        cc[:E] = col[:E]
        iv = torch.full((cap,), float("nan"), device=dev)
        iv[:N] = invdeg
        eic = torch.zeros((2, e_cap), dtype=torch.long, device=dev)
        eic[:, :E] = ei.cuda()
        ops.attach_hints(xc, maker, NV)
        xc._hex_live_rows = torch.tensor([N], dtype=torch.int32, device=dev)
        eic._hex_csr = ops.GraphStructure.from_csr(cap, e_cap, rp, cc, iv)
        return xc, eic

    def step(xd, eid, byte):
        stand_in = PoisonedTorch(byte)
        hip.zero_grad(set_to_none=True)
        with monkeypatch.context() as mp:
            mp.setattr(ops, "torch", stand_in)
            loss, td, q = ops.td_step(hip, xd, eid, None, ptrd, sel=seld, target=tgtd, weights=wd)
            torch.cuda.synchronize()
        assert stand_in.filled >= 2, "the scratch did not come through ops' torch.empty"
        assert q._hex_call.td is not None, "the fused form did not run"
        return (loss.clone(), td.clone(), q.detach()[:N].clone(),
                [None if p.grad is None else p.grad.detach().clone() for p in hip.parameters()], q._hex_call)

    le, tde, qe, ge, call_e = step(*exact(), 0xFF)
    assert call_e.live is None
    l1, td1, q1, g1, call_1 = step(*capacity(), 0xFF)
    l2, td2, q2, g2, _ = step(*capacity(), 0x3F)
    assert call_1.live is not None and call_1.dims[0] == cap and call_e.dims[0] == N
    # the per-graph kernels run the same work: the same bits
    assert torch.equal(l1, le) and torch.equal(td1, tde) and torch.equal(q1, qe)
    assert torch.isfinite(l1).all() and torch.isfinite(td1).all() and torch.isfinite(q1).all()
    # nothing depends on what the scratch or the rows behind the live count held
    assert torch.equal(l2, l1) and torch.equal(td2, td1) and torch.equal(q2, q1)
    for name, a, c in zip(o["names"], g1, g2):
        assert (a is None) == (c is None) and (a is None or torch.equal(a, c)), "%s depends on the poison" % name
    # the float64 rule, for the capacity-sized call and (the same yardstick) the exact-size one
    l64, d64, q64, g64 = o["r64"]
    l32, d32, q32, g32 = o["r32"]
    names = o["names"]
    assert names[0].endswith("convs.0.lin_l.weight") and names[2].endswith("convs.0.lin_r.weight")
    tag = "%s h%d %s" % (case, hidden, "maker" if maker else "breaker")
    worst, worst_col = check_grads(tag, names, g1, g32, g64, 2)
    check_grads(tag + " exact-size", names, ge, g32, g64, 2)
    print("%s: N %d of %d rows, %d graphs, plan %d x %d; worst tensor %s rel %.3g (oracle32 %.3g), worst layer-0 column %s rel "
          "%.3g (oracle32 %.3g)" % (tag, N, cap, b, S, rps, worst[2], worst[0], worst[1], worst_col[2], worst_col[0], worst_col[1]))
    assert abs(l1.item() - l64.item()) <= max(3 * abs(l32.item() - l64.item()), 1e-5 * max(1.0, abs(l64.item())))
    if case == "full":          # the device-side plan is the host's plan: the exact-size call's bits
        for name, a, c in zip(names, g1, ge):
            assert (a is None) == (c is None) and (a is None or torch.equal(a, c)), "%s differs from the exact-size call" % name


# ---- 4. the update as one object ---------------------------------------------------------------------------------------------

def _update_setup(rollouts, graph):
    from gnn_hex_amd.models import get_pre_defined
    from gnn_hex_amd.replay import GraphReplayBuffer, GraphedUpdate
    torch.manual_seed(1)
    online = get_pre_defined("modern_two_headed", model_args(3, 35)).cuda()
    target = copy.deepcopy(online)
    with torch.no_grad():
        for p in target.parameters():
            p.mul_(0.9)                          # a target that differs from the online net until the sync
    buf = GraphReplayBuffer(256, 5, prioritized=True, alpha=0.5)
    buf.put_block(rollouts[0][1][0])
    assert 32 <= len(buf) < 256
    opt = torch.optim.Adam(online.parameters(), lr=1e-3, fused=True, capturable=True)
    upd = GraphedUpdate(buf, online, target, opt, 32, 0.97 ** 2, loss_fn="mse", graph=graph)
    return upd, buf, online, target


def _run_updates(rollouts, graph):
    upd, buf, online, target = _update_setup(rollouts, graph)
    before = [p.detach().clone() for p in online.parameters()]
    torch.manual_seed(7)
    snaps, losses = [], []
    for step in range(6):
        loss, td = upd.step(beta=0.4 + 0.1 * step)
        torch.cuda.synchronize()
        assert td.shape == (32,) and torch.isfinite(td).all()
        losses.append(float(loss))
        snaps.append(([p.detach().clone() for p in online.parameters()], buf.sum_tree.clone(), buf.min_tree.clone(),
                      buf.max_priority.clone()))
        if step == 2:                            # after step 3: the target takes the online weights, in place
            target.load_state_dict(online.state_dict())
        if step == 3:                            # after step 4: new transitions, the fill level changes
            size = len(buf)
            buf.put_block(rollouts[1][1][0])
            assert len(buf) > size
    return upd, before, snaps, losses


def test_graphed_update_equals_the_eager_sequence_step_by_step(rollouts):
    upd_e, before_e, snaps_e, losses_e = _run_updates(rollouts, graph=False)
    upd_g, before_g, snaps_g, losses_g = _run_updates(rollouts, graph=True)
    assert upd_g._graph is not None and upd_g._opt_inside and upd_e._graph is None
    for a, c in zip(before_e, before_g):
        assert torch.equal(a, c), "building the captured update changed the parameters"
    for step, (se, sg) in enumerate(zip(snaps_e, snaps_g)):
        for i, (a, c) in enumerate(zip(se[0], sg[0])):
            assert torch.equal(a, c), "step %d: parameter %d differs" % (step + 1, i)
        assert torch.equal(se[1], sg[1]) and torch.equal(se[2], sg[2]), "step %d: priority trees differ" % (step + 1)
        assert torch.equal(se[3], sg[3]), "step %d: max_priority differs" % (step + 1)
    assert losses_e == losses_g
    assert all(np.isfinite(v) for v in losses_g) and len(set(losses_g)) == len(losses_g), losses_g
    moved = [not torch.equal(a, c) for a, c in zip(before_g, snaps_g[-1][0])]
    assert sum(moved) >= len(moved) // 2, "the optimizer did not move the weights"      # (one head never sees a gradient)
    assert not torch.equal(snaps_g[0][1], snaps_g[-1][1])


def test_graphed_update_with_an_optimizer_that_is_not_capturable(rollouts):
    """An optimizer that cannot be captured is issued right after the replay: the same numbers as the eager sequence -- also
    across a rebuild of the draw buffers (what ``step`` does when a stored graph has more edges than they hold)."""
    from gnn_hex_amd.models import get_pre_defined
    from gnn_hex_amd.replay import GraphReplayBuffer, GraphedUpdate
    results = []
    for graph in (False, True):
        torch.manual_seed(1)
        online = get_pre_defined("modern_two_headed", model_args(3, 35)).cuda()
        target = copy.deepcopy(online)
        buf = GraphReplayBuffer(256, 5, prioritized=True, alpha=0.5)
        buf.put_block(rollouts[0][1][0])
        opt = torch.optim.SGD(online.parameters(), lr=1e-2)
        upd = GraphedUpdate(buf, online, target, opt, 32, 0.97 ** 2, graph=graph)
        assert not upd._opt_inside
        torch.manual_seed(11)
        for i in range(3):
            if i == 2:                           # as if a stored graph had outgrown the static buffers: new ones, a new capture
                old = upd.bufs
                upd.bufs.e_cap = 0
            loss, _ = upd.step(0.5)
        assert upd.bufs is not old and upd.bufs.e_cap == buf.edge_capacity() and (upd._graph is not None) == graph
        torch.cuda.synchronize()
        results.append(([p.detach().clone() for p in online.parameters()], buf.sum_tree.clone(), float(loss)))
    for a, c in zip(results[0][0], results[1][0]):
        assert torch.equal(a, c)
    assert torch.equal(results[0][1], results[1][1]) and results[0][2] == results[1][2]


# ---- 5. refusals -------------------------------------------------------------------------------------------------------------

def test_refusals_name_their_reason(rollouts):
    from gnn_hex_amd import ops
    from gnn_hex_amd.models import get_pre_defined
    from gnn_hex_amd.replay import GraphReplayBuffer, GraphedUpdate
    big = GraphReplayBuffer(8, 12, prioritized=True)
    with pytest.raises(NotImplementedError, match="128 nodes"):
        big.sample_device(4)
    buf = GraphReplayBuffer(256, 5, prioritized=True, alpha=0.5)
    with pytest.raises(ValueError, match="empty"):
        buf.sample_device(4)
    buf.put_block(rollouts[0][1][0])

    def build(model_name, **changes):
        args = model_args(3, changes.pop("hidden", 35))
        for k, v in changes.items():
            setattr(args, k, v)
        m = get_pre_defined(model_name, args).cuda()
        opt = torch.optim.SGD(m.parameters(), lr=1e-2)
        return GraphedUpdate(buf, m, copy.deepcopy(m), opt, 8, 0.9, graph=False)

    for kw in (dict(norm=True), dict(noisy_dqn=True), dict(hidden=128)):
        with pytest.raises(NotImplementedError, match="fused per-graph kernels"):
            build("modern_two_headed", **kw)
    with pytest.raises(NotImplementedError, match="fused per-graph kernels"):
        build("two_headed", norm=False)
    ops.set_math("f16x3")
    try:
        with pytest.raises(NotImplementedError, match="f16x3"):
            build("modern_two_headed")
        x = torch.zeros((27, 3), device="cuda")
        x._hex_live_rows = torch.tensor([27], dtype=torch.int32, device="cuda")
        with pytest.raises(NotImplementedError, match="f16x3"):
            ops.td_step(None, x, None, sel=torch.zeros(1, dtype=torch.long, device="cuda"),
                        target=torch.zeros(1, device="cuda"))
    finally:
        ops.set_math("fp32")
    ok = build("modern_two_headed")                       # the supported configuration is accepted ...
    buf.put_block(rollouts[0][1][1])                      # ... until the buffer holds both sides
    with pytest.raises(ValueError, match="both sides"):
        buf.sample_device(8)
    with pytest.raises(ValueError, match="both sides"):
        ok.step()
    with pytest.raises(ValueError, match="both sides"):
        build("modern_two_headed")
