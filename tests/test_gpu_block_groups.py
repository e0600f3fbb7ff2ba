"""The one-launch SAGE stack kernels on batches with more row blocks than can be resident at once: the table's blocks run in
groups of whole graphs, one launch per group and direction (hexgnn_sage_stack_call.group_starts, data.block_groups / pack_groups).

The budget is driven down with hexgnn_stack_reserve_cus so that small batches need groups: the 63-graph Hex-5..13 list has 63
blocks in the caller's order and runs as three groups under a budget of 24.  A block's arithmetic depends on the table only,
not on which launch ran it: grouped results equal those of ONE launch over the same table bit for bit."""
import contextlib
import ctypes
import time

import pytest
import torch

from helpers import make_pair, sel_and_targets
from test_gpu_stack_blocks import _close, _data_list

pytestmark = pytest.mark.gpu

MIX63 = [5 + (g % 9) for g in range(63)]          # board sizes; Hex-k has k * k + 2 nodes
K_SAGE_FWD, K_SAGE_BWD = 0, 1                     # HEXGNN_K_SAGE_FWD / _BWD


@contextlib.contextmanager
def _budget(blocks=None):
    """The resident-workgroup budget reduced to ``blocks`` (None: the device's own); reserve and stack mode restored."""
    from gnn_hex_amd import _lib, ops
    L = _lib.lib()
    prev = L.hexgnn_stack_reserve_cus(0)
    try:
        budget0 = ops.stack_block_budget(torch.device("cuda"))
        if blocks is not None:
            assert budget0 >= blocks
            L.hexgnn_stack_reserve_cus(budget0 - blocks)
            assert ops.stack_block_budget(torch.device("cuda")) == blocks
        yield L, budget0
    finally:
        L.hexgnn_stack_reserve_cus(prev)
        L.hexgnn_debug_stack_mode(-1, 0)
        L.hexgnn_profile_enable(-1)


def _step(model, bt, sel, tgt):
    """One training step: (Q, every gradient, final_conv_grads -- the backward's tap output)."""
    model.zero_grad(set_to_none=True)
    q = model(bt.x, bt.edge_index, bt.batch, bt.ptr)
    torch.nn.functional.mse_loss(torch.as_tensor(q).reshape(-1)[sel], tgt).backward()
    torch.cuda.synchronize()
    return (torch.as_tensor(q).detach().clone(), [p.grad.detach().clone() for p in model.parameters() if p.grad is not None],
            model.final_conv_grads.detach().clone())


def _same_bits(a, b):
    return torch.equal(a[0], b[0]) and len(a[1]) == len(b[1]) and all(torch.equal(x, y) for x, y in zip(a[1], b[1])) \
        and torch.equal(a[2], b[2])


def _near(a, b):
    """The bounds tests/test_gpu_stack_blocks.py uses between launch forms: 3e-5 on Q, 1e-4 on gradients, scale-relative."""
    return _close(a[0], b[0]) and len(a[1]) == len(b[1]) and all(_close(x, y, 1e-4) for x, y in zip(a[1], b[1]))


def _launches(L, cls, fn):
    cnt, tot = ctypes.c_int(0), ctypes.c_float(0)
    L.hexgnn_profile_enable(cls)
    try:
        fn()
        torch.cuda.synchronize()
        assert L.hexgnn_profile_read(ctypes.byref(cnt), ctypes.byref(tot)) == 0
    finally:
        L.hexgnn_profile_enable(-1)
    return cnt.value


def _grouped_batch(dl, pack, budget):
    from gnn_hex_amd.data import Batch
    bt = Batch.from_data_list(dl, pack=pack, groups=True)
    assert getattr(bt.edge_index, "_hex_blocks", None) is None          # over the budget: no plain table
    tbl, nb, groups = bt.edge_index._hex_block_groups
    assert nb == tbl.numel() - 1 and groups[0] == 0 and groups[-1] == nb
    assert all(0 < b - a <= budget for a, b in zip(groups, groups[1:]))
    return bt, tbl.cpu().tolist(), list(groups)


@pytest.mark.parametrize("pack", [False, True], ids=["callers-order", "packed"])
def test_groups_equal_one_launch_over_the_same_table(pack):
    """5 + 2 layers: six hidden-input layers per direction, so three launches are neither one nor one per layer.  Covers the
    tap output (final_conv_grads) and the per-layer launches, and blocks delayed unevenly (seeds 11..13)."""
    from gnn_hex_amd.data import attach_blocks
    hip, _ = make_pair(5, 110, seed=3)
    dl = _data_list(MIX63)
    with _budget(24) as (L, budget0):
        assert budget0 >= 63
        bt, starts, groups = _grouped_batch(dl, pack, 24)
        assert groups == ([0, 24, 46] if pack else [0, 23, 47, 63])
        if pack:
            assert sorted(bt.order.tolist()) == list(range(63))
        sel, tgt = sel_and_targets(bt.ptr.cpu(), seed=5)
        sel, tgt = sel.cuda(), tgt.cuda()
        got = _step(hip, bt, sel, tgt)
        assert hip._fca.gs.groups is not None and hip._fca.gs.blocks is None
        assert torch.isfinite(got[0]).all()
        assert _launches(L, K_SAGE_FWD, lambda: _step(hip, bt, sel, tgt)) == len(groups) - 1
        assert _launches(L, K_SAGE_BWD, lambda: _step(hip, bt, sel, tgt)) == len(groups) - 1
        for seed in (11, 12, 13):
            L.hexgnn_debug_stack_mode(-1, seed)
            assert _same_bits(_step(hip, bt, sel, tgt), got), seed
        L.hexgnn_debug_stack_mode(0, 0)                                 # per-layer launches: the groups are ignored
        layerwise = _step(hip, bt, sel, tgt)
        assert _launches(L, K_SAGE_FWD, lambda: _step(hip, bt, sel, tgt)) == 6
        L.hexgnn_debug_stack_mode(-1, 0)
        assert _near(got, layerwise)
        # the same table as ONE launch, with the reserve lifted
        L.hexgnn_stack_reserve_cus(0)
        del bt.edge_index._hex_block_groups
        attach_blocks(bt.edge_index, starts)
        one = _step(hip, bt, sel, tgt)
        assert hip._fca.gs.groups is None and hip._fca.gs.blocks[1] == len(starts) - 1
        assert _launches(L, K_SAGE_FWD, lambda: _step(hip, bt, sel, tgt)) == 1
        assert _same_bits(got, one)
        assert L.hexgnn_stack_status(1) == 0


def test_groups_are_opt_in_and_only_for_batches_that_would_run_per_layer():
    """where the default 128-row blocks fit the budget, one launch over them is faster than two over aligned
    blocks, so such a batch never gets groups; and nothing changes for a caller who does not ask."""
    from gnn_hex_amd.data import Batch
    from gnn_hex_amd.replay import GraphReplayBuffer
    dl = _data_list([13] * 24)                    # 4104 rows: 33 default blocks, 48 aligned ones
    with _budget(16):
        for pack in (False, True):
            bt = Batch.from_data_list(dl, pack=pack)
            assert not hasattr(bt.edge_index, "_hex_blocks") and not hasattr(bt.edge_index, "_hex_block_groups")
    with _budget(40):                             # the default blocks fit, the aligned ones do not
        for pack in (False, True):
            bt = Batch.from_data_list(dl, pack=pack, groups=True)
            assert not hasattr(bt.edge_index, "_hex_block_groups")
    assert GraphReplayBuffer(16, 13, prioritized=False).group_blocks is False


def test_large_boards_in_groups_against_the_oracle():
    """Hex-13 alone, 48 blocks under a budget of 16, against the CPU oracle with the comparison of tests/test_gpu_fullsize.py."""
    from gnn_hex_amd.data import Batch
    TOL = 1e-4
    hip, ref = make_pair(4, 110, seed=4)
    dl = _data_list([13] * 24)
    with _budget(16) as (L, _):
        bt, starts, groups = _grouped_batch(dl, False, 16)
        assert len(starts) - 1 == 48 and groups == [0, 16, 32, 48]
        sel, tgt = sel_and_targets(bt.ptr.cpu(), seed=2)
        q, _, _ = _step(hip, bt, sel.cuda(), tgt.cuda())
        assert L.hexgnn_stack_status(1) == 0
        grads = {k: p.grad.detach().clone() for k, p in hip.named_parameters() if p.grad is not None}
        assert _launches(L, K_SAGE_FWD, lambda: _step(hip, bt, sel.cuda(), tgt.cuda())) == 3
    ref.zero_grad(set_to_none=True)
    q_ref = ref(bt.x.cpu(), bt.edge_index.cpu(), bt.batch.cpu(), bt.ptr.cpu())
    torch.nn.functional.mse_loss(q_ref[sel], tgt).backward()
    err = (q.cpu() - q_ref.detach()).abs().max().item()
    assert err < TOL, "Q max abs err %g" % err
    g_ref = dict(ref.named_parameters())
    for k, p in hip.named_parameters():
        if g_ref[k].grad is None:
            assert k not in grads, k
            continue
        gerr = (grads[k].cpu() - g_ref[k].grad).abs().max().item()
        assert gerr < TOL * max(1.0, g_ref[k].grad.abs().max().item()), "%s grad max abs err %g" % (k, gerr)


class _Conv(torch.nn.Module):
    def __init__(self, cin, cout):
        super().__init__()
        self.lin_l = torch.nn.Linear(cin, cout, bias=True)
        self.lin_r = torch.nn.Linear(cin, cout, bias=False)


def test_two_backwards_over_one_forward():
    """ops.sage_stack (SageStackFn) on a grouped batch; the progress counters are never reset between the launches of a call nor
    between two backwards: every block's word sits at the common value when its group's launch starts."""
    from gnn_hex_amd import ops
    from gnn_hex_amd.data import Batch
    torch.manual_seed(21)
    dl = _data_list(MIX63)
    convs = torch.nn.ModuleList([_Conv(3 if i == 0 else 110, 110) for i in range(5)]).cuda()
    with torch.no_grad():
        for c in convs[1:]:
            c.lin_r.weight.mul_(2.0)
    with _budget(16) as (L, _):                   # groups of different sizes: 16, 16, 16, 15
        bt, starts, groups = _grouped_batch(dl, False, 16)
        assert groups == [0, 16, 32, 48, 63]
        n = int(bt.x.shape[0])
        up = torch.randn(n, 110, device="cuda")
        gs = ops.GraphStructure(bt.edge_index, n)
        assert gs.groups is not None and gs.groups[2] == tuple(groups)
        y = ops.sage_stack(bt.x, gs, 3, 110, convs)
        loss = (y * up).sum()
        assert _launches(L, K_SAGE_BWD, lambda: loss.backward(retain_graph=True)) == 4
        g1 = [p.grad.clone() for p in convs.parameters()]
        for p in convs.parameters():
            p.grad = None
        loss.backward()
        torch.cuda.synchronize()
        g2 = [p.grad.clone() for p in convs.parameters()]
        assert all(torch.isfinite(g).all() and g.abs().max() > 0 for g in g1)
        assert all(torch.equal(a, b) for a, b in zip(g1, g2))
        # and the per-layer launches agree
        L.hexgnn_debug_stack_mode(0, 0)
        for p in convs.parameters():
            p.grad = None
        y0 = ops.sage_stack(bt.x, gs, 3, 110, convs)
        (y0 * up).sum().backward()
        torch.cuda.synchronize()
        assert _close(y.detach(), y0.detach())
        assert all(_close(a, p.grad, 1e-4) for a, p in zip(g1, convs.parameters()))
        assert L.hexgnn_stack_status(1) == 0


def test_a_cut_that_an_edge_crosses_is_an_error_not_a_wait():
    from gnn_hex_amd.data import Batch, attach_block_groups, blocks_for_order
    hip, _ = make_pair(3, 110, seed=5)
    dl = _data_list([13] * 24)
    with _budget(16) as (L, _):
        good = Batch.from_data_list(dl, groups=True)
        with torch.no_grad():
            hip(good.x, good.edge_index, good.batch, good.ptr)          # (first-call costs stay out of the timed call)
        torch.cuda.synchronize()
        assert L.hexgnn_stack_status(1) == 0
        bad = Batch.from_data_list(dl, groups=True)
        starts = blocks_for_order([171] * 24)
        del bad.edge_index._hex_block_groups
        attach_block_groups(bad.edge_index, starts, [0, 15, 31, 47, 48])      # odd cuts: between the two blocks of a graph
        t0 = time.perf_counter()
        with torch.no_grad():
            q = torch.as_tensor(hip(bad.x, bad.edge_index, bad.batch, bad.ptr))
        torch.cuda.synchronize()
        elapsed = time.perf_counter() - t0
        assert L.hexgnn_stack_status(1) == -1                           # HEXGNN_EINVAL, and the word is cleared
        assert not torch.isfinite(q).all()                              # the cut graphs' rows cannot pass for a result
        assert elapsed < 1.0, "the crossed cut waited: %.2f s" % elapsed
        with torch.no_grad():
            q = torch.as_tensor(hip(good.x, good.edge_index, good.batch, good.ptr))
        torch.cuda.synchronize()
        assert torch.isfinite(q).all() and L.hexgnn_stack_status(1) == 0


def test_uniform_hex13_batch_at_its_natural_size():
    """256 Hex-13 boards, 512 blocks, no reserve: two groups of 256 on a device with 256 CUs."""
    from gnn_hex_amd.data import Batch, block_groups, blocks_for_order
    hip, _ = make_pair(3, 110, seed=6)
    dl = _data_list([13]) * 256
    with _budget(None) as (L, budget0):
        sizes = [171] * 256
        want = block_groups(sizes, blocks_for_order(sizes), budget0)
        if budget0 == 256:
            assert want == [0, 256, 512]
        assert want is not None and len(want) > 2, "a device with %d CUs runs this batch in one launch" % budget0
        bt, starts, groups = _grouped_batch(dl, False, budget0)
        assert len(starts) - 1 == 512 and groups == want
        sel, tgt = sel_and_targets(bt.ptr.cpu(), seed=3)
        sel, tgt = sel.cuda(), tgt.cuda()
        got = _step(hip, bt, sel, tgt)
        assert _launches(L, K_SAGE_FWD, lambda: _step(hip, bt, sel, tgt)) == len(want) - 1
        L.hexgnn_debug_stack_mode(0, 0)
        layerwise = _step(hip, bt, sel, tgt)
        assert _near(got, layerwise) and torch.isfinite(got[0]).all()
        assert L.hexgnn_stack_status(1) == 0


def test_grouped_step_captured_and_replayed():
    from gnn_hex_amd.graphs import GraphedStep
    hip, _ = make_pair(4, 110, seed=7)
    params = list(hip.parameters())
    dl = _data_list([13] * 24)
    with _budget(16) as (L, _):
        bt, _, groups = _grouped_batch(dl, True, 16)
        assert len(groups) == 4
        sel, tgt = sel_and_targets(bt.ptr.cpu(), seed=4)
        sel, tgt = sel.cuda(), tgt.cuda()

        def fn():
            for p in params:
                p.grad = None
            q = hip(bt.x, bt.edge_index, bt.batch, bt.ptr)
            loss = torch.nn.functional.mse_loss(torch.as_tensor(q).reshape(-1)[sel], tgt)
            loss.backward()
            return loss

        loss_e = fn().detach().clone()
        torch.cuda.synchronize()
        grads_e = [None if p.grad is None else p.grad.detach().clone() for p in params]
        g = GraphedStep(fn, params)
        for _ in range(2):
            loss = g.replay()
            torch.cuda.synchronize()
            assert torch.equal(loss, loss_e)
            for p, ge in zip(params, grads_e):
                assert (p.grad is None) if ge is None else torch.equal(p.grad, ge)
        assert L.hexgnn_stack_status(1) == 0


def test_replay_draws_over_the_budget_carry_groups():
    """GraphReplayBuffer on Hex-13 under a budget of 16: a draw of 48 comes packed, with the table in groups on both batches,
    aligned with its indices; Q equals that of the same transitions collated without tables (per-layer launches)."""
    import numpy as np
    from gnn_hex_amd.data import Batch
    from gnn_hex_amd.multi_env_manager import Env_manager
    from gnn_hex_amd.replay import GraphReplayBuffer
    from test_gpu_replay import _play
    rng = np.random.default_rng(7)
    mgr = Env_manager(6, 13, gamma=0.97, n_steps=[1])
    obs0, states, actions, rewards, dones, expl = _play(mgr, 40, rng)
    maker, _ = mgr.get_transitions(obs0, states, actions, rewards, dones, expl)
    assert len(maker) >= 48
    buf = GraphReplayBuffer(256, 13, prioritized=False, group_blocks=True)
    buf.put(maker)
    hip, _ = make_pair(4, 110, seed=6)
    with _budget(16) as (L, _):
        idx, w, s, s2, a, r, d = buf.sample(48)
        ih = idx.cpu().tolist()
        for bt, col in ((s, 0), (s2, 3)):
            gs = bt.edge_index._hex_csr
            assert gs.blocks is None and gs.groups is not None
            tbl, nb, groups, _ = gs.groups
            starts = tbl.cpu().tolist()
            assert starts[0] == 0 and starts[-1] == int(bt.x.shape[0]) and all(0 < q - p <= 128 for p, q in zip(starts, starts[1:]))
            assert groups[0] == 0 and groups[-1] == nb and all(0 < q - p <= 16 for p, q in zip(groups, groups[1:]))
            rows = set(bt.ptr.cpu().tolist())
            assert all(starts[g] in rows for g in groups)               # every cut is a graph start
            ref = Batch.from_data_list([maker[i][col] for i in ih])
            assert torch.equal(bt.x, ref.x) and torch.equal(bt.edge_index, ref.edge_index) and torch.equal(bt.ptr, ref.ptr)
        assert a.cpu().tolist() == [int(maker[i][1]) for i in ih]
        assert np.allclose(r.cpu().numpy(), [maker[i][2] for i in ih])
        with torch.no_grad():
            q1 = torch.as_tensor(hip(s.x, s.edge_index, s.batch, s.ptr)).clone()
            assert hip._fca.gs.groups is not None
            ref = Batch.from_data_list([maker[i][0] for i in ih])
            assert not hasattr(ref.edge_index, "_hex_block_groups")    # no table: one launch per layer
            q0 = torch.as_tensor(hip(ref.x, ref.edge_index, ref.batch, ref.ptr))
            assert hip._fca.gs.groups is None and hip._fca.gs.blocks is None
        torch.cuda.synchronize()
        assert _close(q1, q0) and torch.isfinite(q1).all() and L.hexgnn_stack_status(1) == 0
