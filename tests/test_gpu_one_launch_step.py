"""ops.td_step as ONE launch for the forward, the TD loss and the backward's data chain (hexgnn_qnet_step_td).

Every case runs the same update twice in one process, ``ops.set_one_launch_step(True)`` against ``(False)`` (the two launches
hexgnn_qnet_forward_td / hexgnn_qnet_backward_flat_td), and asks for the same bits in loss, td, Q and every parameter gradient and
for the same status word.  No case uses a workload shape: the batches hold 1, 3 and 9 boards of Hex-2 .. Hex-11 (6 to 123 rows:
graphs of at most 64 rows, whose waves 4-7 own no rows, graphs of 65 to 128 rows, pad rows in the last tile)."""
import copy

import pytest
import torch

from helpers import batch_tensors, model_args, sel_and_targets

pytestmark = pytest.mark.gpu

# hidden widths: one tile, two tiles (the drain path), three landing buffers, the first width with aliased scratch, NT = 7
WIDTHS = [8, 24, 35, 64, 110]
# (body, head) layers: the smallest the family allows, and 3 + 2
DEPTHS = [(1, 1), (3, 2)]
BATCHES = {1: [8], 3: [2, 11, 5], 9: [2, 3, 5, 7, 8, 11, 3, 7, 2]}
LOSSES = [("mse", False), ("mse", True), ("huber", False), ("huber", True)]


def _pair(body, head, hidden, seed=3):
    from gnn_hex_amd.models import get_pre_defined
    from oracle.model_ref import get_pre_defined_ref
    torch.manual_seed(seed)
    ref = get_pre_defined_ref("modern_two_headed", model_args(body, hidden, head_layers=head))
    hip = get_pre_defined("modern_two_headed", model_args(body, hidden, head_layers=head))
    hip.load_state_dict(ref.state_dict())
    return hip.cuda(), ref


def _dev(*ts):
    return tuple(None if t is None else t.cuda() for t in ts)


def _step(hip, on, batch, sel, tgt, w=None, loss_fn="mse", expect_one_launch=None, **kw):
    """One td_step with the switch at ``on``: everything the comparison looks at, cloned (the gradients are views of a buffer the
    next step writes again), and the status word, which is read and cleared."""
    from gnn_hex_amd import ops
    prev = ops._ONE_LAUNCH_STEP
    ops.set_one_launch_step(on)
    try:
        hip.zero_grad(set_to_none=True)
        out = ops.td_step(hip, *batch, sel=sel, target=tgt, weights=w, loss_fn=loss_fn, **kw)
        if kw.get("defer_lower"):
            ops.finish_backward(out[3])
        torch.cuda.synchronize()
    finally:
        ops.set_one_launch_step(prev)
    call = getattr(out[2], "_hex_call", None)
    status = None
    if call is not None:
        status = int(call.gs.status.item())
        call.gs.status.zero_()
    if expect_one_launch is not None:
        assert call is not None and call.td is not None, "the fused form did not run"
        # (True: the one launch ran AND the backward took its data chain instead of running the chain again)
        assert (call.step_ws is True) == (expect_one_launch and on) and call.step_ws in (None, True), "the step took the other entry"
    fcg = getattr(hip, "final_conv_grads", None)          # the gradient of the body's output, handed to the model's hook
    return dict(loss=out[0].detach().clone(), td=out[1].detach().clone(), q=out[2].detach().clone(), status=status,
                fcg=None if fcg is None else fcg.detach().clone(),
                grads={k: p.grad.detach().clone() for k, p in hip.named_parameters() if p.grad is not None})


def _bits(t):
    return t.contiguous().reshape(-1).view(torch.int32)


def _same(tag, a, b):
    """The same bits (NaNs included: both forms poison with the same constant) and the same status word."""
    for k in ("loss", "td", "q"):
        assert a[k].shape == b[k].shape and torch.equal(_bits(a[k]), _bits(b[k])), "%s: %s differs" % (tag, k)
    assert a["status"] == b["status"], "%s: status %s against %s" % (tag, a["status"], b["status"])
    if "fcg" in a and "fcg" in b:
        assert (a["fcg"] is None) == (b["fcg"] is None), tag
        assert a["fcg"] is None or torch.equal(_bits(a["fcg"]), _bits(b["fcg"])), "%s: final_conv_grads differ" % tag
    assert a["grads"].keys() == b["grads"].keys() and len(a["grads"]) > 0, tag
    for k in a["grads"]:
        assert torch.equal(_bits(a["grads"][k]), _bits(b["grads"][k])), "%s: gradient %s differs" % (tag, k)


@pytest.mark.parametrize("body,head", DEPTHS, ids=["1+1", "3+2"])
@pytest.mark.parametrize("hidden", WIDTHS)
def test_one_launch_has_the_bits_of_two(hidden, body, head):
    hip, _ = _pair(body, head, hidden)
    torch.manual_seed(7)
    for b, sizes in BATCHES.items():
        for maker in (True, False):
            x, ei, bv, ptr = batch_tensors("D0", sizes, maker=maker)
            sel, tgt = sel_and_targets(ptr)
            w = torch.rand(b) + 0.5
            batch = _dev(x, ei, bv, ptr)
            seld, tgtd, wd = _dev(sel, tgt, w)
            for loss_fn, weighted in LOSSES:
                one = _step(hip, True, batch, seld, tgtd, wd if weighted else None, loss_fn, expect_one_launch=True)
                two = _step(hip, False, batch, seld, tgtd, wd if weighted else None, loss_fn, expect_one_launch=True)
                assert one["status"] == 0 and torch.isfinite(one["loss"]).item()
                _same("hidden %d, %d+%d layers, %d graphs, maker %s, %s%s"
                      % (hidden, body, head, b, maker, loss_fn, " weighted" if weighted else ""), one, two)


@pytest.mark.parametrize("hidden", [35, 110])
def test_dense_graphs_walk_the_global_csr(hidden):
    """The suite's degree-60 stress graphs (tests/test_gpu_model.py): rows above 16 neighbours and about 5 900 edges per graph;
    directed edges make the transposed CSR differ from the forward's.  Only the 110-wide half walks the global CSR (2848 edges fit
    the LDS arrays at NT = 7); at hidden 35 the arrays take 8192 edges (hexgnn_qnet_csr_capacity) and these graphs stay in LDS -- there
    the case is the long-row gather of the LDS path.  The global-CSR fallback at every tile count:
    tests/test_gpu_fused_instantiations.py."""
    from test_gpu_model import _random_batch
    hip, _ = _pair(3, 2, hidden, seed=23)
    x, ei, bv, ptr = _random_batch([100, 100], seed=7, directed=True, p_edge=0.6)
    assert ei.shape[1] > 2 * 3800 and int(torch.bincount(ei[1]).max()) > 16
    sel, tgt = sel_and_targets(ptr)
    batch = _dev(x, ei, bv, ptr)
    seld, tgtd = _dev(sel, tgt)
    one = _step(hip, True, batch, seld, tgtd, expect_one_launch=True)
    two = _step(hip, False, batch, seld, tgtd, expect_one_launch=True)
    assert one["status"] == 0
    _same("dense graphs, hidden %d" % hidden, one, two)


@pytest.mark.parametrize("maker", [True, False], ids=["maker", "breaker"])
def test_mid_game_boards(maker):
    """Boards from oracle.env_ref.random_position (kind "D1"): dead and captured cells removed, rows of every degree."""
    hip, _ = _pair(3, 2, 110)
    x, ei, bv, ptr = batch_tensors("D1", [11, 7, 8, 5, 11], maker=maker)
    sel, tgt = sel_and_targets(ptr)
    batch = _dev(x, ei, bv, ptr)
    seld, tgtd = _dev(sel, tgt)
    for loss_fn in ("mse", "huber"):
        one = _step(hip, True, batch, seld, tgtd, None, loss_fn, expect_one_launch=True)
        two = _step(hip, False, batch, seld, tgtd, None, loss_fn, expect_one_launch=True)
        assert one["status"] == 0
        _same("mid-game, maker %s, %s" % (maker, loss_fn), one, two)


@pytest.mark.parametrize("hidden", [35, 110])
def test_selection_outside_its_graph_gives_the_same_nans_and_status_16(hidden):
    hip, _ = _pair(3, 2, hidden)
    x, ei, bv, ptr = batch_tensors("D0", [5, 7, 3, 8, 2], maker=True)
    sel, tgt = sel_and_targets(ptr)
    sel = sel.clone()
    sel[2] = sel[3]                      # graph 2's entry names a node of graph 3
    batch = _dev(x, ei, bv, ptr)
    seld, tgtd = _dev(sel, tgt)
    one = _step(hip, True, batch, seld, tgtd, expect_one_launch=True)
    two = _step(hip, False, batch, seld, tgtd, expect_one_launch=True)
    assert one["status"] == 16 and two["status"] == 16
    assert torch.isnan(one["loss"]).item() and torch.isnan(one["td"][2]).item() and not torch.isnan(one["td"][3]).item()
    _same("selection outside its graph, hidden %d" % hidden, one, two)


def test_a_batch_with_a_13x13_board_runs_as_before():
    """171 rows do not fit a workgroup: the batch takes the layer-major kernels whatever the switch says."""
    hip, _ = _pair(3, 2, 35)
    x, ei, bv, ptr = batch_tensors("D0", [7, 13, 5], maker=True)
    sel, tgt = sel_and_targets(ptr)
    batch = _dev(x, ei, bv, ptr)
    seld, tgtd = _dev(sel, tgt)
    one = _step(hip, True, batch, seld, tgtd)
    two = _step(hip, False, batch, seld, tgtd)
    assert torch.isfinite(one["loss"]).item()
    _same("13 x 13 board", one, two)


def test_defer_lower_runs_the_two_launches():
    hip, _ = _pair(3, 2, 110)
    x, ei, bv, ptr = batch_tensors("D0", [11, 7, 8], maker=True)
    sel, tgt = sel_and_targets(ptr)
    batch = _dev(x, ei, bv, ptr)
    seld, tgtd = _dev(sel, tgt)
    staged = _step(hip, True, batch, seld, tgtd, expect_one_launch=False, defer_lower=True)
    two = _step(hip, False, batch, seld, tgtd, expect_one_launch=False)
    one = _step(hip, True, batch, seld, tgtd, expect_one_launch=True)
    _same("defer_lower", staged, two)
    _same("defer_lower against the one launch", staged, one)


def test_a_capacity_sized_batch_runs_the_two_launches():
    """Rows behind ``x._hex_live_rows`` hold NaN and are never read; the live form keeps its own backward entry."""
    from gnn_hex_amd import ops
    hip, _ = _pair(3, 2, 35)
    x, ei, bv, ptr = batch_tensors("D0", [7, 5, 7, 3], maker=True)
    sel, tgt = sel_and_targets(ptr)
    N, cap, dev = int(ptr[-1]), int(ptr[-1]) + 77, torch.device("cuda")
    gs0 = ops.GraphStructure(ei.cuda(), N)
    E, e_cap = gs0.e, gs0.e + 64
    ptrd, seld, tgtd = _dev(ptr, sel, tgt)

    def exact():
        xd, eid = x.cuda(), ei.cuda()
        ops.attach_hints(xd, True, 51)
        eid._hex_csr = ops.GraphStructure.from_csr(N, E, gs0.rowptr.clone(), gs0.col.clone(), gs0.invdeg.clone())
        return xd, eid, None, ptrd

    def capacity():
        xc = torch.full((cap, 3), float("nan"), device=dev)
        xc[:N] = x.cuda()
        rp = torch.full((cap + 1,), E, dtype=torch.int32, device=dev)
        rp[:N + 1] = gs0.rowptr
        cc = torch.zeros(e_cap, dtype=torch.int32, device=dev)
        cc[:E] = gs0.col[:E]
        iv = torch.full((cap,), float("nan"), device=dev)
        iv[:N] = gs0.invdeg
        eic = torch.zeros((2, e_cap), dtype=torch.long, device=dev)
        eic[:, :E] = ei.cuda()
        ops.attach_hints(xc, True, 51)
        xc._hex_live_rows = torch.tensor([N], dtype=torch.int32, device=dev)
        eic._hex_csr = ops.GraphStructure.from_csr(cap, e_cap, rp, cc, iv)
        return xc, eic, None, ptrd

    live_on = _step(hip, True, capacity(), seld, tgtd, expect_one_launch=False)
    live_off = _step(hip, False, capacity(), seld, tgtd, expect_one_launch=False)
    one = _step(hip, True, exact(), seld, tgtd, expect_one_launch=True)
    for r in (live_on, live_off):          # (rows behind the live count are never written)
        r["q"], r["fcg"] = r["q"][:N], r["fcg"][:N]
    _same("capacity-sized batch", live_on, live_off)
    _same("capacity-sized batch against the exact-size one launch", live_on, one)


def test_captured_step_replays_the_eager_bits_across_weight_updates():
    """Three replays of a captured one-launch step, the weights moved between them: the bits of the eager two-launch sequence."""
    from gnn_hex_amd import ops
    from gnn_hex_amd.graphs import GraphedStep
    hip, _ = _pair(3, 2, 110, seed=0)
    state = copy.deepcopy(hip.state_dict())
    x, ei, bv, ptr = batch_tensors("D1", [11, 7, 8, 11, 5, 3], maker=True)
    sel, tgt = sel_and_targets(ptr)
    xd, eid, bvd, ptrd, seld, tgtd = _dev(x, ei, bv, ptr, sel, tgt)
    ops.attach_hints(xd, True, int((ptr[1:] - ptr[:-1]).max()))       # no host sync inside a capture
    eid._hex_grouped = True
    plist = list(hip.parameters())

    def update():
        with torch.no_grad():
            for p in plist:
                if p.grad is not None:
                    p.sub_(p.grad, alpha=0.05)

    eager = []
    for _ in range(3):
        eager.append(_step(hip, False, (xd, eid, bvd, ptrd), seld, tgtd, expect_one_launch=True))
        update()
    torch.cuda.synchronize()
    assert not torch.equal(eager[0]["q"], eager[2]["q"]), "the weight update did not change the step"
    hip.load_state_dict(state)

    def fn():
        for p in plist:
            p.grad = None
        out = ops.td_step(hip, xd, eid, bvd, ptrd, sel=seld, target=tgtd)
        assert out[2]._hex_call.step_ws is True, "the captured step did not take the one launch"
        return out

    assert ops._ONE_LAUNCH_STEP, "this test captures the default form"
    g = GraphedStep(fn, plist)
    hip.load_state_dict(state)            # (the warm-up steps moved nothing, but the capture starts from the saved weights anyway)
    for k in range(3):
        loss_g, td_g, q_g = g.replay()[:3]
        torch.cuda.synchronize()
        got = dict(loss=loss_g.detach().clone(), td=td_g.detach().clone(), q=q_g.detach().clone(), status=0,
                   grads={n: p.grad.detach().clone() for n, p in hip.named_parameters() if p.grad is not None})
        _same("replay %d" % k, got, eager[k])
        update()
    torch.cuda.synchronize()


def test_both_forms_meet_the_float64_rule_at_110_columns():
    """Both forms could be wrong together: the 110-wide case is also held to the float64 rule of tests/test_gpu_model.py
    (|Q - Q64| < 2e-6; every gradient tensor whose float64 norm exceeds 1e-6 within 5e-3 of it, norm-wise)."""
    hip, ref = _pair(3, 2, 110, seed=5)
    ref64 = copy.deepcopy(ref).double()
    x, ei, bv, ptr = batch_tensors("D1", [11, 7, 8, 11, 5, 3, 11, 2, 7], maker=True)
    sel, tgt = sel_and_targets(ptr)
    q64 = ref64(x.double(), ei, bv, ptr)
    torch.nn.functional.mse_loss(q64[sel], tgt.double()).backward()
    g64 = {k: p.grad for k, p in ref64.named_parameters() if p.grad is not None}
    batch = _dev(x, ei, bv, ptr)
    seld, tgtd = _dev(sel, tgt)
    one = _step(hip, True, batch, seld, tgtd, expect_one_launch=True)
    eq = (one["q"].cpu().double() - q64.detach()).abs().max().item()
    eg = max(((one["grads"][k].cpu().double() - g64[k]).norm() / g64[k].norm()).item() for k in g64 if g64[k].norm() > 1e-6)
    print("one launch against float64: max |Q - Q64| %.3g, worst relative gradient-tensor error %.3g" % (eq, eg))
    assert eq < 2e-6 and eg < 5e-3
