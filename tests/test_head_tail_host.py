"""CPU side of tests/test_gpu_head_tail.py and tests/test_gpu_hexara_kernels.py: the torch expressions those files use as their
reference agree with the oracle's own modules at float64 round-off, the weight-seed search meets its condition for every case the
GPU tests run, and the head entry points' size queries answer degenerate shapes on the host."""
import copy

import pytest
import torch

from helpers import (HEAD_MODE_WIDTHS, HEAD_WIDE, HEAD_WIDTHS, MARGIN, HeadCases, batch_tensors, head_params, head_tail_ref, model_args,
                     policy_ref, sage_scalar_ref)

ROUND_OFF = 1e-12


def _tail_of(model, x, ei):
    """(h behind the maker head's SAGE layers, its advantage linear, its value head) of an oracle Q-network."""
    head = model.maker_head
    return head.gnn(model.gnn(x[:, :2], ei), ei), head.linear, head.value_head


@pytest.mark.parametrize("family", ["modern_two_headed", "two_headed"])
def test_tail_expression_is_the_oracles_head_and_dueling_combine(family):
    from oracle.model_ref import get_pre_defined_ref
    torch.manual_seed(3)
    model = get_pre_defined_ref(family, model_args(2, 12)).double()
    x, ei, batch, ptr = batch_tensors("D1", [3, 5, 4], maker=True)
    x = x.double()
    b = ptr.numel() - 1
    with torch.no_grad():
        h, lin, val = _tail_of(model, x, ei)
        assert hasattr(val, "layers") == (family == "modern_two_headed")
        adv, value = model.maker_head(model.gnn(x[:, :2], ei), ei, batch)
        q3, v3 = head_tail_ref(h, batch, b, 3, lin, val)
        assert (q3 - adv.reshape(-1)).abs().max() < ROUND_OFF and (v3 - value.reshape(-1)).abs().max() < ROUND_OFF
        assert (head_tail_ref(h, batch, b, 4, lin, val)[0] - adv.reshape(-1)).abs().max() < ROUND_OFF
        assert (head_tail_ref(h, batch, b, 0, lin, val)[0] - model(x, ei, batch, ptr)).abs().max() < ROUND_OFF
        v1, q1 = model(x, ei, batch, ptr, seperate=True)
        got_q, got_v = head_tail_ref(h, batch, b, 1, lin, val)
        assert (got_q - q1).abs().max() < ROUND_OFF and (got_v - v1).abs().max() < ROUND_OFF
        q2 = model(x, ei, batch, ptr, advantages_only=True).reshape(-1)
        assert (head_tail_ref(h, batch, b, 2, lin, val)[0] - q2).abs().max() < ROUND_OFF
    assert [tuple(p.shape) for p in head_params(lin, val)][:2] == [(1, 12), (1,)]


def test_tail_expression_gives_an_empty_graph_the_value_of_zeros():
    """HeadNetworkRef drops trailing empty graphs (scatter without dim_size); the expression keeps them: pooled zeros, no rows."""
    from helpers import head_modules
    lin, val = head_modules("mlp", 6, 0)
    h = torch.randn(5, 6, generator=torch.Generator().manual_seed(1)).double()
    batch = torch.tensor([0, 0, 2, 2, 2])
    with torch.no_grad():
        q, v = head_tail_ref(h, batch, 4, 3, lin.double(), val.double())
        zero = val(torch.zeros(1, 24, dtype=torch.float64)).reshape(())
    assert q.shape == (5,) and v.shape == (4,) and float(v[1]) == float(zero) and float(v[3]) == float(zero)


@pytest.mark.parametrize("swap_allowed", [True, False])
def test_hexara_expressions_are_the_oracles_model(swap_allowed):
    from oracle.hexara_ref import get_current_model_ref
    torch.manual_seed(5)
    m = get_current_model_ref(hidden_channels=12, hidden_layers=2, policy_layers=2, value_layers=2, swap_allowed=swap_allowed).double()
    x, ei, batch, ptr = batch_tensors("D1", [3, 4, 3], maker=True)
    x = x.clone()
    x[:, 2] = 0.0
    x[int(ptr[1]) - 1, 2] = 1.0          # last row of graph 0 only: a slot
    x[int(ptr[1]), 2] = 1.0              # first row of graph 1 only: none
    x[int(ptr[2]), 2] = 1.0              # first row of the last graph only: a slot
    x = x.double()
    b = ptr.numel() - 1
    with torch.no_grad():
        pi, value, gi, optr = m(x, ei, batch, ptr)
        embeds = m.gnn(x, ei)
        policy = m.my_modules["policy_head"]
        hp = embeds
        for conv in policy.convs[:-1]:
            hp = torch.relu(conv(hp, ei))
        last = policy.convs[-1]
        pi_raw = sage_scalar_ref(hp, ei, last.lin_l.weight, last.lin_l.bias, last.lin_r.weight)
        assert (pi_raw - policy(embeds, ei).reshape(-1)).abs().max() < ROUND_OFF
        hv = m.my_modules["value_head"](embeds, ei)
        zero = torch.nn.Linear(12, 1).double()
        zero.weight.zero_(), zero.bias.zero_()
        _, v1 = head_tail_ref(hv, batch, b, 1, zero, m.my_modules["value_linear"])
        assert (v1 - value).abs().max() < ROUND_OFF
        _, ss = head_tail_ref(hv, batch, b, 3, zero, m.my_modules["swap_linear"])
        got_pi, got_gi, got_ptr = policy_ref(pi_raw, ss, x, ptr, swap_allowed)
    assert torch.equal(got_gi, gi) and torch.equal(got_ptr, optr) and (got_pi - pi).abs().max() < ROUND_OFF
    sizes = (ptr[1:] - ptr[:-1] - 2).tolist()
    assert (optr[1:] - optr[:-1]).tolist() == ([sizes[0] + 1, sizes[1], sizes[2] + 1] if swap_allowed else sizes)


def _searched():
    out = []
    for kind, widths in (("mlp", HEAD_WIDTHS + [HEAD_WIDE]), ("linear", HEAD_WIDTHS)):
        out += [(kind, "full", w, "randn") for w in widths] + [(kind, "full", w, "ties") for w in HEAD_MODE_WIDTHS]
        out += [(kind, name, w, fam) for name in ("row1", "rows1025") for w, fam in ((35, "randn"), (128, "ties"), (3, "randn"))]
    return out + [("mlp", "rows1025", HEAD_WIDE, "randn"), ("mlp", "full", HEAD_WIDE, "ties")]


def test_the_searched_cases_are_the_gpu_files_cases():
    import test_gpu_head_tail
    assert sorted(set(c[:4] for c in test_gpu_head_tail.CASES)) == sorted(set(_searched()))


@pytest.mark.parametrize("kind,name,hidden,family", _searched(), ids=["%s-%s-h%d-%s" % c for c in _searched()])
def test_a_weight_seed_meets_the_relu_margin(kind, name, hidden, family):
    seed, margin = HeadCases().seed(kind, name, hidden, family)
    assert margin >= MARGIN
    print("%s %s hidden %d %s: weight seed %d, smallest |ReLU input| / rms %.3g" % (kind, name, hidden, family, seed, margin))


def _align(v, a=256):
    return (v + a - 1) // a * a


def test_head_size_queries_on_degenerate_shapes():
    """hexgnn_head_saved_bytes / hexgnn_head_backward_workspace_bytes and the Linear tail's: pure host arithmetic.  An unsupported
    width (0, 257; above 128 for the Linear tail's workspace) or a negative count answers 0; n = 0 and b = 0 are legal and keep one
    slot where a kernel indexes by max(b, 1); hidden 1 has H / 2 = 0 and keeps one z slot."""
    from gnn_hex_amd import _lib
    L = _lib.lib()
    for hidden in (0, 257, -1):
        assert L.hexgnn_head_saved_bytes(5, 2, hidden) == 0 and L.hexgnn_head_backward_workspace_bytes(5, 2, hidden) == 0
        assert L.hexgnn_head_linear_backward_workspace_bytes(5, 2, hidden) == 0
    assert L.hexgnn_head_linear_backward_workspace_bytes(5, 2, 129) == 0 and L.hexgnn_head_backward_workspace_bytes(5, 2, 129) > 0
    for n, b in ((-1, 2), (5, -1)):
        assert L.hexgnn_head_saved_bytes(n, b, 35) == 0 and L.hexgnn_head_backward_workspace_bytes(n, b, 35) == 0
        assert L.hexgnn_head_linear_saved_bytes(n, b) == 0 and L.hexgnn_head_linear_backward_workspace_bytes(n, b, 35) == 0
    for n, b, hidden in ((0, 0, 35), (0, 3, 35), (7, 0, 35), (7, 3, 1), (7, 3, 2), (6140, 30, 128), (6140, 30, 144), (7, 3, 256)):
        hp, h2 = (hidden + 15) // 16 * 16, max(hidden // 2, 1)
        saved = _align(4 * n) + _align(4 * b * 4 * hidden) + 2 * _align(4 * b * hidden) + _align(4 * b * h2) + _align(4 * b)
        assert L.hexgnn_head_saved_bytes(n, b, hidden) == saved, (n, b, hidden)
        ws = _align(4 * n) + _align(4 * b * h2) + _align(4 * b) + _align(4 * max(b, 1) * (hp + 1))
        assert L.hexgnn_head_backward_workspace_bytes(n, b, hidden) == ws, (n, b, hidden)
        assert L.hexgnn_head_linear_saved_bytes(n, b) == _align(4 * n) + _align(4 * b)
        if hidden <= 128:
            lin = _align(4 * max(b, 1)) + 2 * _align(4 * max(b, 1) * (hp + 1))
            assert L.hexgnn_head_linear_backward_workspace_bytes(n, b, hidden) == lin, (n, b, hidden)
    # the calls themselves refuse these shapes before they touch the device
    assert L.hexgnn_head_forward(0, 0, 1, 0, *([None] * 12)) == -2 and L.hexgnn_head_forward(0, 0, 257, 0, *([None] * 12)) == -2
    assert L.hexgnn_head_forward(0, 0, 0, 0, *([None] * 12)) == -2
    assert L.hexgnn_head_backward(0, 0, 1, 0, *([None] * 16), 0, None) == -2
    assert L.hexgnn_head_backward(0, 0, 257, 8, *([None] * 16), 0, None) == -2
    assert L.hexgnn_head_linear_forward(0, 0, 0, 0, *([None] * 10)) == -2 and L.hexgnn_head_linear_forward(0, 0, 129, 0, *([None] * 10)) == -2
    assert L.hexgnn_head_linear_backward(0, 0, 257, 0, *([None] * 13), 0, None) == -2
    assert L.hexgnn_head_forward(0, 0, 35, 5, *([None] * 12)) == -1 and L.hexgnn_head_forward(-1, 0, 35, 0, *([None] * 12)) == -1
