"""The HexAra head kernels of csrc/hexara_head.hip called directly: ops.sage_scalar / SageScalarFn (sage_scalar_dots_kernel,
sage_scalar_gather_kernel, sage_scalar_bwd_kernel) and ops.PolicyLogSoftmaxFn (policy_lsm_fwd_kernel / policy_lsm_bwd_kernel), under the
float64 rule of tests/test_gpu_wide_parity.py (same helpers, same constants): outputs within max(3 x the fp32 expression's own
distance from float64, 5e-6), gradients within max(3 x its own, 2e-3) in relative norm; index outputs exact.  Until here both ran only
inside SAGE_torch_script, on boards: widths 16, 35, 60, 110, segments up to 122 entries, at most 64 graphs, feature 2 equal on every
row of a graph.

1. Scalar SAGE layer.  Reference helpers.sage_scalar_ref: out = b + h . w_r + mean over in-edges of h . w_l through scatter_ref, in
   float64 and fp32.  Graphs: tests/test_gpu_model.py::_random_batch (directed, three duplicated edges, row n - 1 without in-edges,
   row n - 2 without out-edges) with p_edge = max(0.08, 24 / n), so that rows with more than 16 in-edges exist from 63 rows on;
   n = 1, 63, 64, 65, 128, 129, 255, 256, 257, 1000 (the 64-row blocks of sage_scalar_dots / _bwd_kernel and their per-block
   partials, the 256-row blocks of the gather) x widths 2, 3, 16, 35, 60, 127, 128; h ~ N(0, 1), SAGEConvRef(H, 1) at torch's
   default init (seed 0), loss sum(out * R).  out, dh, d_wl, d_wr, d_bias under the rule; once more with 0xFF in the backward's
   workspace and twice for the same bits.
2. Policy log-softmax.  Reference helpers.policy_ref: the surgery loop and scatter_log_softmax_ref of oracle/hexara_ref.py on a given
   pi_raw, should_swap, x, ptr.  Batches: graphs of 3, 4, 130, 257, 258, 259, 260, 514, 515, 700 rows (1, 2, 128, 255..258, 512, 513,
   698 entries in front of the swap slot), 300 three-row graphs (299 graphs in front of the last: the slot count of earlier graphs
   strides 256 over them), one graph alone; swap_allowed both ways; logits ~ N(0, 1) and ~ U(-30, 30).  out_gi, out_ptr and the live
   length exact; pi, d_pi_raw, d_should_swap under abs_bound against float64; d_pi_raw of terminal rows and d_should_swap of
   graphs without a slot exactly 0; sum(exp(pi)) per segment against 1 under the same abs_bound (the fp32 expression's own
   deviation is the yardstick).

Which case has a different expected value when the kernel gets it wrong:
  * segments past 256 -- the 259-, 260-, 514-, 515- and 700-row graphs: entries 256.. of a segment take the second and third trip
    of the stride-256 loops; one that is skipped changes the segment's log-sum-exp (every pi of it) and leaves its own pi and
    d_pi_raw unwritten; the swap slot behind 256, 257, 258, 512 entries is entry k = r1 - r0 of the LAST trip.  In the 300-graph
    batch every segment start behind graph 256 depends on the second trip of the slot count (out_ptr, out_gi, where pi lands).
  * the first-row / last-row swap probe -- feature 2 is set on the first row only (graphs 0, 4, 8, ..), on the last row only
    (1, 5, ..), on no row (2, 6, ..) or on all (3, 7, ..): probing the wrong end of any graph of the first two kinds moves every
    later out_ptr by one.  The last graph is run both ways: first row only (a slot; the last-row rule would give none) and last
    row only (no slot; the last-row rule would give one).  With b = 1 the only graph is the last one.

Measured on the MI355X (printed per case).  Per output the case that came closest to its bound, in brackets the fp32 expression's own
distance from float64 in the same case:

  sage_scalar   out 2.57e-7 (2.57e-7)   dh 5.53e-8 (5.21e-8)   d_wl 6.32e-7 (7.59e-7)   d_wr 7.98e-7 (2.62e-7)   d_bias 1.05e-6 (5.25e-7)
  policy        pi 1.91e-6 (1.91e-6; the largest absolute figure is 3.59e-6 (3.59e-6) on U(-30, 30): one ulp of a log-probability
                near -60)   d_pi_raw 5.23e-7 (7.34e-7)   d_should_swap 1.18e-7 (9.07e-8)   sum exp(pi) 4.49e-7 (4.13e-7)

pi reaches 0.33 of its bound, everything else stays below 0.11; 24 of the 434 figures lie above three times the fp32 expression's own
and rest on a floor, all below 0.11 of it.

Against libraries with one value-only change in hexara_head.hip (built aside, never committed): policy_lsm_fwd_kernel counting the
swap slots of the first 256 earlier graphs only fails the four swap_allowed cases of the 300-graph batch and nothing else; its
sum of exponentials stopping after two trips (512 entries) fails the eight cases of the 3..700-row batch and nothing else;
swap_flag probing the last row of every graph fails all twelve swap_allowed cases (both settings of the last graph) and nothing else.
"""
import copy

import pytest
import torch

from helpers import (PoisonedTorch, QnetCases, abs_bound, policy_inputs, policy_ref_run, rel_bound, sage_scalar_ref)
from test_gpu_model import _random_batch

pytestmark = pytest.mark.gpu

CONST = QnetCases.CONST


# ---- 1. the scalar SAGE layer ------------------------------------------------------------------------------------------------------

SAGE_ROWS = [1, 63, 64, 65, 128, 129, 255, 256, 257, 1000]
SAGE_WIDTHS = [2, 3, 16, 35, 60, 127, 128]
SAGE_NAMES = ["d_wl", "d_bias", "d_wr"]
_graphs, _sage = {}, {}


def _graph(n):
    if n not in _graphs:
        _, ei, _, _ = _random_batch([n], seed=500 + n, directed=True, p_edge=max(0.08, 24.0 / n))
        indeg, outdeg = torch.bincount(ei[1], minlength=n), torch.bincount(ei[0], minlength=n)
        if n > 3:
            assert int(indeg.max()) > 16 and int(indeg[n - 1]) == 0 and int(outdeg[n - 2]) == 0
            assert ei.shape[1] > torch.unique(ei, dim=1).shape[1], "no duplicated edge"
            assert not torch.equal(torch.sort(ei[0] * n + ei[1]).values, torch.sort(ei[1] * n + ei[0]).values), "not directed"
        else:
            assert ei.shape[1] == 0
        _graphs[n] = ei
    return _graphs[n]


def _sage_run(conv, h, ei, r):
    for p in conv.parameters():
        p.grad = None
    h = h.detach().clone().requires_grad_(True)
    out = sage_scalar_ref(h, ei, conv.lin_l.weight, conv.lin_l.bias, conv.lin_r.weight)
    (out * r).sum().backward()
    return dict(out=out.detach(), dh=h.grad, grads=[conv.lin_l.weight.grad, conv.lin_l.bias.grad, conv.lin_r.weight.grad])


def _sage_oracle(n, hidden):
    from oracle.model_ref import SAGEConvRef
    if (n, hidden) not in _sage:
        ei = _graph(n)
        gen = torch.Generator().manual_seed(n * 131 + hidden)
        h, r = torch.randn(n, hidden, generator=gen), torch.rand(n, generator=gen) * 2 - 1
        torch.manual_seed(0)
        conv = SAGEConvRef(hidden, 1)
        _sage[(n, hidden)] = dict(ei=ei, h=h, r=r, conv=conv, r64=_sage_run(copy.deepcopy(conv).double(), h.double(), ei, r.double()),
                                  r32=_sage_run(conv, h, ei, r))
    return _sage[(n, hidden)]


def _sage_dev(o, n, hidden):
    from gnn_hex_amd import ops
    conv = copy.deepcopy(o["conv"]).cuda()
    hd = o["h"].cuda().requires_grad_(True)
    gs = ops.GraphStructure(o["ei"].cuda(), n)
    out = ops.sage_scalar(hd, gs, hidden, conv)
    (out * o["r"].cuda()).sum().backward()
    torch.cuda.synchronize()
    return dict(out=out.detach(), dh=hd.grad, grads=[conv.lin_l.weight.grad, conv.lin_l.bias.grad, conv.lin_r.weight.grad])


def _sage_check(tag, o, res):
    r64, r32 = o["r64"], o["r32"]
    assert tuple(res["out"].shape) == tuple(r64["out"].shape) and tuple(res["dh"].shape) == tuple(r64["dh"].shape)
    figs = {"out": abs_bound(tag, "out", res["out"], r32["out"], r64["out"], CONST),
            "dh": rel_bound(tag, "dh", res["dh"], r32["dh"], r64["dh"])}
    for name, g, a32, a64 in zip(SAGE_NAMES, res["grads"], r32["grads"], r64["grads"]):
        assert g is not None and tuple(g.shape) == tuple(a64.shape), name
        figs[name] = rel_bound(tag, name, g, a32, a64)
    print("%s: " % tag + "; ".join("%s %.3g (fp32 %.3g)" % ((k,) + v) for k, v in figs.items()))


def _sage_same_bits(tag, a, b):
    for name, ta, tb in [("out", a["out"], b["out"]), ("dh", a["dh"], b["dh"])] + list(zip(SAGE_NAMES, a["grads"], b["grads"])):
        assert bool(torch.isfinite(tb).all()), "%s %s: not finite" % (tag, name)
        assert torch.equal(ta, tb), "%s: %s differs" % (tag, name)


@pytest.mark.parametrize("hidden", SAGE_WIDTHS)
@pytest.mark.parametrize("n", SAGE_ROWS)
def test_sage_scalar_against_float64(n, hidden, monkeypatch):
    from gnn_hex_amd import ops
    tag = "sage_scalar n %d hidden %d" % (n, hidden)
    o = _sage_oracle(n, hidden)
    res = _sage_dev(o, n, hidden)
    _sage_check(tag, o, res)
    _sage_same_bits(tag + " again", res, _sage_dev(o, n, hidden))
    stand_in = PoisonedTorch(0xFF)
    with monkeypatch.context() as mp:
        mp.setattr(ops, "torch", stand_in)
        poisoned = _sage_dev(o, n, hidden)
    assert stand_in.filled >= 1, "the scratch of this path did not come through ops' torch.empty"
    _sage_same_bits(tag + " poisoned", res, poisoned)


# ---- 2. the policy log-softmax ----------------------------------------------------------------------------------------------------

_policy = {}
POLICY_CASES = [(name, last, family, swap) for name in ("rows", "many", "one") for last in ("first", "last")
                for family in ("unit", "spread") for swap in (True, False)]


def _policy_oracle(name, last, family, swap):
    key = (name, last, family, swap)
    if key not in _policy:
        inp = policy_inputs(name, last, family)
        _policy[key] = dict(inp=inp, r64=policy_ref_run(inp, swap, torch.float64), r32=policy_ref_run(inp, swap, torch.float32))
    return _policy[key]


def _policy_dev(inp, swap):
    from gnn_hex_amd import ops
    raw = inp["pi_raw"].cuda().requires_grad_(True)
    ss = inp["should_swap"].cuda().requires_grad_(True) if swap else None
    pi, gi, optr = ops.PolicyLogSoftmaxFn.apply(raw, ss, inp["x"].cuda(), inp["ptr"].to(torch.int32).cuda(), inp["b"], swap)
    live = int(optr[-1])
    (pi[:live] * inp["r"][:live].cuda()).sum().backward()
    torch.cuda.synchronize()
    return dict(pi=pi.detach()[:live], gi=gi[:live], ptr=optr, live=live, cap=pi.numel(), d_raw=raw.grad, d_ss=ss.grad if swap else None)


def _segment_sums(pi, optr):
    e = pi.detach().cpu().double().exp()
    p = optr.tolist()
    return torch.stack([e[p[g]:p[g + 1]].sum() for g in range(len(p) - 1)])


@pytest.mark.parametrize("name,last,family,swap", POLICY_CASES, ids=["%s-%s-%s-swap%d" % c for c in POLICY_CASES])
def test_policy_log_softmax_against_float64(name, last, family, swap):
    o = _policy_oracle(name, last, family, swap)
    inp, r64, r32 = o["inp"], o["r64"], o["r32"]
    tag = "policy %s last graph %s %s swap_allowed %s" % (name, last, family, swap)
    # the input does what the docstring says: the two probe rules disagree on the last graph
    lo, hi = int(inp["ptr"][-2]), int(inp["ptr"][-1])
    first, final = bool(inp["x"][lo, 2] != 0), bool(inp["x"][hi - 1, 2] != 0)
    assert first != final and first == (last == "first")
    slots = (r64["ptr"][1:] - r64["ptr"][:-1]) - (inp["ptr"][1:] - inp["ptr"][:-1] - 2)
    assert torch.equal(r32["ptr"], r64["ptr"]) and torch.equal(r32["gi"], r64["gi"]) and set(slots.tolist()) <= {0, 1}
    assert int(slots[-1]) == int(swap and first)
    if swap and inp["b"] > 4:
        assert slots[:4].tolist() == [0, 1, 0, 1]
    res = _policy_dev(inp, swap)
    assert res["cap"] == inp["n"] - 2 * inp["b"] + (inp["b"] if swap else 0)
    assert res["live"] == r64["pi"].numel() == int(r64["ptr"][-1])
    assert res["ptr"].dtype == torch.int64 and torch.equal(res["ptr"].cpu(), r64["ptr"])
    assert res["gi"].dtype == torch.int64 and torch.equal(res["gi"].cpu(), r64["gi"])
    figs = {"pi": abs_bound(tag, "pi", res["pi"], r32["pi"], r64["pi"], CONST),
            "d_pi_raw": abs_bound(tag, "d_pi_raw", res["d_raw"], r32["d_raw"], r64["d_raw"], CONST)}
    terminal = torch.cat([inp["ptr"][:-1], inp["ptr"][:-1] + 1])
    assert float(res["d_raw"].cpu()[terminal].abs().max()) == 0.0, "%s: a terminal row has a gradient" % tag
    assert float(r64["d_raw"][terminal].abs().max()) == 0.0
    if swap:
        figs["d_should_swap"] = abs_bound(tag, "d_should_swap", res["d_ss"], r32["d_ss"], r64["d_ss"], CONST)
        assert float(res["d_ss"].cpu()[slots == 0].abs().max() if bool((slots == 0).any()) else 0.0) == 0.0, \
            "%s: a graph without a swap slot has a swap gradient" % tag
    else:
        assert res["d_ss"] is None
    figs["sum exp(pi)"] = abs_bound(tag, "segment sum of exp(pi)", _segment_sums(res["pi"], r64["ptr"]),
                                    _segment_sums(r32["pi"], r64["ptr"]), _segment_sums(r64["pi"], r64["ptr"]), CONST)
    assert float((_segment_sums(r64["pi"], r64["ptr"]) - 1).abs().max()) < 1e-12
    again = _policy_dev(inp, swap)
    for k in ("pi", "gi", "ptr", "d_raw", "d_ss"):
        assert (res[k] is None and again[k] is None) or torch.equal(res[k], again[k]), "%s: %s differs between two runs" % (tag, k)
    print("%s: " % tag + "; ".join("%s %.3g (fp32 %.3g)" % ((k,) + v) for k, v in figs.items()))
