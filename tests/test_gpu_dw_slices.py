"""The batched weight-gradient GEMM (csrc/sage_dw.hip, csrc/sage_dw_kernel.h) at the edges of its host-side slice plan.

The plan (dw_slices_for / dw_rows_per_slice, readable through hexgnn_dw_slice_plan) cuts the n rows of a batch into S slices
per layer; every (slice, layer) workgroup writes one slab of partial sums into the backward's workspace and a reduce kernel
sums the S slabs.  rows_per_slice is rounded up to a multiple of 32 AFTER S is chosen, so the last slices of a launch can start
at or beyond n: they have no row and must still write a slab of zeros, because the workspace is a ``torch.empty`` buffer and
the reduce sums all S slabs.  The whole-model tests elsewhere pick their batch sizes for other reasons; here every batch
is picked THROUGH the query (tests/helpers.py::dw_case_list, asserted to exist by tests/test_host_api.py): graph counts with
and without an empty slice on either side of the first one, the largest one up to 256 graphs, n < 256 (one slice), n just
above a multiple of 1024, hidden 128 / 64 (NT = 8 / 4: the widest tile split, and where the balanced extra wave begins),
the staged backward (two launches of half the layers each) and --norm=True (body and head as two stacks, the head's launch
with the doubled slice cap).  Start-position boards, the sharpened weight state (helpers.sharpen_) at a weight seed whose
ReLU inputs stay clear of zero on that board (_well_conditioned_ref), all three kernel paths.

Every case runs twice with all ``uint8`` scratch of gnn_hex_amd.ops (weight pack, saved state, backward workspace: every
buffer the library carves up itself) pre-filled, once with 0xFF bytes (every float a NaN) and once with 0x3F (finite,
~0.75): Q and all gradients must be finite AND bit-identical between the two, so a result that depends on what the scratch
held fails even where a NaN would have been absorbed (a mask, a max).  Then parity against the float64 oracle with the
rule of tests/test_gpu_parity_tight.py: per gradient tensor ||g - g64|| / ||g64|| <= max(3 x the fp32 oracle's own distance,
2e-3), |Q - Q64| <= max(3 x the fp32 oracle's, 5e-6; 8e-6 on f16x3), vanishing tensors (||g64|| < 1e-6) to 1e-6 absolute.
The hidden layers' bias gradients -- an exact fp32 column sum in both math modes -- are among the tensors and take the same
gate.  The loss is scaled by graphs / 4 (the 64 of test_gpu_parity_tight.py at 256 graphs: the mean over the graphs divides
every gradient by their number), doubled per case until the ORACLE's smallest non-vanishing tensor has |g|max >= 1e-2.
"""
import copy

import pytest
import torch

from helpers import (DW_MODELS, batch_tensors, dw_case_list, dw_has_empty, dw_launches, model_args, sel_and_targets,
                     sharpen_)
from helpers import PoisonedTorch as _PoisonedTorch

pytestmark = pytest.mark.gpu

CASES = {c[0]: c[1:] for c in dw_case_list()}
_cache = {}


def _run(model, x, ei, batch, ptr, sel, tgt, gscale):
    model.zero_grad(set_to_none=True)
    q = model(x, ei, batch, ptr)
    (torch.nn.functional.mse_loss(q[sel], tgt) * gscale).backward()
    return q.detach().clone(), {k: (None if p.grad is None else p.grad.detach().clone()) for k, p in model.named_parameters()}


def _args_of(key, norm):
    layers, hidden, _ = DW_MODELS[key]
    args = model_args(layers, hidden)
    args.norm = bool(norm)
    return args


MARGIN = 2.0 ** -16      # smallest |pre-activation| / rms the weight state of a case may have, see _well_conditioned_ref
_states = {}


def _relu_inputs(model, store):
    """Forward hooks that keep every tensor a ReLU is applied to (oracle/model_ref.py: the SAGE layers' outputs -- with
    --norm=True their norms' outputs -- of the body and of the maker head, and the first layer of the value MLP)."""
    hooks = []
    for tag, gnn in (("body", model.gnn), ("head", model.maker_head.gnn)):
        mods = gnn.convs if gnn.norms is None else gnn.norms
        for l, m in enumerate(mods):
            hooks.append(m.register_forward_hook(lambda mod, inp, out, k="%s.%d" % (tag, l): store.__setitem__(k, out.detach())))
    hooks.append(model.maker_head.value_head.layers[0].register_forward_hook(
        lambda mod, inp, out: store.__setitem__("value", out.detach())))
    return hooks


def _well_conditioned_ref(key, norm):
    """The sharpened oracle of one network, at the first weight seed whose ReLU inputs all stay clear of zero on the start
    board: min |pre-activation| >= 2^-16 x the tensor's rms, in float64.

    Why: a ReLU network is only piecewise smooth, and every graph of a start-position batch is the SAME graph, so a
    pre-activation within fp32 rounding of zero flips its mask in all graphs at once, and one flipped element of layer l
    moves the bias gradients of the layers <= l by 1e-3..5e-3 of their norm whatever the kernels do.  Measured on the MI355X
    at weight seed 0, GNN-L, 21 boards: the float64 pre-activation of (layer 13, node 65, channel 42) is -3.9e-7 of the
    layer's rms; the fused fp32 kernels have it > 0 in all 21 graphs and no other mask differs, and the bias gradients of
    layers 10..13 come out 2.0e-3 / 2.2e-3 / 2.7e-3 / 4.2e-3 off (that one element's term, to three digits: the float64
    oracle with the opposite sign on it is exactly twice as far away); the f16x3 path flips nothing and the layer-major
    path another element of no consequence (both <= 3.3e-6).  That is above the 2e-3 floor, true of any fp32 evaluation,
    and not what this file is after.  The margin comes from the bound this file sets on Q itself: |Q - Q64| <= 5e-6..8e-6 at
    |Q| <= 2 lets a correct evaluation be off by ~4e-6 of its scale, and 2^-16 = 1.5e-5 is four times that.  The seed is
    chosen from the float64 oracle alone, before anything runs on the device."""
    if (key, norm) not in _states:
        from oracle.model_ref import get_pre_defined_ref
        size = DW_MODELS[key][2]
        x, ei, batch, ptr = batch_tensors("D0", [size], maker=True)
        for seed in range(200):
            torch.manual_seed(seed)
            ref = get_pre_defined_ref("modern_two_headed", _args_of(key, norm))
            if norm:
                with torch.no_grad():                  # non-trivial affine parameters (the default is weight 1, bias 0)
                    for k, p in ref.named_parameters():
                        if "norm" in k:
                            p.add_(torch.randn(p.shape) * 0.2)
            sharpen_(ref)
            ref64, pre = copy.deepcopy(ref).double(), {}
            hooks = _relu_inputs(ref64, pre)
            with torch.no_grad():
                ref64(x.double(), ei, batch, ptr)
            for h in hooks:
                h.remove()
            margin = min((t.abs().min() / t.pow(2).mean().sqrt()).item() for t in pre.values())
            if margin >= MARGIN:
                break
        else:
            raise AssertionError("%s: no weight seed below 200 keeps the ReLU inputs clear of zero" % key)
        print("%s%s: weight seed %d, smallest |pre-activation| / rms %.3g" % (key, " norm" if norm else "", seed, margin))
        _states[(key, norm)] = ref
    return copy.deepcopy(_states[(key, norm)])


def _oracle(name):
    """fp32 and float64 oracle results of one case on the sharpened state, computed once per session; the loss scale is
    raised (by powers of two, from the oracle's own gradients only) until the smallest non-vanishing tensor has |g|max >= 1e-2."""
    if name not in _cache:
        key, b, staged, norm = CASES[name]
        size = DW_MODELS[key][2]
        ref = _well_conditioned_ref(key, norm)
        x, ei, batch, ptr = batch_tensors("D0", [size] * b, maker=True)
        sel, tgt = sel_and_targets(ptr)
        ref64 = copy.deepcopy(ref).double()
        gscale = b / 4.0
        for _ in range(12):
            q64, g64 = _run(ref64, x.double(), ei, batch, ptr, sel, tgt.double(), gscale)
            small = min(g.abs().max().item() for g in g64.values() if g is not None and g.norm().item() >= 1e-6)
            if small >= 1e-2:
                break
            gscale *= 2.0
        q32, g32 = _run(ref, x, ei, batch, ptr, sel, tgt, gscale)
        _cache[name] = dict(state=ref.state_dict(), inputs=(x, ei, batch, ptr, sel, tgt), gscale=gscale, q32=q32, g32=g32,
                            q64=q64, g64=g64)
    return _cache[name]


@pytest.fixture(params=[(True, "fp32"), (True, "f16x3"), (False, "fp32")], ids=["fused", "fused-f16x3", "layered"])
def path(request):
    from gnn_hex_amd import ops
    ops.set_fused(request.param[0])
    ops.set_math(request.param[1])
    yield request.param
    ops.set_fused(True)
    ops.set_math("fp32")
    ops.set_grad_stage_hook(None)


@pytest.mark.parametrize("name", sorted(CASES))
def test_slice_plan_edges_with_poisoned_scratch(name, path, monkeypatch):
    from gnn_hex_amd import ops
    from gnn_hex_amd.models import get_pre_defined
    key, b, staged, norm = CASES[name]
    layers, hidden, size = DW_MODELS[key]
    o = _oracle(name)
    x, ei, batch, ptr, sel, tgt = o["inputs"]
    n = int(ptr[-1])
    assert n == x.shape[0] and len(ptr) == b + 1

    # the case is what its id says, on the plan of the library that is loaded now
    fused_kernels = path[0] and not norm and bool(ops.qnet_fused_supported(2, hidden, int((ptr[1:] - ptr[:-1]).max())))
    math = 1 if (fused_kernels and path[1] == "f16x3") else 0
    launches = dw_launches(layers, staged=staged and fused_kernels, norm=norm)
    empty_now = dw_has_empty(n, launches, math)
    for m in (0, 1):
        for role, want in (("first", True), ("last", True), ("before", False), ("after", False)):
            if "m%d-%s" % (m, role) in name:
                assert dw_has_empty(n, dw_launches(layers), m) == want, name
    if "empty" in name:
        assert empty_now, name

    # on the oracle: the signal every bound below is relative to must be there
    compared = [k for k, g in o["g64"].items() if g is not None]
    for k in compared:
        g = o["g64"][k]
        if g.norm().item() >= 1e-6:
            assert g.abs().max().item() >= 1e-2, "%s: |g|max %g at loss scale %g" % (k, g.abs().max().item(), o["gscale"])
    n_head = 2
    want_bias = ["gnn.convs.%d.lin_l.bias" % l for l in range(1, layers)] + \
                ["maker_head.gnn.convs.%d.lin_l.bias" % l for l in range(n_head)]
    assert all(k in compared and o["g64"][k].norm().item() >= 1e-6 for k in want_bias), "hidden-layer bias gradients"

    hip = get_pre_defined("modern_two_headed", _args_of(key, norm))
    hip.load_state_dict(o["state"])
    hip = hip.cuda()
    xd, eid = x.cuda(), ei.cuda()
    xd._hex_is_maker = True
    xd._hex_max_nodes = int((ptr[1:] - ptr[:-1]).max())
    eid._hex_grouped = True
    dev = (xd, eid, batch.cuda(), ptr.cuda(), sel.cuda(), tgt.cuda())
    if staged:
        ops.set_grad_stage_hook(lambda flat, lo, hi: None)      # (restored by the fixture)

    runs = []
    for byte in (0xFF, 0x3F):
        stand_in = _PoisonedTorch(byte)
        with monkeypatch.context() as mp:
            mp.setattr(ops, "torch", stand_in)
            q, g = _run(hip, *dev, o["gscale"])
            torch.cuda.synchronize()
        assert stand_in.filled >= 2, "the scratch of this path did not come through ops' torch.empty"
        runs.append((q, g))
    print("%s %s: n %d, launches %s, math %d, empty slice %s, loss scale %g" % (name, path, n, launches, math, empty_now,
                                                                                 o["gscale"]))
    (q, g), (q2, g2) = runs
    bad = [k for k in ["Q"] + compared
           if not bool(torch.isfinite(q if k == "Q" else g[k]).all())]
    assert not bad, "%s: NaN / Inf with 0xFF scratch in %s" % (name, bad)
    diff = [k for k in ["Q"] + compared
            if not torch.equal(q if k == "Q" else g[k], q2 if k == "Q" else g2[k])]
    assert not diff, "%s: results depend on what the scratch held (0xFF vs 0x3F fill): %s" % (name, diff)

    split = path[1] == "f16x3"
    eq = (q.cpu().double() - o["q64"]).abs().max().item()
    eq32 = (o["q32"].double() - o["q64"]).abs().max().item()
    worst, fails = (0.0, 0.0, ""), []
    for k, g64 in o["g64"].items():
        if g64 is None:
            assert g[k] is None, k
            continue
        assert g[k] is not None, k
        nrm = g64.norm().item()
        if nrm < 1e-6:      # a tensor whose true gradient vanishes is rounding noise in any arithmetic: absolute bound
            err = (g[k].cpu().double() - g64).abs().max().item()
            if not err < 1e-6:
                fails.append("%s: vanishing tensor, abs err %.3g" % (k, err))
            continue
        rel = (g[k].cpu().double() - g64).norm().item() / nrm
        rel32 = (o["g32"][k].double() - g64).norm().item() / nrm
        if rel > worst[0]:
            worst = (rel, rel32, k)
        if not rel <= max(3.0 * rel32, 2e-3):
            fails.append("%s: ||g - g64|| / ||g64|| = %.3g, the fp32 oracle's own %.3g" % (k, rel, rel32))
    print("%s %s: |Q-Q64| %.3g (oracle32 %.3g); worst gradient tensor %s rel %.3g (oracle32 %.3g)"
          % (name, path, eq, eq32, worst[2], worst[0], worst[1]))
    assert eq <= max(3.0 * eq32, 8e-6 if split else 5e-6), "%s: |Q - Q64| %g (fp32 oracle %g)" % (name, eq, eq32)
    assert not fails, "%s: %s" % (name, "; ".join(fails))
