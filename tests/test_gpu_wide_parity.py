"""hidden 129..256 (gnn_hex_amd/csrc/wide.hip) under the float64 rule: all eight padded widths, both ends, odd and even.

tests/test_gpu_wide.py holds these widths to an absolute 1e-4 at hidden 130, 144, 160, 176, 200 and 256: HP 192, 224 and 240 (NT = 12,
14, 15 of wide_gemm_tiled_kernel / wide_dw_tiled_kernel) never launch there, no width is odd (H / 2 of the value MLP rounds at 129 and
255 only), c_in is always 2, no weight-gradient slice has a third 16-row chunk, and nothing runs a stand-alone module backward.  This
file brings the path under the rule of tests/test_gpu_feature_counts.py, with that file's machinery (tests/helpers.py).

Parity rule: ground truth is the oracle in float64, the fp32 oracle gives the yardstick.  max |Q - Q64| <= max(3 x fp32 oracle's,
5e-6), also for out_v and for a stack's y; every gradient tensor ||g - g64|| / ||g64|| <= max(3 x fp32 oracle's own, 2e-3) (absolute
1e-6 when ||g64|| < 1e-6); the same bound for every column k < c_in of layer 0's d_wl / d_wr.  Inputs are chosen from the float64
oracle alone, and every test asserts their conditions again: feature sensitivity > 0.1, layer-0 column share >= 2 %, Q spread >= 0.5,
every |g|max >= 1e-2, no ReLU input within 2^-16 rms of zero; the weight seed is the first below 400 that meets them.

1. Q-network, layer-major path (qnet_hip_call(..., layered=True)), 2 body + 2 head layers, the 196-row batch of
   test_gpu_feature_counts.py.  (hidden, c_in) -> weight seed: (129, 2) 7, (144, 2) 1, (192, 8) 4, (224, 3) 24, (240, 1) 21,
   (255, 2) 10, (256, 2) 8, (160, 4) 1, (176, 5) 8, (208, 7) 55: all eight instantiations of both tiled kernels.  (240, 1) and
   (192, 8) also take x as a 4-byte-aligned view between NaN columns: same bits as dense rows.
2. A 260-node graph (456 rows): wide_head_fwd/bwd_kernel walk a graph's rows with strides 4 and 256, and only a graph above 256 rows
   takes a second trip.  1 body + 2 head layers (with 2 + 2 no seed below 400 meets the ReLU margin at hidden 200 and 256):
   (144, 2) 4, (200, 3) 106, (256, 2) 11, modes 0, 1, 2.
3. Row counts at the edges of the weight-gradient slices, from the plan in wide_stack_backward:
       const int S = kWideSlices, rps = ((n + S - 1) / S + 15) / 16 * 16;                   (kWideSlices = 64)
   n = 1024: 64 full one-chunk slices; 1025: rps 32, slice 32 holds one row, 31 slices empty; 2049: rps 48, three chunks (a buffer is
   written a second time while the other is read), the last live slice ends in a one-row chunk, 21 empty; 3073: rps 64, four chunks;
   15 and 17: one partial chunk / one chunk plus a single-row slice.  One bare SAGEConv(H, H) in the padded layout
   (ops.sage_stack(..., linear_last=True): no ReLU, so no mask can flip at thousands of rows), x ~ U(-1, 1) with requires_grad,
   default init at weight seed 0, a random symmetric graph with about 6 neighbours per row, row n - 1 isolated and row 0 with
   min(300, n - 2) neighbours (a simple graph over 15 or 17 rows has no room for 300).  Loss: scale * sum(y * R) / n, R ~ U(-1, 1).
   With scale = 1 dx of the oracle is ~ 1 / n and cannot reach |g|max >= 1e-2 above a few hundred rows, whatever the seed (dx does
   not depend on x, and R and the init are given); so, as tests/test_gpu_dw_slices.py does, the loss is scaled by the smallest
   power of two (exact in every arithmetic, every relative figure unchanged) at which the ORACLE's four gradients meet 1e-2.
   n = 2049 at hidden 144, 160, 176, 192, 208, 224, 240, 255 (one per HP; 255 pads one zero column); the five others at 240 and 256.
4. HeadNetwork.forward stand-alone with a backward (head modes 3 / 4), hidden 160 and 255: h ~ N(0, 1) [196, H] with requires_grad,
   loss sum(adv * R1) + sum(val * R2); the head of qnet_ref(2, H, 1, 2, seed) at the first seed with the ReLU margin, every
   |g|max >= 1e-2 and, in the oracle, a column of the pooled input whose per-graph minimum is attained by two or more rows (the
   first-index tie routing of the min pool).
5. Scratch independence: cases of 1. and 3. twice under helpers.PoisonedTorch (0xFF / 0x3F in every uint8 buffer of
   gnn_hex_amd.ops): finite and bit-identical.  The wide backward reuses one ``part`` region for the tiled partials, the first
   layer's partials and the column sums, and 51 of its 64 slices are empty on 196 rows.
6. Entry points of a training step at hidden 144 (maker) and 256 (breaker), make_pair(3, H) sharpened, boards [5, 7, 9, 11]:
   ops.td_step (falls back: q._hex_call.td is None), the unmodified loop, ops.double_dqn_targets.

Worst figures measured on the MI355X (printed per case; in brackets the fp32 oracle's own distance from float64 in the same case):

  section                         max |Q - Q64| (or y, adv)   out_v / val            gradient tensor, relative   layer-0 column, relative
  1. widths, strides, (5. qnet)   3.05e-6 (1.63e-6)           3.3e-8  (1.0e-8)       6.65e-6 (8.57e-6)           3.68e-6 (9.13e-7)
  2. 260-node graph               2.33e-6 (1.09e-6)           9.4e-8  (3.5e-8)       4.16e-6 (6.0e-7)            7.31e-7 (4.93e-7)
  3. slice edges, one SAGEConv    1.84e-6 (6.21e-7) [y]       --                     1.69e-7 (2.68e-7)           dx 2.99e-7 (2.12e-7)
  4. stand-alone head             6.98e-7 (5.04e-7) [adv]     6.9e-8  (1.4e-8)       5.69e-7 (3.81e-7)           dh 2.87e-7 (2.03e-7)
  6. td_step                      |td - td64| 9.0e-7          |loss - loss64| 6e-7   1.24e-5 (1.51e-5)           --

The closest any case came to its bound: 0.61 on Q (hidden 256, c_in 2, mode 1: 3.05e-6 of 5e-6); every gradient figure is below
0.01 of its bound.  Of the 176 printed figures 9 lie above three times the fp32 oracle's own and so rest on a floor (2e-3: a layer-0
column at (240, 1) and (224, 3) and gnn.convs.0.lin_l.weight on the 260-node batch, all <= 4.2e-6; 5e-6: out_v 3.3e-8 and val
6.9e-8); the other 167 are within three times the fp32 oracle's own.  Loss scales of section 3: 1 (n 15,
17), 4 (1024, 1025), 8 (2049), 16 (3073).  Weight seeds: 1. and 2. above; 4. hidden 160 -> 5, 255 -> 0; 6. hidden 144 -> 9,
256 -> 0.  The seeds of (160, 4), (176, 5) and (208, 7) are 1, 8 and 55.

Against libraries with one value-only change in wide.hip (built aside, never committed; tests/test_gpu_wide.py passes on all three):
  (a) wide_dw_tiled_kernel stages the prefetched chunk into the buffer being read (stage(buf ^ 1) -> stage(buf)): the 12 slice-edge
      cases with n > 1024 and both single-conv scratch cases fail, nothing else;
  (b) wide_head_fwd_kernel adds v0_b[k - 1] to the value MLP's last hidden unit when H is odd: hidden 129 in modes 0 and 1 (also
      under the scratch fills) and hidden 255 fail, nothing else (mode 2 has no value MLP);
  (c) wide_pack_kernel drops the feature columns >= 2 (q < a.c_in -> q < 2): all 9 cases with c_in >= 3 fail, nothing else.

wide_gemm_kernel (the untiled GEMM) is not tested: gemm() falls through to it only for HP / 16 outside 9..16, and the dispatch
sends only hidden > 128 here.
"""
import copy

import numpy as np
import pytest
import torch

from helpers import (MARGIN, SEEDS, PoisonedTorch, QnetCases, abs_bound, batch_tensors, check_grads, make_pair, model_args, qnet_ref,
                     rel_bound, same_bits, sel_and_targets, sharpen_, stack_params, stack_run)

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 3, 17, 40, 128, 5]
LONG = SIZES + [260]
_s1 = QnetCases(SIZES, 2, 2)
_s2 = QnetCases(LONG, 1, 2)


@pytest.fixture(autouse=True)
def _fp32():
    from gnn_hex_amd import ops
    ops.set_fused(True)
    ops.set_math("fp32")
    yield
    ops.set_fused(True)
    ops.set_math("fp32")


def _refused(c_in, hidden):
    from gnn_hex_amd import _lib
    assert _lib.lib().hexgnn_qnet_supported(c_in, hidden, 128) == 0, "the fused kernels took hidden %d" % hidden


# ---- 1. every padded width on the layer-major Q-network path ------------------------------------------------------------------

WIDTHS = [(129, 2, m) for m in (0, 1, 2)] + [(144, 2, 0), (192, 8, 0), (224, 3, 0)] + [(240, 1, m) for m in (0, 1, 2)] + \
         [(255, 2, 0)] + [(256, 2, m) for m in (0, 1, 2)] + [(160, 4, 0), (176, 5, 0), (208, 7, 0)]


@pytest.mark.parametrize("hidden,c_in,mode", WIDTHS, ids=["h%d-c%d-m%d" % t for t in WIDTHS])
def test_every_padded_width(hidden, c_in, mode):
    _refused(c_in, hidden)
    o, (q, out_v, grads) = _s1.run_case(c_in, hidden, mode, True)
    _s1.check("width hidden %d c_in %d mode %d" % (hidden, c_in, mode), o, q, out_v, grads, c_in, mode, False)


@pytest.mark.parametrize("hidden,c_in", [(240, 1), (192, 8)])
def test_row_stride_above_c_in(hidden, c_in):
    """x as the view buf[:, 1:1+c_in] of a [n, c_in+3] buffer whose other columns are NaN: within the bounds, the bits of dense rows."""
    _refused(c_in, hidden)
    xd = _s1.dev(c_in)[0]
    dense = xd.contiguous()
    buf = torch.full((xd.shape[0], c_in + 3), float("nan"), device="cuda")
    buf[:, 1:1 + c_in] = xd
    view = buf[:, 1:1 + c_in]
    assert dense.stride() == (c_in, 1) and view.stride() == (c_in + 3, 1) and view.data_ptr() % 16 == 4
    res = {}
    for name, xin in (("dense", dense), ("view", view)):
        o, res[name] = _s1.run_case(c_in, hidden, 0, True, x=xin)
        _s1.check("layout %s hidden %d c_in %d" % (name, hidden, c_in), o, res[name][0], None, res[name][2], c_in, 0, False)
    assert torch.equal(view, xd) and bool(torch.isnan(buf[:, 0]).all()) and bool(torch.isnan(buf[:, 1 + c_in:]).all())
    same_bits("layout hidden %d c_in %d" % (hidden, c_in), res["dense"], res["view"])


# ---- 2. a graph longer than 256 rows through the head kernels -------------------------------------------------------------------

LONG_CASES = [(h, c, m) for h, c in ((144, 2), (200, 3), (256, 2)) for m in (0, 1, 2)]


@pytest.mark.parametrize("hidden,c_in,mode", LONG_CASES, ids=["h%d-c%d-m%d" % t for t in LONG_CASES])
def test_graph_above_256_rows(hidden, c_in, mode):
    ptr = _s2.batch(c_in)[3]
    assert int((ptr[1:] - ptr[:-1]).max()) == 260 and int(ptr[-1]) == 456
    o, (q, out_v, grads) = _s2.run_case(c_in, hidden, mode, True)
    _s2.check("long hidden %d c_in %d mode %d" % (hidden, c_in, mode), o, q, out_v, grads, c_in, mode, False)


# ---- 3. row counts at the edges of the weight-gradient slices -------------------------------------------------------------------

K_WIDE_SLICES = 64


def _wide_plan(n):
    """(rows per slice, 16-row chunks of a full slice, empty slices, rows of the last live slice): wide.hip's
    ``const int S = kWideSlices, rps = ((n + S - 1) / S + 15) / 16 * 16;``"""
    s = K_WIDE_SLICES
    rps = ((n + s - 1) // s + 15) // 16 * 16
    live = (n + rps - 1) // rps
    return rps, rps // 16, s - live, n - (live - 1) * rps


def test_the_row_counts_sit_where_this_file_says():
    assert _wide_plan(1024) == (16, 1, 0, 16)
    assert _wide_plan(1025) == (32, 2, 31, 1)
    assert _wide_plan(2049) == (48, 3, 21, 33)          # 33 rows: two full chunks and a one-row chunk
    assert _wide_plan(3073) == (64, 4, 15, 1)
    assert _wide_plan(15) == (16, 1, 63, 15) and _wide_plan(17) == (16, 1, 62, 1)


def _slice_graph(n, seed):
    """A random symmetric simple graph over n rows, about 6 neighbours per row; row n - 1 isolated, row 0 with min(300, n - 2)."""
    rng = np.random.default_rng(seed)
    a, b = rng.integers(0, n - 1, 3 * n), rng.integers(0, n - 1, 3 * n)
    hub = 1 + rng.permutation(n - 2)[:min(300, n - 2)]
    a, b = np.concatenate([a, np.zeros_like(hub)]), np.concatenate([b, hub])
    keep = a != b
    lo, hi = np.minimum(a, b)[keep], np.maximum(a, b)[keep]
    pairs = np.unique(np.stack([lo, hi], 1), axis=0)
    src, dst = np.concatenate([pairs[:, 0], pairs[:, 1]]), np.concatenate([pairs[:, 1], pairs[:, 0]])
    perm = rng.permutation(len(src))
    return torch.from_numpy(np.stack([src[perm], dst[perm]]).astype(np.int64))


_slices = {}


def _single_conv(hidden, seed=0):
    from oracle.model_ref import SAGEConvRef
    torch.manual_seed(seed)
    m = torch.nn.Module()
    m.convs, m.norms = torch.nn.ModuleList([SAGEConvRef(hidden, hidden)]), None        # torch's default init
    return m


def _slice_oracle(n, hidden):
    key = (n, hidden)
    if key not in _slices:
        ei = _slice_graph(n, 1000 + n)
        gen = torch.Generator().manual_seed(n + hidden)
        x = torch.rand(n, hidden, generator=gen) * 2 - 1
        r = torch.rand(n, hidden, generator=gen) * 2 - 1
        m = _single_conv(hidden)
        m64 = copy.deepcopy(m).double()
        y64, g64, dx64 = stack_run("single", m64, x.double(), ei, r.double(), True)
        scale = 1.0
        while min(g.abs().max().item() for g in g64 + [dx64]) * scale < 1e-2 and scale < 2.0 ** 20:
            scale *= 2.0
        y64, g64, dx64 = stack_run("single", m64, x.double(), ei, r.double(), True, scale)
        y32, g32, dx32 = stack_run("single", m, x, ei, r, True, scale)
        deg = torch.bincount(ei[1], minlength=n)
        spread, gmax = (y64.max() - y64.min()).item(), min(g.abs().max().item() for g in g64 + [dx64])
        text = "output spread %.3g (>= 0.5), smallest |g|max %.3g (>= 1e-2) at loss scale %g, degree 0 at row n - 1: %s, largest " \
               "degree %d, mean degree %.2f" % (spread, gmax, scale, int(deg[n - 1]) == 0, int(deg.max()), deg.float().mean().item())
        ok = spread >= 0.5 and gmax >= 1e-2 and int(deg[n - 1]) == 0 and int(deg[0]) >= min(300, n - 2)
        print("oracle single conv n %d hidden %d: %s" % (n, hidden, text))
        _slices[key] = dict(m=m, x=x, ei=ei, r=r, scale=scale, ok=ok, text=text, y64=y64, g64=g64, dx64=dx64, y32=y32, g32=g32,
                            dx32=dx32)
    o = _slices[key]
    assert o["ok"], "n %d hidden %d: %s" % (n, hidden, o["text"])
    return o


def _slice_run(o, n, hidden):
    from gnn_hex_amd import ops
    dev = copy.deepcopy(o["m"]).cuda()
    xd = o["x"].cuda().requires_grad_(True)
    gs = ops.GraphStructure(o["ei"].cuda(), n)
    y = ops.sage_stack(xd, gs, hidden, hidden, list(dev.convs), linear_last=True)
    ((y * o["r"].cuda()).sum() * o["scale"] / n).backward()
    torch.cuda.synchronize()
    return y.detach(), [p.grad for p in stack_params(dev)[1]], xd.grad


SLICE_CASES = [(2049, h) for h in (144, 160, 176, 192, 208, 224, 240, 255)] + \
              [(n, h) for n in (1024, 1025, 3073, 15, 17) for h in (240, 256)]


@pytest.mark.parametrize("n,hidden", SLICE_CASES, ids=["n%d-h%d" % t for t in SLICE_CASES])
def test_slice_edges_single_conv(n, hidden):
    o = _slice_oracle(n, hidden)
    y, grads, dx = _slice_run(o, n, hidden)
    tag = "slices n %d hidden %d" % (n, hidden)
    ey = abs_bound(tag, "y", y, o["y32"], o["y64"], 5e-6)
    worst, _ = check_grads(tag, stack_params(o["m"])[0], grads, o["g32"], o["g64"], hidden, first=())
    assert dx is not None and tuple(dx.shape) == (n, hidden)
    edx = rel_bound(tag, "dx", dx, o["dx32"], o["dx64"])
    print("%s (rps %d, %d chunks, %d empty slices, last live slice %d rows): |y-y64| %.3g (oracle32 %.3g); worst gradient tensor %s "
          "rel %.3g (oracle32 %.3g); dx rel %.3g (oracle32 %.3g)" % ((tag,) + _wide_plan(n) + ey + (worst[2], worst[0], worst[1]) + edx))


# ---- 4. stand-alone head with a backward ------------------------------------------------------------------------------------

_heads = {}


def _head_run(head, h, ei, batch, r1, r2, adv_only):
    head.zero_grad(set_to_none=True)
    h = h.detach().clone().requires_grad_(True)
    if adv_only:
        adv, val = head(h, ei, batch, advantages_only=True), None
        loss = (adv * r1).sum()
    else:
        adv, val = head(h, ei, batch)
        loss = (adv * r1).sum() + (val * r2).sum()
    loss.backward()
    grads = {k: (None if p.grad is None else p.grad.detach().clone()) for k, p in head.named_parameters()}
    return adv.detach(), None if val is None else val.detach(), h.grad.detach().clone(), grads


def _head_conditions(head64, h64, ei, batch, r1, r2, adv_only):
    """ReLU margin, |g|max of dh and of every parameter gradient, and rows that tie for a pooled minimum: (ok, text, results)."""
    pre, hooks = [], []
    for conv in head64.gnn.convs:
        hooks.append(conv.register_forward_hook(lambda mod, inp, out: pre.append(out.detach())))
    if not adv_only:
        hooks.append(head64.value_head.layers[0].register_forward_hook(lambda mod, inp, out: pre.append(out.detach())))
    try:
        res = _head_run(head64, h64, ei, batch, r1, r2, adv_only)
    finally:
        for k in hooks:
            k.remove()
    margin = min((t.abs().min() / t.pow(2).mean().sqrt()).item() for t in pre)
    gmax = min([res[2].abs().max().item()] + [g.abs().max().item() for g in res[3].values() if g is not None])
    hx = torch.relu(pre[len(head64.gnn.convs) - 1])                # the pooled input
    ties = 0
    for g in range(int(batch.max()) + 1):
        rows = hx[batch == g]
        ties += int(((rows == rows.min(0, keepdim=True).values).sum(0) >= 2).sum())
    ok = margin >= MARGIN and gmax >= 1e-2 and ties >= 1
    text = "smallest |ReLU input| / rms %.3g (>= 2^-16), smallest |g|max %.3g (>= 1e-2), (graph, column) pairs whose pooled minimum " \
           "is attained by two or more rows: %d (>= 1)" % (margin, gmax, ties)
    return ok, text, res


def _head_oracle(hidden, adv_only):
    if hidden not in _heads:
        x, ei, batch = _s1.batch(2)[:3]
        gen = torch.Generator().manual_seed(1000 + hidden)
        h = torch.randn(x.shape[0], hidden, generator=gen)
        r1 = torch.rand(x.shape[0], 1, generator=gen) * 2 - 1
        r2 = torch.rand(len(SIZES), 1, generator=gen) * 2 - 1
        for seed in range(SEEDS):
            ref = qnet_ref(2, hidden, 1, 2, seed)
            head64 = copy.deepcopy(ref.maker_head).double()
            if all(_head_conditions(head64, h.double(), ei, batch, r1.double(), r2.double(), a)[0] for a in (False, True)):
                break
        else:
            raise AssertionError("hidden %d: no weight seed below %d meets the head conditions" % (hidden, SEEDS))
        _heads[hidden] = dict(ref=ref, seed=seed, h=h, r1=r1, r2=r2)
    ent = _heads[hidden]
    if adv_only not in ent:
        x, ei, batch = _s1.batch(2)[:3]
        head64 = copy.deepcopy(ent["ref"].maker_head).double()
        ok, text, res64 = _head_conditions(head64, ent["h"].double(), ei, batch, ent["r1"].double(), ent["r2"].double(), adv_only)
        res32 = _head_run(copy.deepcopy(ent["ref"].maker_head), ent["h"], ei, batch, ent["r1"], ent["r2"], adv_only)
        print("oracle head hidden %d advantages_only %s: weight seed %d; %s" % (hidden, adv_only, ent["seed"], text))
        ent[adv_only] = dict(ok=ok, text=text, res64=res64, res32=res32)
    o = ent[adv_only]
    assert o["ok"], "head hidden %d advantages_only %s: %s" % (hidden, adv_only, o["text"])
    return ent, o


@pytest.mark.parametrize("adv_only", [False, True], ids=["raw", "advantages_only"])
@pytest.mark.parametrize("hidden", [160, 255])
def test_standalone_head_backward(hidden, adv_only):
    from gnn_hex_amd.models import get_pre_defined
    ent, o = _head_oracle(hidden, adv_only)
    x, ei, batch = _s1.batch(2)[:3]
    hip = get_pre_defined("modern_two_headed", model_args(1, hidden))
    hip.load_state_dict(ent["ref"].state_dict())
    head = hip.cuda().maker_head
    adv, val, dh, grads = _head_run(head, ent["h"].cuda(), ei.cuda(), batch.cuda(), ent["r1"].cuda(), ent["r2"].cuda(), adv_only)
    torch.cuda.synchronize()
    (a64, v64, dh64, g64), (a32, v32, dh32, g32) = o["res64"], o["res32"]
    tag = "head hidden %d advantages_only %s" % (hidden, adv_only)
    assert tuple(adv.shape) == tuple(a64.shape)
    ea = abs_bound(tag, "adv", adv, a32, a64, 5e-6)
    ev = (0.0, 0.0)
    if not adv_only:
        assert tuple(val.shape) == tuple(v64.shape)
        ev = abs_bound(tag, "val", val, v32, v64, 5e-6)
    names = sorted(g64)
    assert sorted(grads) == names
    worst, _ = check_grads(tag, names, [grads[k] for k in names], [g32[k] for k in names], [g64[k] for k in names], 0, first=())
    edh = rel_bound(tag, "dh", dh, dh32, dh64)
    print("%s: |adv-adv64| %.3g (oracle32 %.3g); |val-val64| %.3g (oracle32 %.3g); worst gradient tensor %s rel %.3g (oracle32 %.3g); "
          "dh rel %.3g (oracle32 %.3g)" % ((tag,) + ea + ev + (worst[2], worst[0], worst[1]) + edh))


# ---- 5. scratch independence ------------------------------------------------------------------------------------------------

def _twice_poisoned(monkeypatch, run):
    from gnn_hex_amd import ops
    out = []
    for byte in (0xFF, 0x3F):
        stand_in = PoisonedTorch(byte)
        with monkeypatch.context() as mp:
            mp.setattr(ops, "torch", stand_in)
            out.append(run())
            torch.cuda.synchronize()
        assert stand_in.filled >= 2, "the scratch of this path did not come through ops' torch.empty"
    return out


@pytest.mark.parametrize("hidden,c_in", [(129, 2), (240, 1), (256, 2)])
def test_qnet_results_do_not_depend_on_the_scratch(hidden, c_in, monkeypatch):
    _refused(c_in, hidden)
    a, b = _twice_poisoned(monkeypatch, lambda: _s1.run_case(c_in, hidden, 0, True)[1])
    tag = "scratch hidden %d c_in %d" % (hidden, c_in)
    for t in [a[0]] + [g for g in a[2] if g is not None]:
        assert bool(torch.isfinite(t).all()), "%s: NaN / Inf with 0xFF scratch" % tag
    same_bits(tag, a, b)
    _s1.check(tag, _s1.oracle(c_in, hidden, 0), a[0], None, a[2], c_in, 0, False)


@pytest.mark.parametrize("n", [1025, 2049])
def test_single_conv_results_do_not_depend_on_the_scratch(n, monkeypatch):
    hidden = 240
    o = _slice_oracle(n, hidden)
    a, b = _twice_poisoned(monkeypatch, lambda: _slice_run(o, n, hidden))
    for name, ta, tb in [("y", a[0], b[0]), ("dx", a[2], b[2])] + list(zip(stack_params(o["m"])[0], a[1], b[1])):
        assert bool(torch.isfinite(ta).all()), "n %d %s: NaN / Inf with 0xFF scratch" % (n, name)
        assert torch.equal(ta, tb), "n %d %s: depends on what the scratch held (0xFF vs 0x3F fill)" % (n, name)


# ---- 6. entry points of a training step ---------------------------------------------------------------------------------------

STEP_CASES = [(144, True), (256, False)]
_steps = {}


def _grads(m):
    return {k: p.grad.detach().clone() for k, p in m.named_parameters() if p.grad is not None}


def _step_ref(hidden, seed):
    from oracle.model_ref import get_pre_defined_ref
    torch.manual_seed(seed)
    return sharpen_(get_pre_defined_ref("modern_two_headed", model_args(3, hidden)))


def _step_margin(ref64, x64, ei, bv, ptr, maker):
    pre, hooks = [], []
    head = ref64.maker_head if maker else ref64.breaker_head
    for mod in list(ref64.gnn.convs) + list(head.gnn.convs) + [head.value_head.layers[0]]:
        hooks.append(mod.register_forward_hook(lambda mod, inp, out: pre.append(out.detach())))
    with torch.no_grad():
        ref64(x64, ei, bv, ptr)
    for k in hooks:
        k.remove()
    assert len(pre) == 6
    return min((t.abs().min() / t.pow(2).mean().sqrt()).item() for t in pre)


def _step_setup(hidden, maker):
    """(HIP model, oracle, batch on the CPU, batch on the device) at the first weight seed whose ReLU inputs keep the margin."""
    key = (hidden, maker)
    if key not in _steps:
        x, ei, bv, ptr = batch_tensors("D1", [5, 7, 9, 11], maker=maker)
        for seed in range(SEEDS):
            margin = _step_margin(_step_ref(hidden, seed).double(), x.double(), ei, bv, ptr, maker)
            if margin >= MARGIN:
                break
        else:
            raise AssertionError("hidden %d: no weight seed below %d keeps the ReLU inputs clear of zero" % (hidden, SEEDS))
        print("step hidden %d maker %s: weight seed %d, smallest |ReLU input| / rms %.3g" % (hidden, maker, seed, margin))
        _steps[key] = (seed, margin)
    seed, margin = _steps[key]
    assert margin >= MARGIN
    hip, ref = make_pair(3, hidden, seed=seed)
    sharpen_(ref)
    hip.load_state_dict(ref.state_dict())
    x, ei, bv, ptr = batch_tensors("D1", [5, 7, 9, 11], maker=maker)
    sel, tgt = sel_and_targets(ptr)
    gen = torch.Generator().manual_seed(5)
    w = torch.rand(4, generator=gen) + 0.5
    cpu = (x, ei, bv, ptr, sel, tgt, w)
    return hip, ref, cpu, tuple(t.cuda() for t in cpu)


def _td_oracle(ref, cpu, loss_fn, dtype):
    x, ei, bv, ptr, sel, tgt, w = cpu
    m = copy.deepcopy(ref).to(dtype)
    d = m(x.to(dtype), ei, bv, ptr)[sel] - tgt.to(dtype)
    l = d * d if loss_fn == "mse" else torch.where(d.abs() <= 1, 0.5 * d * d, d.abs() - 0.5)
    loss = (w.to(dtype) * l).mean()
    loss.backward()
    return loss.detach(), d.detach(), {k: (None if p.grad is None else p.grad.detach().clone()) for k, p in m.named_parameters()}


@pytest.mark.parametrize("loss_fn", ["mse", "huber"])
@pytest.mark.parametrize("hidden,maker", STEP_CASES)
def test_td_step_takes_its_fallback(hidden, maker, loss_fn):
    from gnn_hex_amd import ops
    hip, ref, cpu, dev = _step_setup(hidden, maker)
    hip.zero_grad(set_to_none=True)
    loss, td, q = ops.td_step(hip, *dev[:4], sel=dev[4], target=dev[5], weights=dev[6], loss_fn=loss_fn)
    torch.cuda.synchronize()
    assert q._hex_call.td is None, "hidden %d took the fused loss form" % hidden
    g = _grads(hip)
    loss64, td64, g64 = _td_oracle(ref, cpu, loss_fn, torch.float64)
    loss32, td32, g32 = _td_oracle(ref, cpu, loss_fn, torch.float32)
    assert abs(loss.item() - loss64.item()) <= 1e-5 * max(1.0, abs(loss64.item()))
    assert (td.cpu().double() - td64).abs().max().item() <= 1e-5
    tag = "td_step hidden %d maker %s %s" % (hidden, maker, loss_fn)
    names = [k for k in g64 if g64[k] is not None]
    assert sorted(g) == sorted(names)
    worst, _ = check_grads(tag, names, [g[k] for k in names], [g32[k] for k in names], [g64[k] for k in names], 2, first=(0, 2))
    print("%s: |loss-loss64| %.3g, |td-td64| %.3g, worst gradient tensor %s rel %.3g (oracle32 %.3g); smallest |g64|max %.3g"
          % (tag, abs(loss.item() - loss64.item()), (td.cpu().double() - td64).abs().max().item(), worst[2], worst[0], worst[1],
             min(g64[k].abs().max().item() for k in names)))


@pytest.mark.parametrize("hidden,maker", STEP_CASES)
def test_unmodified_loop_has_the_bits_of_td_loss_and_backward(hidden, maker):
    from gnn_hex_amd import ops
    hip, _, _, dev = _step_setup(hidden, maker)
    hip.zero_grad(set_to_none=True)
    q = hip(*dev[:4])
    loss0, _ = ops.td_loss(q, dev[4], dev[5])
    ops.backward(loss0)
    g0 = _grads(hip)
    hip.zero_grad(set_to_none=True)
    q = hip(*dev[:4])
    loss = torch.nn.functional.mse_loss(q[dev[4]], dev[5])
    loss.backward()
    torch.cuda.synchronize()
    g = _grads(hip)
    assert torch.equal(loss.detach(), loss0.detach())
    assert g.keys() == g0.keys() and len(g0) > 0
    for k in g0:
        assert bool(torch.isfinite(g[k]).all()) and torch.equal(g[k], g0[k]), k


@pytest.mark.parametrize("hidden,maker", STEP_CASES)
def test_double_dqn_targets_have_the_bits_of_the_plain_sequence(hidden, maker):
    from gnn_hex_amd import ops
    online, _, _, dev = _step_setup(hidden, maker)
    target, ref_t = make_pair(3, hidden, seed=_steps[(hidden, maker)][0] + 1)
    target.load_state_dict(sharpen_(ref_t).state_dict())
    gamma_n = 0.99 ** 3
    r = torch.linspace(-1, 1, 4).cuda()
    d = torch.tensor([False, True, False, False]).cuda()
    assert ops._multi_plan([online, target], *dev[:4]) is None
    with torch.no_grad():
        q_on, q_tg = online(*dev[:4]), target(*dev[:4])
    assert not torch.equal(q_on, q_tg)
    a0 = ops.greedy_nodes(q_on, dev[3])
    y, a2 = ops.double_dqn_targets(online, target, *dev[:4], r, d, gamma_n)
    assert a2.dtype == torch.int64 and torch.equal(a2, a0)
    assert y.dtype == torch.float32 and bool(torch.isfinite(y).all()) and torch.equal(y, r + gamma_n * q_tg[a2] * (~d).float())
