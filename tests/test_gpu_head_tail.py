"""ops.HeadTailFn (head_fwd_kernel / head_bwd_kernel of csrc/head.hip; hidden 144: wide_head_*_kernel of csrc/wide.hip) and
ops.HeadLinearTailFn (head_linear_*_kernel) called directly on inputs this file chooses, under the float64 rule.

Until here the two tails ran only behind whole models, on board-sized graphs (the largest 517 rows) against an absolute 1e-4.  The
reference is the tail as a torch expression (helpers.head_tail_ref: the advantage Linear, oracle.model_ref.scatter_ref pooling --
first-index ties, an empty graph pools to 0 --, MLPRef or the Linear value head, the dueling combine), evaluated on the CPU in float64
and again in fp32 from the same fp32 inputs.  Loss: sum(q * R1) + sum(out_v * R2), R ~ U(-1, 1); the "sel" form keeps R1 on one
row per graph only (the shape of a TD-loss gradient).

Rule (the stand-alone head case of tests/test_gpu_wide_parity.py, same helpers and constants): max |q - q64| and |out_v - v64| <=
max(3 x the fp32 expression's own, 5e-6); dh and every parameter gradient ||g - g64|| / ||g64|| <= max(3 x its own, 2e-3) (absolute
1e-6 where ||g64|| < 1e-6); the value head has no gradient in modes 2 and 4.  Input condition, from the float64 expression alone:
every pre-activation of the value MLP's ReLU is at least 2^-16 of its tensor's rms away from 0; the weight seed is the first below
400 that meets it (tests/test_head_tail_host.py runs the same search without a GPU).  h needs no margin for the pooling: max / min
compare the same fp32 values in all three evaluations.

Batches (helpers.head_sizes): "full" = 30 graphs of 1, 2, 3, 15, 16, 17, 30, 31, 32, 33, 34, 47, 48, 49, 63, 64, 65, 66, 127, 128, 129,
255, 256, 257, 1023, 1024, 1025 and 1300 rows in a shuffled order, an empty graph in the middle and one at the end (6140 rows);
"row1" and "rows1025": one graph.  Families: "randn" h ~ N(0, 1); "ties" h = relu(N(0, 1)) with column 0 constant over every graph,
column 1 at its maximum in exactly two rows of opposite parity, column 2 at its maximum in rows 1021 and 1024 of the graphs above
1024 rows.  Widths 2, 3, 16, 35, 62, 63, 64, 65, 66, 110, 127, 128 and 144 (MLP tail; the Linear tail stops at 128): modes 0 and 3 on
every width, all five modes at 35, 66 and 128, on both families there.

Which case has a different expected value when the kernel gets it wrong:
  * rows past 1024 -- the 1025- and 1300-row graphs of "full" and "rows1025": dh of rows 1024.. is dar(row) * lin_w + the pooled
    part, and d lin_w sums dar * h over them; head_bwd_kernel reads dar of those rows back from global memory in three loops
    (dh rows, and both unrolled steps and the scalar tail of the gradient loop: 1025 ends in the tail, 1300 in a 16-row step).
  * unroll tails -- 30 / 31 / 32 / 33 / 34 rows put phase 0 and phase 1 on either side of ``row + 30 < r1``, 15 / 16 / 17 and 47 / 48 / 49
    of ``row + 14 < r1``; a row dropped or taken twice changes pooled sum / mean (out_v, q in mode 0) and d lin_w; 63..66, 255..257
    sit at the strides 64 and 256 of the per-row loops (q, dh of the last rows).
  * the H / 2 pass edge -- widths 62, 63 (H / 2 = 31), 64, 65 (32), 66 (33), 128 (64): a hidden unit lost at k0 = 32 changes
    out_v and d v0_w / d v0_b / d v1_w of that unit.
  * empty graphs -- graphs 14 and 29 of "full": out_v = MLP(0) (modes 1, 3), d v0_b / d v1_w / d v1_b carry their R2, d v0_w gets
    nothing from them; a kernel that pooled +-inf or divided by 0 would give NaN (abs_bound asserts finite).
  * first-index ties -- test_pooled_gradient_lands_on_the_first_row_of_a_tie on the "ties" family: the maximum of columns 0, 1, 2
    and the minimum 0 of nearly every column are attained by several rows, and dh must carry the max / min part on the FIRST of
    them.  Column 1's first row lies in the odd row phase for even graphs and in the even phase for odd ones, so a merge of the
    two phases that prefers either phase fails.  The rule above cannot see this (one misplaced entry per graph and column is a
    1e-3 share of dh's norm, under the 2e-3 floor); that test states exactly which rows may differ from their neighbours.
  * the mask -- test_mask_is_exact: ``mode | 8`` against where(h > 0, dh, 0) of the unmasked call, bit for bit, on "ties".
Segments past 256 and the swap probe: tests/test_gpu_hexara_kernels.py.

Measured on the MI355X (printed per case).  Per output the case that came closest to its bound; in brackets the fp32 expression's
own distance from float64 in the same case; absolute for q / out_v, relative norm for the gradients:

  output   MLP tail (head.hip)        hidden 144 (wide.hip)      Linear tail
  q        4.31e-7 (7.18e-7)          3.74e-7 (4.39e-7)          4.24e-7 (4.96e-7)
  out_v    5.02e-7 (1.00e-6)          1.75e-7 (1.75e-7)          5.59e-8 (1.23e-7)
  dh       8.77e-8 (8.22e-8)          8.62e-8 (8.70e-8)          1.06e-7 (6.93e-8)
  lin_w    1.10e-6 (5.96e-7)          5.91e-7 (1.31e-6)          1.04e-6 (5.96e-7)
  lin_b    7.12e-6 (2.95e-6)          2.46e-6 (4.44e-6)          4.81e-5 (8.23e-5)  ["sel": the row gradients nearly cancel]
  v0_w     1.32e-6 (5.95e-6)          5.36e-7 (7.20e-7)          val_w 6.19e-7 (4.01e-7)
  v0_b     2.52e-7 (8.34e-7)          1.43e-7 (2.03e-6)          val_b 1.59e-6 (3.70e-7)
  v1_w     3.13e-6 (5.08e-6)          6.47e-7 (1.98e-6)
  v1_b     2.36e-6 (1.34e-6)          1.40e-7 (2.03e-6)

No figure is above 0.1 of its bound (out_v, hidden 66, "ties", mode 3: 5.02e-7 of 5e-6); every gradient is below 0.025 of its.  Of
the 912 figures 43 lie above three times the fp32 expression's own and so rest on a floor, all of them below 0.1 of that floor.
Weight seeds: 0 for every case but (MLP, "full", 35, "ties") and (MLP, "full", 144, "ties"), which take seed 1.

Against libraries with one value-only change in head.hip (built aside, never committed), the failing tests of this file:
  (a) the dh loop of head_bwd_kernel reads s_dar[(row - r0) & 1023] for every row: 59 cases of test_tail_against_float64 (every
      MLP case with a graph above 1024 rows) and the scratch test;
  (b) the 16-row step of the gradient loop sums seven of its eight rows: 54 cases and the scratch test;
  (c) head_fwd_kernel adds v0_b[k & 31]: the 24 MLP cases with a value head at widths 66, 110, 127, 128 (H / 2 > 32), nothing below;
  (d) no ``cnt == 0`` reset of the pooled max / min: 42 cases (every MLP case on "full" with a value head), the scratch test, two
      determinism cases (NaN) and test_mask_is_exact in mode 0;
  (e) the merge of the two row phases takes phase 1 only when strictly greater, and (f) ``>=`` instead of ``>`` in the 32-row step
      of the pooling: test_pooled_gradient_lands_on_the_first_row_of_a_tie at 35 and 128, nothing else;
  (g) the mask keeps ``h >= 0``: the four MLP cases of test_mask_is_exact, nothing else;
  (h) the 16-row step of the pooling loads rows 0, 0, 2, 2, 4, 4, 6, 6 of its eight: 42 cases, the routing test, the scratch test.
"""
import copy

import pytest
import torch

from helpers import (HEAD_MODE_WIDTHS, HEAD_NAMES, HEAD_WIDE, HEAD_WIDTHS, MARGIN, HeadCases, PoisonedTorch, head_dev_run, head_modules,
                     head_ref_run, head_same_bits, rel_bound)

pytestmark = pytest.mark.gpu

_cases = HeadCases()
KINDS = {"mlp": HEAD_WIDTHS + [HEAD_WIDE], "linear": HEAD_WIDTHS}


def _case_list():
    out = []
    for kind, widths in KINDS.items():
        for w in widths:
            for mode in (range(5) if w in HEAD_MODE_WIDTHS else (0, 3)):
                out.append((kind, "full", w, "randn", mode, "dense"))
        for w in HEAD_MODE_WIDTHS:
            out += [(kind, "full", w, "ties", mode, "dense") for mode in range(5)]
            out += [(kind, "full", w, fam, 0, "sel") for fam in ("randn", "ties")]
        for name in ("row1", "rows1025"):
            out += [(kind, name, w, fam, mode, "dense") for w, fam in ((35, "randn"), (128, "ties")) for mode in (0, 3)]
        out += [(kind, name, 3, "randn", 1, "dense") for name in ("row1", "rows1025")]
    out += [("mlp", "rows1025", HEAD_WIDE, "randn", 0, "dense"), ("mlp", "full", HEAD_WIDE, "ties", 1, "dense")]
    return out


CASES = _case_list()


def _id(c):
    return "%s-%s-h%d-%s-m%d-%s" % c


@pytest.mark.parametrize("case", CASES, ids=[_id(c) for c in CASES])
def test_tail_against_float64(case):
    kind, name, hidden, family, mode, loss = case
    o, res = _cases.run(*case)
    _cases.check(_id(case), kind, o, res, mode)


def test_the_batches_are_what_this_file_says():
    inp = _cases.inputs("full", 35, "ties")
    sizes, ptr, h = inp["sizes"], inp["ptr"], inp["h"]
    assert len(sizes) == 30 and sizes[14] == 0 and sizes[29] == 0 and inp["n"] == 6140 and max(sizes) == 1300
    assert abs(float((h == 0).float().mean()) - 0.5) < 0.05
    first_in_odd_phase = first_in_even_phase = 0
    for g, cnt in enumerate(sizes):
        rows = h[int(ptr[g]):int(ptr[g + 1])]
        if cnt == 0:
            continue
        assert float(rows[:, 0].max()) == float(rows[:, 0].min())
        if cnt >= 2:
            top = (rows[:, 1] == rows[:, 1].max()).nonzero().reshape(-1).tolist()
            assert len(top) == 2 and (top[0] + top[1]) % 2 == 1
            first_in_odd_phase += top[0] % 2
            first_in_even_phase += 1 - top[0] % 2
        if cnt > 1024:
            assert (rows[:, 2] == rows[:, 2].max()).nonzero().reshape(-1).tolist() == [1021, 1024]
    assert first_in_odd_phase >= 5 and first_in_even_phase >= 5


# ---- where the pooled part of dh lands ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("hidden", [35, 128, HEAD_WIDE])
def test_pooled_gradient_lands_on_the_first_row_of_a_tie(hidden):
    """Mode 3 with R1 = 0: dh is the pooled part alone, and within a graph every row of a column receives the SAME bits (the
    sum and mean parts) except the first row that attains the column's maximum and the first that attains its minimum.  Under the
    dense loss a max part on the wrong one of two tied rows is a 1e-3 share of dh's norm, below the 2e-3 floor of the rule; here it
    is an exact statement about which rows differ.  The expected rows come from h by torch.argmax over (h == extremum) (first
    index), the float64 expression must show the same pattern, and its max / min parts must not vanish against the common part."""
    o = _cases.oracle("mlp", "full", hidden, "ties", 3)
    inp = o["inp"]
    h, ptr, b = inp["h"], inp["ptr"], inp["b"]
    zero = torch.zeros_like(inp["r1"])
    lin, val = head_modules("mlp", hidden, o["seed"])
    d32_all = head_ref_run(lin, val, h, inp["batch"], b, 3, zero, inp["r2"])["dh"]
    d64_all = head_ref_run(copy.deepcopy(lin).double(), copy.deepcopy(val).double(), h.double(), inp["batch"], b, 3, zero.double(),
                           inp["r2"].double())["dh"]
    res = head_dev_run("mlp", o["ps"], h, ptr.to(torch.int32).cuda(), b, hidden, 3, zero, inp["r2"])
    dh_all = res["dh"].cpu()
    rel_bound("routing hidden %d" % hidden, "dh", dh_all, d32_all, d64_all)
    cols = torch.arange(hidden)
    tied = 0
    for g, cnt in enumerate(inp["sizes"]):
        if cnt < 3:
            continue
        r0 = int(ptr[g])
        hh, d64, dh = h[r0:r0 + cnt], d64_all[r0:r0 + cnt], dh_all[r0:r0 + cnt]
        at_max, at_min = hh == hh.max(0).values, hh == hh.min(0).values
        tied += int((at_max.sum(0) > 1).sum()) + int((at_min.sum(0) > 1).sum())
        special = torch.zeros(cnt, hidden, dtype=torch.bool)
        special[at_max.int().argmax(0), cols] = True               # torch.argmax: the first of several maxima
        special[at_min.int().argmax(0), cols] = True
        plain = (~special).int().argmax(0)                          # a row of every column that holds neither extremum
        base64, base = d64[plain, cols], dh[plain, cols]
        assert torch.equal(d64 != base64, special), "graph %d: the float64 expression routes differently" % g
        assert bool(((d64 - base64).abs() >= MARGIN * base64.abs())[special].all()), "graph %d: a max / min part vanishes" % g
        wrong = (dh != base) != special
        assert not bool(wrong.any()), "graph %d (%d rows): dh differs from the common part in (row, column) %s, expected %s" \
            % (g, cnt, (dh != base).nonzero().tolist()[:6], special.nonzero().tolist()[:6])
    assert tied > 20 * hidden, tied


# ---- scratch independence and determinism ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind,hidden", [("mlp", 66), ("mlp", HEAD_WIDE), ("linear", 66)])
def test_results_do_not_depend_on_the_scratch(kind, hidden, monkeypatch):
    """One full pass with 0xFF in every uint8 buffer of gnn_hex_amd.ops (the saved block and the backward's workspace: NaN as
    floats, -1 as the saved row indices): finite, and the bits of the unpoisoned run."""
    from gnn_hex_amd import ops
    case = (kind, "full", hidden, "ties", 0, "dense")
    o, plain = _cases.run(*case)
    stand_in = PoisonedTorch(0xFF)
    with monkeypatch.context() as mp:
        mp.setattr(ops, "torch", stand_in)
        _, poisoned = _cases.run(*case)
        torch.cuda.synchronize()
    assert stand_in.filled >= 2, "the scratch of this path did not come through ops' torch.empty"
    for t in [poisoned["q"], poisoned["dh"]] + poisoned["grads"]:
        assert bool(torch.isfinite(t).all()), "%s: NaN / Inf with 0xFF scratch" % _id(case)
    head_same_bits(_id(case), plain, poisoned)
    _cases.check(_id(case) + " poisoned", kind, o, poisoned, 0)


DET = [("mlp", 128, 1), ("mlp", 63, 0), ("mlp", HEAD_WIDE, 0), ("linear", 128, 1), ("linear", 35, 3)]


@pytest.mark.parametrize("kind,hidden,mode", DET)
def test_two_runs_give_the_same_bits(kind, hidden, mode):
    case = (kind, "full", hidden, "randn", mode, "dense")
    head_same_bits(_id(case), _cases.run(*case)[1], _cases.run(*case)[1])


# ---- HEXGNN_HEAD_MASK_DH through the C entry points ----------------------------------------------------------------------------

MASK_DH = 8


def _raw_backward(kind, o, hidden, mode, mask):
    """hexgnn_head[_linear]_forward once, then the backward with ``mode`` and with ``mode | 8`` on the SAME saved block:
    ([dh [n, hp], parameter gradients...] unmasked, the same masked, h [n, hp])."""
    from gnn_hex_amd import _lib, ops
    L = _lib.lib()
    inp = o["inp"]
    n, b = inp["n"], inp["b"]
    st = ops._stream()
    hpad = ops.as_padded(inp["h"].cuda(), hidden, trust_pads=False)
    gptr = inp["ptr"].to(torch.int32).cuda()
    ps = [p.cuda().contiguous() for p in o["ps"]]
    dq, dv = o["r1"].cuda(), inp["r2"].cuda()
    q, out_v = torch.empty(n, device="cuda"), torch.empty(b, device="cuda")
    if kind == "mlp":
        saved = torch.empty(L.hexgnn_head_saved_bytes(n, b, hidden), dtype=torch.uint8, device="cuda")
        _lib.check(L.hexgnn_head_forward(n, b, hidden, mode, gptr.data_ptr(), hpad.data_ptr(), *[p.data_ptr() for p in ps],
                                         q.data_ptr(), out_v.data_ptr(), saved.data_ptr(), st), "hexgnn_head_forward")
        ws_bytes = L.hexgnn_head_backward_workspace_bytes(n, b, hidden)
    else:
        saved = torch.empty(L.hexgnn_head_linear_saved_bytes(n, b), dtype=torch.uint8, device="cuda")
        _lib.check(L.hexgnn_head_linear_forward(n, b, hidden, mode, gptr.data_ptr(), hpad.data_ptr(), *[p.data_ptr() for p in ps],
                                                q.data_ptr(), out_v.data_ptr(), saved.data_ptr(), st), "hexgnn_head_linear_forward")
        ws_bytes = L.hexgnn_head_linear_backward_workspace_bytes(n, b, hidden)
    out = []
    for m in (mode, mode | mask):
        dh = torch.full_like(hpad, float("nan"))
        g = [torch.full_like(p, float("nan")) for p in ps]
        ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device="cuda")
        if kind == "mlp":
            rc = L.hexgnn_head_backward(n, b, hidden, m, gptr.data_ptr(), hpad.data_ptr(), ps[0].data_ptr(), ps[2].data_ptr(),
                                        ps[4].data_ptr(), saved.data_ptr(), dq.data_ptr(), dv.data_ptr(), dh.data_ptr(),
                                        *[t.data_ptr() for t in g], ws.data_ptr(), ws_bytes, st)
        else:
            rc = L.hexgnn_head_linear_backward(n, b, hidden, m, gptr.data_ptr(), hpad.data_ptr(), ps[0].data_ptr(), ps[2].data_ptr(),
                                               saved.data_ptr(), dq.data_ptr(), dv.data_ptr(), dh.data_ptr(),
                                               *[t.data_ptr() for t in g], ws.data_ptr(), ws_bytes, st)
        _lib.check(rc, "head backward mode %d" % m)
        torch.cuda.synchronize()
        out.append([dh] + g)
    return out[0], out[1], hpad


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("kind", ["mlp", "linear"])
@pytest.mark.parametrize("hidden", [35, 128])
@pytest.mark.parametrize("mode", [0, 2])
def test_mask_is_exact(kind, hidden, mode):
    """What ops.qnet_backward passes on the layered path: dh * [h > 0] written by the tail itself.  About half of "ties" is exactly
    0 (and the pad columns of width 35 are), so the masked dh differs from the unmasked one in half its entries."""
    o = _cases.oracle(kind, "full", hidden, "ties", mode)
    plain, masked, hpad = _raw_backward(kind, o, hidden, mode, MASK_DH)
    live = len(HEAD_NAMES[kind]) if mode == 0 else 2              # mode 2 writes no value-head gradient
    for t in plain[:1 + live]:
        assert bool(torch.isfinite(t).all())
    want = torch.where(hpad > 0, plain[0], torch.zeros_like(plain[0]))
    assert int((_bits(want) != _bits(plain[0])).sum()) > hpad.numel() // 4
    assert torch.equal(_bits(masked[0]), _bits(want)), "dh of mode | 8 is not where(h > 0, dh, 0)"
    for name, a, m in zip(HEAD_NAMES[kind][:live], plain[1:], masked[1:]):
        assert torch.equal(_bits(a), _bits(m)), "%s differs under mode | 8" % name
    # and the unmasked call is the one the autograd function makes
    res = head_dev_run(kind, o["ps"], o["inp"]["h"], o["inp"]["ptr"].to(torch.int32).cuda(), o["inp"]["b"], hidden, mode, o["r1"],
                       o["inp"]["r2"])
    assert torch.equal(res["dh"], plain[0][:, :hidden])
