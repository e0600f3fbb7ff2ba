"""Every instantiation of the fused per-graph kernels -- tile counts NT = 1..7 x kernel form x the home of the graph's CSR -- against
the float64 oracle and against each other.

The kernels of qnet_fused_kernels.h are compiled once per column-tile count NT = ceil(hidden / 16), and the same body text runs as
the two-launch forward / backward, the forward with the TD loss in its tail (hexgnn_qnet_forward_td), the one-launch TD step
(qnet_step_kernel<NT>, the top layer handed over in registers) and the job-table forward (qnet_fwd_kernel<NT, 0, JOBS>).  Each is its
own code object; "the same text passed at another NT" says little about one nobody ran.

Widths: 13, 29, 45, 61, 77, 80, 93, 96, 112 -- one per NT, two (one padded, one full-tile) for NT 5 and 6, which no other file
takes through the TD tail, the step kernel or the job form; 112 is the largest supported width and has no pad column.
Model: ``modern_two_headed``, 3 body + 2 head layers, ``helpers.sharpen_``.

Batches (``test_gpu_model._random_batch``: directed edges, duplicates, isolated rows):
  edges  graphs of 1, 2, 3, 16, 17, 64, 65, 112, 113, 127, 128 rows (tile and wave edges; 64 | 65 is where the waves 4-7 start to
         own rows), p_edge 0.08;
  dense  128, 40, 100, 128 rows; the 128-row graphs have more than 8192 edges (the global-CSR fallback at EVERY width:
         load_nbrs_global, gather_global_tail, the first layer's global loop), the 100-row graph between 2849 and 8192 (in LDS up to
         NT 6, global at NT 7), the 40-row graph is sparse: LDS and global graphs in one launch;
  cap    four 128-row graphs of exactly cap, cap + 1, cap // 2 and cap + 1000 edges, cap = hexgnn_qnet_csr_capacity(hidden)
         (8192 at NT 1..6, 2848 at NT 7): the last edge count kept in LDS and the first one that is not.
One selected row per graph (``helpers.spread_selection``: every second graph's is its last row, so rows of the upper waves and row
127 are selected), weights ~ U(0.5, 1.5), targets ~ U(-1, 1).

Per (batch, width) the weight seed is the first below 400 at which the float64 oracle alone has no ReLU input within 2^-16 of its
tensor's rms of zero, a Q spread >= 0.5 and |g|max >= 1e-2 in every gradient tensor (``helpers.TdCases``); every test asserts it.

Cases, each asserting the kernel form it ran:
  1. three calls (model, ops.td_loss, ops.backward) in exact fp32 under the float64 rule of ``helpers.QnetCases.check``:
     max |Q - Q64| <= max(3 x the fp32 oracle's, 5e-6), every gradient tensor and both layer-0 columns ||g - g64|| / ||g64|| <=
     max(3 x the fp32 oracle's, 2e-3), the loss by the bound of tests/test_gpu_device_draw.py; status word 0;
  2. ops.td_step with the TD loss in the forward's tail (two launches): the bits of 1 in Q, td, loss and every gradient;
  3. ops.td_step as one launch: the bits of 1; "huber" without weights against its own three calls;
  4. ops.multi_forward([m, m2]): each set has the bits of that model's own forward;
  5. 1 and 2 under f16x3: 2 has the bits of 1; on ``edges`` the float64 rule with 8e-6 on Q; on ``dense`` and ``cap`` the bar of
     test_gpu_model.test_dense_graph_exceeds_lds_csr_capacity (1e-4 on Q, 1e-4 max(1, |g|max) per gradient element, against
     the fp32 oracle) with the float64 distances printed.

Worst figures measured on the MI355X over the nine widths (each test prints its own, the module the worst per form; in brackets
the fp32 oracle's own distance from float64 in the same case).  Cases 2, 3 and 4 are bit-equal to case 1, so the exact-fp32 rows
hold for the TD tail, the one-launch step and the job form as well:

  math, batch      max |Q - Q64|         gradient tensor, relative     layer-0 column, relative
  fp32,  edges     1.77e-6  (1.38e-6)    2.55e-6  (2.25e-6)            3.74e-6  (1.19e-6)
  fp32,  dense     2.22e-6  (9.25e-7)    2.36e-6  (1.90e-6)            1.54e-6  (1.01e-6)
  fp32,  cap       1.59e-6  (1.18e-6)    6.35e-6  (2.65e-6)            1.80e-6  (2.87e-6)
  f16x3, edges     1.64e-6  (1.38e-6)    3.53e-6  (2.13e-6)            1.14e-6  (5.0e-7)
  f16x3, dense     2.36e-6  (1.62e-6)    8.81e-6  (5.94e-6)            (printed only: held to 1e-4 against the fp32 oracle)
  f16x3, cap       1.09e-6  (9.53e-7)    9.38e-6  (4.38e-6)            (printed only)

No Q figure came closer than 0.45 of its bound (the 5e-6 constant everywhere); every gradient figure is below 1 % of its bound,
which is the 2e-3 floor in every case.  f16x3 on the degree-60 graphs stays within 2.2 x the fp32 oracle's own distance from float64.  All 135 tests
pass; no defect was found in any instantiation.

That the file bites -- two libraries with one in-bounds arithmetic change each, run once through this file:
  (i)  ``gather_global_tail`` skips a row's last neighbour (loop bound ``e_abs_e - 1``): 36 fail, 99 pass.  The failures are
       cases 1 and 5 on ``dense`` and ``cap`` at all nine widths (|Q - Q64| 0.024 .. 0.149 against a bound of 5e-6; f16x3 the
       same figures against 1e-4).  Every ``edges`` case passes (no graph leaves LDS), and so do cases 2, 3 and 4 on every batch:
       all forms share the changed gather and stay bit-equal to each other -- only the oracle sees it.
  (ii) the step kernel's backward takes ``cy.idg`` as 1.f: the 27 one-launch cases (case 3, every batch and width) fail with
       "gradient 0 differs" (Q, td and loss are the forward's and stay equal); the other 108 pass.
"""
import functools

import pytest
import torch

from helpers import TdCases, abs_bound, check_grads, csr_capacity, graph_edge_counts, truncated_graphs

pytestmark = pytest.mark.gpu

WIDTHS = [13, 29, 45, 61, 77, 80, 93, 96, 112]
BATCHES = ["edges", "dense", "cap"]
BODY, HEAD = 3, 2
EDGE_SIZES = [1, 2, 3, 16, 17, 64, 65, 112, 113, 127, 128]
DENSE_SIZES, DENSE_P = [128, 40, 100, 128], [0.6, 0.08, 0.6, 0.6]


def _edges():
    from test_gpu_model import _random_batch
    return _random_batch(EDGE_SIZES, seed=11, p_edge=0.08)


def _dense():
    """Four graphs of their own density: each drawn alone, then joined."""
    from test_gpu_model import _random_batch
    xs, eis, bv, ptr = [], [], [], [0]
    for g, (n, p) in enumerate(zip(DENSE_SIZES, DENSE_P)):
        x, ei, _, _ = _random_batch([n], seed=40 + g, p_edge=p)
        xs.append(x)
        eis.append(ei + ptr[-1])
        bv.append(torch.full((n,), g, dtype=torch.long))
        ptr.append(ptr[-1] + n)
    return torch.cat(xs), torch.cat(eis, 1), torch.cat(bv), torch.tensor(ptr, dtype=torch.long)


def _cap_counts(cap):
    return [cap, cap + 1, cap // 2, cap + 1000]


def _cap(cap):
    from test_gpu_model import _random_batch
    return truncated_graphs(_random_batch, 128, _cap_counts(cap), seed=60, p_edge=0.75)


def _batches(name, hidden):
    """(builder, key): ``cap`` is one batch per capacity, not per width."""
    if name == "cap":
        cap = csr_capacity(hidden)
        return functools.partial(_cap, cap), "cap%d" % cap
    return {"edges": _edges, "dense": _dense}[name], name


# what TdCases' search found (first seed below 400 that meets the conditions); evaluated again at every use, searched again if it fails
RECORDED_SEEDS = {
    ("edges", 13): 1, ("edges", 29): 4, ("edges", 45): 4, ("edges", 61): 0, ("edges", 77): 0, ("edges", 80): 24, ("edges", 93): 43, ("edges", 96): 51, ("edges", 112): 44,
    ("dense", 13): 1, ("dense", 29): 5, ("dense", 45): 0, ("dense", 61): 3, ("dense", 77): 6, ("dense", 80): 38, ("dense", 93): 5, ("dense", 96): 3, ("dense", 112): 79,
    ("cap8192", 13): 3, ("cap8192", 29): 0, ("cap8192", 45): 6, ("cap8192", 61): 5, ("cap8192", 77): 10, ("cap8192", 80): 0, ("cap8192", 93): 53, ("cap8192", 96): 65,
    ("cap2848", 112): 11,
}
_cases = TdCases(BODY, HEAD, _batches, RECORDED_SEEDS)
_figures = {}


@pytest.fixture(autouse=True)
def _switches():
    from gnn_hex_amd import ops
    ops.set_fused(True)
    ops.set_math("fp32")
    ops.set_one_launch_step(True)
    yield
    ops.set_fused(True)
    ops.set_math("fp32")
    ops.set_one_launch_step(True)


@pytest.fixture(scope="module", autouse=True)
def _summary():
    yield
    for (form, quantity), (e, e32, close) in sorted(_figures.items()):
        print("worst %-12s %-22s %.3g (%.3g); closest to its bound %.3g" % (form, quantity, e, e32, close))


def _note(form, quantity, e, e32, floor):
    ent = _figures.setdefault((form, quantity), [0.0, 0.0, 0.0])
    if e >= ent[0]:
        ent[0], ent[1] = e, e32
    ent[2] = max(ent[2], e / max(3.0 * e32, floor))


@functools.lru_cache(maxsize=None)
def _model(name, hidden, other=False):
    """The HIP model of a case at its oracle's weights; ``other``: the same shape at another seed (the job form's second set)."""
    o = _cases.oracle(name, hidden)
    hip = _cases.hip(_cases.ref(hidden, o["seed"] + 1000) if other else o["ref"], hidden)
    assert [k for k, _ in hip.named_parameters()] == o["names"]
    return hip


@functools.lru_cache(maxsize=None)
def _dev(name, hidden):
    return tuple(t.cuda() for t in _cases.oracle(name, hidden)["inputs"])


def _bits(t):
    return t.contiguous().reshape(-1).view(torch.int32)


def _result(hip, loss, td, q, call):
    """Everything a comparison looks at, cloned; the status word is read and cleared."""
    torch.cuda.synchronize()
    status = int(call.gs.status.item())
    call.gs.status.zero_()
    return dict(loss=loss.detach().clone(), td=td.detach().clone(), q=q.detach().reshape(-1).clone(), status=status,
                grads=[None if p.grad is None else p.grad.detach().clone() for p in hip.parameters()])


def _three_calls(name, hidden, loss_fn="mse", weighted=True):
    from gnn_hex_amd import ops
    hip = _model(name, hidden)
    x, ei, bv, ptr, sel, tgt, w = _dev(name, hidden)
    hip.zero_grad(set_to_none=True)
    q = hip(x, ei, bv, ptr)
    call = hip.__dict__.get("_fca")
    assert isinstance(call, ops._QNetCall) and not call.layered and call.td is None, "the batch did not take the fused kernels"
    assert call.math == (1 if ops.get_math() == "f16x3" else 0)
    loss, td = ops.td_loss(q, sel, tgt, w if weighted else None, loss_fn)
    ops.backward(loss)
    return _result(hip, loss, td, q, call)


def _td_step(name, hidden, one_launch, loss_fn="mse", weighted=True):
    from gnn_hex_amd import ops
    hip = _model(name, hidden)
    x, ei, bv, ptr, sel, tgt, w = _dev(name, hidden)
    ops.set_one_launch_step(one_launch)
    hip.zero_grad(set_to_none=True)
    loss, td, q = ops.td_step(hip, x, ei, bv, ptr, sel=sel, target=tgt, weights=w if weighted else None, loss_fn=loss_fn)
    call = q._hex_call
    assert isinstance(call, ops._QNetCall) and not call.layered and call.td is not None, "the TD tail did not run"
    if one_launch:
        assert call.step_ws is True, "the step did not take the one launch"
    else:
        assert call.step_ws is None, "the step took the one launch"
    return _result(hip, loss, td, q, call)


@functools.lru_cache(maxsize=None)
def _baseline(name, hidden, math):
    """Case 1's result in one math mode, once per session (the callers set the mode; it is part of the key)."""
    from gnn_hex_amd import ops
    assert ops.get_math() == math
    return _three_calls(name, hidden)


def _same(tag, a, b):
    for k in ("loss", "td", "q"):
        assert a[k].shape == b[k].shape and torch.equal(_bits(a[k]), _bits(b[k])), "%s: %s differs" % (tag, k)
    assert a["status"] == b["status"] == 0, "%s: status %s and %s" % (tag, a["status"], b["status"])
    assert len(a["grads"]) == len(b["grads"]) and any(g is not None for g in a["grads"])
    for i, (ga, gb) in enumerate(zip(a["grads"], b["grads"])):
        assert (ga is None) == (gb is None) and (ga is None or torch.equal(_bits(ga), _bits(gb))), "%s: gradient %d differs" % (tag, i)


def _float64_rule(tag, form, o, res, const):
    r32, r64 = o["r32"], o["r64"]
    assert res["status"] == 0, "%s: status %d" % (tag, res["status"])
    eq = abs_bound(tag, "Q", res["q"], r32["q"], r64["q"], const)
    names = o["names"]
    assert names[0].endswith("convs.0.lin_l.weight") and names[2].endswith("convs.0.lin_r.weight")
    worst, worst_col = check_grads(tag, names, res["grads"], r32["grads"], r64["grads"], 2)
    l, l32, l64 = res["loss"].item(), r32["loss"].item(), r64["loss"].item()
    print("%s: |Q-Q64| %.3g (oracle32 %.3g); worst gradient tensor %s rel %.3g (oracle32 %.3g); worst layer-0 column %s rel %.3g "
          "(oracle32 %.3g); |loss-loss64| %.3g (oracle32 %.3g)" % (tag, eq[0], eq[1], worst[2], worst[0], worst[1], worst_col[2],
                                                                  worst_col[0], worst_col[1], abs(l - l64), abs(l32 - l64)))
    assert abs(l - l64) <= max(3 * abs(l32 - l64), 1e-5 * max(1.0, abs(l64))), "%s: loss %.9g, float64 %.9g" % (tag, l, l64)
    _note(form, "max |Q - Q64|", eq[0], eq[1], const)
    _note(form, "gradient tensor, rel", worst[0], worst[1], 2e-3)
    _note(form, "layer-0 column, rel", worst_col[0], worst_col[1], 2e-3)


def _float64_distances(tag, o, res):
    """Printed only: (max |Q - Q64|, worst relative gradient-tensor distance) and the fp32 oracle's own."""
    r32, r64 = o["r32"], o["r64"]
    dist = lambda q, g: ((q.cpu().double() - r64["q"]).abs().max().item(),                                      # noqa: E731
                         max(((a.cpu().double() - c).norm() / c.norm()).item() for a, c in zip(g, r64["grads"]) if c is not None))
    d, d32 = dist(res["q"], res["grads"]), dist(r32["q"], r32["grads"])
    print("%s: |Q-Q64| %.3g (oracle32 %.3g); worst gradient tensor rel %.3g (oracle32 %.3g)" % (tag, d[0], d32[0], d[1], d32[1]))
    return d, d32


def _check_batch(name, hidden, o):
    """What the batch is there for, asserted on the batch itself."""
    x, ei, bv, ptr = o["inputs"][:4]
    sizes, edges = (ptr[1:] - ptr[:-1]).tolist(), graph_edge_counts(ei, ptr)
    cap = csr_capacity(hidden)
    last = ((o["inputs"][4] - ptr[:-1]) == (ptr[1:] - ptr[:-1]) - 1).tolist()
    assert all(last[0::2]) and max(sizes) == 128
    if name == "edges":
        assert sizes == EDGE_SIZES and max(edges) <= cap
        assert (o["inputs"][4] - ptr[:-1]).tolist()[10] == 127 and int(torch.bincount(ei[1]).max()) > 16
    elif name == "dense":
        assert sizes == DENSE_SIZES and edges[0] > 8192 and edges[3] > 8192 and 2849 <= edges[2] <= 8192 and edges[1] <= 2848
        assert (o["inputs"][4] - ptr[:-1]).tolist()[0] == 127
        assert any(e > cap for e in edges) and any(e <= cap for e in edges)
    else:
        assert sizes == [128] * 4 and edges == _cap_counts(cap)


@pytest.mark.parametrize("hidden", WIDTHS)
@pytest.mark.parametrize("name", BATCHES)
def test_three_calls_meet_the_float64_rule(name, hidden):
    o = _cases.oracle(name, hidden)
    _check_batch(name, hidden, o)
    _float64_rule("%s hidden %d three calls" % (name, hidden), "fp32 " + name, o, _baseline(name, hidden, "fp32"), 5e-6)


@pytest.mark.parametrize("hidden", WIDTHS)
@pytest.mark.parametrize("name", BATCHES)
def test_td_tail_has_the_bits_of_three_calls(name, hidden):
    _cases.oracle(name, hidden)
    _same("%s hidden %d TD tail" % (name, hidden), _td_step(name, hidden, False), _baseline(name, hidden, "fp32"))


@pytest.mark.parametrize("hidden", WIDTHS)
@pytest.mark.parametrize("name", BATCHES)
def test_one_launch_has_the_bits_of_three_calls(name, hidden):
    _cases.oracle(name, hidden)
    _same("%s hidden %d one launch" % (name, hidden), _td_step(name, hidden, True), _baseline(name, hidden, "fp32"))
    _same("%s hidden %d one launch, huber" % (name, hidden), _td_step(name, hidden, True, "huber", False),
          _three_calls(name, hidden, "huber", False))


@pytest.mark.parametrize("hidden", WIDTHS)
@pytest.mark.parametrize("name", BATCHES)
def test_job_form_has_the_bits_of_each_forward(name, hidden):
    from gnn_hex_amd import ops
    _cases.oracle(name, hidden)
    models = [_model(name, hidden), _model(name, hidden, True)]
    x, ei, bv, ptr = _dev(name, hidden)[:4]
    with torch.no_grad():
        plain = [m(x, ei, bv, ptr).detach().reshape(-1).clone() for m in models]
    for m in models:
        call = m.__dict__.get("_fca")
        assert isinstance(call, ops._QNetCall) and not call.layered
    assert ops._multi_plan(models, x, ei, bv, ptr) is not None, "the job form does not apply"
    multi = ops.multi_forward(models, x, ei, bv, ptr)
    torch.cuda.synchronize()
    assert len(multi) == 2 and not torch.equal(plain[0], plain[1])
    for k in (0, 1):
        assert multi[k].shape == plain[k].shape and torch.equal(_bits(multi[k]), _bits(plain[k])), (name, hidden, k)
    assert torch.equal(_bits(plain[0]), _bits(_baseline(name, hidden, "fp32")["q"]))


@pytest.mark.parametrize("hidden", WIDTHS)
@pytest.mark.parametrize("name", BATCHES)
def test_f16x3_three_calls_and_td_tail(name, hidden):
    from gnn_hex_amd import ops
    o = _cases.oracle(name, hidden)
    ops.set_math("f16x3")
    base = _baseline(name, hidden, "f16x3")
    tag = "%s hidden %d f16x3" % (name, hidden)
    _same(tag + " TD tail", _td_step(name, hidden, False), base)
    if name == "edges":
        _float64_rule(tag, "f16x3 edges", o, base, 8e-6)
        return
    # nobody has measured f16x3 under the float64 rule on degree-60 graphs: the project's bar for them, against the fp32 oracle
    r32 = o["r32"]
    assert base["status"] == 0, "%s: status %d" % (tag, base["status"])
    d, d32 = _float64_distances(tag, o, base)
    _note("f16x3 " + name, "max |Q - Q64| (printed)", d[0], d32[0], 1e-4)
    _note("f16x3 " + name, "gradient tensor, rel (printed)", d[1], d32[1], 1.0)
    assert torch.isfinite(base["q"]).all()
    err = (base["q"].cpu() - r32["q"]).abs().max().item()
    assert err < 1e-4, "%s: Q max abs err %g" % (tag, err)
    for nm, g, g32 in zip(o["names"], base["grads"], r32["grads"]):
        assert (g is None) == (g32 is None), nm
        if g is not None:
            gerr, scale = (g.cpu() - g32).abs().max().item(), max(1.0, g32.abs().max().item())
            assert torch.isfinite(g).all() and gerr < 1e-4 * scale, "%s: %s max abs err %g (scale %g)" % (tag, nm, gerr, scale)
