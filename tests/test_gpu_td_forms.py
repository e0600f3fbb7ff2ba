"""GPU: the four forms of the TD loss give the same bits at the Huber boundary.

The forms: ``ops.td_step`` (the loss formed in the fused forward's tail), ``td_loss`` + ``ops.backward`` (the one-launch forward +
backward kernel), ``td_loss`` + ``loss.backward()`` (forward kernel, then the scatter kernel) and ``td_loss`` under ``no_grad``
(forward kernel alone).  The targets put the TD errors on, just inside and just outside ``|d| = 1`` -- where Huber changes branch and
its derivative's clamp starts to bite -- and at 0.  Nothing here is a recorded value: the references are torch's own fp32
expressions (single multiplications in the kernels' order) and, for the loss, its float64 evaluation."""
import functools

import pytest
import torch

from helpers import batch_tensors, make_pair, sharpen_

pytestmark = pytest.mark.gpu

# board sizes: at most 11 (123 nodes), so that every graph runs on the per-graph kernels and td_step takes its forward-tail form
SIZES = [5, 9, 11, 7, 10, 6]


def _bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@functools.lru_cache(maxsize=None)
def _setup():
    """Model, batch, one selected node per graph, and targets built from one forward's Q (all fp32).  q - (q - 1) rounds, so the
    node of a graph is its first candidate at which the fp32 difference q - target lands where the graph's case wants it; the
    weights are sharpened because a fresh model's Q stay inside one binade per graph (0.5 .. 1), where nextafter(q - 1) moves the
    target by half an ulp of 1 and the difference rounds back to exactly 1 at every node."""
    hip = sharpen_(make_pair(3, 16, seed=7)[0])
    dev = tuple(t.cuda() for t in batch_tensors("D0", SIZES))
    ptr = dev[3].tolist()
    with torch.no_grad():
        q = hip(*dev).detach().float()
    inf = torch.tensor(float("inf"), device="cuda")
    cases = [(lambda v: v - 1, lambda d: d == 1),                                   # on the boundary
             (lambda v: v + 1, lambda d: d == -1),
             (lambda v: v.clone(), lambda d: d == 0),
             (lambda v: v - 3, lambda d: d > 2),                                    # far outside
             (lambda v: torch.nextafter(v - 1, -inf), lambda d: d > 1),             # just outside
             (lambda v: torch.nextafter(v - 1, inf), lambda d: d < 1)]              # just inside
    sel, tgt = [], []
    for g, (target_of, wanted) in enumerate(cases):
        rows = torch.arange(ptr[g] + 2, ptr[g + 1], device="cuda")
        t = target_of(q[rows])
        first = int(torch.nonzero(wanted(q[rows] - t))[0])
        sel.append(rows[first])
        tgt.append(t[first])
    w = (torch.rand(len(SIZES), generator=torch.Generator().manual_seed(3)) + 0.5).cuda()
    return hip, dev, torch.stack(sel), torch.stack(tgt), w


def _grads(m):
    return {k: p.grad.detach().clone() for k, p in m.named_parameters() if p.grad is not None}


@pytest.mark.parametrize("loss_fn", ["mse", "huber"])
def test_td_forms_agree_bitwise_at_the_huber_boundary(loss_fn):
    from gnn_hex_amd import ops
    assert ops.get_math() == "fp32"
    hip, dev, sel, tgt, w = _setup()
    k = len(SIZES)
    forms = {}
    # forward tail
    hip.zero_grad(set_to_none=True)
    loss, td, q = ops.td_step(hip, *dev, sel=sel, target=tgt, weights=w, loss_fn=loss_fn)
    assert q._hex_call.td is not None, "the forward-tail form did not run (fell back to the three calls)"
    forms["td_step"] = (loss.detach().clone(), td.clone(), _grads(hip))
    q0 = q.detach().float().clone()
    # the three calls, both ways through the loss's backward
    for name in ("ops.backward", "loss.backward"):
        hip.zero_grad(set_to_none=True)
        loss, td = ops.td_loss(hip(*dev), sel, tgt, w, loss_fn)
        if name == "ops.backward":
            ops.backward(loss)
        else:
            loss.backward()
        forms[name] = (loss.detach().clone(), td.clone(), _grads(hip))
    with torch.no_grad():
        loss, td = ops.td_loss(q0, sel, tgt, w, loss_fn)
    forms["no_grad"] = (loss.clone(), td.clone(), None)
    torch.cuda.synchronize()

    # td against torch, then every form against the first
    d = q0[sel] - tgt
    assert d[0] == 1 and d[1] == -1 and d[2] == 0 and d[3] > 2 and 1 < d[4] < 1 + 1e-6 and 1 - 1e-6 < d[5] < 1
    ref = forms["td_step"]
    assert ref[2]
    for name, (loss, td, grads) in forms.items():
        print(name, loss.item(), td.tolist())
        assert _bits(td, d), (name, td.tolist(), d.tolist())
        assert _bits(loss, ref[0]), (name, loss.item(), ref[0].item())
        if grads is not None:
            assert grads.keys() == ref[2].keys()
            for key in grads:
                assert _bits(grads[key], ref[2][key]), (name, key)

    # d loss / d q of the standalone kernels: ((1 / k) * w) * dterm(d), single fp32 multiplications in that order
    dterm = 2 * d if loss_fn == "mse" else d.clamp(-1, 1)
    want = torch.zeros_like(q0)
    want[sel] = ((torch.ones((), device="cuda") / k) * w) * dterm
    for name in ("ops.backward", "loss.backward"):
        ql = q0.clone().requires_grad_(True)
        loss, _ = ops.td_loss(ql, sel, tgt, w, loss_fn)
        if name == "ops.backward":
            ops.backward(loss)
        else:
            loss.backward()
        assert _bits(ql.grad, want), (name, ql.grad[sel].tolist(), want[sel].tolist())

    # the loss in float64, within test_td_loss_matches_torch's bound
    d64 = q0[sel].double() - tgt.double()
    l64 = d64 * d64 if loss_fn == "mse" else torch.where(d64.abs() <= 1, 0.5 * d64 * d64, d64.abs() - 0.5)
    ref64 = (w.double() * l64).mean().item()
    assert abs(ref[0].item() - ref64) < 1e-5 * max(1.0, abs(ref64))
