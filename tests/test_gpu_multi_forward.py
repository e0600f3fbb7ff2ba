"""GPU: several networks over one batch in ONE forward launch (ops.multi_forward), its device-built job table
(ops.forward_jobs) and the double-DQN targets formed from it (ops.double_dqn_targets).

* every set's Q is bit-equal to that model's ordinary forward -- at every tile count the kernel has a path for (hidden 16 / 24 /
  35 / 110 = 1 / 2 / 3 / 7 column tiles; 2 = the drained-MFMA path), on batches that mix graphs of at most 64 rows (spare
  waves move the weights) with larger ones, with more jobs than the device has CUs, for both heads and both ways a CSR arrives;
* and within the project's bar of the CPU oracle (1e-4; 1e-5 of the float64 oracle in the sharpened state);
* the job table is the stable descending sort of the graph sizes, expanded by the number of sets;
* targets and argmax are bit-equal to greedy_nodes + the torch expression on the ordinary forwards (never compared with the
  oracle: a near-tie in the argmax may flip between fp32 and fp64);
* where the fused form does not apply, the call returns what the plain sequence returns."""
import copy
import functools

import numpy as np
import pytest
import torch

from helpers import batch_tensors, make_pair, sharpen_

pytestmark = pytest.mark.gpu

MIXED = [5, 7, 8, 11, 6, 9]
GAMMA_N = 0.99 ** 3
# (body layers, hidden, graphs): 3 / 7 / 2 / 1 column tiles
SHAPES = {"h35": (3, 35, 37), "h110": (15, 110, 24), "h24": (3, 24, 37), "h16": (3, 16, 37)}


def _sizes(b):
    return (MIXED * (b // len(MIXED) + 1))[:b]


@functools.lru_cache(maxsize=None)
def _pairs(layers, hidden, sharp=False):
    """Two (HIP model, CPU oracle) pairs with different weights (seeds 11, 12)."""
    out = []
    for seed in (11, 12):
        hip, ref = make_pair(layers, hidden, seed=seed)
        if sharp:
            sharpen_(ref)
            hip.load_state_dict(ref.state_dict())
        out.append((hip, ref))
    return out


@functools.lru_cache(maxsize=None)
def _batch(kind, sizes, maker=True):
    cpu = batch_tensors(kind, list(sizes), maker=maker)
    return cpu, tuple(t.cuda() for t in cpu)


def _plain(models, dev):
    with torch.no_grad():
        return [m(*dev) for m in models]


@functools.lru_cache(maxsize=None)
def _case(name):
    layers, hidden, b = SHAPES[name]
    from gnn_hex_amd import ops
    pairs = _pairs(layers, hidden)
    models = [p[0] for p in pairs]
    cpu, dev = _batch("D1", tuple(_sizes(b)))
    plain = _plain(models, dev)
    multi2 = ops.multi_forward(models, *dev)
    multi1 = ops.multi_forward(models[1:], *dev)
    torch.cuda.synchronize()
    with torch.no_grad():
        oracle = [p[1](*cpu) for p in pairs]
    return plain, multi2, multi1, oracle, cpu[3]


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_each_set_has_the_bits_of_its_own_forward(name):
    plain, multi2, multi1, _, ptr = _case(name)
    sizes = np.diff(ptr.numpy())
    assert sizes.min() <= 64 < sizes.max() <= 128          # spare-wave graphs and full ones in one launch
    assert len(multi2) == 2 and len(multi1) == 1
    assert not torch.equal(plain[0], plain[1])              # the two sets do differ
    for k in (0, 1):
        assert multi2[k].shape == plain[k].shape and torch.equal(multi2[k], plain[k]), (name, k)
    assert torch.equal(multi1[0], plain[1])


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_each_set_against_the_cpu_oracle(name):
    _, multi2, _, oracle, _ = _case(name)
    for k in (0, 1):
        err = (multi2[k].cpu() - oracle[k]).abs().max().item()
        print("%s set %d: max abs err vs oracle %.3g" % (name, k, err))
        assert err <= 1e-4, (name, k, err)


def test_sharpened_state_against_the_float64_oracle():
    from gnn_hex_amd import ops
    pairs = _pairs(3, 35, sharp=True)
    cpu, dev = _batch("D1", tuple(_sizes(37)))
    qs = ops.multi_forward([p[0] for p in pairs], *dev)
    for k, (_, ref) in enumerate(pairs):
        with torch.no_grad():
            q64 = copy.deepcopy(ref).double()(cpu[0].double(), *cpu[1:])
        assert float(q64.max() - q64.min()) > 0.5          # Q is not flat in this state
        err = (qs[k].cpu().double() - q64).abs().max().item()
        print("sharpened set %d: max abs err vs float64 oracle %.3g" % (k, err))
        assert err <= 1e-5, (k, err)


@pytest.mark.parametrize("what", ["b1", "b300", "breaker"])
def test_bit_equality_on_other_batches(what):
    from gnn_hex_amd import ops
    models = [p[0] for p in _pairs(3, 35)]
    if what == "b1":
        _, dev = _batch("D1", (9,))
    elif what == "b300":          # 600 jobs on 256 CUs: a second round of dispatch
        _, dev = _batch("D1", tuple(([5, 6, 7] * 100)))
    else:
        _, dev = _batch("D1", tuple(_sizes(37)), False)
    plain = _plain(models, dev)
    multi = ops.multi_forward(models, *dev)
    for k in (0, 1):
        assert torch.equal(multi[k], plain[k]), (what, k)


def test_csr_from_the_env_manager_and_from_the_grouped_build():
    from gnn_hex_amd import ops
    from gnn_hex_amd.multi_env_manager import Env_manager
    models = [p[0] for p in _pairs(3, 35)]
    mgr = Env_manager(24, 7)
    rng = np.random.default_rng(0)
    obs = mgr.reset()
    for _ in range(5):
        obs, _, _, _ = mgr.step([int(v[rng.integers(len(v))]) for v in mgr.get_valid_actions()])
    bt = obs.to_batch()
    assert bt.edge_index._hex_csr is not None and bt.edge_index._hex_csr.n == bt.x.shape[0]
    args = (bt.x, bt.edge_index, bt.batch, bt.ptr)
    plain = _plain(models, args)
    multi = ops.multi_forward(models, *args)
    for k in (0, 1):
        assert torch.equal(multi[k], plain[k]), k
    # a collated batch (edges grouped by graph, int64 ptr, size hints): the one-launch build
    _, dev = _batch("D1", tuple(_sizes(37)))
    x, ei = dev[0].clone(), dev[1].clone()
    ops.attach_hints(x, True, int(np.diff(dev[3].cpu().numpy()).max()))
    ei._hex_grouped = True
    plain = _plain(models, (x, ei, dev[2], dev[3]))
    multi = ops.multi_forward(models, x, ei, dev[2], dev[3])
    for k in (0, 1):
        assert torch.equal(multi[k], plain[k]), k


@pytest.mark.parametrize("kind,sizes", [("D1", tuple(_sizes(37))), ("D0", (7,) * 9), ("D1", (9,)), ("D1", tuple([5, 6, 7] * 100))],
                         ids=["mixed", "equal", "b1", "b300"])
@pytest.mark.parametrize("k", [1, 2, 4])
def test_job_table_is_the_stable_descending_sort(kind, sizes, k):
    from gnn_hex_amd import ops
    cpu, dev = _batch(kind, sizes)
    nodes = np.diff(cpu[3].numpy())
    jobs = ops.forward_jobs(dev[3], k).cpu().numpy()
    order = np.argsort(-nodes, kind="stable")
    want = (np.repeat(order, k) << 2) | np.tile(np.arange(k), len(order))
    assert jobs.dtype == np.int32 and np.array_equal(jobs, want)
    g, s = jobs >> 2, jobs & 3
    assert sorted(zip(g.tolist(), s.tolist())) == [(a, c) for a in range(len(nodes)) for c in range(k)]     # a permutation
    sz = nodes[g]
    assert np.all(sz[:-1] >= sz[1:])
    first = g[::k]
    assert all(first[i] < first[i + 1] for i in range(len(first) - 1) if nodes[first[i]] == nodes[first[i + 1]])
    if kind == "D0":              # start boards of one size: all node counts equal, the identity order
        assert len(set(nodes.tolist())) == 1 and np.array_equal(first, np.arange(len(nodes)))
    elif len(nodes) > 1:
        assert len(set(nodes.tolist())) > 1 and not np.array_equal(first, np.arange(len(nodes)))


@pytest.mark.parametrize("done_kind", ["mixed", "all", "none"])
def test_targets_have_the_bits_of_the_plain_sequence(done_kind):
    from gnn_hex_amd import ops
    online, target = [p[0] for p in _pairs(3, 35, sharp=True)]
    _, dev = _batch("D1", tuple(_sizes(37)))
    b = 37
    gen = torch.Generator().manual_seed(5)
    r = (torch.rand(b, generator=gen) * 2 - 1).cuda()
    d = {"mixed": torch.rand(b, generator=gen) < 0.4, "all": torch.ones(b, dtype=torch.bool),
         "none": torch.zeros(b, dtype=torch.bool)}[done_kind].cuda()
    q_on, q_tg = _plain([online, target], dev)
    y, a2 = ops.double_dqn_targets(online, target, *dev, r, d, GAMMA_N)
    want_a2 = ops.greedy_nodes(q_on, dev[3])
    assert a2.dtype == torch.int64 and torch.equal(a2, want_a2)
    assert y.dtype == torch.float32 and torch.equal(y, r + GAMMA_N * q_tg[a2] * (~d).float())
    assert len(set((a2 - dev[3][:-1]).tolist())) > 1            # the argmax is not the same rank everywhere


def test_target_kernel_propagates_nan_like_torch():
    """The C entry point on hand-made Q arrays: an infinite q_val at a done graph is inf * 0 = NaN, as in torch; first maximum
    on ties; the two terminal rows of a graph never win."""
    from gnn_hex_amd import _lib, ops
    ptr = torch.tensor([0, 5, 9, 16], dtype=torch.int32, device="cuda")
    q_sel = torch.tensor([9., 9., 1., 3., 3.,   9., 9., -1., -2.,   0., 0., 0., 0., 0., 0., 7.], device="cuda")
    q_val = torch.tensor([0., 0., 0., 2., 5.,   0., 0., float("inf"), 4.,   0., 0., 0., 0., 0., 0., -float("inf")], device="cuda")
    r = torch.tensor([0.5, -1.0, 0.25], device="cuda")
    d = torch.tensor([False, True, False], device="cuda")
    y = torch.empty(3, device="cuda")
    a2 = torch.empty(3, dtype=torch.int64, device="cuda")
    _lib.check(_lib.lib().hexgnn_dqn_targets(3, ptr.data_ptr(), q_sel.data_ptr(), q_val.data_ptr(), r.data_ptr(),
                                             d.view(torch.uint8).data_ptr(), GAMMA_N, y.data_ptr(), a2.data_ptr(), ops._stream()))
    assert a2.tolist() == [3, 7, 15]
    want = r + GAMMA_N * q_val[a2] * (~d).float()
    assert torch.isnan(want[1]) and want[2] == -float("inf")
    assert torch.equal(torch.isnan(y), torch.isnan(want)) and torch.equal(y[[0, 2]], want[[0, 2]])
    assert torch.equal(y.view(torch.int32)[[0, 2]], want.view(torch.int32)[[0, 2]])


def _tie_cases():
    """Q arrays over graphs of 3, 70, 2 and 140 nodes with exact ties for the maximum among the candidates (rows 2.. of a graph;
    candidate c sits on lane c % 64 of pass c // 64 of the one wave that scans the graph).  The two terminal rows hold a larger
    value still: they must never win."""
    ptr = [0, 3, 73, 75, 215]
    cases = {}

    def make(name, ties70, ties140, base=None):
        q = torch.linspace(-1.0, -0.5, ptr[-1]) if base is None else base.clone()
        for g in range(4):
            q[ptr[g]:ptr[g] + 2] = 9.0
        for r0, ties in ((ptr[1], ties70), (ptr[3], ties140)):
            for c in ties:
                q[r0 + 2 + c] = 1.0
        cases[name] = q

    make("lanes i, i+1", [20, 21], [100, 101])
    make("same lane, a later pass", [2, 66], [7, 71, 135])
    make("the two halves of the wave", [40, 5], [64 + 33, 64 + 2])
    make("a later pass on a lower lane", [67, 10], [130, 9, 70])
    make("every candidate tied", range(68), range(138))
    gen = torch.Generator().manual_seed(9)
    make("few distinct values", [], [], base=torch.randint(0, 3, (ptr[-1],), generator=gen).float())
    return ptr, cases


def test_one_argmax_rule_for_acting_and_targets():
    """ops.greedy_nodes (hexgnn_select_actions) and the a2 of hexgnn_dqn_targets against torch.argmax over each graph's candidates --
    the first maximum -- and against each other; a two-node graph has no candidate: rank -1, i.e. ptr[g] - 1, from both."""
    from gnn_hex_amd import _lib, ops
    ptr_l, cases = _tie_cases()
    ptr = torch.tensor(ptr_l, dtype=torch.int32, device="cuda")
    b = len(ptr_l) - 1
    r = torch.zeros(b, device="cuda")
    d = torch.zeros(b, dtype=torch.uint8, device="cuda")
    for name, q_cpu in cases.items():
        want = [ptr_l[g] + 2 + int(torch.argmax(q_cpu[ptr_l[g] + 2:ptr_l[g + 1]])) if ptr_l[g + 1] - ptr_l[g] > 2 else ptr_l[g] - 1
                for g in range(b)]
        q = q_cpu.cuda()
        y = torch.empty(b, device="cuda")
        a2 = torch.empty(b, dtype=torch.int64, device="cuda")
        _lib.check(_lib.lib().hexgnn_dqn_targets(b, ptr.data_ptr(), q.data_ptr(), q.data_ptr(), r.data_ptr(), d.data_ptr(),
                                                 GAMMA_N, y.data_ptr(), a2.data_ptr(), ops._stream()))
        greedy = ops.greedy_nodes(q, ptr)
        assert greedy.tolist() == want, name
        assert a2.tolist() == want, name
        assert torch.equal(greedy, a2), name
        assert want[2] == ptr_l[2] - 1


def _targets_plain(online, target, dev, r, d):
    from gnn_hex_amd import ops
    q_on, q_tg = _plain([online, target], dev)
    a2 = ops.greedy_nodes(q_on, dev[3])
    return r + GAMMA_N * q_tg[a2] * (~d).float(), a2, q_on, q_tg


@pytest.mark.parametrize("why", ["hex13", "f16x3", "depth"])
def test_fallback_is_taken_and_returns_the_plain_values(why):
    from gnn_hex_amd import ops
    online, target = [p[0] for p in _pairs(3, 16)]
    if why == "hex13":                     # 171-node graphs: beyond the per-graph kernels
        _, dev = _batch("D0", (13, 13, 13))
    else:
        _, dev = _batch("D1", tuple(_sizes(7)))
    if why == "depth":
        target = make_pair(4, 16, seed=12)[0]
    b = int(dev[3].numel()) - 1
    r = torch.linspace(-1, 1, b).cuda()
    d = (torch.arange(b) % 3 == 0).cuda()
    try:
        if why == "f16x3":
            ops.set_math("f16x3")
        assert ops._multi_plan([online, target], *dev) is None
        y0, a0, q_on, q_tg = _targets_plain(online, target, dev, r, d)
        qs = ops.multi_forward([online, target], *dev)
        y, a2 = ops.double_dqn_targets(online, target, *dev, r, d, GAMMA_N)
    finally:
        ops.set_math("fp32")
    assert torch.equal(qs[0], q_on) and torch.equal(qs[1], q_tg)
    assert torch.equal(a2, a0) and torch.equal(y, y0)


def test_bystanders_are_left_alone_and_the_call_repeats_its_bits():
    from gnn_hex_amd import ops
    models = [p[0] for p in _pairs(3, 35)]
    _, dev = _batch("D1", tuple(_sizes(37)))
    for m in models:
        m.zero_grad(set_to_none=True)
    before = [m.__dict__.get("_fca") for m in models]
    first = ops.multi_forward(models, *dev)
    assert ops._multi_plan(models, *dev) is not None            # (the fused form, not the fallback)
    for _ in range(5):
        again = ops.multi_forward(models, *dev)
        assert all(torch.equal(a, f) for a, f in zip(again, first))
    for m, fca in zip(models, before):
        assert all(p.grad is None for p in m.parameters())
        assert m.__dict__.get("_fca") is fca
    with pytest.raises(ValueError):
        ops.multi_forward(models * 3, *dev)
    from gnn_hex_amd._lib import HexGnnError
    with pytest.raises(HexGnnError):
        ops.multi_forward(models, *[t.cpu() for t in dev])
