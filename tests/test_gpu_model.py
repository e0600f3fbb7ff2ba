"""GPU parity: HIP path (through the C ABI) vs the CPU oracle on the same seeded inputs.

Tolerance: 1e-4 absolute on Q-values and on every parameter gradient (fp32; BASELINE.json north_star);
integer outputs (CSR, graph ptr) bit-exact.
"""
import numpy as np
import pytest
import torch

from helpers import batch_tensors, make_pair, sel_and_targets

pytestmark = pytest.mark.gpu
TOL = 1e-4


@pytest.fixture(params=[(True, "fp32"), (True, "f16x3"), (False, "fp32")], ids=["fused", "fused-f16x3", "layered"],
                autouse=True)
def _all_paths(request):
    """Every parity test runs through the fused per-graph kernels (exact fp32 MFMA and the split-precision f16x3
    math) and through the general layer-major kernels (graphs > 128 nodes or hidden > 112 always take the latter).
    The SAME 1e-4 bar applies to all three."""
    from gnn_hex_amd import ops
    ops.set_fused(request.param[0])
    ops.set_math(request.param[1])
    yield
    ops.set_fused(True)
    ops.set_math("fp32")


def _step(model, x, ei, batch, ptr, sel, tgt, **kw):
    model.zero_grad(set_to_none=True)
    q = model(x, ei, batch, ptr, **kw)
    loss = torch.nn.functional.mse_loss(q[sel], tgt)
    loss.backward()
    return q.detach(), {k: (p.grad.detach().clone() if p.grad is not None else None)
                        for k, p in model.named_parameters()}


def _compare(hip, ref, x, ei, batch, ptr, tol=TOL, grad_norm_rel=None):
    sel, tgt = sel_and_targets(ptr)
    q_ref, g_ref = _step(ref, x, ei, batch, ptr, sel, tgt)
    dev = "cuda"
    q_hip, g_hip = _step(hip, x.to(dev), ei.to(dev), batch.to(dev), ptr.to(dev), sel.to(dev), tgt.to(dev))
    torch.cuda.synchronize()
    assert q_hip.shape == q_ref.shape
    err = (q_hip.cpu() - q_ref).abs().max().item()
    assert err < tol, "Q max abs err %g" % err
    for k in g_ref:
        if g_ref[k] is None:
            assert g_hip[k] is None, "%s: reference grad is None, HIP grad is not" % k
            continue
        assert g_hip[k] is not None, "%s: missing grad" % k
        if grad_norm_rel is not None:      # norm-wise criterion (stress inputs whose summands dwarf the result)
            d = (g_hip[k].cpu() - g_ref[k]).norm().item()
            assert d <= grad_norm_rel * max(1.0, g_ref[k].norm().item()), "%s grad rel norm err %g" % (k, d)
            continue
        gerr = (g_hip[k].cpu() - g_ref[k]).abs().max().item()
        # 1e-4 absolute while the gradient tensor is O(1) (every board-graph case); relative to its largest entry when
        # that exceeds 1 (synthetic dense graphs push pooled sums, hence value-head gradients, into the hundreds)
        scale = max(1.0, g_ref[k].abs().max().item())
        assert gerr < tol * scale, "%s grad max abs err %g (scale %g)" % (k, gerr, scale)
    return err


def test_csr_build_bit_exact():
    from gnn_hex_amd import ops
    x, ei, batch, ptr = batch_tensors("D1", [5, 7, 11, 6, 13, 9])
    n = x.shape[0]
    gs = ops.GraphStructure(ei.cuda(), n)
    torch.cuda.synchronize()
    src, dst = ei[0].numpy(), ei[1].numpy()
    order = np.lexsort((src, dst))
    rowptr = np.zeros(n + 1, dtype=np.int64)
    np.add.at(rowptr, dst + 1, 1)
    rowptr = np.cumsum(rowptr)
    assert np.array_equal(gs.rowptr.cpu().numpy(), rowptr)
    assert np.array_equal(gs.col.cpu().numpy()[: ei.shape[1]], src[order])
    order_t = np.lexsort((dst, src))
    rowptr_t = np.zeros(n + 1, dtype=np.int64)
    np.add.at(rowptr_t, src + 1, 1)
    assert np.array_equal(gs.rowptr_t.cpu().numpy(), np.cumsum(rowptr_t))
    assert np.array_equal(gs.col_t.cpu().numpy()[: ei.shape[1]], dst[order_t])
    deg = np.diff(rowptr)
    assert np.array_equal(gs.invdeg.cpu().numpy()[:n], (1.0 / np.maximum(deg, 1)).astype(np.float32))
    gs.check()
    gptr, b = ops.graph_ptr(batch.cuda(), None, n, "cuda")
    assert b == 6 and np.array_equal(gptr.cpu().numpy(), ptr.numpy())
    # the one-launch build for grouped (collated) batches must give exactly the same structure
    gg = ops.GraphStructure(ei.cuda(), n, gptr, b)
    torch.cuda.synchronize()
    for name in ("rowptr", "rowptr_t", "invdeg"):
        assert torch.equal(getattr(gg, name), getattr(gs, name)), name
    assert torch.equal(gg.col[: ei.shape[1]], gs.col[: ei.shape[1]]) and torch.equal(gg.col_t[: ei.shape[1]], gs.col_t[: ei.shape[1]])
    gg.check()


def test_grouped_csr_build_random_playout_batch():
    """256 mid-game Hex-11 boards of very different sizes (3..123 nodes): the one-launch build must equal the general one
    (regression: a flat pointer into the workgroup's LDS faulted on exactly this kind of batch)."""
    from gnn_hex_amd import ops
    x, ei, batch, ptr = batch_tensors("D1", [11] * 256)
    n = x.shape[0]
    ref = ops.GraphStructure(ei.cuda(), n)
    gptr = torch.empty(257, dtype=torch.int32, device="cuda")
    gg = ops.GraphStructure(ei.cuda(), n, gptr, 256, ptr64=ptr.cuda())
    torch.cuda.synchronize()
    gg.check()
    assert torch.equal(gptr.long().cpu(), ptr)
    for name in ("rowptr", "rowptr_t", "invdeg"):
        assert torch.equal(getattr(gg, name), getattr(ref, name)), name
    e = ei.shape[1]
    assert torch.equal(gg.col[:e], ref.col[:e]) and torch.equal(gg.col_t[:e], ref.col_t[:e])


def test_grouped_csr_build_edge_cases():
    """Grouped build: empty graphs, a graph without edges, directed (asymmetric) edges, isolated nodes, and the status
    bit when the batch is not actually grouped."""
    from gnn_hex_amd import ops
    # graphs of 3, 0, 2, 4 nodes; graph 2 has no edges; graph 3 is directed
    ptr = torch.tensor([0, 3, 3, 5, 9])
    ei = torch.tensor([[0, 1, 2, 0, 5, 6, 8, 8, 5],
                       [1, 0, 0, 2, 6, 5, 5, 7, 7]])
    n = 9
    gptr = ptr.to(torch.int32).cuda()
    gs = ops.GraphStructure(ei.cuda(), n)
    gg = ops.GraphStructure(ei.cuda(), n, gptr, 4)
    torch.cuda.synchronize()
    for name in ("rowptr", "rowptr_t", "invdeg"):
        assert torch.equal(getattr(gg, name), getattr(gs, name)), name
    assert torch.equal(gg.col[:9], gs.col[:9]) and torch.equal(gg.col_t[:9], gs.col_t[:9])
    gg.check()
    bad = ops.GraphStructure(ei.flip(1).contiguous().cuda(), n, gptr, 4)      # graphs in reverse order: not grouped
    torch.cuda.synchronize()
    with pytest.raises(IndexError):
        bad.check()


def test_grouped_csr_build_graph_of_exactly_2048_nodes():
    """The one-launch build takes graphs up to 2048 nodes; at exactly 2048 the last row's end lies past the scanned range
    (regression: it was read from uninitialised LDS).  2049 nodes must raise status bit 8."""
    from gnn_hex_amd import ops
    rng = np.random.default_rng(9)
    for n0 in (2047, 2048):
        sizes = [n0, 5]
        off, eis = 0, []
        for n in sizes:
            m = 6 * n
            s, d = rng.integers(0, n, m), rng.integers(0, n, m)
            s[:4] = n - 1                                   # make sure the last row has out- and in-edges
            d[4:8] = n - 1
            eis.append(np.stack([s, d]) + off)
            off += n
        ei = torch.from_numpy(np.concatenate(eis, 1).astype(np.int64)).cuda()
        gptr = torch.tensor([0, sizes[0], off], dtype=torch.int32, device="cuda")
        gs = ops.GraphStructure(ei, off)
        gg = ops.GraphStructure(ei, off, gptr, 2)
        torch.cuda.synchronize()
        gg.check()
        e = ei.shape[1]
        for name in ("rowptr", "rowptr_t", "invdeg"):
            assert torch.equal(getattr(gg, name), getattr(gs, name)), (n0, name)
        assert torch.equal(gg.col[:e], gs.col[:e]) and torch.equal(gg.col_t[:e], gs.col_t[:e])
    ei = torch.tensor([[0, 2048], [2048, 0]], dtype=torch.int64, device="cuda")
    big = ops.GraphStructure(ei, 2049, torch.tensor([0, 2049], dtype=torch.int32, device="cuda"), 1)
    torch.cuda.synchronize()
    with pytest.raises(IndexError):
        big.check()


@pytest.mark.parametrize("maker", [True, False])
def test_gnn_s_hex7_start_positions(maker):
    hip, ref = make_pair(10, 35)
    x, ei, batch, ptr = batch_tensors("D0", [7] * 32, maker=maker)
    _compare(hip, ref, x, ei, batch, ptr)


def test_gnn_s_hex7_random_positions():
    hip, ref = make_pair(10, 35, seed=3)
    x, ei, batch, ptr = batch_tensors("D1", [7] * 32)
    _compare(hip, ref, x, ei, batch, ptr)


def test_gnn_l_hex11():
    hip, ref = make_pair(15, 110)
    x, ei, batch, ptr = batch_tensors("D1", [11] * 16, maker=False)
    _compare(hip, ref, x, ei, batch, ptr)


def test_mixed_sizes_ragged():
    hip, ref = make_pair(15, 110, seed=5)
    sizes = [5 + (g % 9) for g in range(27)]
    x, ei, batch, ptr = batch_tensors("D1", sizes)
    _compare(hip, ref, x, ei, batch, ptr)


@pytest.mark.parametrize("hidden", [16, 24, 33, 64, 72, 96, 112, 128])
def test_other_widths(hidden):
    hip, ref = make_pair(3, hidden, seed=hidden)
    x, ei, batch, ptr = batch_tensors("D1", [5, 6, 7, 8])
    _compare(hip, ref, x, ei, batch, ptr)


def test_seperate_and_advantages_only():
    hip, ref = make_pair(4, 35, seed=2)
    x, ei, batch, ptr = batch_tensors("D1", [7] * 8)
    xc, eic, bc, pc = x.cuda(), ei.cuda(), batch.cuda(), ptr.cuda()
    v_ref, a_ref = ref(x, ei, batch, ptr, seperate=True)
    v_hip, a_hip = hip(xc, eic, bc, pc, seperate=True)
    assert (v_hip.cpu() - v_ref).abs().max() < TOL and (a_hip.cpu() - a_ref).abs().max() < TOL
    ao_ref = ref(x, ei, batch, ptr, advantages_only=True)
    ao_hip = hip(xc, eic, bc, pc, advantages_only=True)
    assert ao_hip.shape == ao_ref.shape == (x.shape[0], 1)
    assert (ao_hip.cpu() - ao_ref).abs().max() < TOL
    # gradients through the two-output form.  This synthetic loss sums over ALL nodes, so gradients reach |g| ~ 30
    # (the metric's mse step stays below ~2): the 1e-4 bar is applied relative to the tensor's scale when that exceeds 1.
    for m, args in ((ref, (x, ei, batch, ptr)), (hip, (xc, eic, bc, pc))):
        m.zero_grad(set_to_none=True)
        v, a = m(*args, seperate=True)
        (v.sum() * 0.5 + (a * a).sum()).backward()
    for (k, p), (_, pr) in zip(hip.named_parameters(), ref.named_parameters()):
        if pr.grad is None:
            assert p.grad is None
        else:
            assert (p.grad.cpu() - pr.grad).abs().max() < TOL * max(1.0, pr.grad.abs().max().item()), k
    # advantages_only: the value head gets no gradient
    for m, args in ((ref, (x, ei, batch, ptr)), (hip, (xc, eic, bc, pc))):
        m.zero_grad(set_to_none=True)
        m(*args, advantages_only=True).sum().backward()
    for (k, p), (_, pr) in zip(hip.named_parameters(), ref.named_parameters()):
        if pr.grad is None:
            assert p.grad is None, k
        else:
            assert (p.grad.cpu() - pr.grad).abs().max() < TOL * max(1.0, pr.grad.abs().max().item()), k


def test_single_graph_no_batch_vector_and_no_grad():
    hip, ref = make_pair(5, 35, seed=7)
    x, ei, _, _ = batch_tensors("D0", [7])
    with torch.no_grad():
        q_ref = ref(x, ei)
        q_hip = hip(x.cuda(), ei.cuda())
    assert (q_hip.cpu() - q_ref).abs().max() < TOL
    # dueling identity (GN0/models.py:571-584): mean over the graph of Q equals tanh(value)
    v, a = hip(x.cuda(), ei.cuda(), seperate=True)
    assert abs(q_hip.mean().item() - v.item()) < 1e-5
    assert q_hip.abs().max() < 5


def test_mixed_side_batch_asserts_like_reference():
    hip, _ = make_pair(3, 16)
    x, ei, batch, ptr = batch_tensors("D0", [5, 5])
    x[0, 2] = 0.0
    with pytest.raises(AssertionError):
        hip(x.cuda(), ei.cuda(), batch.cuda(), ptr.cuda())


def test_wrong_size_hint_poisons_the_output_instead_of_returning_garbage():
    """A stale / wrong largest-graph hint sends a 150-node graph to the 128-row fused kernel: the kernel must flag it in
    the status word AND write NaN into that graph's Q values (the other graphs stay correct)."""
    from gnn_hex_amd import ops
    if ops.get_math() != "fp32" or not ops._FUSED_ENABLED:
        pytest.skip("fused kernels only, once")
    hip, ref = make_pair(3, 35, seed=24)
    x, ei, batch, ptr = _random_batch([20, 150, 16], seed=8, directed=False, p_edge=0.03)
    xd = ops.attach_hints(x.cuda(), is_maker=True, max_nodes=100)          # a lie: the second graph has 150 nodes
    with torch.no_grad():
        q = hip(xd, ei.cuda(), batch.cuda(), ptr.cuda())
        q_ref = ref(x, ei, batch, ptr)
    torch.cuda.synchronize()
    p0, p1, p2 = int(ptr[1]), int(ptr[2]), int(ptr[3])
    assert torch.isnan(q[p0:p1]).all()
    assert (q[:p0].cpu() - q_ref[:p0]).abs().max() < TOL and (q[p1:p2].cpu() - q_ref[p1:p2]).abs().max() < TOL


def test_sticky_status_word_reports_once_and_clears():
    """The one-launch CSR build ORs into one long-lived error word per device (no memset per batch): the first check()
    after an error raises and clears it, later healthy batches check clean."""
    from gnn_hex_amd import ops
    if ops.get_math() != "fp32" or not ops._FUSED_ENABLED:
        pytest.skip("mode-independent")
    ei = torch.tensor([[0, 1, 3, 4], [1, 0, 4, 3]]).cuda()
    gptr = torch.tensor([0, 3, 5], dtype=torch.int32, device="cuda")
    good = ops.GraphStructure(ei, 5, gptr, 2)
    good.check()
    bad = ops.GraphStructure(torch.tensor([[4, 0], [0, 4]]).cuda(), 5, gptr, 2)       # edges between the two graphs
    assert bad.status is good.status is ops.sticky_status("cuda")
    with pytest.raises(IndexError):
        good.check()                 # sticky: whoever checks first hears about it ...
    bad.check()                      # ... and the word is clear again
    ops.GraphStructure(ei, 5, gptr, 2).check()


def test_stale_hints_are_dropped_after_in_place_edit():
    """Host-side hints (side to move, largest graph) are stamped with the tensor's version: editing x in place afterwards
    must make the model fall back to the reference's own device check instead of trusting the stale side."""
    from gnn_hex_amd import ops
    hip, ref = make_pair(3, 16, seed=8)
    x, ei, batch, ptr = batch_tensors("D0", [5, 7], maker=True)
    xd = ops.attach_hints(x.cuda(), is_maker=True, max_nodes=51)
    assert ops.hints_of(xd) == (True, 51)
    xd[:, 2] = 0.0                                   # now the breaker is to move; the hint says maker
    assert ops.hints_of(xd) == (None, None)
    x2 = x.clone()
    x2[:, 2] = 0.0
    with torch.no_grad():
        q = hip(xd, ei.cuda(), batch.cuda(), ptr.cuda())
        q_ref = ref(x2, ei, batch, ptr)               # breaker head
    assert (q.cpu() - q_ref).abs().max() < TOL


def test_final_conv_acts_and_hook():
    hip, ref = make_pair(4, 35, seed=9)
    x, ei, batch, ptr = batch_tensors("D1", [7] * 4)
    q_ref = ref(x, ei, batch, ptr)
    q_ref.sum().backward()
    q = hip(x.cuda(), ei.cuda(), batch.cuda(), ptr.cuda())
    q.sum().backward()
    assert (hip.final_conv_acts.cpu() - ref.final_conv_acts).abs().max() < TOL
    assert (hip.final_conv_grads.cpu() - ref.final_conv_grads).abs().max() < TOL


def test_cpu_tensors_fail_loudly():
    from gnn_hex_amd._lib import HexGnnError
    hip, _ = make_pair(3, 16)
    x, ei, batch, ptr = batch_tensors("D0", [5])
    with pytest.raises(HexGnnError):
        hip(x, ei, batch, ptr)


def test_gradients_form_one_flat_buffer():
    """The fused backward writes every parameter gradient into ONE buffer in model.parameters() order, which is what
    lets gnn_hex_amd.dist.GradSync all-reduce it in place (no flatten / unflatten copies)."""
    from gnn_hex_amd import ops
    from gnn_hex_amd.dist import GradSync
    if not ops._FUSED_ENABLED:
        pytest.skip("layered path allocates per-stack gradients")
    hip, _ = make_pair(4, 35, seed=1)
    x, ei, batch, ptr = batch_tensors("D1", [7] * 4)
    q = hip(x.cuda(), ei.cuda(), batch.cuda(), ptr.cuda())
    q.sum().backward()
    active = [p for p in hip.parameters() if p.grad is not None]
    flat = GradSync._adopt_flat(active)
    assert flat is not None and flat.numel() == sum(p.numel() for p in active)
    assert torch.equal(flat, torch.cat([p.grad.reshape(-1) for p in active]))


def _random_batch(sizes, seed, directed=True, p_edge=0.08):
    """Arbitrary (non-board) graphs: directed edges, duplicate edges, isolated nodes -- the reference model accepts any
    edge_index (torch_geometric semantics: mean over in-edges, duplicates counted, isolated -> 0)."""
    rng = np.random.default_rng(seed)
    xs, eis, bv, ptr, off = [], [], [], [0], 0
    for g, n in enumerate(sizes):
        x = np.zeros((n, 3), np.float32)
        x[:, 0] = rng.integers(0, 9, n)
        x[: min(2, n), 1] = 1
        x[:, 2] = 1.0
        m = rng.random((n, n)) < p_edge
        np.fill_diagonal(m, False)
        if n > 3:
            m[:, n - 1] = False          # node n-1 has no in-edges
            m[n - 2, :] = False          # node n-2 has no out-edges
        src, dst = np.nonzero(m)
        if not directed:
            src, dst = np.concatenate([src, dst]), np.concatenate([dst, src])
        if len(src) > 4:                 # duplicate a few edges
            dup = rng.integers(0, len(src), 3)
            src, dst = np.concatenate([src, src[dup]]), np.concatenate([dst, dst[dup]])
        perm = rng.permutation(len(src))
        xs.append(x)
        eis.append(np.stack([src[perm], dst[perm]]).astype(np.int64) + off)
        bv.append(np.full(n, g, np.int64))
        off += n
        ptr.append(off)
    return (torch.from_numpy(np.concatenate(xs)), torch.from_numpy(np.concatenate(eis, 1)),
            torch.from_numpy(np.concatenate(bv)), torch.tensor(ptr, dtype=torch.long))


@pytest.mark.parametrize("directed", [True, False])
def test_arbitrary_graphs_directed_duplicates_isolated(directed):
    hip, ref = make_pair(4, 35, seed=21)
    x, ei, batch, ptr = _random_batch([1, 2, 17, 40, 64, 128, 5, 90], seed=3, directed=directed)
    _compare(hip, ref, x, ei, batch, ptr)


@pytest.mark.parametrize("hidden", [64, 80, 96, 110, 128])
def test_big_random_graphs_on_the_layer_major_path(hidden):
    """Graphs of several hundred nodes with edges ALL OVER the graph (not board-like): on the layer-major kernels most
    neighbours of a row then live in another 128-row block -- the global-memory side of the mixed LDS / global gather of round 3
    (hidden 49..112; 128 keeps the all-global schedule) carries most of the load, every neighbour slot, the wave-uniform skip
    mask and rows with more than sixteen in-edges (the CSR tail path) are exercised, directed edges make the transposed
    gather of the backward differ from the forward's.  Q and every gradient against the oracle."""
    from gnn_hex_amd import ops
    if ops._FUSED_ENABLED and ops.get_math() != "fp32":
        pytest.skip("graphs above 128 nodes run layer-major whatever the switches say: once per switch state is enough")
    hip, ref = make_pair(3, hidden, seed=27)
    x, ei, batch, ptr = _random_batch([300, 40, 517, 129, 7], seed=hidden, directed=True, p_edge=0.02)
    deg = torch.bincount(ei[1], minlength=x.shape[0])
    assert int(deg.max()) > 16 and int((deg == 0).sum()) > 0           # the tail path and empty rows are both present
    _compare(hip, ref, x, ei, batch, ptr)
    x, ei, batch, ptr = _random_batch([260, 260], seed=hidden + 1, directed=False, p_edge=0.012)
    _compare(hip, ref, x, ei, batch, ptr)


def test_graph_size_boundary_128_129():
    """128 nodes still fits a workgroup's LDS (fused path); one 129-node graph sends the batch down the layered path."""
    hip, ref = make_pair(3, 35, seed=22)
    x, ei, batch, ptr = _random_batch([128, 127, 16], seed=5, directed=False, p_edge=0.04)
    _compare(hip, ref, x, ei, batch, ptr)
    x, ei, batch, ptr = _random_batch([129, 16, 200], seed=6, directed=False, p_edge=0.03)
    _compare(hip, ref, x, ei, batch, ptr)


def test_dense_graph_exceeds_lds_csr_capacity():
    """A graph whose edge list does not fit the LDS CSR cache (u8 columns; 2848 edges at hidden 110, hexgnn_qnet_csr_capacity)
    walks the global CSR: about 5 900 edges per graph here.  At a width of 96 or less the cache takes 8192 edges and these graphs
    would stay in LDS; tests/test_gpu_fused_instantiations.py has graphs beyond that for every tile count."""
    hip, ref = make_pair(3, 110, seed=23)
    from gnn_hex_amd import ops
    x, ei, batch, ptr = _random_batch([100, 100], seed=7, directed=True, p_edge=0.6)
    assert ei.shape[1] > 2 * 3800
    # degree-60 random graphs with features up to 8 are far outside the board-graph domain (degree <= ~12) and make the
    # gradient sums cancel heavily: the hardest case for the split-precision math, held to the same bar as exact fp32.
    _compare(hip, ref, x, ei, batch, ptr)


def test_split_math_is_fp32_class_against_float64():
    """Accuracy of both arithmetic modes of the fused kernels measured against the SAME oracle evaluated in float64
    (GNN-L, Hex-11 mid-game boards, loss gradients): the f16x3 split (22-bit products, fp32 accumulate) must sit within
    a small factor of the exact-fp32 MFMA path's own rounding error, i.e. both are fp32-class results."""
    import copy
    from gnn_hex_amd import ops
    hip, ref = make_pair(15, 110, seed=5)
    ref64 = copy.deepcopy(ref).double()
    x, ei, batch, ptr = batch_tensors("D1", [11] * 24, maker=True)
    sel, tgt = sel_and_targets(ptr)
    q64, g64 = _step(ref64, x.double(), ei, batch, ptr, sel, tgt.double())
    errs = {}
    if ops.get_math() != "fp32" or not ops._FUSED_ENABLED:
        pytest.skip("mode-independent: runs once (it sets both math modes itself)")
    for math in ("fp32", "f16x3"):      # the autouse fixture restores the defaults afterwards
        ops.set_math(math)
        q, g = _step(hip, x.cuda(), ei.cuda(), batch.cuda(), ptr.cuda(), sel.cuda(), tgt.cuda())
        torch.cuda.synchronize()
        eq = (q.cpu().double() - q64).abs().max().item()
        # tensors whose true gradient vanishes (the advantage bias: the dueling mean removes it) are pure rounding noise
        eg = max(((g[k].cpu().double() - g64[k]).norm() / g64[k].norm()).item()
                 for k in g64 if g64[k] is not None and g64[k].norm() > 1e-6)
        errs[math] = (eq, eg)
    print("max |Q - Q64| and worst relative gradient-tensor error:", errs)
    # measured on MI355X: Q 1.7e-7 (fp32) / 2.7e-7 (f16x3); gradients 7.7e-4 / 6.3e-4 (the random-init network
    # saturates tanh, so its gradients are ill-conditioned in ANY fp32 arithmetic; the CPU fp32 oracle itself: 3.0e-4)
    assert errs["fp32"][0] < 2e-6 and errs["f16x3"][0] < 2e-6
    assert errs["fp32"][1] < 5e-3 and errs["f16x3"][1] < 5e-3
    assert errs["f16x3"][0] <= 4 * errs["fp32"][0] + 1e-7
    assert errs["f16x3"][1] <= 2 * errs["fp32"][1] + 1e-5


def test_graphed_step_replays_bit_identical_gradients():
    """A whole step (CSR build + forward + loss + backward) captured into a HIP graph and replayed must reproduce the
    eager step's Q loss and gradients bit for bit, for two captured batches (maker / breaker) sharing one model."""
    from gnn_hex_amd.graphs import GraphedStep
    hip, _ = make_pair(4, 35, seed=3)
    params = list(hip.parameters())
    batches = []
    for maker in (True, False):
        x, ei, batch, ptr = batch_tensors("D1", [7, 5, 7, 6], maker=maker)
        sel, tgt = sel_and_targets(ptr)
        xd = x.cuda()
        xd._hex_is_maker = maker
        xd._hex_max_nodes = int((ptr[1:] - ptr[:-1]).max())
        batches.append((xd, ei.cuda(), batch.cuda(), ptr.cuda(), sel.cuda(), tgt.cuda()))

    def make_fn(bt):
        def fn():
            for p in params:
                p.grad = None
            q = hip(bt[0], bt[1], bt[2], bt[3])
            loss = torch.nn.functional.mse_loss(q[bt[4]], bt[5])
            loss.backward()
            return loss
        return fn

    eager = []
    for bt in batches:
        loss = make_fn(bt)()
        torch.cuda.synchronize()
        eager.append((loss.detach().clone(), [None if p.grad is None else p.grad.detach().clone() for p in params]))
        del loss    # see GraphedStep: no autograd graph built on the default stream may be alive at capture time
    g0 = GraphedStep(make_fn(batches[0]), params)
    g1 = GraphedStep(make_fn(batches[1]), params, pool=g0.pool())
    for rep in range(2):
        for g, (loss_e, grads_e) in zip((g0, g1), eager):
            loss = g.replay()
            torch.cuda.synchronize()
            assert torch.equal(loss, loss_e)
            for p, ge in zip(params, grads_e):
                if ge is None:
                    assert p.grad is None
                else:
                    assert torch.equal(p.grad, ge)


@pytest.mark.parametrize("loss_fn", ["mse", "huber"])
@pytest.mark.parametrize("weighted", [False, True])
def test_td_loss_matches_torch(loss_fn, weighted):
    """Fused TD loss (gather + loss + mean; memset + scatter backward) vs the torch expression it replaces, including
    duplicate selections, importance weights and an upstream gradient scale."""
    from gnn_hex_amd import ops
    if ops.get_math() != "fp32" or not ops._FUSED_ENABLED:
        pytest.skip("mode-independent")
    gen = torch.Generator().manual_seed(11)
    n, k = 5000, 257
    q0 = (torch.randn(n, generator=gen) * 1.5)
    sel = torch.randint(0, n, (k,), generator=gen)
    sel[5] = sel[17]                       # a duplicate
    tgt = torch.randn(k, generator=gen)
    w = torch.rand(k, generator=gen) + 0.1 if weighted else None
    qr = q0.clone().requires_grad_(True)
    d = qr[sel] - tgt
    el = d * d if loss_fn == "mse" else torch.nn.functional.huber_loss(qr[sel], tgt, reduction="none", delta=1.0)
    ref = (el * w).mean() if weighted else el.mean()
    (ref * 0.7).backward()
    qh = q0.clone().cuda().requires_grad_(True)
    loss, td = ops.td_loss(qh, sel.cuda(), tgt.cuda(), None if w is None else w.cuda(), loss_fn)
    (loss * 0.7).backward()
    torch.cuda.synchronize()
    assert abs(loss.item() - ref.item()) < 1e-5 * max(1.0, abs(ref.item()))
    assert torch.allclose(td.cpu(), d.detach(), atol=1e-6)
    assert torch.allclose(qh.grad.cpu(), qr.grad, atol=1e-7)
    assert not td.requires_grad


@pytest.mark.parametrize("loss_fn", ["mse", "huber"])
def test_td_loss_one_launch_form_is_bit_identical(loss_fn):
    """``ops.backward(loss)`` (one launch: loss, td and d loss / d q together, no ones-fill, no scatter launch) against
    ``loss.backward()`` on the same inputs (forward launch + ``hexgnn_td_loss_backward``): loss, td and the gradient must
    agree bit for bit -- with duplicated selections (twice and five times the same node), out-of-range entries, weights,
    and more than one 1024-node range / 1024-entry chunk."""
    from gnn_hex_amd import ops
    if ops.get_math() != "fp32" or not ops._FUSED_ENABLED:
        pytest.skip("mode-independent")
    gen = torch.Generator().manual_seed(23)
    n, k = 5000, 2300
    q0 = (torch.randn(n, generator=gen) * 1.5)
    sel = torch.randint(0, n, (k,), generator=gen)
    sel[5] = sel[17]
    sel[100:105] = sel[99]
    sel[7] = -1
    sel[8] = n + 3
    tgt = torch.randn(k, generator=gen)
    w = torch.rand(k, generator=gen) + 0.1
    outs = []
    for fused in (False, True):
        qh = q0.clone().cuda().requires_grad_(True)
        loss, td = ops.td_loss(qh, sel.cuda(), tgt.cuda(), w.cuda(), loss_fn)
        if fused:
            ops.backward(loss)
        else:
            loss.backward()
        torch.cuda.synchronize()
        outs.append((loss.detach().clone(), td.clone(), qh.grad.clone()))
    for name, a, b in zip(("loss", "td", "grad"), outs[0], outs[1]):
        if not torch.equal(a, b):
            bad = torch.nonzero((a != b).reshape(-1)).reshape(-1)[:8].tolist()
            cnt = [(i, int((sel == i).sum())) for i in bad] if name == "grad" else bad
            raise AssertionError("%s differs at %s: %s vs %s" % (name, cnt, a.reshape(-1)[bad].tolist(), b.reshape(-1)[bad].tolist()))
    # a scaled loss is not the root of the pass: ops.backward must fall through to autograd
    qh = q0.clone().cuda().requires_grad_(True)
    loss, _ = ops.td_loss(qh, sel.cuda(), tgt.cuda(), w.cuda(), loss_fn)
    ops.backward(loss * 0.5)
    assert torch.allclose(qh.grad, outs[0][2] * 0.5, rtol=1e-6, atol=1e-9)
    # no gradient wanted: the forward-only launch
    with torch.no_grad():
        l2, td2 = ops.td_loss(q0.cuda(), sel.cuda(), tgt.cuda(), w.cuda(), loss_fn)
    assert torch.equal(l2, outs[0][0]) and torch.equal(td2, outs[0][1])


def test_direct_gradient_form_matches_the_autograd_form():
    """The eager fast path (ops.QNetDirectFn: parameters are not autograd inputs, the backward assigns p.grad itself) against
    the autograd form (ops.QNetFusedFn: 57 inputs / 57 returned gradients): Q and every gradient bit-identical, for all three
    output modes; gradients ACCUMULATE when the caller did not clear them (a second backward, retain_graph); a frozen
    parameter or a tensor hook on a parameter sends the model back to the autograd form; a head-tail weight changed in place
    before the backward is an error on both forms."""
    from gnn_hex_amd import ops
    if not ops._FUSED_ENABLED:
        pytest.skip("a test of the fused path")
    hip, _ = make_pair(4, 35, seed=71)
    x, ei, batch, ptr = batch_tensors("D1", [7, 6, 7, 5, 7], maker=True)
    sel, tgt = sel_and_targets(ptr)
    xd, eid = x.cuda(), ei.cuda()
    ops.attach_hints(xd, True, int((ptr[1:] - ptr[:-1]).max()))
    eid._hex_grouped = True
    bv, pt, sd, td = batch.cuda(), ptr.cuda(), sel.cuda(), tgt.cuda()

    def run(**kw):
        hip.zero_grad(set_to_none=True)
        out = hip(xd, eid, bv, pt, **kw)
        if kw.get("seperate"):
            loss = (out[0] ** 2).mean() + torch.nn.functional.mse_loss(out[1][sd], td)
        else:
            loss = torch.nn.functional.mse_loss(out.reshape(-1)[sd], td)
        loss.backward()
        outs = out if isinstance(out, tuple) else (out,)
        return [o.detach().clone() for o in outs], {k: (None if p.grad is None else p.grad.clone()) for k, p in hip.named_parameters()}

    for kw in ({}, {"seperate": True}, {"advantages_only": True}):
        ops.set_direct_grads(True)
        o1, g1 = run(**kw)
        assert isinstance(hip.__dict__["_fca"], ops._QNetCall)             # the direct path ran
        ops.set_direct_grads(False)
        try:
            o2, g2 = run(**kw)
        finally:
            ops.set_direct_grads(True)
        for a, b_ in zip(o1, o2):
            assert torch.equal(a, b_)
        for k in g1:
            assert (g1[k] is None) == (g2[k] is None), (kw, k)
            if g1[k] is not None:
                assert torch.equal(g1[k], g2[k]), (kw, k)
    # final_conv_acts / final_conv_grads on the direct path
    _, g = run()
    assert hip.final_conv_acts.shape == (x.shape[0], 35) and hip.final_conv_grads.shape == (x.shape[0], 35)
    # accumulation: backward twice through one graph without clearing -> twice the gradient
    hip.zero_grad(set_to_none=True)
    q = hip(xd, eid, bv, pt)
    loss = torch.nn.functional.mse_loss(q[sd], td)
    loss.backward(retain_graph=True)
    loss.backward()
    for k, p in hip.named_parameters():
        if g[k] is not None:
            assert torch.allclose(p.grad, 2 * g[k], rtol=1e-6, atol=1e-9), k
    # a frozen parameter: the autograd form takes over and leaves that parameter without a gradient
    hip.gnn.convs[1].lin_l.weight.requires_grad_(False)
    try:
        _, gf = run()
        assert not isinstance(hip.__dict__.get("_fca"), ops._QNetCall)
        assert gf["gnn.convs.1.lin_l.weight"] is None
        assert torch.equal(gf["gnn.convs.0.lin_l.weight"], g["gnn.convs.0.lin_l.weight"])
    finally:
        hip.gnn.convs[1].lin_l.weight.requires_grad_(True)
        hip.__dict__.pop("_fused_cache", None)
    # ops.td_loss + ops.backward: the network's backward runs on the caller's thread, without the autograd engine; same bits
    # as loss.backward() through autograd, and the spent graph refuses a second pass
    outs = []
    for direct in (False, True):
        hip.zero_grad(set_to_none=True)
        qq = hip(xd, eid, bv, pt)
        loss, _ = ops.td_loss(qq, sd, td)
        assert hasattr(loss, "_hex_direct")
        if direct:
            ops.backward(loss)
            with pytest.raises(RuntimeError, match="spent"):
                loss.backward()
        else:
            loss.backward()
        outs.append({k: (None if p.grad is None else p.grad.clone()) for k, p in hip.named_parameters()})
    for k in outs[0]:
        assert (outs[0][k] is None) == (outs[1][k] is None), k
        if outs[0][k] is not None:
            assert torch.equal(outs[0][k], outs[1][k]), k
    assert hip.final_conv_acts.shape == (x.shape[0], 35)
    # inference under no_grad: direct forward without an autograd node
    with torch.no_grad():
        qn = hip(xd, eid, bv, pt)
    assert torch.equal(qn, q.detach()) and not qn.requires_grad
    # a head-tail weight edited in place between forward and backward (as optimizer.step() does) raises on the autograd form
    # as well: its backward reads the head tail's weights live, like the direct form's
    ops.set_direct_grads(False)
    try:
        q = hip(xd, eid, bv, pt)
        assert not isinstance(hip.__dict__.get("_fca"), ops._QNetCall)
        loss = torch.nn.functional.mse_loss(q[sd], td)
        with torch.no_grad():
            hip.maker_head.linear.weight.add_(1e-3)
        with pytest.raises(RuntimeError, match="modified in place"):
            loss.backward()
    finally:
        ops.set_direct_grads(True)


def test_randomised_configurations():
    """Seeded sweep over widths, depths, batch shapes, edge densities, directed / symmetric graphs, both CSR builds and both
    arithmetic modes of the fused kernels against the oracle (1e-4 on Q, 1e-4 relative to max(1, |g|max) on gradients)."""
    from gnn_hex_amd import ops
    if ops.get_math() != "fp32" or not ops._FUSED_ENABLED:
        pytest.skip("mode-independent: sets the modes itself")
    rng = np.random.default_rng(2026)
    for case in range(30):
        hidden = int(rng.choice([16, 30, 35, 48, 64, 80, 96, 110]))
        layers = int(rng.integers(1, 6))
        sizes = [int(rng.integers(3, 129)) for _ in range(int(rng.integers(1, 9)))]
        p_edge = float(rng.choice([0.02, 0.06, 0.15]))
        grouped = bool(rng.integers(0, 2))
        math = str(rng.choice(["fp32", "f16x3"]))
        hip, ref = make_pair(layers, hidden, seed=case)
        x, ei, batch, ptr = _random_batch(sizes, seed=case, directed=bool(rng.integers(0, 2)), p_edge=p_edge)
        sel, tgt = sel_and_targets(ptr)
        q_ref, g_ref = _step(ref, x, ei, batch, ptr, sel, tgt)
        ops.set_math(math)
        xd, eid = x.cuda(), ei.cuda()
        xd._hex_is_maker, xd._hex_max_nodes = True, max(sizes)
        if grouped:
            eid._hex_grouped = True
        q, g = _step(hip, xd, eid, batch.cuda(), ptr.cuda(), sel.cuda(), tgt.cuda())
        torch.cuda.synchronize()
        tag = "case %d: hidden %d, %d layers, sizes %s, p %.2f, grouped %s, %s" % (case, hidden, layers, sizes, p_edge, grouped, math)
        assert (q.cpu() - q_ref).abs().max().item() < TOL, tag
        for k in g_ref:
            if g_ref[k] is None:
                assert g[k] is None, tag
                continue
            scale = max(1.0, g_ref[k].abs().max().item())
            assert (g[k].cpu() - g_ref[k]).abs().max().item() < TOL * scale, tag + " " + k


def test_full_batch_is_bit_reproducible_and_paths_agree():
    """The BASELINE batch shape (GNN-L, 256 Hex-11 boards: every CU busy, both waves of every SIMD contending for the MFMA
    pipe) run repeatedly: Q and every gradient must be bit-identical from run to run (the kernels have no float atomics and
    a timing-dependent hazard between MFMAs and the fillers issued around them would show up here first), and the fused
    kernels must agree with the layer-major kernels, which share no code with the filler structure."""
    from gnn_hex_amd import ops
    if not ops._FUSED_ENABLED:
        pytest.skip("a test of the fused kernels (both arithmetic modes)")
    hip, _ = make_pair(15, 110, seed=11)
    x, ei, batch, ptr = batch_tensors("D1", [11] * 256, maker=True)
    sel, tgt = sel_and_targets(ptr)
    args = [t.cuda() for t in (x, ei, batch, ptr, sel, tgt)]
    q0, g0 = _step(hip, *args)
    for _ in range(12):
        q, g = _step(hip, *args)
        assert torch.equal(q, q0)
        for k in g0:
            assert (g[k] is None) == (g0[k] is None)
            if g0[k] is not None:
                assert torch.equal(g[k], g0[k]), k
    ops.set_fused(False)
    try:
        ql, gl = _step(hip, *args)
    finally:
        ops.set_fused(True)
    assert (ql - q0).abs().max().item() < TOL
    for k in g0:
        if g0[k] is not None:
            scale = max(1.0, g0[k].abs().max().item())
            assert (gl[k] - g0[k]).abs().max().item() < TOL * scale, k
