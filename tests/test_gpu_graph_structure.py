"""GPU: the graph-structure kernels of csr.hip against a numpy reference (helpers.csr_reference) at the sizes where they change
path.  Integer work: every comparison is array_equal, there is no tolerance in this file.

What each section reaches (the thresholds are csr.hip's own constants):

  A  general build      one scan tile (n + 1 = 1024) / two (n = 1024) / three (2048); 258 tiles, so csr_scan_fix_kernel's
                        256-stride loop over the tile totals takes a second trip; a 257-long row given in descending order; the
                        four-memset branch with poisoned buffers
  B  grouped build      1024 edges per graph (4 register-kept edges x 256 threads), kCsrLdsEdges = 3072 (LDS fill / global fill),
                        kPer = 8 scan entries per thread (7, 8, 9 and 2040, 2041 nodes), kCsrMaxGraph = 2048 nodes -- each on both
                        sides, with the target graph in the middle, first (eb = 0) and last (it writes rowptr[n]) of its batch
  C  the edge search    1, 255, 256, 257, 65 535, 65 536, 65 537 edges: the rounds of the 256-ary search
  D  status contract    bits 1 and 4 on every path that can raise them, the sticky word, the general build's private word
  E  row-block table    the device-built table of block_table_body against data.blocks_for_order: 128/129 and 192/193 splits, empty
                        graphs, the 512-graph chunk, b mod 4 != 0
  F  graph_ptr, pad_rows, unpad_rows

Every build is compared with the reference FIRST; builds are compared with one another only after that."""
import ctypes as C

import numpy as np
import pytest
import torch

from helpers import csr_reference

pytestmark = pytest.mark.gpu

POISON = 0x5a5a5a5a


# ---- inputs ------------------------------------------------------------------------------------------------------------------

def _multigraph(rng, n, e):
    """e random directed edges over nodes 0 .. n - 1 (multi-edges and self loops included), in shuffled order."""
    if e == 0:
        return np.zeros((2, 0), dtype=np.int64)
    assert n > 0
    ei = np.stack([rng.integers(0, n, e), rng.integers(0, n, e)]).astype(np.int64)
    return ei[:, rng.permutation(e)]


def _collate(graphs):
    """graphs = [(nodes, local [2, e] edges)] -> (edge_index [2, E], ptr [b + 1], edge offsets [b + 1]), all int64 numpy."""
    ptr, eptr, parts = [0], [0], []
    for nodes, ei in graphs:
        parts.append(ei + ptr[-1])
        ptr.append(ptr[-1] + nodes)
        eptr.append(eptr[-1] + ei.shape[1])
    return np.concatenate(parts, 1).astype(np.int64), np.array(ptr, dtype=np.int64), np.array(eptr, dtype=np.int64)


def _dev(a, dtype=torch.int64):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).cuda()


def _got(gs, n, e):
    torch.cuda.synchronize()
    return (gs.rowptr.cpu().numpy(), gs.col.cpu().numpy()[:e], gs.rowptr_t.cpu().numpy(), gs.col_t.cpu().numpy()[:e],
            gs.invdeg.cpu().numpy()[:n])


NAMES = ("rowptr", "col", "rowptr_t", "col_t", "invdeg")


def _assert_same(got, want, what):
    for name, g, w in zip(NAMES, got, want):
        assert g.shape == w.shape, "%s: %s has shape %s, the reference %s" % (what, name, g.shape, w.shape)
        if not np.array_equal(g, w):
            bad = np.flatnonzero(g != w)
            raise AssertionError("%s: %s differs from the reference at %d of %d entries, first at %d: %s against %s"
                                 % (what, name, bad.size, g.size, bad[0], g[bad[0]], w[bad[0]]))


def _sticky():
    from gnn_hex_amd import ops
    return ops.sticky_status("cuda")


@pytest.fixture(scope="module")
def pack():
    """The ``pack`` tuple of GraphStructure.grouped as ops.py builds it at its deferred-build call site, for one small model
    (2 raw features, hidden 16, 2 layers): (c_in, hidden, layers, wl, bl, wr pointer arrays, wpack address)."""
    from gnn_hex_amd import _lib
    c_in, hidden, layers = 2, 16, 2
    gen = torch.Generator().manual_seed(0)
    params = []
    for l in range(layers):
        k = c_in if l == 0 else hidden
        params += [torch.randn(hidden, k, generator=gen).cuda(), torch.randn(hidden, generator=gen).cuda(),
                   torch.randn(hidden, k, generator=gen).cuda()]
    vp = C.c_void_p * layers
    arrays = [vp(*[t.data_ptr() for t in params[i::3]]) for i in range(3)]
    nbytes = _lib.lib().hexgnn_sage_stack_pack_bytes(c_in, hidden, layers)
    assert nbytes > 0
    wpack = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    tup = (c_in, hidden, layers, arrays[0], arrays[1], arrays[2], wpack.data_ptr())
    yield tup
    del params, wpack


# ---- A. general build -------------------------------------------------------------------------------------------------------------

def _general_case(name):
    rng = np.random.default_rng(11)
    if name == "n0":
        return 0, np.zeros((2, 0), dtype=np.int64)
    if name == "n1-e0":
        return 1, np.zeros((2, 0), dtype=np.int64)
    if name == "n1-loops":
        return 1, np.zeros((2, 3), dtype=np.int64)
    if name == "hub257":
        # row 17 has in-degree >= 257, node 400 out-degree >= 257: both given in DESCENDING order with duplicates, so the one-thread
        # insertion sort of that row does the most work it can (257 stays: thousands would take seconds)
        n = 600
        ei = _multigraph(rng, n, 2 * n)
        desc = np.sort(np.concatenate([rng.integers(0, n, 200), rng.integers(0, n, 57)]))[::-1]
        desc[40:60] = desc[40]
        hub_in = np.stack([desc, np.full(257, 17)])
        hub_out = np.stack([np.full(257, 400), desc])
        return n, np.concatenate([hub_in, ei, hub_out], 1).astype(np.int64)
    n = int(name[1:])
    ei = _multigraph(rng, n, 2 * n)
    if n > 262144:
        # in- and out-edges on the last row and on row 262 144 (the first of tile 256: its prefix is the sum the fix kernel's second
        # trip finishes), so a wrong tile prefix shows in col as well as in rowptr
        for k, row in enumerate((n - 1, 262144)):
            ei[0, 16 * k:16 * k + 8] = row
            ei[1, 16 * k + 8:16 * k + 16] = row
        ei = ei[:, rng.permutation(ei.shape[1])]
    return n, ei


GENERAL = ["n0", "n1-e0", "n1-loops", "n1023", "n1024", "n2048", "n263200", "hub257"]


@pytest.mark.parametrize("name", GENERAL)
def test_general_build(name):
    from gnn_hex_amd import ops
    n, ei = _general_case(name)
    e = ei.shape[1]
    if name == "n263200":
        assert (n + 1 + 1023) // 1024 == 258
    if name == "hub257":
        assert np.bincount(ei[1], minlength=n)[17] >= 257 and np.bincount(ei[0], minlength=n)[400] >= 257
    want = csr_reference(ei[0], ei[1], n)
    gs = ops.GraphStructure(_dev(ei), n)
    _assert_same(_got(gs, n, e), want, "general build %s" % name)
    gs.check()


@pytest.mark.parametrize("name", ["n0", "n1-loops", "n1024", "n2048"])
def test_general_build_separate_poisoned_buffers(name):
    """The caller's buffers laid out apart (the four-memset branch of hexgnn_csr_build), every one of them poisoned, the status
    word included: the same result, status 0, and the guard words between the buffers untouched."""
    from gnn_hex_amd import _lib, ops
    L = _lib.lib()
    n, ei = _general_case(name)
    e = ei.shape[1]
    ws_bytes = L.hexgnn_csr_workspace_bytes(n, e)
    ws_ints = (ws_bytes + 3) // 4
    gap = 16
    sizes = [n + 1, n + 1, 1, ws_ints, max(e, 1), max(e, 1)]          # rowptr, rowptr_t, status, workspace, col, col_t
    offs, o = [], gap
    for s in sizes:
        offs.append(o)
        o += (s + gap + 15) // 16 * 16
    buf = torch.full((o,), POISON, dtype=torch.int32, device="cuda")
    invdeg = torch.full((max(n, 1),), float("nan"), device="cuda")
    base = buf.data_ptr()
    p = [base + 4 * x for x in offs]
    eid = _dev(ei)
    src, dst = (eid[0].data_ptr(), eid[1].data_ptr()) if e else (None, None)
    rc = L.hexgnn_csr_build(n, e, src, dst, p[0], p[4], p[1], p[5], invdeg.data_ptr(), p[2], p[3], ws_bytes, ops._stream())
    assert rc == 0
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    part = [host[x:x + s] for x, s in zip(offs, sizes)]
    assert part[2][0] == 0, "status %d" % part[2][0]
    got = (part[0], part[4][:e], part[1], part[5][:e], invdeg.cpu().numpy()[:n])
    _assert_same(got, csr_reference(ei[0], ei[1], n), "general build, separate buffers, %s" % name)
    used = np.zeros(o, dtype=bool)
    for x, s in zip(offs, sizes):
        used[x:x + s] = True
    assert (host[~used] == POISON).all(), "a guard word between the buffers was written"


# ---- B. grouped build: one graph under test among neighbours ------------------------------------------------------------------------

TARGETS = ([(40, e) for e in (0, 1, 255, 256, 257, 1023, 1024, 1025, 3071, 3072, 3073, 5000)]
           + [(k, 6 * k) for k in (7, 8, 9, 2040, 2041, 2047, 2048)] + [(1, 5), (0, 0)])
ENDS = [(40, 0), (40, 1), (40, 1025), (40, 3073), (8, 48), (2048, 6 * 2048), (1, 5), (0, 0)]
GROUPED = [("mid", t) for t in TARGETS] + [(pos, t) for pos in ("first", "last") for t in ENDS]


def _grouped_batch(pos, nodes, edges):
    rng = np.random.default_rng(1000 * nodes + edges)
    target = (nodes, _multigraph(rng, nodes, edges))
    none = np.zeros((2, 0), dtype=np.int64)
    edgeless, empty, small = (3, none), (0, none), (4, _multigraph(rng, 4, 9))
    if pos == "mid":
        graphs = [edgeless, empty, target, empty, small]
    elif pos == "first":
        graphs = [target, empty, edgeless, empty, small]
    else:
        graphs = [edgeless, empty, small, empty, target]
    return _collate(graphs)


def _grouped_forms(ei, n, ptr, eptr, pack, edge_ptr_forms=True):
    """The one-launch build of one batch through every entry, one at a time: yields (name, structure, the int32 ranges it returned
    or None) -- a generator, so that a caller which expects a status bit sees it from the build that raised it."""
    from gnn_hex_amd import ops
    b = len(ptr) - 1
    eid = _dev(ei)
    yield "int32 ranges", ops.GraphStructure(eid, n, _dev(ptr, torch.int32), b), None
    g64 = torch.full((b + 1,), -7, dtype=torch.int32, device="cuda")
    yield "ptr64", ops.GraphStructure(eid, n, g64, b, ptr64=_dev(ptr)), g64
    for with_eptr in ((False, True) if edge_ptr_forms else (False,)):
        t = _dev(ei)
        if with_eptr:
            t._hex_edge_ptr = _dev(eptr)
        gs = ops.GraphStructure.grouped(t, n, b, _dev(ptr), pack=pack, device_blocks=True)
        yield "pack_b%s" % (" + edge offsets" if with_eptr else ""), gs, gs.gptr


@pytest.mark.parametrize("pos,target", GROUPED, ids=["%s-n%d-e%d" % (p, t[0], t[1]) for p, t in GROUPED])
def test_grouped_build(pos, target, pack):
    ei, ptr, eptr = _grouped_batch(pos, *target)
    n, e = int(ptr[-1]), ei.shape[1]
    want = csr_reference(ei[0], ei[1], n)
    first = None
    for name, gs, gptr in _grouped_forms(ei, n, ptr, eptr, pack):
        what = "grouped build (%s), target %s of %d nodes and %d edges" % (name, pos, target[0], target[1])
        got = _got(gs, n, e)
        _assert_same(got, want, what)
        if gptr is not None:
            assert np.array_equal(gptr.cpu().numpy(), ptr), what
        gs.check()
        if first is None:
            first = got
        else:
            _assert_same(got, first, what + " against the int32 form")


# ---- C. the edge search ---------------------------------------------------------------------------------------------------------------

def _search_batch(total):
    """Two-node graphs with k parallel edges each (k differs by at most one between them), `total` edges in all; runs of edgeless
    graphs at the front (3), in the middle (4) and at the end (3): both searches of such a graph land on the same index."""
    rng = np.random.default_rng(total)
    m = min(total, 300)
    counts = [total // m + (1 if i < total % m else 0) for i in range(m)]
    assert sum(counts) == total and min(counts) >= 1
    counts = [0] * 3 + counts[:m // 2] + [0] * 4 + counts[m // 2:] + [0] * 3
    return _collate([(2, _multigraph(rng, 2, k)) for k in counts])


@pytest.mark.parametrize("total", [1, 255, 256, 257, 65535, 65536, 65537])
def test_grouped_edge_search(total):
    from gnn_hex_amd import ops
    ei, ptr, eptr = _search_batch(total)
    n, e, b = int(ptr[-1]), ei.shape[1], len(ptr) - 1
    assert e == total
    want = csr_reference(ei[0], ei[1], n)
    eid = _dev(ei)
    g64 = torch.full((b + 1,), -7, dtype=torch.int32, device="cuda")
    forms = [("int32 ranges", ops.GraphStructure(eid, n, _dev(ptr, torch.int32), b)),
             ("ptr64", ops.GraphStructure(eid, n, g64, b, ptr64=_dev(ptr)))]
    for name, gs in forms:
        what = "edge search, %d edges (%s)" % (total, name)
        got = _got(gs, n, e)
        _assert_same(got, want, what)
        # graph by graph: every graph's slice is the reference of that graph alone, moved to its edge offset
        for g in range(b):
            r0, e0, e1 = int(ptr[g]), int(eptr[g]), int(eptr[g + 1])
            loc = csr_reference(ei[0, e0:e1] - r0, ei[1, e0:e1] - r0, 2)
            assert np.array_equal(got[0][r0:r0 + 3] - e0, loc[0]) and np.array_equal(got[2][r0:r0 + 3] - e0, loc[2]), (what, g)
            assert np.array_equal(got[1][e0:e1] - r0, loc[1]) and np.array_equal(got[3][e0:e1] - r0, loc[3]), (what, g)
            assert np.array_equal(got[4][r0:r0 + 2], loc[4]), (what, g)
        gs.check()
    assert np.array_equal(g64.cpu().numpy(), ptr)


# ---- D. status contract -------------------------------------------------------------------------------------------------------------------
# Once a bit is set the arrays are unspecified: these tests assert the bit and that the call returns, nothing else.  Every case
# ends with the shared sticky word at zero again.

def _status_batch():
    rng = np.random.default_rng(5)
    return _collate([(6, _multigraph(rng, 6, 14)), (5, _multigraph(rng, 5, 11)), (7, _multigraph(rng, 7, 12))])


def _bad_id_cases():
    """Node ids outside [0, n) that keep the edge list grouped: (name, edge_index).  2^32 + 3 has a valid id in its low 32 bits: the
    comparison has to be made on the int64."""
    ei, ptr, eptr = _status_batch()
    n, e = int(ptr[-1]), ei.shape[1]
    cases = []
    a = ei.copy(); a[0, int(eptr[1]) + 2] = -1; cases.append(("src = -1", a))
    a = ei.copy(); a[:, e - 1] = (n - 1, n); cases.append(("dst = n, the last edge", a))
    a = ei.copy(); a[0, 4] = 2 ** 32 + 3; cases.append(("src = 2^32 + 3", a))
    a = ei.copy(); a[:, 0] = (0, -1); cases.append(("dst = -1, the first edge", a))
    return cases, ptr, eptr


def _expect_flag(gs, bit, what):
    """The build returned; its status word carries `bit`; check() raises and (sticky word) clears."""
    torch.cuda.synchronize()
    word = int(gs.status.item())
    assert word & bit, "%s: status %d lacks bit %d" % (what, word, bit)
    with pytest.raises(IndexError):
        gs.check()
    if gs.status is _sticky():
        assert int(gs.status.item()) == 0, what


@pytest.mark.parametrize("k", range(4), ids=["src-neg", "dst-n-last", "src-2p32", "dst-neg-first"])
def test_status_bit_1(k, pack):
    from gnn_hex_amd import ops
    cases, ptr, eptr = _bad_id_cases()
    name, ei = cases[k]
    n = int(ptr[-1])
    assert int(_sticky().item()) == 0
    gs = ops.GraphStructure(_dev(ei), n)                        # the general build first
    _expect_flag(gs, 1, "general build, " + name)
    assert gs.status is not _sticky() and int(_sticky().item()) == 0
    b = len(ptr) - 1
    eid = _dev(ei)
    for form in ("int32 ranges", "ptr64", "pack_b", "pack_b + edge offsets"):
        if form == "int32 ranges":
            gs = ops.GraphStructure(eid, n, _dev(ptr, torch.int32), b)
        elif form == "ptr64":
            gs = ops.GraphStructure(eid, n, torch.empty(b + 1, dtype=torch.int32, device="cuda"), b, ptr64=_dev(ptr))
        else:
            t = _dev(ei)
            if form.endswith("offsets"):
                t._hex_edge_ptr = _dev(eptr)
            gs = ops.GraphStructure.grouped(t, n, b, _dev(ptr), pack=pack, device_blocks=True)
        _expect_flag(gs, 1, "grouped build (%s), %s" % (form, name))


def test_status_bit_4_edge_between_graphs_and_ungrouped_batch(pack):
    from gnn_hex_amd import ops
    ei, ptr, eptr = _status_batch()
    n = int(ptr[-1])
    assert int(_sticky().item()) == 0
    cross = ei.copy()
    cross[0, int(eptr[1]) + 1] = 2                               # an edge of graph 1 whose source lies in graph 0
    blocks = [ei[:, int(eptr[g]):int(eptr[g + 1])] for g in range(3)]
    ungrouped = np.concatenate([blocks[1], blocks[0], blocks[2]], 1)      # graph 1's edges in front of graph 0's
    eptr_u = np.array([0, blocks[1].shape[1], int(eptr[2]), int(eptr[3])])
    for name, bad, ep in (("edge between two graphs", cross, eptr), ("batch not grouped", ungrouped, eptr_u)):
        for form, gs, _ in _grouped_forms(bad, n, ptr, ep, pack, edge_ptr_forms=False):
            _expect_flag(gs, 4, "%s (%s)" % (name, form))
        t = _dev(bad)
        t._hex_edge_ptr = _dev(ep)
        gs = ops.GraphStructure.grouped(t, n, len(ptr) - 1, _dev(ptr), pack=pack, device_blocks=True)
        _expect_flag(gs, 4, "%s (pack_b + edge offsets)" % name)


@pytest.mark.parametrize("kind", ["a0>a1", "a1>e", "first!=0", "last!=e"])
def test_status_bit_4_edge_offsets_that_do_not_tile(kind, pack):
    from gnn_hex_amd import ops
    ei, ptr, eptr = _status_batch()
    n, e = int(ptr[-1]), ei.shape[1]
    ep = eptr.copy()
    if kind == "a0>a1":
        ep[1], ep[2] = eptr[2], eptr[1]
    elif kind == "a1>e":
        ep[2] = e + 2
    elif kind == "first!=0":
        ep[0] = 1
    else:
        ep[3] = e - 1
    assert int(_sticky().item()) == 0
    t = _dev(ei)
    t._hex_edge_ptr = _dev(ep)
    gs = ops.GraphStructure.grouped(t, n, 3, _dev(ptr), pack=pack, device_blocks=True)
    _expect_flag(gs, 4, "edge offsets %s (%s)" % (ep.tolist(), kind))


def test_sticky_word_survives_a_clean_build_until_check(pack):
    """A flagged build followed by a clean one: the clean build ORs nothing and clears nothing, so the bit is still there; check()
    reports and clears it; the next clean build checks clean and matches the reference."""
    from gnn_hex_amd import ops
    ei, ptr, eptr = _status_batch()
    n, e, b = int(ptr[-1]), ei.shape[1], 3
    want = csr_reference(ei[0], ei[1], n)
    bad = ei.copy()
    bad[0, 0] = n - 1                                            # an edge of graph 0 from a node of graph 2
    assert int(_sticky().item()) == 0
    for build in (lambda a: ops.GraphStructure(_dev(a), n, _dev(ptr, torch.int32), b),
                  lambda a: ops.GraphStructure.grouped(_dev(a), n, b, _dev(ptr), pack=pack, device_blocks=True)):
        flagged = build(bad)
        clean = build(ei)
        torch.cuda.synchronize()
        assert int(_sticky().item()) == 4
        with pytest.raises(IndexError):
            clean.check()
        flagged.check()                                          # cleared by the first report
        again = build(ei)
        _assert_same(_got(again, n, e), want, "clean build after check()")
        again.check()
        assert int(_sticky().item()) == 0


def test_general_build_clears_its_own_status_word():
    """The general build owns its status word: a poisoned word in front of a clean build reads 0 afterwards, in front of a flagged
    build exactly 1."""
    from gnn_hex_amd import _lib, ops
    L = _lib.lib()
    ei, ptr, _ = _status_batch()
    n, e = int(ptr[-1]), ei.shape[1]
    bad = ei.copy()
    bad[1, 3] = n
    for edges, word in ((ei, 0), (bad, 1)):
        ws_bytes = L.hexgnn_csr_workspace_bytes(n, e)
        rp, rpt = (torch.full((n + 1,), POISON, dtype=torch.int32, device="cuda") for _ in range(2))
        col, col_t = (torch.full((e,), POISON, dtype=torch.int32, device="cuda") for _ in range(2))
        status = torch.full((1,), POISON, dtype=torch.int32, device="cuda")
        ws = torch.full(((ws_bytes + 3) // 4,), POISON, dtype=torch.int32, device="cuda")
        invdeg = torch.empty(n, device="cuda")
        eid = _dev(edges)
        rc = L.hexgnn_csr_build(n, e, eid[0].data_ptr(), eid[1].data_ptr(), rp.data_ptr(), col.data_ptr(), rpt.data_ptr(),
                                col_t.data_ptr(), invdeg.data_ptr(), status.data_ptr(), ws.data_ptr(), ws_bytes, ops._stream())
        assert rc == 0
        torch.cuda.synchronize()
        assert int(status.item()) == word
    assert int(_sticky().item()) == 0


# ---- E. device-built row-block table ------------------------------------------------------------------------------------------------------

def _cycle(b):
    return [g % 6 for g in range(b)]


TABLES = {
    "splits": [0, 1, 127, 128, 129, 0, 191, 192, 193, 320, 321, 0],
    "fill-128": [64, 64, 1],
    "zeros": [0] * 7,
    "b511": _cycle(511), "b512": _cycle(512), "b513": _cycle(513), "b1025": _cycle(1025),
}


def _table_fits(sizes, n=None):
    from gnn_hex_amd import data, ops
    n = sum(sizes) if n is None else n
    budget = ops.stack_block_budget()
    return len(data.blocks_for_order(sizes)) - 1 <= budget and (n + 127) // 128 <= budget, budget


def _device_table(sizes, n, pack):
    from gnn_hex_amd import ops
    ptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    ei = torch.empty((2, 0), dtype=torch.int64, device="cuda")
    assert getattr(ei, "_hex_blocks", None) is None
    gs = ops.GraphStructure.grouped(ei, n, len(sizes), _dev(ptr), pack=pack, device_blocks=True)
    torch.cuda.synchronize()
    assert gs.blocks is not None, "no table was built"
    tbl, budget = gs.blocks
    assert budget == ops.stack_block_budget() and tbl.numel() == budget + 1
    return gs, tbl.cpu().numpy(), budget, ptr


def test_table_cases_fit_the_budget():
    """Only the 1025-graph case may be skipped for a small block budget: every other case has to run."""
    for name, sizes in TABLES.items():
        fits, budget = _table_fits(sizes)
        assert fits or name == "b1025", "%s does not fit a budget of %d blocks" % (name, budget)
    assert _table_fits([100, 100], 300)[0]


@pytest.mark.parametrize("name", list(TABLES))
def test_device_block_table(name, pack):
    from gnn_hex_amd import data
    sizes = TABLES[name]
    n = sum(sizes)
    fits, budget = _table_fits(sizes)
    if not fits:
        print("%s: needs %d blocks, the budget is %d" % (name, len(data.blocks_for_order(sizes)) - 1, budget))
        pytest.skip("%s needs more row blocks than the budget of %d" % (name, budget))
    gs, tbl, budget, ptr = _device_table(sizes, n, pack)
    starts = data.blocks_for_order(sizes)
    want = np.array(starts + [n] * (budget + 1 - len(starts)))
    assert np.array_equal(tbl, want), "%s: table %s, blocks_for_order %s" % (name, tbl[:len(starts) + 2], starts)
    # the CSR workgroups ran behind the table's one: an edgeless batch is all-zero row starts and 1 / max(0, 1)
    assert np.array_equal(gs.gptr.cpu().numpy(), ptr)
    assert not gs.rowptr.any() and not gs.rowptr_t.any() and bool((gs.invdeg[:n] == 1).all())
    gs.check()


def test_device_block_table_ranges_inconsistent_with_n(pack):
    """Ranges that end at 200 for a batch of 300 rows: the plain 128-row partition of n."""
    gs, tbl, budget, _ = _device_table([100, 100], 300, pack)
    assert np.array_equal(tbl, np.array([0, 128, 256] + [300] * (budget - 2)))
    gs.check()


# ---- F. graph_ptr, pad_rows, unpad_rows ---------------------------------------------------------------------------------------------------

def _graph_ptr_cases():
    # 40 graphs over 1000 nodes (four workgroups): 0..2 empty, 3..10 hold nodes 0..255, 11..14 are empty -- the run straddles node
    # 256, so the first thread of the second workgroup fills it --, 15..36 hold the rest with 20 and 21 empty, 37..39 empty
    counts = np.zeros(40, dtype=np.int64)
    counts[3:11] = 32
    counts[15:37] = 37
    counts[[20, 21]] = 0
    counts[36] += 1000 - counts.sum()
    big = np.repeat(np.arange(40), counts)
    return {
        "n0-b0": (np.zeros(0, dtype=np.int64), 0),
        "n0-b3": (np.zeros(0, dtype=np.int64), 3),
        "n1": (np.array([2]), 5),
        "empties": (np.array([2, 2, 2, 5, 6, 6]), 9),
        "n1000": (big, 40),
        "clamped": (np.array([-3, -1, 0, 1, 1, 4, 6, 8, 8]), 6),
    }


@pytest.mark.parametrize("name", ["n0-b0", "n0-b3", "n1", "empties", "n1000", "clamped"])
def test_graph_ptr(name):
    from gnn_hex_amd import _lib, ops
    batch, b = _graph_ptr_cases()[name]
    n = batch.size
    if name == "n1000":
        assert n == 1000 and batch[255] == 10 and batch[256] == 15 and batch[0] == 3 and batch[-1] == 36 and (n + 255) // 256 == 4
        assert not ((batch == 20) | (batch == 21)).any()
    want = np.searchsorted(np.clip(batch, 0, b - 1), np.arange(b + 1), "left")
    out = torch.full((b + 3,), POISON, dtype=torch.int32, device="cuda")
    bd = _dev(batch)
    rc = _lib.lib().hexgnn_graph_ptr(n, b, bd.data_ptr() if n else None, out.data_ptr(), ops._stream())
    assert rc == 0
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert np.array_equal(got[:b + 1], want), (name, got[:b + 1], want)
    assert (got[b + 1:] == POISON).all()


def test_graph_ptr_through_ops():
    from gnn_hex_amd import ops
    batch = np.array([1, 1, 1, 4, 4, 5])
    gptr, b = ops.graph_ptr(_dev(batch), None, batch.size, "cuda")
    assert b == 6 and np.array_equal(gptr.cpu().numpy(), np.searchsorted(batch, np.arange(7), "left"))
    ptr = torch.tensor([0, 3, 3, 6])
    gptr, b = ops.graph_ptr(None, ptr, 6, "cuda")
    assert b == 3 and gptr.dtype == torch.int32 and torch.equal(gptr.cpu().long(), ptr)


def _bits(t):
    return t.contiguous().view(torch.int32).cpu().numpy()


@pytest.mark.parametrize("hidden", [2, 35, 110, 128, 129, 255, 256])
def test_pad_and_unpad_rows(hidden):
    """pad: the source is a column slice of a wider tensor (stride hidden + 3), the destination starts as NaN -- every data column
    bit-equal, every pad column exactly 0.  unpad: into a column slice of a wider NaN canvas -- only the `hidden` columns change.
    pad -> unpad is the identity."""
    from gnn_hex_amd import _lib, ops
    L = _lib.lib()
    hp = L.hexgnn_padded_width(hidden)
    assert hp >= hidden and hp % 16 == 0
    gen = torch.Generator().manual_seed(hidden)
    for n in (0, 1, 300):
        wide = torch.randn(n, hidden + 3, generator=gen)
        if n:
            wide[0, 1] = -0.0
            wide[n - 1, hidden] = float("inf")
            wide[n // 2, 1 + hidden // 2] = 1e-41                  # a denormal: copied, not flushed
        wide = wide.cuda()
        src = wide[:, 1:1 + hidden]
        padded = torch.full((n, hp), float("nan"), device="cuda")
        rc = L.hexgnn_pad_rows(n, hidden, src.data_ptr() if n else None, hidden + 3, padded.data_ptr() if n else None,
                               ops._stream())
        assert rc == 0
        torch.cuda.synchronize()
        assert np.array_equal(_bits(padded[:, :hidden]), _bits(src)), (hidden, n)
        assert not _bits(padded[:, hidden:]).any(), (hidden, n)    # +0.0 in every pad column
        canvas = torch.full((n, hidden + 5), float("nan"), device="cuda")
        rc = L.hexgnn_unpad_rows(n, hidden, padded.data_ptr() if n else None, canvas[:, 2:].data_ptr() if n else None,
                                 hidden + 5, ops._stream())
        assert rc == 0
        torch.cuda.synchronize()
        assert np.array_equal(_bits(canvas[:, 2:2 + hidden]), _bits(src)), (hidden, n)
        assert bool(torch.isnan(canvas[:, :2]).all()) and bool(torch.isnan(canvas[:, 2 + hidden:]).all()), (hidden, n)
