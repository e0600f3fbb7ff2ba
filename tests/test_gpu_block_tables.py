"""Row-block tables and groups of the one-launch SAGE stack kernels (gnn_hex_amd/csrc/sage_stack.hip) under the float64 rule, at one
width per tile count.

tests/test_gpu_stack_blocks.py and tests/test_gpu_block_groups.py compare HIP with HIP (table against default blocks against
per-layer launches, 3e-5 / 1e-4 scale-relative) at hidden 110 on Hex boards: a cut Hex-13 graph has two blocks (block_of() never
bisects), no row has more than 16 neighbours (no table block holds a long row), and hidden 17..48 (NT = 3, no LDS row copy), 49..96
(NT = 4..6) and 113..128 (NT = 8, per-slot factors in the backward) never ran on a table.  This file runs the table path against the
float64 oracle with the machinery of tests/helpers.py, on the smallest batch that has every geometric case.

Batch: feature_batch([200, 40, 129, 1, 2, 3, 17], c_in 2, seed 102, p_edge 0.06), 392 rows.  Tables (asserted literally, with the
wave counts of helpers.table_geometry, by tests/test_block_table_geometry.py without a device and again by every test here before it
launches anything):
  head64   blocks_for_order(sizes)            [0, 64, 132, 200, 240, 304, 369, 392]   the 200-row graph spans three blocks: bisection
  head0    blocks_for_order(sizes, head=0)    [0, 128, 240, 368, 392]                 block 1 = a 72-row tail + a whole graph; block 3
                                                                                      starts with a cut graph's last row
  packed   pack_order(sizes)                  [0, 64, 132, 200, 264, 329, 392]        order [0, 2, 1, 6, 5, 4, 3]: batch, R, selections
                                                                                      and targets carried to it
  default  no table                           the yardstick: a failure on a table alone isolates the table path
Groups: head64 under a budget of 3 -> [0, 3, 6, 7], head0 under 2 -> [0, 2, 4] (data.block_groups), attached with
attach_block_groups.

Parity rule (tests/test_gpu_feature_counts.py, unchanged): ground truth is the oracle in float64, the fp32 oracle gives the
yardstick.  max |y - y64| (|Q - Q64|, out_v) <= max(3 x the fp32 oracle's, 5e-6); every gradient tensor ||g - g64|| / ||g64|| <=
max(3 x the fp32 oracle's own, 2e-3) (absolute 1e-6 for a vanishing tensor), and the same for the two columns of layer 0's d_wl /
d_wr.  Inputs are chosen from the float64 oracle alone and asserted by every test: feature sensitivity > 0.1, layer-0 column share
>= 2 %, output spread >= 0.5, every |g|max >= 1e-2, no ReLU input within 2^-16 rms of zero; the weight seed is the first below 400
that meets them.

A. ops.sage_stack on a four-layer stack (raw first layer, the other three in one launch: waits at it = 1 and it = 2), loss
   scale * sum(y * R) / n.  Hidden 35, 64, 80, 96, 110, 128 (NT = 3..8; 35 and 110 pad columns) on all four tables; groups at 35, 110,
   128 on both group lists.  Weight seeds (the same in the caller's and in the packed order): 35 -> 1, 64 -> 4, 80 -> 0, 96 -> 7,
   110 -> 12, 128 -> 7; every width keeps its fourth layer; loss scale 1 everywhere.
A'. Hidden 35, 110, 128 on head0 with the same sizes at p_edge 0.04: twelve of its thirteen remote-reading waves have no row above 16
   neighbours (at 0.06 twelve of thirteen have one).  Weight seeds 0, 4, 36.
B. The Q-network on the layer-major path (qnet_hip_call(..., layered=True)), 3 body + 2 head layers as one stack of five, structure
   GraphStructure.grouped over an edge_index that carries the table: hidden 35, 110, 128 on packed and head0 in mode 0, hidden 110 on
   packed in modes 1 and 2 and on the head64 groups.  Weight seeds: 35 -> 2, 110 -> 38, 128 -> 7.
C. Hidden 35, 64, 128 on head64 with the blocks delayed unevenly (hexgnn_debug_stack_mode(-1, seed), seeds 11, 12, 13): the bits of
   the undelayed run, status word 0.

Every case of A and B asserts, with CUs un-reserved, that the block budget holds the table, that the structure carries the attached
table (or groups), through hexgnn_profile_enable / hexgnn_profile_read that the hidden layers ran as ONE forward and ONE backward
launch (one per group), and that hexgnn_stack_status(1) == 0 afterwards: a fall-back to per-layer launches or to default blocks
cannot pass for coverage.

Worst figures measured on the MI355X (printed per case; in brackets the fp32 oracle's own distance from float64 in the same case):

  section                       max |y - y64| / |Q - Q64|   out_v                 gradient tensor, relative   layer-0 column, relative
  A, A'. stack, tables, groups  4.41e-6 (3.07e-6)           --                    6.85e-7 (5.81e-7)           6.83e-7 (3.85e-7)
  B. Q-network, layer-major     1.63e-6 (1.39e-6)           3.7e-8 (1.5e-8)       6.62e-6 (6.57e-6)           2.69e-6 (6.21e-7)

The closest any case came to its bound: 0.48 on y (hidden 110: 4.41e-6 of 3 x 3.07e-6); every gradient figure is below 0.01 of
its bound.  Of the 127 printed figures 2 lie above three times the fp32 oracle's own and so rest on a floor (2e-3:
the layer-0 column gnn.convs.0.lin_r.weight[:, 0] at hidden 128 on packed and head0, 2.7e-6); no output figure needs the 5e-6 constant.

Against libraries with one value-only change in sage_stack.hip (built aside, never committed), all 45 cases of this file and
tests/test_gpu_stack_blocks.py, test_gpu_block_groups.py, test_gpu_stack_kernels.py once each:
  (a) the forward's add of the tail ring's fourth landing buffer takes tb[2][c] instead of xs[c]: all 24 cases at hidden 64, 80, 96
      and 110 of A, A' and B fail on y / Q (|y - y64| 1.0..2.5, |Q - Q64| 0.8..0.9), default blocks included; hidden 35 and 128 (no
      tail ring) and section C (bits against bits) pass.  Of the three existing files 11 tests fail (hidden 64 and 110).
  (b) the backward's add of a remote row is scaled by the wave's own 1 / deg (sc) instead of the source row's (rs[rb]): the same 24
      cases fail on convs.0.lin_l.weight (relative 0.15..0.47; the Q-network 0.08..0.34), every y and Q passes.  8 existing tests
      fail.  The variant "rs[0] instead of rs[rb]" is no change at all: the backward's ring has ONE landing buffer (kGRing = 1), so rb
      is 0 in every instantiation of that line.
  (c) the backward at the all-global widths scales every slot by ns[0] instead of ns[k]: all 18 cases at hidden 35 and 128 fail
      (convs.0.lin_l.weight relative 0.40..0.77, the Q-network 0.04), hidden 64..110 pass.  Of the existing files only
      test_gpu_stack_kernels.py's per-layer comparison at hidden 48 and 128 fails, on default blocks: no existing test ran these
      widths on a table.
The three changes also fail on the default blocks: each alters a value that every cut graph reads, whatever cut it.  What only a table
can get wrong (block_of's answer, a block start that is no multiple of 128, the groups' clamps) decides addresses and waits, which
a value-only change must not touch (a wrong wait shows as a stale row or as a time-out, not as a value of its own); those are held
by the literal tables, the wave counts, the launch counts and the status word above, and by section C.
"""
import contextlib
import copy
import ctypes

import pytest
import torch

from helpers import (TABLE_GROUPS, TABLE_ORDER, TABLE_P_EDGE, TABLE_P_EDGE_SPARSE, TABLE_SIZES, TABLE_STARTS, TABLE_WAVES,
                     TABLE_WAVES_MIN, TABLE_WAVES_SPARSE, TABLE_WAVES_SPARSE_MIN, QnetCases, abs_bound, check_grads, feature_batch,
                     reorder_graphs, stack_oracle, stack_params, table_geometry)

pytestmark = pytest.mark.gpu

K_SAGE_FWD, K_SAGE_BWD = 0, 1                     # HEXGNN_K_SAGE_FWD / _BWD
ROWS, GRAPHS = 392, 7
WIDTHS = [35, 64, 80, 96, 110, 128]               # NT = 3, 4, 5, 6, 7, 8
LAYERS = {h: 4 for h in WIDTHS}                   # (a width without a weight seed below SEEDS would drop to 3: none does)
TABLES = ["default", "head64", "head0", "packed"]
_stacks, _geometry = {}, {}
_q_plain = QnetCases(TABLE_SIZES, 3, 2, p_edge=TABLE_P_EDGE)
_q_packed = QnetCases(TABLE_SIZES, 3, 2, p_edge=TABLE_P_EDGE, order=TABLE_ORDER)


@pytest.fixture(autouse=True)
def _fp32():
    from gnn_hex_amd import ops
    ops.set_fused(True)
    ops.set_math("fp32")
    yield
    ops.set_fused(True)
    ops.set_math("fp32")


def _blocks(table):
    return len(TABLE_STARTS[table]) - 1 if table != "default" else (ROWS + 127) // 128


def _has_its_waves(table, p_edge=TABLE_P_EDGE):
    """The table's literal starts and wave counts, on the host (once per session), before anything touches the device."""
    from gnn_hex_amd.data import block_groups, blocks_for_order, pack_order
    if table == "default":
        return
    if p_edge != TABLE_P_EDGE:
        assert (table, p_edge) == ("head0", TABLE_P_EDGE_SPARSE)
        if "sparse" not in _geometry:
            _, ei, _, ptr = feature_batch(TABLE_SIZES, 2, seed=102, p_edge=p_edge)
            _geometry["sparse"] = table_geometry(ei, TABLE_STARTS[table], ptr)
        got = _geometry["sparse"]
        assert {k: got[k] for k in TABLE_WAVES_SPARSE} == TABLE_WAVES_SPARSE, got
        assert all(got[k] >= v for k, v in TABLE_WAVES_SPARSE_MIN.items()), got
        return
    if table not in _geometry:
        x, ei, _, ptr = feature_batch(TABLE_SIZES, 2, seed=102, p_edge=TABLE_P_EDGE)
        if table == "packed":
            x, ei, _, ptr, _ = reorder_graphs(x, ei, ptr, TABLE_ORDER)
        assert int(x.shape[0]) == ROWS and ptr.numel() == GRAPHS + 1
        _geometry[table] = table_geometry(ei, TABLE_STARTS[table], ptr)
    got = _geometry[table]
    assert {"head64": blocks_for_order(TABLE_SIZES), "head0": blocks_for_order(TABLE_SIZES, head=0),
            "packed": pack_order(TABLE_SIZES)[1]}[table] == TABLE_STARTS[table]
    assert pack_order(TABLE_SIZES)[0] == TABLE_ORDER
    if table in TABLE_GROUPS:
        budget, groups = TABLE_GROUPS[table]
        assert block_groups(TABLE_SIZES, TABLE_STARTS[table], budget) == groups
    assert {k: got[k] for k in TABLE_WAVES[table]} == TABLE_WAVES[table], got
    assert all(got[k] >= v for k, v in TABLE_WAVES_MIN[table].items()), got
    if table == "head0":
        assert len(got["mixed"]) >= 1 and len(got["last_row_first"]) >= 1, got


@contextlib.contextmanager
def _library(nb):
    """CUs un-reserved, the status word cleared, the block budget above the table; reserve, stack mode and profile restored."""
    from gnn_hex_amd import _lib, ops
    L = _lib.lib()
    prev = L.hexgnn_stack_reserve_cus(0)
    try:
        torch.cuda.synchronize()
        L.hexgnn_stack_status(1)
        assert ops.stack_block_budget(torch.device("cuda")) >= nb
        yield L
    finally:
        L.hexgnn_stack_reserve_cus(prev)
        L.hexgnn_debug_stack_mode(-1, 0)
        L.hexgnn_profile_enable(-1)


def _read_launches(L):
    cnt, tot = ctypes.c_int(0), ctypes.c_float(0)
    torch.cuda.synchronize()
    assert L.hexgnn_profile_read(ctypes.byref(cnt), ctypes.byref(tot)) == 0
    L.hexgnn_profile_enable(-1)
    return cnt.value


def _attach(ei_dev, table, grouped):
    """The table on the device copy of the edge list; returns the launches one direction of the hidden layers must take."""
    from gnn_hex_amd.data import attach_block_groups, attach_blocks
    if table == "default":
        assert not grouped
        return 1
    if grouped:
        groups = TABLE_GROUPS[table][1]
        attach_block_groups(ei_dev, TABLE_STARTS[table], groups)
        return len(groups) - 1
    attach_blocks(ei_dev, TABLE_STARTS[table])
    return 1


def _carries(gs, table, grouped):
    if table == "default":
        assert gs.blocks is None and gs.groups is None
    elif grouped:
        assert gs.blocks is None and gs.groups is not None
        assert gs.groups[0].cpu().tolist() == TABLE_STARTS[table] and gs.groups[1] == _blocks(table)
        assert list(gs.groups[2]) == TABLE_GROUPS[table][1]
    else:
        assert gs.groups is None and gs.blocks is not None
        assert gs.blocks[0].cpu().tolist() == TABLE_STARTS[table] and gs.blocks[1] == _blocks(table)


# ---- A. the stack alone ---------------------------------------------------------------------------------------------------------

def _stack_oracle(hidden, packed, p_edge=TABLE_P_EDGE):
    key = (hidden, packed, p_edge)
    if key not in _stacks:
        _stacks[key] = stack_oracle("stack", 2, hidden, TABLE_SIZES, layers=LAYERS[hidden], p_edge=p_edge,
                                    order=TABLE_ORDER if packed else None)
    o = _stacks[key]
    assert o["ok"] and len(o["m"].convs) == LAYERS[hidden] and tuple(o["x"].shape) == (ROWS, 2), o["text"]
    return o


def _stack_step(L, o, hidden, table, grouped=False, count=True):
    """One forward and backward of the oracle's stack through ops.sage_stack on ``table``: (y, gradients, forward launches,
    backward launches of the hidden layers)."""
    from gnn_hex_amd import ops
    ei_dev = o["ei"].cuda()
    _attach(ei_dev, table, grouped)
    gs = ops.GraphStructure(ei_dev, ROWS)
    _carries(gs, table, grouped)
    dev = copy.deepcopy(o["m"]).cuda()
    xd, rd = o["x"].cuda(), o["r"].cuda()
    fwd = bwd = None
    if count:
        L.hexgnn_profile_enable(K_SAGE_FWD)
    y = ops.sage_stack(xd, gs, 2, hidden, list(dev.convs))
    if count:
        fwd = _read_launches(L)
        L.hexgnn_profile_enable(K_SAGE_BWD)
    ((y * rd).sum() * o["scale"] / ROWS).backward()
    if count:
        bwd = _read_launches(L)
    torch.cuda.synchronize()
    return y.detach(), [p.grad for p in stack_params(dev)[1]], fwd, bwd


def _stack_case(hidden, table, grouped=False, p_edge=TABLE_P_EDGE):
    _has_its_waves(table, p_edge)
    o = _stack_oracle(hidden, table == "packed", p_edge)
    with _library(_blocks(table)) as L:
        want = len(TABLE_GROUPS[table][1]) - 1 if grouped else 1
        y, grads, fwd, bwd = _stack_step(L, o, hidden, table, grouped)
        assert (fwd, bwd) == (want, want), "hidden layers: %s forward and %s backward launches, %d expected" % (fwd, bwd, want)
        assert L.hexgnn_stack_status(1) == 0
    tag = "stack hidden %d %s%s%s" % (hidden, table, " groups" if grouped else "",
                                      "" if p_edge == TABLE_P_EDGE else " p_edge %g" % p_edge)
    assert tuple(y.shape) == (ROWS, hidden)
    ey = abs_bound(tag, "y", y, o["y32"], o["y64"], 5e-6)
    worst, worst_col = check_grads(tag, stack_params(o["m"])[0], grads, o["g32"], o["g64"], 2)
    print("%s: |y-y64| %.3g (oracle32 %.3g); worst gradient tensor %s rel %.3g (oracle32 %.3g); worst layer-0 column %s rel %.3g "
          "(oracle32 %.3g)" % (tag, ey[0], ey[1], worst[2], worst[0], worst[1], worst_col[2], worst_col[0], worst_col[1]))


@pytest.mark.parametrize("table", TABLES)
@pytest.mark.parametrize("hidden", WIDTHS)
def test_stack_on_every_table(hidden, table):
    _stack_case(hidden, table)


@pytest.mark.parametrize("table", ["head64", "head0"])
@pytest.mark.parametrize("hidden", [35, 110, 128])
def test_stack_in_groups(hidden, table):
    _stack_case(hidden, table, grouped=True)


@pytest.mark.parametrize("hidden", [35, 110, 128])
def test_stack_on_head0_without_long_rows(hidden):
    """The same sizes at p_edge 0.04: twelve of head0's thirteen remote-reading waves have no row above 16 neighbours (at 0.06
    twelve have one), so a remote wave here does not wait for its own block."""
    _stack_case(hidden, "head0", p_edge=TABLE_P_EDGE_SPARSE)


# ---- B. the Q-network on the layer-major path -----------------------------------------------------------------------------------

QNET = [(h, 0, t, False) for h in (35, 110, 128) for t in ("packed", "head0")] + [(110, 1, "packed", False), (110, 2, "packed", False),
                                                                                 (110, 0, "head64", True)]


@pytest.mark.parametrize("hidden,mode,table,grouped", QNET, ids=["h%d-m%d-%s%s" % (h, m, t, "-groups" if g else "")
                                                                for h, m, t, g in QNET])
def test_qnet_layer_major_on_a_table(hidden, mode, table, grouped):
    from gnn_hex_amd import ops
    _has_its_waves(table)
    cases = _q_packed if table == "packed" else _q_plain
    o = cases.oracle(2, hidden, mode)
    ptr = cases.batch(2)[3]
    assert ptr.tolist() == ([0, 200, 329, 369, 386, 389, 391, 392] if table == "packed" else [0, 200, 240, 369, 370, 372, 375, 392])
    with _library(_blocks(table)) as L:
        def structure():
            ei_dev, ptr_dev = cases.dev(2)[1:3]
            want = _attach(ei_dev, table, grouped)
            return ops.GraphStructure.grouped(ei_dev, ROWS, GRAPHS, ptr_dev), want

        kept = {}
        gs, want = structure()
        _, (q, out_v, grads) = cases.run_case(2, hidden, mode, True, gs=gs, out=kept)
        assert kept["gs"] is gs
        _carries(kept["gs"], table, grouped)
        for cls in (K_SAGE_FWD, K_SAGE_BWD):                            # the same call again, its launches counted
            gs2, _ = structure()
            L.hexgnn_profile_enable(cls)
            cases.run_case(2, hidden, mode, True, gs=gs2)
            got = _read_launches(L)
            assert got == want, "hidden layers: %d launches of class %d, %d expected" % (got, cls, want)
        assert L.hexgnn_stack_status(1) == 0
    cases.check("qnet hidden %d mode %d %s%s" % (hidden, mode, table, " groups" if grouped else ""), o, q, out_v, grads, 2, mode,
                False)


# ---- C. progress counters at the widths that never ran delayed -------------------------------------------------------------------

@pytest.mark.parametrize("hidden", [35, 64, 128])
def test_delayed_blocks_give_the_same_bits(hidden):
    _has_its_waves("head64")
    o = _stack_oracle(hidden, False)
    with _library(_blocks("head64")) as L:
        y0, g0, fwd, bwd = _stack_step(L, o, hidden, "head64")
        assert (fwd, bwd) == (1, 1)
        assert bool(torch.isfinite(y0).all())
        for seed in (11, 12, 13):
            L.hexgnn_debug_stack_mode(-1, seed)
            y, g, _, _ = _stack_step(L, o, hidden, "head64", count=False)
            assert torch.equal(y, y0), "hidden %d seed %d: y differs" % (hidden, seed)
            assert len(g) == len(g0) and all(torch.equal(a, b) for a, b in zip(g, g0)), "hidden %d seed %d: a gradient differs" \
                % (hidden, seed)
        L.hexgnn_debug_stack_mode(-1, 0)
        assert L.hexgnn_stack_status(1) == 0
