"""Groups of a row-block table (data.block_groups / pack_groups, hexgnn_sage_stack_call.group_starts): a batch whose table has more
blocks than can be resident at once runs the one-launch stack kernels group after group, each group a range of blocks that
holds whole graphs.  Host side only: the cutting, and the entry points' argument checks (made before the device is touched)."""
import ctypes
import itertools
import random

import pytest

from gnn_hex_amd.data import block_groups, blocks_for_order, pack_groups, pack_order

MIX63 = [k * k + 2 for k in (5 + g % 9 for g in range(63))]          # Hex-5..13 round robin; Hex-k has k^2 + 2 nodes


def _caller(sizes, budget):
    starts = blocks_for_order(sizes)
    return len(starts) - 1, block_groups(sizes, starts, budget)


@pytest.mark.parametrize("sizes,budget,blocks,groups", [
    (MIX63, 24, 63, [0, 23, 47, 63]),
    (MIX63, 16, 63, [0, 16, 32, 48, 63]),
    ([171] * 24, 16, 48, [0, 16, 32, 48]),
    ([171] * 256, 256, 512, [0, 256, 512]),                           # uniform Hex-13 replay batch
    ([171] * 256, 192, 512, [0, 192, 384, 512]),                      # ... while the overlap reserve is on
    ([227] * 170, 256, 510, [0, 255, 510]),                           # Hex-15: three blocks per graph
    ([123] * 256, 192, 256, [0, 192, 256]),                           # Hex-11 on a 113..128-wide model, reserve on
], ids=["mix63-24", "mix63-16", "hex13x24", "hex13x256", "hex13x256-reserve", "hex15x170", "hex11x256-reserve"])
def test_worked_cases_in_the_callers_order(sizes, budget, blocks, groups):
    assert _caller(sizes, budget) == (blocks, groups)


def test_worked_case_in_pack_order():
    order, starts = pack_order(MIX63)
    assert len(starts) - 1 == 58
    assert block_groups([MIX63[g] for g in order], starts, 24) == [0, 24, 48, 58]


def test_a_graph_longer_than_the_budget_has_no_groups():
    sizes = [363] * 5                                                 # Hex-19: four blocks per graph
    starts = blocks_for_order(sizes)
    assert len(starts) - 1 == 20 and block_groups(sizes, starts, 2) is None
    assert pack_groups(sizes, max_blocks=2) == ([0, 1, 2, 3, 4], None, None)
    assert block_groups(sizes, starts, 4) == [0, 4, 8, 12, 16, 20]


def test_table_cap_and_degenerate_arguments():
    sizes = [171] * 257                                               # 514 blocks: above the 512 counters of a call
    starts = blocks_for_order(sizes)
    assert len(starts) - 1 == 514 and block_groups(sizes, starts, 256) is None
    assert block_groups([171], blocks_for_order([171]), 256) == [0, 2]            # everything fits: one group
    assert block_groups([171], None, 256) is None and block_groups([171], blocks_for_order([171]), 0) is None
    assert block_groups([171, 5], blocks_for_order([171]), 256) is None           # a table of another batch
    assert pack_groups([]) == ([], None, None)


def _cut_candidates(sizes, starts):
    rows, row = {0}, 0
    for s in sizes:
        row += s
        rows.add(row)
    return [i for i, s in enumerate(starts) if s in rows]


def _check_groups(sizes, starts, groups, budget):
    nb = len(starts) - 1
    cand = _cut_candidates(sizes, starts)
    assert groups[0] == 0 and groups[-1] == nb
    assert all(g in cand for g in groups), "a cut is not a graph start"
    assert all(0 < b - a <= budget for a, b in zip(groups, groups[1:]))
    inner = [c for c in cand if 0 < c < nb]
    if len(inner) <= 12:                      # no valid cutting has fewer groups
        for k in range(len(groups) - 2):
            for cuts in itertools.combinations(inner, k):
                g = [0] + list(cuts) + [nb]
                assert not all(b - a <= budget for a, b in zip(g, g[1:])), "fewer groups: %r against %r" % (g, groups)


@pytest.mark.parametrize("seed", range(40))
def test_random_sizes(seed):
    rng = random.Random(seed)
    few = seed % 2 == 0                       # half of the draws small enough for the brute-force minimum
    sizes = [rng.choice([3, 17, 27, 51, 64, 100, 128, 129, 171, 256, 300, 402]) for _ in range(rng.randint(1, 9 if few else 90))]
    starts = blocks_for_order(sizes)
    nb = len(starts) - 1
    for budget in sorted({1, 2, 3, 4, 5, max(1, nb // 3), max(1, nb // 2), nb}):
        groups = block_groups(sizes, starts, budget)
        cand = _cut_candidates(sizes, starts)
        feasible = all(b - a <= budget for a, b in zip(cand, cand[1:]))
        assert (groups is not None) == feasible
        if groups is not None:
            _check_groups(sizes, starts, groups, budget)
        order, pstarts, pgroups = pack_groups(sizes, max_blocks=budget)
        assert sorted(order) == list(range(len(sizes)))
        if pgroups is None:
            assert pstarts is None and order == list(range(len(sizes)))
        else:
            psizes = [sizes[g] for g in order]
            assert pstarts[0] == 0 and pstarts[-1] == sum(sizes) and all(0 < b - a <= 128 for a, b in zip(pstarts, pstarts[1:]))
            _check_groups(psizes, pstarts, pgroups, budget)
            # the better of pack_order's two layouts, the head-block form on a tie
            n_head = block_groups(*_layout(sizes, 64), budget)
            n_flat = block_groups(*_layout(sizes, 0), budget)
            best = min(len(g) for g in (n_head, n_flat) if g is not None)
            assert len(pgroups) == best
            if n_head is not None and len(n_head) == best:
                assert pstarts == _layout(sizes, 64)[1]


def _layout(sizes, head):
    from gnn_hex_amd.data import _pack_layout
    order, starts = _pack_layout(sizes, 128, head)
    return [sizes[g] for g in order], starts


def test_pack_order_and_blocks_for_order_keep_their_results():
    sizes = [(5 + g % 9) ** 2 + 2 for g in range(256)]
    order, starts = pack_order(sizes)
    assert len(starts) - 1 <= 256 and pack_order(sizes, max_blocks=200)[1] is not None
    assert pack_order([171] * 256, max_blocks=256) == (list(range(256)), None)     # over the budget: still no plain table
    assert pack_groups([171] * 256, max_blocks=256)[2] == [0, 256, 512]
    assert pack_groups(MIX63, max_blocks=24)[2] == [0, 24, 46]                     # the 128-row pieces need fewer blocks here


def _ints(vals):
    return (ctypes.c_int * len(vals))(*vals)


@pytest.mark.parametrize("direction", ["forward", "backward"])
def test_group_lists_are_validated_on_the_host(direction):
    from gnn_hex_amd import _lib
    L = _lib.lib()
    table = _ints([0] * 600)                  # stands in for the device table: a rejected call never reads it
    one = ctypes.c_void_p(16)                 # (nor any other pointer)

    def call(block_starts, num_blocks, group_starts, num_groups):
        ptrs = {name: one for name, kind in _lib.SageStackCall._fields_ if kind is ctypes.c_void_p}
        d = _lib.SageStackCall(**dict(
            ptrs, struct_bytes=_lib.SAGE_STACK_CALL_BYTES, n=640, c_in=110, hidden=110, num_layers=3, x_stride=112, need_backward=1,
            flags=0, wl=None, bl=None, wr=None, workspace_bytes=1 << 30, nw=None, nb=None, n_live=None, dx=None, tap_layer=-1,
            tap_out=None, block_starts=ctypes.cast(block_starts, ctypes.c_void_p), num_blocks=num_blocks,
            group_starts=ctypes.cast(group_starts, ctypes.c_void_p), num_groups=num_groups))
        return (L.hexgnn_sage_stack_call_forward if direction == "forward" else L.hexgnn_sage_stack_call_backward)(d, None)

    assert call(None, 0, _ints([0, 5]), 1) == -1                      # groups without a table
    assert call(table, 5, None, 2) == -1                              # ... without a list
    assert call(table, 5, _ints([0, 3, 2, 5]), 3) == -1               # not ascending
    assert call(table, 5, _ints([1, 3, 5]), 2) == -1                  # wrong first entry
    assert call(table, 5, _ints([0, 3, 4]), 2) == -1                  # wrong last entry
    assert call(table, 5, _ints([0, 2, 2, 5]), 3) == -1               # an empty group
    assert call(table, 513, _ints([0, 256, 513]), 2) == -1            # more blocks than progress counters
    assert call(table, 5, _ints([0, 5]), -1) == -1
