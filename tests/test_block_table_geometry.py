"""The batch of tests/test_gpu_block_tables.py on the host: its three row-block tables are what gnn_hex_amd.data makes of its graph
sizes, and every table has the waves that the one-launch stack kernels treat differently (tests/helpers.py: table_geometry) --
counted here without a device, and asserted again by every GPU test before it launches anything."""
import numpy as np
import pytest
import torch

from gnn_hex_amd.data import block_groups, blocks_for_order, pack_order
from helpers import (TABLE_GROUPS, TABLE_ORDER, TABLE_P_EDGE, TABLE_P_EDGE_SPARSE, TABLE_SIZES, TABLE_STARTS, TABLE_WAVES, TABLE_WAVES_MIN,
                     TABLE_WAVES_SPARSE, TABLE_WAVES_SPARSE_MIN, feature_batch, reorder_graphs, table_geometry)


def _batch(table, p_edge=TABLE_P_EDGE):
    x, ei, bv, ptr = feature_batch(TABLE_SIZES, 2, seed=102, p_edge=p_edge)
    if table == "packed":
        x, ei, bv, ptr, _ = reorder_graphs(x, ei, ptr, TABLE_ORDER)
    return x, ei, bv, ptr


def test_the_tables_are_what_the_collation_makes():
    assert sum(TABLE_SIZES) == 392
    assert blocks_for_order(TABLE_SIZES) == TABLE_STARTS["head64"] == [0, 64, 132, 200, 240, 304, 369, 392]
    assert blocks_for_order(TABLE_SIZES, head=0) == TABLE_STARTS["head0"] == [0, 128, 240, 368, 392]
    order, starts = pack_order(TABLE_SIZES)
    assert order == TABLE_ORDER == [0, 2, 1, 6, 5, 4, 3]
    assert starts == TABLE_STARTS["packed"] == [0, 64, 132, 200, 264, 329, 392]
    assert [b - a for a, b in zip(starts, starts[1:])] == [64, 68, 68, 64, 65, 63]
    assert TABLE_GROUPS == {"head64": (3, [0, 3, 6, 7]), "head0": (2, [0, 2, 4])}
    for name, (budget, groups) in TABLE_GROUPS.items():
        assert block_groups(TABLE_SIZES, TABLE_STARTS[name], budget) == groups


def test_reordering_keeps_every_graph():
    x, ei, bv, ptr = _batch("head64")
    xp, eip, bvp, ptrp, rows = reorder_graphs(x, ei, ptr, TABLE_ORDER)
    assert ptrp.tolist() == [0, 200, 329, 369, 386, 389, 391, 392] and torch.equal(xp, x[rows])
    assert torch.equal(bvp, torch.bucketize(torch.arange(392), ptrp[1:], right=True))
    assert eip.shape == ei.shape
    old = {(int(a), int(b)) for a, b in ei.t().tolist()}
    assert {(int(rows[a]), int(rows[b])) for a, b in eip.t().tolist()} == old
    gp = torch.bucketize(eip[1], ptrp[1:], right=True)
    assert bool((gp[1:] >= gp[:-1]).all())                             # still grouped by graph, in graph order


@pytest.mark.parametrize("table", ["head64", "head0", "packed"])
def test_every_table_has_its_waves(table):
    x, ei, bv, ptr = _batch(table)
    got = table_geometry(ei, TABLE_STARTS[table], ptr)
    print(table, got)
    assert {k: got[k] for k in TABLE_WAVES[table]} == TABLE_WAVES[table]
    assert all(got[k] >= v for k, v in TABLE_WAVES_MIN[table].items())
    assert got["next_only"] + got["prev_only"] + got["both"] + got["far"] == got["remote_short"] + got["remote_long"]
    assert got["idle"] == sum(8 - (b - a + 15) // 16 for a, b in zip(TABLE_STARTS[table], TABLE_STARTS[table][1:]))
    if table == "head0":
        assert got["mixed"] == [1, 3] and got["last_row_first"] == [3]
    else:
        assert got["mixed"] == [] and got["last_row_first"] == []


def test_head0_at_the_lower_edge_probability():
    """p_edge 0.04: the other side of head0's split into remote waves with and without a long row."""
    assert TABLE_P_EDGE_SPARSE == 0.04
    x, ei, bv, ptr = _batch("head0", TABLE_P_EDGE_SPARSE)
    got = table_geometry(ei, TABLE_STARTS["head0"], ptr)
    print(got)
    assert (got["remote_short"], got["remote_long"]) == (12, 1)
    assert {k: got[k] for k in TABLE_WAVES_SPARSE} == TABLE_WAVES_SPARSE
    assert all(got[k] >= v for k, v in TABLE_WAVES_SPARSE_MIN.items())


def test_geometry_of_a_hand_made_table():
    """Six rows in blocks [0, 2), [2, 4), [4, 6); row 0 reads rows 2 and 4, row 3 reads row 1, row 5 reads rows 0..4."""
    ei = np.array([[2, 4, 1, 0, 1, 2, 3, 4], [0, 0, 3, 5, 5, 5, 5, 5]])
    got = table_geometry(ei, [0, 2, 4, 6])
    assert got["far"] == 2 and got["prev_only"] == 1 and got["next_only"] == got["both"] == 0
    assert got["remote_short"] == 3 and got["remote_long"] == 0 and got["idle"] == 21
    assert got["slot3"] == 1                                            # row 5: slot 3 holds row 3, of block 1
