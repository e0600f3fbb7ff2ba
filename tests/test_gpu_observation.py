"""GPU: ``gnn_hex_amd.observation.ObsTarget``, the one owner of the batched observation layout, taken on its own.

1. An exact target and a capacity target filled from the same boards agree bit for bit on the live prefix of every array, and
   the capacity target keeps its sentinel everywhere behind it -- from live envs (``observe_env``) and from a replay buffer's
   stored snapshots (``observe_states``; ``GraphReplayBuffer.sample``'s batch, which tests/test_gpu_replay.py ties to the env, is
   the reference there).
2. ``clear_tail`` empties exactly the CSR rows behind the live total, at Hex-12 (146 nodes per board: the path that needs it).
3. The degenerate exact targets (no graphs; graphs without edges) construct, host side only.
4. ``inputs``: fresh tensor objects over the same storage, each with the hints it was asked for.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SENTINEL = -7
INT_FIELDS = ("backmap", "batch_vec", "edge_local", "edge_global")


def _poison(t):
    t.x.fill_(float("nan"))
    t.gs.invdeg.fill_(float("nan"))
    for a in (t.gs.rowptr, t.gs.col) + tuple(getattr(t, f) for f in INT_FIELDS):
        a.fill_(SENTINEL)


def _random_moves(mgr, moves, rng):
    mgr.reset()
    for _ in range(moves):
        mgr.step([int(v[rng.integers(len(v))]) for v in mgr.get_valid_actions()])


def _assert_prefix_equal_and_tail_untouched(cap, ex, N, E):
    torch.cuda.synchronize()
    assert tuple(ex.x.shape) == (N, 3) and tuple(ex.edge_local.shape) == tuple(ex.edge_global.shape) == (2, E)
    assert 0 < N < cap.x.shape[0] and 0 < E < cap.E, "a tail behind the live rows and columns"
    assert torch.equal(cap.x[:N], ex.x) and torch.equal(cap.backmap[:N], ex.backmap)
    assert torch.equal(cap.batch_vec[:N], ex.batch_vec)
    assert torch.equal(cap.edge_local[:, :E], ex.edge_local) and torch.equal(cap.edge_global[:, :E], ex.edge_global)
    assert torch.equal(cap.gs.rowptr[:N + 1], ex.gs.rowptr) and torch.equal(cap.gs.col[:E], ex.gs.col[:E])
    assert torch.equal(cap.gs.invdeg[:N], ex.gs.invdeg[:N])
    assert int(ex.gs.rowptr[N]) == E and not torch.isnan(ex.x).any() and int(ex.gs.col[:E].min()) >= 0
    assert torch.isnan(cap.x[N:]).all() and torch.isnan(cap.gs.invdeg[N:]).all()
    assert (cap.gs.rowptr[N + 1:] == SENTINEL).all() and (cap.gs.col[E:] == SENTINEL).all()
    assert (cap.backmap[N:] == SENTINEL).all() and (cap.batch_vec[N:] == SENTINEL).all()
    assert (cap.edge_local[:, E:] == SENTINEL).all() and (cap.edge_global[:, E:] == SENTINEL).all()


# ---- 1. exact and capacity targets ---------------------------------------------------------------------------------------

def test_exact_and_capacity_targets_agree_from_live_envs():
    from gnn_hex_amd.multi_env_manager import Env_manager
    from gnn_hex_amd.observation import ObsTarget
    k = 6
    mgr = Env_manager(k, 5)
    _random_moves(mgr, 4, np.random.default_rng(0))
    sizes, nv, e_start = mgr._sizes, mgr._nv, int(mgr._base_sizes[0, 1])
    N, E = int(sizes[:, 0].sum()), int(sizes[:, 1].sum())
    assert len({tuple(s) for s in sizes.tolist()}) > 1 and (sizes[:, 0] < nv).all(), "sizes differ, below the start size"
    assert N <= k * nv and E <= k * e_start, "the capacity target holds these boards"
    ex = ObsTarget.exact(sizes, mgr.device)
    ex.observe_env(mgr._h)
    cap = ObsTarget.capacity(k, nv, e_start, mgr.device, zeroed=False)
    _poison(cap)
    cap.set_offsets(sizes)
    cap.observe_env(mgr._h)
    assert cap.node_off.tolist() == ex.node_off.tolist() == ex.node_off_host.tolist() and cap.node_off.dtype == torch.int32
    assert cap.edge_off.tolist() == ex.edge_off.tolist() == ex.edge_off_host.tolist() and cap.ptr is None
    _assert_prefix_equal_and_tail_untouched(cap, ex, N, E)
    # ... and the exact target is what observe() hands out
    obs = mgr.observe()
    assert torch.equal(obs.x, ex.x) and torch.equal(obs.edge_global, ex.edge_global) and torch.equal(obs.backmap, ex.backmap)
    assert obs.node_off == ex.node_off_host.tolist() and obs.edge_off == ex.edge_off_host.tolist()


def test_exact_and_capacity_targets_agree_from_stored_snapshots():
    from gnn_hex_amd.multi_env_manager import Env_manager
    from gnn_hex_amd.observation import ObsTarget
    from gnn_hex_amd.replay import GraphReplayBuffer
    rng = np.random.default_rng(1)
    mgr = Env_manager(6, 5, gamma=0.97, n_steps=[1])
    obs0 = obs = mgr.reset()
    states, actions, rewards, dones = [], [], [], []
    for _ in range(8):
        ranks = [int(rng.integers(2, obs.node_off[i + 1] - obs.node_off[i])) for i in range(mgr.num_envs)]
        obs, r, d, _ = mgr.step(mgr.validate_actions(obs, ranks))
        states.append(obs); actions.append(ranks); rewards.append(r); dones.append(d)
    expl = [np.zeros(mgr.num_envs, dtype=bool)] * 8
    buf = GraphReplayBuffer(32, 5, prioritized=True)
    buf.put(mgr.get_transitions(obs0, states, actions, rewards, dones, expl)[0])
    assert len(buf) >= 3
    k = 3
    idx, _, want, _, _, _, _ = buf.sample(k, generator=torch.Generator(device="cuda").manual_seed(2))
    host = idx.cpu().numpy()
    sizes = np.stack([buf.n_nodes[host], buf.n_edges[host]], axis=1)
    N, E = int(sizes[:, 0].sum()), int(sizes[:, 1].sum())
    e_cap = buf.edge_capacity()
    assert N <= k * buf.nv and E <= k * e_cap, "the capacity target holds these boards"
    slots32 = idx.to(torch.int32)
    ex = ObsTarget.exact(sizes, buf.device, with_ptr=True)
    ex.observe_states(buf.hex_size, buf.adj, buf.alive, buf.side, slots32)
    cap = ObsTarget.capacity(k, buf.nv, e_cap, buf.device, zeroed=False, with_ptr=True)
    _poison(cap)
    cap.set_offsets(sizes)
    cap.observe_states(buf.hex_size, buf.adj, buf.alive, buf.side, slots32)
    _assert_prefix_equal_and_tail_untouched(cap, ex, N, E)
    ws = want.edge_index._hex_csr
    assert torch.equal(ex.x, want.x) and torch.equal(ex.edge_global, want.edge_index) and torch.equal(ex.batch_vec, want.batch)
    assert torch.equal(ex.ptr, want.ptr) and ex.ptr.dtype == torch.int64 and ex.ptr.tolist() == ex.node_off.tolist()
    assert torch.equal(ex.gs.rowptr, ws.rowptr) and torch.equal(ex.gs.col[:E], ws.col[:E])
    assert torch.equal(ex.gs.invdeg[:N], ws.invdeg[:N])


# ---- 2. clear_tail -------------------------------------------------------------------------------------------------------

def test_clear_tail_empties_the_rows_behind_the_live_total():
    from gnn_hex_amd.multi_env_manager import Env_manager
    from gnn_hex_amd.observation import ObsTarget
    k = 3
    mgr = Env_manager(k, 12)
    nv, e_start = mgr._nv, int(mgr._base_sizes[0, 1])
    assert nv == 146
    cap = ObsTarget.capacity(k, nv, e_start, mgr.device, zeroed=True, tail_clear=True)
    mgr.reset()
    cap.set_offsets(mgr._sizes)
    cap.observe_env(mgr._h)                      # the start position fills every row
    rng = np.random.default_rng(0)
    for _ in range(6):
        mgr.step([int(v[rng.integers(len(v))]) for v in mgr.get_valid_actions()])
    sizes = mgr._sizes
    N, E = int(sizes[:, 0].sum()), int(sizes[:, 1].sum())
    assert N < k * nv and E <= k * e_start, "the capacity target holds these boards, with a tail"
    cap.set_offsets(sizes)
    cap.observe_env(mgr._h)
    torch.cuda.synchronize()
    assert int(cap.node_off[k]) == N and int(cap.edge_off[k]) == E
    assert (cap.gs.rowptr[N + 1:] > E).any(), "a stale row behind the live total: without one this test shows nothing"
    before = {f: getattr(cap, f).clone() for f in ("x",) + INT_FIELDS}
    before.update(rowptr=cap.gs.rowptr.clone(), col=cap.gs.col.clone(), invdeg=cap.gs.invdeg.clone())
    cap.clear_tail()
    torch.cuda.synchronize()
    assert (cap.gs.rowptr[N + 1:] == E).all()
    assert torch.equal(cap.gs.rowptr[:N + 1], before["rowptr"][:N + 1])
    assert torch.equal(cap.gs.col, before["col"]) and torch.equal(cap.gs.invdeg, before["invdeg"])
    for f in ("x",) + INT_FIELDS:
        assert torch.equal(getattr(cap, f), before[f]), f


# ---- 3. degenerate exact targets (host-side shape logic: nothing is launched) -----------------------------------------------

def test_degenerate_exact_targets_construct():
    from gnn_hex_amd.observation import ObsTarget
    none = ObsTarget.exact(np.zeros((0, 2), dtype=np.int64), "cuda", with_ptr=True)
    assert none.k == 0 and none.E == 0 and tuple(none.x.shape) == (0, 3)
    assert tuple(none.edge_local.shape) == tuple(none.edge_global.shape) == (2, 0)
    assert none.node_off.tolist() == none.edge_off.tolist() == none.ptr.tolist() == [0]
    assert none.gs.n == 0 and none.gs.e == 0 and none.gs.rowptr.numel() == 1
    bare = ObsTarget.exact(np.array([[3, 0], [2, 0]], dtype=np.int64), "cuda")
    assert bare.k == 2 and bare.E == 0 and tuple(bare.x.shape) == (5, 3)
    assert tuple(bare.edge_local.shape) == tuple(bare.edge_global.shape) == (2, 0)
    assert bare.edge_local.dtype == bare.edge_global.dtype == torch.long
    assert bare.node_off.tolist() == [0, 3, 5] and bare.edge_off.tolist() == [0, 0, 0] and bare.ptr is None
    assert bare.gs.col.numel() == 1 and bare.gs.invdeg.numel() == 5
    tail = bare._tail()                        # without edges the kernels get x's address for both edge lists
    assert tail[2] == 0 and tail[5] == tail[6] == bare.x.data_ptr() != 0


# ---- 4. the model's inputs -----------------------------------------------------------------------------------------------

def test_inputs_are_fresh_views_with_their_own_hints():
    from gnn_hex_amd import ops
    from gnn_hex_amd.observation import ObsTarget
    k, nv = 2, 27
    cap = ObsTarget.capacity(k, nv, 10, "cuda", zeroed=True)
    x1, e1 = cap.inputs(True, nv)
    x2, e2 = cap.inputs(False, nv, live_rows=True)
    assert x1 is not x2 and x1 is not cap.x and e1 is not e2 and e1 is not cap.edge_global
    assert x1.data_ptr() == x2.data_ptr() == cap.x.data_ptr() and x1.shape == x2.shape == cap.x.shape
    assert e1.data_ptr() == e2.data_ptr() == cap.edge_global.data_ptr() and e1.shape == cap.edge_global.shape
    assert e1._hex_csr is cap.gs and e2._hex_csr is cap.gs
    assert x1._hex_is_maker is True and x2._hex_is_maker is False
    assert ops.hints_of(x1) == (True, nv) and ops.hints_of(x2) == (False, nv)
    assert not hasattr(x1, "_hex_live_rows") and not hasattr(cap.x, "_hex_is_maker")
    live = x2._hex_live_rows
    assert live.dtype == torch.int32 and live.numel() == 1 and live.data_ptr() == cap.node_off[k:].data_ptr()
    x1.add_(0)                                 # an in-place edit: the hints no longer describe the tensor
    assert ops.hints_of(x1) == (None, None)
