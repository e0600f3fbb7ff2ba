"""GPU: n-step transitions assembled and stored on the device (hexgnn_transitions_assemble, hexgnn_replay_store_dev,
multi_env_manager.DeviceTransitionFeed, DeviceRollout.run_continue) against the host path run on the SAME rollout arrays:
``run_end`` -> ``RolloutStitcher.assemble`` -> ``put_block``.  Integer logic, exact fp64 products and the same sum order: every
comparison is ``torch.equal`` / ``==``, nothing has a tolerance.  (The host path itself is held to oracle/env_ref.py by
tests/test_gpu_replay.py::test_vectorised_transition_assembly_equals_list_form.)"""
import copy

import numpy as np
import pytest
import torch

from helpers import model_args

pytestmark = pytest.mark.gpu

SENTINEL = -77


def _model(seed=0):
    from gnn_hex_amd.models import get_pre_defined
    torch.manual_seed(seed)
    return get_pre_defined("modern_two_headed", model_args(3, 35)).cuda()


def _setup(hex_size, k, T, n_steps, prune, eps, seed, graph=False):
    from gnn_hex_amd.multi_env_manager import DeviceRollout, Env_manager
    model = _model(seed)
    mgr = Env_manager(k, hex_size, gamma=0.97, n_steps=list(n_steps), prune_exploratories=prune)
    mgr.reset()
    rollout = DeviceRollout(mgr, model, steps=T, eps=eps, graph=graph)
    torch.manual_seed(1000 + seed)
    return model, mgr, rollout


def _buffers(hex_size, capacity, poison=True):
    from gnn_hex_amd.replay import GraphReplayBuffer
    out = []
    for _ in range(2):
        buf = GraphReplayBuffer(capacity, hex_size, prioritized=True, alpha=0.5)
        if poison:          # every ring slot starts as a sentinel: a slot no store names must keep it
            buf.adj.fill_(0x5a5a5a5a5a5a5a5a)
            buf.alive.fill_(7)
            buf.side.fill_(9)
            buf.action.fill_(SENTINEL)
            buf.reward.fill_(-2.5)
            buf.sizes_dev.fill_(SENTINEL)
        out.append(buf)
    return out


def _poison_lists(feed):
    for t in (feed.src_step, feed.env, feed.action, feed.next_step):
        t.fill_(SENTINEL)
    feed.reward.fill_(-2.5)
    feed.done.fill_(5)


def _assert_lists_equal_blocks(feed, blocks, tag):
    """The device lists and counts against the two TransitionBlocks, entry for entry; entries behind the counts untouched."""
    torch.cuda.synchronize()
    count = feed.count.cpu().numpy()
    for s, blk in enumerate(blocks):
        n = len(blk)
        assert int(count[s]) == n, "%s side %d: %d transitions on the device, %d on the host" % (tag, s, int(count[s]), n)
        assert n <= feed.list_len
        for name in ("src_step", "env", "action", "next_step"):
            got = getattr(feed, name)[s].cpu().numpy()
            assert (got[:n] == getattr(blk, name)).all(), (tag, s, name)
            assert (got[n:] == SENTINEL).all(), (tag, s, name, "entries behind the count were written")
        rew = feed.reward[s].cpu().numpy()
        assert rew[:n].tobytes() == np.ascontiguousarray(blk.reward, dtype=np.float32).tobytes(), (tag, s, "reward")
        assert (rew[n:] == -2.5).all()
        done = feed.done[s].cpu().numpy()
        assert (done[:n] == blk.done.astype(np.uint8)).all() and (done[n:] == 5).all(), (tag, s, "done")


def _assert_buffers_equal(a, b, tag, max_sizes=True):
    for name in ("adj", "alive", "side", "action", "reward", "done", "sizes_dev", "sum_tree", "min_tree", "max_priority"):
        assert torch.equal(getattr(a, name), getattr(b, name)), "%s: %s differs" % (tag, name)
    assert (a.pos, a.size) == (b.pos, b.size), (tag, a.pos, a.size, b.pos, b.size)
    for name in ("n_nodes", "n_edges", "side_host"):
        assert (getattr(a, name) == getattr(b, name)).all(), "%s: host mirror %s differs" % (tag, name)
    if max_sizes:
        assert (a._max_nodes, a._max_edges) == (b._max_nodes, b._max_edges), tag
    if a.size:
        assert a.mover_side() == b.mover_side(), tag
    words = b._ring_words.cpu().tolist()
    assert words == [b.pos, b.size], "%s: the device's ring words %r, the host's %r" % (tag, words, [b.pos, b.size])


def _candidates(n_steps, T, k, first):
    """Windows one push considers: every start move once per n_step (the first push has no windows that reach back)."""
    return sum((T - 2 * n + 1 if first else T) * k for n in n_steps)


# ---- 1. assemble alone ------------------------------------------------------------------------------------------------------

WARM_PLIES = 12        # short rollouts start mid-game, so that three of them see games end (a Hex-5 game has at most 25 moves)


@pytest.mark.parametrize("short", [True, False], ids=["T-keep", "T-16"])
@pytest.mark.parametrize("k", [1, 6, 65])
@pytest.mark.parametrize("prune", [True, False], ids=["prune", "no-prune"])
@pytest.mark.parametrize("n_steps", [[1], [2], [1, 3]], ids=["n1", "n2", "n1-3"])
def test_assemble_equals_the_stitched_host_assembly(n_steps, prune, k, short):
    from gnn_hex_amd.multi_env_manager import DeviceTransitionFeed, RolloutStitcher
    keep = 2 * max(n_steps) - 1
    T = keep + 1 if short else 16
    _, mgr, rollout = _setup(5, k, T, n_steps, prune, 0.5, seed=3)
    for _ in range(WARM_PLIES // T if short else 0):
        rollout.run()
    feed = DeviceTransitionFeed(rollout, *_buffers(5, 4096, poison=False))
    stitch = RolloutStitcher(mgr)
    assert feed.keep == stitch.keep == keep and feed.list_len == (T // 2) * len(n_steps) * k
    terminal, full, emitted, candidates = [0, 0], 0, 0, 0
    for r in range(3):
        res = rollout.run()                                   # the host's read-back of the run ...
        blocks = stitch.assemble(res)
        _poison_lists(feed)
        feed.push()                                           # ... and the device's view of the same arrays
        _assert_lists_equal_blocks(feed, blocks, "rollout %d" % r)
        for s, blk in enumerate(blocks):
            terminal[s] += int(blk.done.sum())
            full += int((~blk.done).sum())
            emitted += len(blk)
        candidates += _candidates(n_steps, T, k, r == 0)
    feed.settle()
    # What the rollouts must have exercised: properties of the host blocks alone, asked of the cases with at least 6 envs (one
    # env with pruning at eps = 0.5 keeps a 4-move window with probability 1/8: a dozen windows can all be pruned)
    if not prune:
        assert emitted == candidates
    if k >= 6:
        assert full > 0, "no full window"
        assert terminal[0] > 0 and terminal[1] > 0, "terminal transitions per side: %r" % terminal
        if prune:
            assert emitted < candidates, "no window was dropped by pruning"


# ---- 2. store -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("hex_size", [5, 8, 12], ids=["hex5-W1", "hex8-W2", "hex12-W3"])
def test_store_equals_put_block(hex_size):
    from gnn_hex_amd.multi_env_manager import DeviceTransitionFeed, RolloutStitcher
    k, T, C = 10, 16, 100
    _, mgr, rollout = _setup(hex_size, k, T, [2], True, 0.1, seed=4)
    assert mgr._words == {5: 1, 8: 2, 12: 3}[hex_size]
    A, B = _buffers(hex_size, C), _buffers(hex_size, C)
    feed = DeviceTransitionFeed(rollout, *B)
    stitch = RolloutStitcher(mgr)
    wrapped = overwrote = False
    for r in range(3):
        res = rollout.run()
        sizes_host = mgr._sizes.copy()                        # (run_end's: a record that settles later is older, and must not win)
        blocks = stitch.assemble(res)
        before = [(buf.pos, buf.size) for buf in A]
        for buf, blk in zip(A, blocks):
            buf.put_block(blk)
        _poison_lists(feed)
        feed.push()
        _assert_lists_equal_blocks(feed, blocks, "rollout %d" % r)
        out = feed.settle()
        assert out["games"] == int(res.dones.sum())
        wins = sum(1 for t in res.infos for info in t if info and info["episode_metrics"]["return"] == 1)
        lens = sum(info["episode_metrics"]["length"] for t in res.infos for info in t if info)
        assert (out["maker_wins"], out["length_sum"]) == (wins, lens)
        assert mgr._sizes.dtype == sizes_host.dtype and (mgr._sizes == sizes_host).all()
        for s, (a, b) in enumerate(zip(A, B)):
            _assert_buffers_equal(a, b, "rollout %d side %d" % (r, s))
            leaves = feed.leaves[s].cpu().numpy()
            n = len(blocks[s])
            assert (leaves[:n] == (before[s][0] + np.arange(n)) % C).all() and (leaves[n:] == -1).all()
        for (pos, size), buf, blk in zip(before, A, blocks):
            wrapped |= pos + len(blk) > C
            overwrote |= size == C and len(blk) > 0
    assert wrapped and overwrote, "the ring did not wrap (%r) / no live slot was overwritten (%r)" % (wrapped, overwrote)
    # (slots no store named still hold their sentinel only while the ring is not full: compared with A throughout)


# ---- 3. edge limit ------------------------------------------------------------------------------------------------------------

def test_edge_limit_drops_what_a_draw_could_not_hold():
    from gnn_hex_amd.multi_env_manager import DeviceTransitionFeed, RolloutStitcher, TransitionBlock
    k, T, C = 6, 16, 100
    _, mgr, rollout = _setup(5, k, T, [1], True, 0.3, seed=5)
    e_start = int(mgr._base_sizes[0, 1])
    limit = e_start - 1
    A, B = _buffers(5, C), _buffers(5, C)
    feed = DeviceTransitionFeed(rollout, *B, edge_limit=limit)
    stitch = RolloutStitcher(mgr)
    seen = [0, 0]
    for r in range(3):
        res = rollout.run()
        blocks = stitch.assemble(res)
        dropped = 0
        for s, (buf, blk) in enumerate(zip(A, blocks)):
            edges = lambda step, env: e_start if step < 0 else (blk.obs_list[step].edge_off[env + 1] -      # noqa: E731
                                                                  blk.obs_list[step].edge_off[env])
            es = np.array([edges(int(a), int(e)) for a, e in zip(blk.src_step, blk.env)], dtype=np.int64)
            en = np.array([edges(int(a), int(e)) for a, e in zip(blk.next_step, blk.env)], dtype=np.int64)
            keep = (es <= limit) & (en <= limit)
            assert not keep[blk.done].any()                  # a terminal transition's next state is the start position
            dropped += int((~keep).sum())
            seen[s] = max(seen[s], int(max(es.max(), en.max())) if len(es) else 0)
            buf.put_block(TransitionBlock(blk.obs_list, blk.start_obs, blk.maker_side, blk.src_step[keep], blk.env[keep],
                                          blk.action[keep], blk.reward[keep], blk.next_step[keep], blk.done[keep]))
        assert dropped > 0 and sum(len(b) for b in blocks) > dropped, "nothing dropped, or nothing kept"
        feed.push()
        with pytest.raises(RuntimeError, match=r"^%d transitions were dropped" % dropped):
            feed.settle()
        assert feed._pending is None                          # the record is consumed, the mirrors are current
        for s, (a, b) in enumerate(zip(A, B)):
            _assert_buffers_equal(a, b, "rollout %d side %d" % (r, s), max_sizes=False)
            assert b._max_edges == seen[s] > limit >= a._max_edges, (b._max_edges, seen[s], a._max_edges)      # the largest SEEN
            assert int(b.sizes_dev[:, 1][b.sizes_dev[:, 1] != SENTINEL].max()) <= limit


# ---- 4. closed loop -----------------------------------------------------------------------------------------------------------

def _loop(device_store):
    from gnn_hex_amd.multi_env_manager import DeviceRollout, DeviceTransitionFeed, Env_manager, RolloutStitcher
    from gnn_hex_amd.replay import GraphedUpdate
    online = _model(6)
    target = copy.deepcopy(online)
    with torch.no_grad():
        for p in target.parameters():
            p.mul_(0.9)
    opt = torch.optim.Adam(online.parameters(), lr=1e-3, fused=True, capturable=True)
    mgr = Env_manager(6, 5, gamma=0.97, n_steps=[2])
    mgr.reset()
    rollout = DeviceRollout(mgr, online, steps=16, eps=0.3, graph=True)
    bufs = _buffers(5, 256, poison=False)
    feed = DeviceTransitionFeed(rollout, *bufs) if device_store else None
    stitch = RolloutStitcher(mgr)
    upd, snaps = {}, []
    torch.manual_seed(12)
    for it in range(6):
        if device_store:
            if it == 0:
                rollout.run_begin()
            else:
                rollout.run_continue()
            feed.push()
        else:
            for buf, blk in zip(bufs, stitch.assemble(rollout.run())):
                buf.put_block(blk)
        for s, buf in enumerate(bufs):
            if s not in upd:
                upd[s] = GraphedUpdate(buf, online, target, opt, 16, 0.97 ** 2, loss_fn="mse", graph=True)
            upd[s].step(beta=0.5)
        state = mgr._state()
        snaps.append(([p.detach().clone() for p in online.parameters()],
                      [(b.sum_tree.clone(), b.min_tree.clone(), b.max_priority.clone()) for b in bufs], state))
    if device_store:
        feed.settle()
        assert feed.games > 0
    return snaps, bufs, mgr


def test_closed_loop_equals_the_host_loop_bit_for_bit():
    host, bufs_h, mgr_h = _loop(False)
    dev, bufs_d, mgr_d = _loop(True)
    for it, (h, d) in enumerate(zip(host, dev)):
        for i, (a, c) in enumerate(zip(h[0], d[0])):
            assert torch.equal(a, c), "iteration %d: parameter %d differs" % (it + 1, i)
        for s, (a, c) in enumerate(zip(h[1], d[1])):
            assert all(torch.equal(x, y) for x, y in zip(a, c)), "iteration %d: priority trees of side %d differ" % (it + 1, s)
        assert sorted(h[2]) == sorted(d[2])
        for name in h[2]:
            assert (h[2][name] == d[2][name]).all(), "iteration %d: env state %s differs" % (it + 1, name)
    assert not torch.equal(host[0][0][0], host[-1][0][0])
    for a, b in zip(bufs_h, bufs_d):
        assert (a.pos, a.size) == (b.pos, b.size) and a.size > 16
    assert (mgr_h._sizes == mgr_d._sizes).all()


# ---- 5. refusals and protocol ----------------------------------------------------------------------------------------------------

def test_refusals_and_protocol():
    from gnn_hex_amd.multi_env_manager import DeviceRollout, DeviceTransitionFeed, Env_manager, RolloutStitcher
    from gnn_hex_amd.replay import GraphReplayBuffer
    k, T = 6, 16
    model, mgr, rollout = _setup(5, k, T, [2], True, 0.3, seed=7)
    L = (T // 2) * k
    good = lambda: GraphReplayBuffer(128, 5, prioritized=True)      # noqa: E731
    with pytest.raises(ValueError, match="prioritized"):
        DeviceTransitionFeed(rollout, good(), GraphReplayBuffer(128, 5, prioritized=False))
    with pytest.raises(ValueError, match="hex_size"):
        DeviceTransitionFeed(rollout, GraphReplayBuffer(128, 6, prioritized=True), good())
    with pytest.raises(ValueError, match="capacity"):
        DeviceTransitionFeed(rollout, good(), GraphReplayBuffer(L - 1, 5, prioritized=True))
    elsewhere = good()
    elsewhere.device = torch.device("cuda", torch.cuda.current_device() + 1)
    with pytest.raises(ValueError, match="another device"):
        DeviceTransitionFeed(rollout, elsewhere, good())
    one = good()
    with pytest.raises(ValueError, match="two buffers"):
        DeviceTransitionFeed(rollout, one, one)
    mgr3 = Env_manager(2, 5, gamma=0.97, n_steps=[3])
    mgr3.reset()
    with pytest.raises(ValueError, match="at least"):
        DeviceTransitionFeed(DeviceRollout(mgr3, model, steps=4, eps=0.1, graph=False), good(), good())

    A, B = [good(), good()], [good(), good()]
    feed = DeviceTransitionFeed(rollout, *B)
    stitch = RolloutStitcher(mgr)
    with pytest.raises(RuntimeError, match="issue one first"):
        feed.push()
    with pytest.raises(RuntimeError, match="run_begin"):
        rollout.run_continue()
    res = rollout.run()
    blocks = stitch.assemble(res)
    for buf, blk in zip(A, blocks):
        buf.put_block(blk)
    feed.push()
    with pytest.raises(RuntimeError, match="issue one first"):
        feed.push()                                           # the same run twice
    # len() of a buffer with an unsettled store: the settled value (it waits for the record), and the mirrors with it
    assert feed._pending is not None and B[0].size == 0
    assert len(B[0]) == len(A[0]) > 0 and feed._pending is None and len(B[1]) == len(A[1])
    # a host put_block after a device store lands behind it in the ring
    blocks2 = stitch.assemble(rollout.run())
    for buf, blk in zip(A, blocks2):
        buf.put_block(blk)
    feed.push()
    assert feed._pending is not None
    for s in (0, 1):
        A[s].put_block(blocks2[1 - s])                        # (any block: what matters is where it lands)
        B[s].put_block(blocks2[1 - s])                        # settles the device store first
        assert A[s]._sides == B[s]._sides and len(A[s]._sides[0]) == 2
        A[s]._sides, B[s]._sides = ({0}, {0}), ({0}, {0})     # (mover_side() refuses a buffer of both sides: not the point)
        _assert_buffers_equal(A[s], B[s], "host store behind a device store, side %d" % s)
    assert feed._pending is None
    # a continued run needs no run_end, and the next host-issued run needs its sizes settled
    rollout.run_continue()
    with pytest.raises(RuntimeError, match="settle"):
        rollout.run_begin()
    feed.push()
    feed.settle()
    rollout.run_begin()
    feed.push()
    # a manager reset under the feed
    mgr.reset()
    with pytest.raises(RuntimeError, match="reset, resized or stepped"):
        rollout.run_continue()
    rollout.run_begin()
    with pytest.raises(RuntimeError, match=r"feed\.reset\(\)"):
        feed.push()
    feed.reset()
    feed.push()
    assert feed.settle() is not None and feed.settle() is None
