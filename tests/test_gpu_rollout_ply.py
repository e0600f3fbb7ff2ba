"""GPU: the self-play ply with the exploration schedule on the device (hexgnn_rollout_ply, hexgnn_frames_add,
multi_env_manager.EpsSchedule, DeviceRollout(eps=EpsSchedule)).  The one-launch ply is held to the three launches it replaces
(hexgnn_select_actions -> hexgnn_env_step -> hexgnn_env_export) on the same inputs, the epsilon it computes to
``EpsSchedule.value``, and a rollout with a constant schedule to the rollout with the same float, alone and under the device
store.  Integer logic and one float32 comparison: every check is ``==`` / ``torch.equal``, nothing has a tolerance."""
import ctypes as C

import numpy as np
import pytest
import torch

from helpers import model_args

pytestmark = pytest.mark.gpu

EINVAL = -1
DEV = "cuda"


def _model(layers, hidden, seed=0):
    from gnn_hex_amd.models import get_pre_defined
    torch.manual_seed(seed)
    return get_pre_defined("modern_two_headed", model_args(layers, hidden)).cuda()


def _manager(k, hex_size, **kw):
    from gnn_hex_amd.multi_env_manager import Env_manager
    mgr = Env_manager(k, hex_size, **kw)
    mgr.reset()
    return mgr


class _Ply:
    """Output arrays of one ply + a full export of the env handle behind it."""

    def __init__(self, mgr):
        k, nv, W = mgr.num_envs, mgr._nv, mgr._words
        z = lambda *shape, dtype: torch.full(shape, -9, dtype=dtype, device=DEV)      # noqa: E731
        self.h, self.k = mgr._h, k
        self.vert, self.rank, self.expl = z(k, dtype=torch.int32), z(k, dtype=torch.int32), z(k, dtype=torch.uint8)
        self.result = z(k, 5, dtype=torch.int32)
        self.adj, self.alive = z(k, nv, W, dtype=torch.int64), z(k, nv, dtype=torch.uint8)
        self.mt, self.tm = z(k, dtype=torch.int32), z(k, dtype=torch.int32)
        self.rm, self.rb = z(k, nv, dtype=torch.int16), z(k, nv, dtype=torch.int16)
        self.snap_adj, self.snap_alive = z(k, nv, W, dtype=torch.int64), z(k, nv, dtype=torch.uint8)
        self.eps = torch.full((1,), -1.0, dtype=torch.float32, device=DEV)

    def export(self):
        from gnn_hex_amd import _lib, ops
        _lib.check(_lib.lib().hexgnn_env_export(self.h, self.adj.data_ptr(), self.alive.data_ptr(), self.mt.data_ptr(),
                                               self.tm.data_ptr(), self.rm.data_ptr(), self.rb.data_ptr(), ops._stream()))

    def three_launches(self, gptr, q, backmap, eps, u, reset_maker_turn):
        from gnn_hex_amd import _lib, ops
        L, st = _lib.lib(), ops._stream()
        _lib.check(L.hexgnn_select_actions(self.k, gptr.data_ptr(), q.data_ptr(), backmap.data_ptr(), float(eps), u.data_ptr(),
                                           self.vert.data_ptr(), self.rank.data_ptr(), self.expl.data_ptr(), st))
        _lib.check(L.hexgnn_env_step(self.h, self.vert.data_ptr(), 1, 1, reset_maker_turn, self.result.data_ptr(), st))
        self.export()

    def call(self, gptr, q, backmap, u, sched, frames, frame_add, reset_maker_turn):
        from gnn_hex_amd import _lib
        return _lib.RolloutCall(
            struct_bytes=C.sizeof(_lib.RolloutCall), frame_add=frame_add, reset_maker_turn=reset_maker_turn,
            gptr=gptr.data_ptr(), q=q.data_ptr(), backmap=backmap.data_ptr(), u=u.data_ptr(), sched=sched.data_ptr(),
            frames=frames.data_ptr(), action_vertex=self.vert.data_ptr(), action_rank=self.rank.data_ptr(),
            exploratory=self.expl.data_ptr(), result=self.result.data_ptr(), adj_out=self.snap_adj.data_ptr(),
            alive_out=self.snap_alive.data_ptr(), eps_out=self.eps.data_ptr())

    def one_launch(self, *args):
        from gnn_hex_amd import _lib, ops
        c = self.call(*args)
        _lib.check(_lib.lib().hexgnn_rollout_ply(self.h, C.byref(c), ops._stream()), "hexgnn_rollout_ply")
        self.export()


def _assert_plies_equal(a, b, tag):
    for name in ("vert", "rank", "expl", "result", "adj", "alive", "mt", "tm", "rm", "rb"):
        assert torch.equal(getattr(a, name), getattr(b, name)), "%s: %s differs" % (tag, name)
    assert torch.equal(b.snap_adj, a.adj) and torch.equal(b.snap_alive, a.alive), "%s: the snapshot slot differs" % tag


# ---- 1. the kernel against the three launches it replaces ------------------------------------------------------------------

@pytest.mark.parametrize("e", [0.0, 0.5, 1.0], ids=["greedy", "eps-half", "eps-one"])
@pytest.mark.parametrize("k", [3, 70])
@pytest.mark.parametrize("hex_size,nv,words", [(5, 27, 1), (8, 66, 2), (12, 146, 3), (14, 198, 4), (16, 258, 5)],
                         ids=["hex5-W1", "hex8-W2", "hex12-W3", "hex14-W4", "hex16-generic"])
def test_one_launch_equals_select_step_export(hex_size, nv, words, k, e):
    from gnn_hex_amd import _lib, ops
    from gnn_hex_amd.multi_env_manager import EpsSchedule
    from gnn_hex_amd.observation import ObsTarget
    L = _lib.lib()
    mgr_a, mgr_b = _manager(k, hex_size), _manager(k, hex_size)
    assert (mgr_a._nv, mgr_a._words) == (nv, words)
    A, B = _Ply(mgr_a), _Ply(mgr_b)
    obs = ObsTarget.capacity(k, nv, int(mgr_a._base_sizes[0, 1]), DEV, zeroed=True)
    obs.set_offsets(mgr_a._sizes)
    sched = EpsSchedule(e, e, 1000).to_device(DEV)
    frames = torch.zeros(1, dtype=torch.int64, device=DEV)
    gen = torch.Generator().manual_seed(100 * hex_size + k)
    finished = explored = greedy = 0
    maker = True
    for t in range(32):
        obs.observe_env(A.h)
        # multiples of 0.25: ties are common, the first maximum decides
        q = (torch.randn(k * nv, generator=gen) * 4).round().div(4).to(DEV)
        u = torch.rand((k, 2), generator=gen).to(DEV)
        A.three_launches(obs.node_off, q, obs.backmap, e, u, int(not maker))
        B.one_launch(obs.node_off, q, obs.backmap, u, sched, frames, t * k, int(not maker))
        _assert_plies_equal(A, B, "ply %d" % t)
        assert B.eps.item() == float(np.float32(e))
        res = A.result.cpu().numpy()
        assert not res[:, 4].any(), "ply %d: an illegal action" % t
        finished += int((res[:, 0] >= 0).sum())
        explored += int(A.expl.sum())
        greedy += k - int(A.expl.sum())
        _lib.check(L.hexgnn_env_offsets(k, A.result.data_ptr(), obs.node_off.data_ptr(), obs.edge_off.data_ptr(), ops._stream()))
        maker = not maker
    assert int(frames.item()) == 0                         # the ply reads the counter, it never writes it
    if hex_size == 5:
        assert finished >= k, "32 plies on 25 cells: every env finishes a game"
    if e == 0.5:
        assert explored > 0 and greedy > 0
    elif e == 0.0:
        assert explored == 0
    else:
        assert greedy == 0


# ---- 2. the schedule as the kernel evaluates it ----------------------------------------------------------------------------

@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_epsilon_follows_the_schedule_and_a_rewritten_block(graph):
    from gnn_hex_amd.multi_env_manager import DeviceRollout, EpsSchedule
    k, T = 5, 16
    mgr = _manager(k, 5)
    sched = EpsSchedule(1.0, 0.0, 10 * k, burnin=2 * k)
    ro = DeviceRollout(mgr, _model(3, 16), steps=T, eps=sched, graph=graph)
    assert int(ro.frames.item()) == 0 and ro.frames_issued == 0        # the captured warm-up's frames are taken back
    ro.run()
    want = np.array([sched.value(t * k) for t in range(T)], dtype=np.float32)
    assert ro.eps_log.cpu().numpy().tobytes() == want.tobytes()
    assert want[0] == 1.0 and want[2] == 1.0 and 0.0 < want[5] < 1.0 and want[12] == 0.0      # burnin, decay, end: all inside one run
    assert int(ro.frames.item()) == T * k == ro.frames_issued
    ro.run()
    assert ro.eps_log.cpu().numpy().tobytes() == np.zeros(T, dtype=np.float32).tobytes()      # all `final`
    assert int(ro.frames.item()) == 2 * T * k == ro.frames_issued
    # another schedule, the counter rewound: the same rollout object (and capture) follows
    sched.update(init=0.5, final=0.25, decay_frames=7 * k, burnin=k)
    ro.set_frames(0)
    ro.run()
    want2 = np.array([sched.value(t * k) for t in range(T)], dtype=np.float32)
    assert want2[0] == 0.5 and want2[-1] == 0.25 and len(set(want2.tolist())) > 4
    assert ro.eps_log.cpu().numpy().tobytes() == want2.tobytes()
    assert int(ro.frames.item()) == T * k == ro.frames_issued
    ro.set_frames(3 * k + 1)                                               # a count that is no multiple of the env count
    ro.run()
    want3 = np.array([sched.value(3 * k + 1 + t * k) for t in range(T)], dtype=np.float32)
    assert ro.eps_log.cpu().numpy().tobytes() == want3.tobytes()


def test_fixed_epsilon_rollout_has_no_schedule_members():
    from gnn_hex_amd.multi_env_manager import DeviceRollout
    mgr = _manager(2, 5)
    ro = DeviceRollout(mgr, _model(3, 16), steps=2, eps=0.25, graph=False)
    assert ro.schedule is None and ro.eps == 0.25 and ro.frames is None and ro.eps_log is None
    with pytest.raises(RuntimeError, match="EpsSchedule"):
        ro.set_frames(0)
    ro.run()
    assert ro.frames_issued == 4


# ---- 3. a constant schedule against the same float ---------------------------------------------------------------------------

def _run_twice(hex_size, eps, graph):
    from gnn_hex_amd.multi_env_manager import DeviceRollout
    mgr = _manager(6, hex_size)
    ro = DeviceRollout(mgr, _model(3, 16, seed=hex_size), steps=8, eps=eps, graph=graph)
    out = []
    for r in range(2):
        torch.manual_seed(50 + r)
        res = ro.run()
        out.append((res, ro.adj.clone(), ro.alive.clone()))
    return out, mgr


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("hex_size", [5, 8, 12], ids=["hex5", "hex8", "hex12-layer-major"])
def test_constant_schedule_equals_the_float_rollout(hex_size, graph):
    from gnn_hex_amd.multi_env_manager import EpsSchedule
    e = 0.3
    want, mgr_f = _run_twice(hex_size, e, graph)
    got, mgr_s = _run_twice(hex_size, EpsSchedule(e, e, 1000), graph)
    assert mgr_f._nv > 128 if hex_size == 12 else mgr_f._nv <= 128
    explored = 0
    for r, ((a, a_adj, a_alive), (b, b_adj, b_alive)) in enumerate(zip(want, got)):
        for name in ("actions", "vertices", "rewards", "dones", "exploratories"):
            assert np.array_equal(getattr(a, name), getattr(b, name)), "run %d: %s differs" % (r, name)
        assert len(a.states) == len(b.states) == 9
        for t, (sa, sb) in enumerate(zip(a.states, b.states)):
            assert (sa.node_off, sa.edge_off, sa.is_maker) == (sb.node_off, sb.edge_off, sb.is_maker), (r, t)
        assert torch.equal(a_adj, b_adj) and torch.equal(a_alive, b_alive), "run %d: snapshot rings differ" % r
        explored += int(a.exploratories.sum())
    assert 0 < explored < 2 * 8 * 6
    assert (mgr_f._sizes == mgr_s._sizes).all()
    sa, sb = mgr_f._state(), mgr_s._state()
    for name in sa:
        assert (sa[name] == sb[name]).all(), name


# ---- 4. the device store on top ------------------------------------------------------------------------------------------------

def _assert_buffers_equal(a, b, tag):
    """(the comparison of tests/test_gpu_device_store.py)"""
    for name in ("adj", "alive", "side", "action", "reward", "done", "sizes_dev", "sum_tree", "min_tree", "max_priority"):
        assert torch.equal(getattr(a, name), getattr(b, name)), "%s: %s differs" % (tag, name)
    assert (a.pos, a.size) == (b.pos, b.size), (tag, a.pos, a.size, b.pos, b.size)
    for name in ("n_nodes", "n_edges", "side_host"):
        assert (getattr(a, name) == getattr(b, name)).all(), "%s: host mirror %s differs" % (tag, name)
    assert (a._max_nodes, a._max_edges) == (b._max_nodes, b._max_edges), tag
    words = b._ring_words.cpu().tolist()
    assert words == [b.pos, b.size], "%s: the device's ring words %r, the host's %r" % (tag, words, [b.pos, b.size])


def _store_loop(eps):
    from gnn_hex_amd.multi_env_manager import DeviceRollout, DeviceTransitionFeed
    from gnn_hex_amd.replay import GraphReplayBuffer
    mgr = _manager(6, 5, gamma=0.97, n_steps=[2])
    ro = DeviceRollout(mgr, _model(3, 16, seed=9), steps=16, eps=eps, graph=True)
    bufs = [GraphReplayBuffer(256, 5, prioritized=True, alpha=0.5) for _ in range(2)]
    feed = DeviceTransitionFeed(ro, *bufs)
    torch.manual_seed(77)
    for it in range(3):
        if it == 0:
            ro.run_begin()
        else:
            ro.run_continue()
        feed.push()
    feed.settle()
    return bufs, feed, ro


def test_device_store_on_a_constant_schedule_equals_the_float_loop():
    from gnn_hex_amd.multi_env_manager import EpsSchedule
    e = 0.3
    bufs_f, feed_f, _ = _store_loop(e)
    bufs_s, feed_s, ro = _store_loop(EpsSchedule(e, e, 1000))
    for s, (a, b) in enumerate(zip(bufs_f, bufs_s)):
        _assert_buffers_equal(a, b, "side %d" % s)
        assert a.size > 0
    assert (feed_f.games, feed_f.maker_wins, feed_f.length_sum) == (feed_s.games, feed_s.maker_wins, feed_s.length_sum)
    assert feed_f.games > 0
    assert int(ro.frames.item()) == ro.frames_issued == 3 * 16 * 6          # run_continue advances the counter as run_begin does


# ---- 5. the error path ------------------------------------------------------------------------------------------------------------

def test_no_playable_vertex_and_missing_schedule_words():
    from gnn_hex_amd import _lib, ops
    from gnn_hex_amd.multi_env_manager import EpsSchedule
    L = _lib.lib()
    k = 3
    mgr_a, mgr_b = _manager(k, 5), _manager(k, 5)
    nv, W = mgr_a._nv, mgr_a._words
    # every playable vertex dead: the two terminals alone, no edge; odd side flags and move counts that must survive
    adj = torch.zeros((k, nv, W), dtype=torch.int64, device=DEV)
    alive = torch.zeros((k, nv), dtype=torch.uint8, device=DEV)
    alive[:, :2] = 1
    mt = torch.tensor([1, 0, 1], dtype=torch.int32, device=DEV)
    tm = torch.tensor([7, 8, 9], dtype=torch.int32, device=DEV)
    rm = torch.full((k, nv), -1, dtype=torch.int16, device=DEV)
    rb = torch.full((k, nv), -1, dtype=torch.int16, device=DEV)
    rm[0, 5], rm[0, 6], rb[1, 3], rb[1, 4] = 6, 5, 4, 3
    for m in (mgr_a, mgr_b):
        _lib.check(L.hexgnn_env_import(m._h, adj.data_ptr(), alive.data_ptr(), mt.data_ptr(), tm.data_ptr(), rm.data_ptr(),
                                       rb.data_ptr(), ops._stream()))
    A, B = _Ply(mgr_a), _Ply(mgr_b)
    gptr = torch.arange(0, 2 * k + 1, 2, dtype=torch.int32, device=DEV)      # two nodes per graph: the terminals
    q = torch.tensor([0.5, -1.0, 2.0, 2.0, 0.0, 3.0], dtype=torch.float32, device=DEV)
    backmap = torch.tensor([0, 1] * k, dtype=torch.int64, device=DEV)
    u = torch.zeros((k, 2), dtype=torch.float32, device=DEV)                  # u < eps: would explore if there were a move
    sched = EpsSchedule(1.0, 1.0, 10).to_device(DEV)
    frames = torch.zeros(1, dtype=torch.int64, device=DEV)
    A.three_launches(gptr, q, backmap, 1.0, u, 1)
    B.one_launch(gptr, q, backmap, u, sched, frames, 0, 1)
    _assert_plies_equal(A, B, "no playable vertex")
    for P in (A, B):
        assert P.rank.tolist() == [-1] * k and P.vert.tolist() == [-1] * k and P.expl.tolist() == [0] * k
        assert P.result.tolist() == [[-1, 7, 2, 0, 1], [-1, 8, 2, 0, 1], [-1, 9, 2, 0, 1]]
        assert torch.equal(P.adj, adj) and torch.equal(P.alive, alive) and torch.equal(P.mt, mt) and torch.equal(P.tm, tm)
        assert torch.equal(P.rm, rm) and torch.equal(P.rb, rb)
    assert torch.equal(B.snap_adj, adj) and torch.equal(B.snap_alive, alive)

    # the same boards under DeviceRollout, both ply forms: run_end says which kind of illegal action it was (rank -1: the graph
    # had nothing to pick from, or no finite advantage), with the env's graph size at that step
    from gnn_hex_amd.multi_env_manager import DeviceRollout
    mgr_c = _manager(k, 5)
    st = mgr_c._state_tensors()
    st.update(adj=adj, alive=alive, mt=torch.ones(k, dtype=torch.int32, device=DEV), tm=tm, rm=rm, rb=rb,
              sizes=np.array([[2, 0]] * k, dtype=np.int64), onturn="m")
    mgr_c._restore_state_tensors(st)
    for e in (0.0, EpsSchedule(0.0, 0.0, 0)):
        ro = DeviceRollout(mgr_c, _model(3, 16), steps=2, eps=e, graph=False)
        with pytest.raises(ValueError, match=r"^illegal action at step 0 for env 0 \(rank -1, vertex -1, exploratory 0, nodes 2\)$"):
            ro.run()

    # a missing schedule block / frame counter (and every other required pointer) is refused on the host: nothing is launched
    fresh = _Ply(mgr_b)
    for field in ("sched", "frames", "gptr", "q", "backmap", "u", "action_vertex", "action_rank", "exploratory", "result",
                  "adj_out", "alive_out"):
        c = fresh.call(gptr, q, backmap, u, sched, frames, 0, 1)
        setattr(c, field, None)
        assert L.hexgnn_rollout_ply(mgr_b._h, C.byref(c), ops._stream()) == EINVAL, field
    c = fresh.call(gptr, q, backmap, u, sched, frames, -1, 1)
    assert L.hexgnn_rollout_ply(mgr_b._h, C.byref(c), ops._stream()) == EINVAL          # frames played earlier in a run: not negative
    torch.cuda.synchronize()
    for name in ("vert", "rank", "result", "snap_adj"):
        assert (getattr(fresh, name) == -9).all(), "%s was written by a refused call" % name
    fresh.export()
    assert torch.equal(fresh.adj, adj) and torch.equal(fresh.tm, tm)
    # eps_out alone may be missing
    c = fresh.call(gptr, q, backmap, u, sched, frames, 0, 1)
    c.eps_out = None
    assert L.hexgnn_rollout_ply(mgr_b._h, C.byref(c), ops._stream()) == 0
    torch.cuda.synchronize()
    assert fresh.rank.tolist() == [-1] * k and fresh.result[:, 4].tolist() == [1] * k

    # hexgnn_frames_add
    assert L.hexgnn_frames_add(None, 1, ops._stream()) == EINVAL
    _lib.check(L.hexgnn_frames_add(frames.data_ptr(), 2 ** 33 + 5, ops._stream()))
    _lib.check(L.hexgnn_frames_add(frames.data_ptr(), 7, ops._stream()))
    assert int(frames.item()) == 2 ** 33 + 12
