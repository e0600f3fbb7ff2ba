"""Drop-in mirror of ``graph_game.multi_env_manager.Env_manager`` (graph_game/multi_env_manager.py:16-165) on the
HIP board-graph builder (gnn_hex_amd/csrc/env.hip, C ABI ``hexgnn_env_*``).

Same constructor, attributes and methods; ``step`` returns ``(states, rewards, dones, infos)`` with the reference's
reward / reset / side-to-move conventions.  ``states`` is an ``ObsList``: it behaves as the reference's
``List[Data]`` (len / index / iterate -> ``Data(x, edge_index, backmap)`` views) but is backed by ONE batched device
observation, so ``Batch.from_data_list(states)`` costs nothing and carries the sorted CSR the model kernels consume.
All game logic runs on the GPU; there is no python/CPU game fallback.  ``cnn_rep=True`` (CNN input planes) is outside
the hot path and raises NotImplementedError.
"""
from __future__ import annotations

import ctypes as C
import time
from typing import List, Tuple, Union

import numpy as np
import torch

from . import _lib, ops
from .data import Batch, Data
from .observation import ObsTarget, acting_forward, live_norm_of, prefix_offsets


class ObsList:
    """List[Data]-compatible view of one batched observation of all envs."""

    def __init__(self, x, edge_local, edge_global, backmap, batch_vec, node_off, edge_off, gs, is_maker, max_nodes,
                 snap=None):
        self._snap = snap          # (adj [k,nv,W] i64, alive [k,nv] u8) board snapshot the replay buffer stores
        self.x, self.edge_local, self.edge_global, self.backmap = x, edge_local, edge_global, backmap
        self.batch_vec = batch_vec
        self.node_off, self.edge_off = node_off, edge_off     # host lists, len num_envs+1
        self.gs, self.is_maker, self.max_nodes = gs, is_maker, max_nodes
        self._ptr = None
        self._items = {}

    def __len__(self):
        return len(self.node_off) - 1

    def __getitem__(self, i):
        if isinstance(i, slice):
            return [self[j] for j in range(*i.indices(len(self)))]
        if i < 0:
            i += len(self)
        d = self._items.get(i)
        if d is None:
            n0, n1 = self.node_off[i], self.node_off[i + 1]
            e0, e1 = self.edge_off[i], self.edge_off[i + 1]
            d = Data(x=self.x[n0:n1], edge_index=self.edge_local[:, e0:e1], backmap=self.backmap[n0:n1])
            ops.attach_hints(d.x, self.is_maker, n1 - n0)
            d._hex_src = (self, i)
            self._items[i] = d
        return d

    def snapshot(self):
        if self._snap is None:
            raise ValueError("this observation was taken without board snapshots (Env_manager.record_snapshots=False)")
        return self._snap

    def __iter__(self):
        return (self[i] for i in range(len(self)))

    def to_batch(self) -> Batch:
        """The whole observation as a ``Batch`` (what ``Batch.from_data_list(list(states))`` would build)."""
        b = Batch()
        if self._ptr is None:
            self._ptr = torch.tensor(self.node_off, dtype=torch.long, device=self.x.device)
        b.x, b.edge_index, b.batch, b.ptr, b.backmap = self.x, self.edge_global, self.batch_vec, self._ptr, self.backmap
        b._num_graphs = len(self)
        ops.attach_hints(b.x, self.is_maker, self.max_nodes)
        b.edge_index._hex_csr = self.gs
        return b


class TransitionBlock:
    """Array form of a list of transitions ``(s, a, r, s', done)`` of ONE side: states are referenced as
    ``(index into obs_list, env)`` instead of being materialised as ``Data`` objects; ``next_step == -1`` means the
    start position (terminal transitions, multi_env_manager.py:150-158).  Consumed by ``GraphReplayBuffer.put_block``."""

    def __init__(self, obs_list, start_obs, maker_side, src_step, env, action, reward, next_step, done):
        self.obs_list, self.start_obs, self.maker_side = obs_list, start_obs, maker_side
        self.src_step, self.env, self.action = src_step, env, action
        self.reward, self.next_step, self.done = reward, next_step, done

    def __len__(self):
        return int(self.env.shape[0])


class SnapObs(ObsList):
    """An observation known only as board snapshots + graph sizes (what a device rollout records per step).  It carries
    everything the replay path needs (``snapshot()``, ``node_off`` / ``edge_off``, ``is_maker``); the ``Data`` views of
    an ``ObsList`` are not materialised."""

    def __init__(self, snap, sizes: np.ndarray, is_maker: bool, owner=None):
        self._owner = owner        # (DeviceRollout, run number): the snapshot is a view into that rollout's ring
        node_off, edge_off = prefix_offsets(sizes[:, 0], sizes[:, 1])
        super().__init__(None, None, None, None, None, node_off.tolist(), edge_off.tolist(), None, is_maker,
                         int(sizes[:, 0].max()) if sizes.shape[0] else 0, snap)

    def snapshot(self):
        if self._owner is not None and self._owner[0]._run_no != self._owner[1]:
            raise RuntimeError("stale rollout observation: DeviceRollout.run() has been called again and overwrote the "
                               "snapshot ring this observation views; store a run's transitions (put_block) before the "
                               "next run, or keep RolloutResult.detach() copies")
        return super().snapshot()

    def __getitem__(self, i):
        raise TypeError("a rollout observation holds board snapshots only; re-observe it through GraphReplayBuffer")

    def to_batch(self):
        raise TypeError("a rollout observation holds board snapshots only; re-observe it through GraphReplayBuffer")


class RolloutResult:
    """Histories of one ``DeviceRollout.run()``: ``states[0]`` is the observation the first move was chosen from,
    ``states[t+1]`` the one after move ``t``; ``actions`` are node ranks inside ``states[t]`` (the model's output index,
    what the reference stores), ``vertices`` the vertex ids played.  Host arrays; the snapshots stay on the device."""

    def __init__(self, states, actions, vertices, rewards, dones, exploratories, infos):
        self.states, self.actions, self.vertices = states, actions, vertices
        self.rewards, self.dones, self.exploratories, self.infos = rewards, dones, exploratories, infos

    def detach(self) -> "RolloutResult":
        """Give the states their own copies of the board snapshots.  By default they VIEW the rollout's snapshot ring,
        which the next ``run()`` overwrites (using such a state afterwards raises); a detached result stays valid."""
        for st in self.states:
            if st._owner is not None:
                st._snap = tuple(t.clone() for t in st._snap)
                st._owner = None
        return self


class EpsSchedule:
    """The exploration schedule of the published training recipes (``--init_eps / --final_eps / --eps_decay_frames``, reference
    README.md:5-8,48) in the form ``hexgnn_rollout_ply`` reads from device memory: epsilon is ``init`` for the first ``burnin``
    env frames, then moves linearly to ``final`` over ``decay_frames`` frames and stays there.  The trainer that owns the
    reference's schedule is in its un-vendored Rainbow submodule: the formula is the one include/hexgnn.h fixes (parity unpinned).

    ``value(frame)`` is the host mirror of the kernel's evaluation, bit for bit; ``to_device`` hands out the 32-byte block a
    ``DeviceRollout`` points its plies at, and ``update`` rewrites every block handed out in place, so a captured rollout follows
    a changed schedule without a new capture."""

    def __init__(self, init: float, final: float, decay_frames: int, burnin: int = 0):
        self._blocks = {}
        self._set(init, final, decay_frames, burnin)

    def _set(self, init, final, decay_frames, burnin):
        init, final = float(init), float(final)
        if not (0.0 <= init <= 1.0 and 0.0 <= final <= 1.0):
            raise ValueError("epsilon is a probability: init and final in [0, 1]")
        if int(decay_frames) != decay_frames or int(burnin) != burnin or decay_frames < 0 or burnin < 0:
            raise ValueError("decay_frames and burnin are whole, non-negative frame counts")
        self.init, self.final, self.decay_frames, self.burnin = init, final, int(decay_frames), int(burnin)

    def value(self, frame: int) -> np.float32:
        """Epsilon at env frame ``frame``: float64 operations rounded one by one, then one rounding to float32."""
        f = int(frame)
        if f < self.burnin:
            return np.float32(self.init)
        p = min(1.0, float(f - self.burnin) / float(self.decay_frames)) if self.decay_frames > 0 else 1.0
        return np.float32(self.init + (self.final - self.init) * p)

    def _words(self) -> torch.Tensor:
        return torch.from_numpy(np.concatenate([np.array([self.init, self.final], dtype=np.float64).view(np.int64),
                                                np.array([self.burnin, self.decay_frames], dtype=np.int64)]))

    def to_device(self, device) -> torch.Tensor:
        """The block ``double init, double final, int64 burnin, int64 decay`` as an int64 [4] tensor on ``device`` (one per
        device, shared by every rollout that runs this schedule there)."""
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        blk = self._blocks.get(device)
        if blk is None:
            blk = self._blocks[device] = self._words().to(device)
        return blk

    def update(self, init=None, final=None, decay_frames=None, burnin=None) -> None:
        """Change the schedule (arguments left out keep their value) and rewrite the device blocks in place, stream-ordered."""
        self._set(self.init if init is None else init, self.final if final is None else final,
                  self.decay_frames if decay_frames is None else decay_frames, self.burnin if burnin is None else burnin)
        for blk in self._blocks.values():
            blk.copy_(self._words())


class DeviceRollout:
    """``steps`` lock-step moves of every env of an ``Env_manager`` as a closed device loop: observation (HIP builder) ->
    Q-network forward (advantages only) -> epsilon-greedy -> env step with dead/captured removal and auto reset -> graph
    sizes prefix-summed on the device -> board snapshot.  Nothing is read back between the moves; with ``graph=True`` the
    whole sequence is ONE HIP graph (``gnn_hex_amd.graphs``), so a rollout costs one launch + one read-back.  The
    reference does this with a Python loop over envs per move (graph_game/multi_env_manager.py:76-103 +
    GN0/RainbowDQN/evaluate_elo.py:253-275).  ``steps`` must be even so the side to move is the same before and after;
    the model's weights are read at run time (training between runs is fine, ``grow_*`` needs a new rollout).
    ``run_continue()`` issues a run without the host's sizes and without a read-back; ``DeviceTransitionFeed`` consumes it.

    ``eps`` is a float, frozen for the rollout's life (under ``graph=True`` it is a kernel argument of the captured graph), or an
    ``EpsSchedule``: every ply then computes its epsilon on the device from the schedule's block and the frame counter
    ``frames`` (int64 [1], advanced by ``steps * num_envs`` behind every run), and picks, moves and snapshots in one launch
    (``hexgnn_rollout_ply``), so the published decay runs under one capture and through ``run_continue``.  ``eps_log`` (float32
    [steps]) holds the epsilon every ply of the last run used; ``frames_issued`` is the host's count of the frames of every run
    issued so far (no synchronisation: ``schedule.value(rollout.frames_issued)`` is the epsilon the next run starts with);
    ``set_frames(n)`` sets both (resuming from a checkpoint)."""

    def __init__(self, mgr: "Env_manager", model, steps: int = 16, eps: Union[float, EpsSchedule] = 0.05, graph: bool = True):
        if steps < 2 or steps % 2:
            raise ValueError("steps must be a positive even number")
        self._live_norm = live_norm_of(model)
        self.mgr, self.model, self.T = mgr, model, steps
        self.schedule = eps if isinstance(eps, EpsSchedule) else None
        self.eps = None if self.schedule is not None else float(eps)
        self.start_side = mgr.global_onturn
        dev = mgr.device
        k, nv, W = mgr.num_envs, mgr._nv, mgr._words
        # capacity-sized observation (every env at the start position); the tail clear only where the forward needs it
        self.obs = ObsTarget.capacity(k, nv, int(mgr._base_sizes[0, 1]), dev, zeroed=True,
                                      tail_clear=nv > 128 or self._live_norm)
        T = steps
        self.vert = torch.zeros((T, k), dtype=torch.int32, device=dev)
        self.rank = torch.zeros((T, k), dtype=torch.int32, device=dev)
        self.expl = torch.zeros((T, k), dtype=torch.uint8, device=dev)
        self.result = torch.zeros((T, k, 5), dtype=torch.int32, device=dev)
        self.uni = torch.zeros((T, k, 2), dtype=torch.float32, device=dev)
        self.adj = torch.zeros((T + 1, k, nv, W), dtype=torch.int64, device=dev)
        self.alive = torch.zeros((T + 1, k, nv), dtype=torch.uint8, device=dev)
        self._mt = torch.zeros(k, dtype=torch.int32, device=dev)
        self._tm = torch.zeros(k, dtype=torch.int32, device=dev)
        self._run_no = 0           # bumped by every run(): results of earlier runs view overwritten snapshots
        self._settled_run = 0      # the run up to which mgr._sizes is current (run_end, or DeviceTransitionFeed.settle)
        self.sizes0_dev = torch.zeros((k, 2), dtype=torch.int32, device=dev)     # run_continue: graph sizes at the run's start
        self._sizes0_host = None   # the same for a run issued by run_begin (host-known)
        self._graph = None
        self.frames = self.eps_log = self._sched_dev = None
        self.frames_issued = 0
        if self.schedule is not None:
            self.frames = torch.zeros(1, dtype=torch.int64, device=dev)
            self.eps_log = torch.zeros(T, dtype=torch.float32, device=dev)
            self._sched_dev = self.schedule.to_device(self.frames.device)
        if graph:
            from .graphs import GraphedStep
            self.obs.set_offsets(mgr._sizes)
            state = self.mgr._state_tensors()
            self._graph = GraphedStep(self._body, warmup=1)
            self.mgr._restore_state_tensors(state)      # warm-up + capture played moves: put the boards back
            if self.frames is not None:
                self.frames.zero_()                     # ... and the frame counter the warm-up advanced
        self._mgr_touch = mgr._touch

    # -- pieces ----------------------------------------------------------------------------------------
    def _export(self, slot: int):
        _lib.check(_lib.lib().hexgnn_env_export(self.mgr._h, self.adj[slot].data_ptr(), self.alive[slot].data_ptr(),
                                               self._mt.data_ptr(), self._tm.data_ptr(), None, None, ops._stream()),
                   "hexgnn_env_export")

    def _body(self):
        L = _lib.lib()
        mgr, k, obs = self.mgr, self.mgr.num_envs, self.obs
        self._export(0)
        maker = self.start_side == "m"
        for t in range(self.T):
            obs.observe_env(mgr._h)
            adv = acting_forward(self.model, obs, maker, mgr._nv, self._live_norm)
            if self.schedule is not None:
                u = self.uni[t]
                u.uniform_()
                # pick, move with auto reset (finished envs restart on the side everyone moves to next) and snapshot t + 1
                call = _lib.RolloutCall(
                    struct_bytes=C.sizeof(_lib.RolloutCall), frame_add=t * k, reset_maker_turn=int(not maker),
                    gptr=obs.node_off.data_ptr(), q=adv.reshape(-1).data_ptr(), backmap=obs.backmap.data_ptr(), u=u.data_ptr(),
                    sched=self._sched_dev.data_ptr(), frames=self.frames.data_ptr(), action_vertex=self.vert[t].data_ptr(),
                    action_rank=self.rank[t].data_ptr(), exploratory=self.expl[t].data_ptr(), result=self.result[t].data_ptr(),
                    adj_out=self.adj[t + 1].data_ptr(), alive_out=self.alive[t + 1].data_ptr(),
                    eps_out=self.eps_log[t:].data_ptr())
                _lib.check(L.hexgnn_rollout_ply(mgr._h, C.byref(call), ops._stream()), "hexgnn_rollout_ply")
                _lib.check(L.hexgnn_env_offsets(k, self.result[t].data_ptr(), obs.node_off.data_ptr(),
                                                obs.edge_off.data_ptr(), ops._stream()), "hexgnn_env_offsets")
                maker = not maker
                continue
            u = None
            if self.eps > 0:
                u = self.uni[t]
                u.uniform_()
            _lib.check(L.hexgnn_select_actions(k, obs.node_off.data_ptr(), adv.reshape(-1).data_ptr(),
                                               obs.backmap.data_ptr(), self.eps, u.data_ptr() if u is not None else None,
                                               self.vert[t].data_ptr(), self.rank[t].data_ptr(), self.expl[t].data_ptr(),
                                               ops._stream()), "hexgnn_select_actions")
            # finished envs restart on the side everyone moves to next (multi_env_manager.py:98-101)
            _lib.check(L.hexgnn_env_step(mgr._h, self.vert[t].data_ptr(), 1, 1, int(not maker), self.result[t].data_ptr(),
                                         ops._stream()), "hexgnn_env_step")
            _lib.check(L.hexgnn_env_offsets(k, self.result[t].data_ptr(), obs.node_off.data_ptr(),
                                            obs.edge_off.data_ptr(), ops._stream()), "hexgnn_env_offsets")
            self._export(t + 1)
            maker = not maker
        if self.schedule is not None:
            _lib.check(L.hexgnn_frames_add(self.frames.data_ptr(), self.T * k, ops._stream()), "hexgnn_frames_add")

    # -- public ----------------------------------------------------------------------------------------
    def set_frames(self, n: int) -> None:
        """Set the frame counter the schedule is evaluated at (device word and host count), e.g. when resuming a checkpoint."""
        if self.schedule is None:
            raise RuntimeError("this rollout plays with a fixed epsilon: build it with an EpsSchedule")
        if n < 0:
            raise ValueError("a frame count is not negative")
        self.frames.fill_(int(n))
        self.frames_issued = int(n)

    def run(self) -> RolloutResult:
        return self.run_end(self.run_begin())

    def run_begin(self):
        """Issue the rollout (stream-ordered, nothing is waited for) and return a handle for ``run_end``.  Work issued
        between the two calls runs behind the rollout on the GPU while the host is free -- e.g. a learner that starts the
        next rollout before it issues this iteration's updates (the actor then plays with weights one iteration old).
        The previous run's observations must have been stored (``put_block``) by now: this run overwrites their ring."""
        mgr = self.mgr
        if mgr.global_onturn != self.start_side:
            raise RuntimeError("this rollout was built with %r to move" % self.start_side)
        if getattr(self, "_open", False):
            raise RuntimeError("run_begin() called twice without run_end()")
        if self._settled_run != self._run_no and self._mgr_touch == mgr._touch:
            raise RuntimeError("the last run was issued by run_continue() and its graph sizes have not reached the host yet: "
                               "DeviceTransitionFeed.settle() first")
        sizes0 = mgr._sizes.copy()
        self._sizes0_host, self._mgr_touch = sizes0, mgr._touch
        self._run_no += 1
        self.frames_issued += self.T * mgr.num_envs
        self.obs.set_offsets(mgr._sizes)
        if self._graph is not None:
            self._graph.replay()
        else:
            self._body()
        self._open = True
        return (self._run_no, sizes0)

    def run_continue(self) -> None:
        """Issue a run that continues the previous one with nothing from the host: the observation offsets are the ones the
        previous run's last ``hexgnn_env_offsets`` left on the device, so the previous run needs no ``run_end`` and
        ``mgr._sizes`` may lag (``DeviceTransitionFeed.settle`` refreshes it).  The run's histories are consumed on the device
        (``DeviceTransitionFeed.push``).  ``RuntimeError`` before the first run and when the manager was reset, resized or
        stepped by hand since the previous run was issued: the device-side offsets then describe other boards."""
        mgr = self.mgr
        if self._run_no == 0:
            raise RuntimeError("run_continue() continues a previous run: issue the first one with run_begin()")
        if self._mgr_touch != mgr._touch or mgr.global_onturn != self.start_side:
            raise RuntimeError("the manager was reset, resized or stepped since the previous run: start again with run_begin()")
        self.sizes0_dev.copy_(self.result[self.T - 1, :, 2:4])     # (before the run overwrites its result words)
        self._sizes0_host = None
        self._run_no += 1
        self.frames_issued += self.T * mgr.num_envs
        if self._graph is not None:
            self._graph.replay()
        else:
            self._body()
        self._open = False

    def run_end(self, handle) -> RolloutResult:
        mgr = self.mgr
        run_no, sizes0 = handle
        if not getattr(self, "_open", False) or run_no != self._run_no:
            raise RuntimeError("run_end() needs the handle of the rollout issued last")
        self._open = False
        self._settled_run = run_no
        owner = (self, run_no)
        res = self.result.cpu().numpy()                      # the only read-back (also the synchronisation point)
        if res[:, :, 4].any():
            # (the error path alone reads these; rank -1: no finite advantage among the graph's non-terminal nodes, or no such node)
            t, i = (int(v) for v in np.argwhere(res[:, :, 4])[0])
            nodes = int(sizes0[i, 0]) if t == 0 else int(res[t - 1, i, 2])
            raise ValueError("illegal action at step %d for env %d (rank %d, vertex %d, exploratory %d, nodes %d)"
                             % (t, i, int(self.rank[t, i]), int(self.vert[t, i]), int(self.expl[t, i]), nodes))
        ranks = self.rank.cpu().numpy().astype(np.int64)
        verts = self.vert.cpu().numpy().astype(np.int64)
        expl = self.expl.cpu().numpy().astype(bool)
        T, k = self.T, mgr.num_envs
        dones = res[:, :, 0] >= 0
        rewards = np.zeros((T, k), dtype=float)
        infos = [[{} for _ in range(k)] for _ in range(T)]
        now = time.perf_counter()
        maker = self.start_side == "m"
        states = [SnapObs((self.adj[0], self.alive[0]), sizes0, maker, owner)]
        for t in range(T):
            mover_is_maker = maker
            for i in np.nonzero(dones[t])[0]:
                winner_is_maker = res[t, i, 0] == 0
                n = int(res[t, i, 1])
                infos[t][i]["episode_metrics"] = {
                    "return": 1 if winner_is_maker else -1,
                    "discounted_return": float(mgr.gamma ** n if winner_is_maker else -(mgr.gamma ** n)),
                    "length": n,
                    "time": now - mgr._creation_time[i],
                }
                rewards[t, i] = 1 if winner_is_maker == mover_is_maker else -1
                mgr._creation_time[i] = now
            maker = not maker
            states.append(SnapObs((self.adj[t + 1], self.alive[t + 1]), res[t, :, 2:4].astype(np.int64), maker, owner))
        mgr._sizes = res[-1, :, 2:4].astype(np.int64)
        mgr.last_obs = None
        return RolloutResult(states, ranks, verts, rewards, dones, expl, infos)


class RolloutStitcher:
    """Transitions across rollout boundaries.  An n-step transition that starts in move i needs the histories up to move
    i + 2 n_step, so the last 2 n_step - 1 moves of a rollout cannot produce transitions on their own (3 of 16 moves at
    n_step = 2).  The stitcher keeps that tail -- observations as detached snapshot copies, actions, rewards, dones,
    exploratory flags -- and prepends it to the next rollout's histories: every move of a continuous self-play stream then
    starts exactly one transition per n_step, and none twice (windows of a shorter n_step that were already complete in the
    previous rollout are skipped).

        stitch = RolloutStitcher(mgr)
        maker_block, breaker_block = stitch.assemble(rollout.run())      # instead of mgr.assemble_transitions(...)
    """

    def __init__(self, mgr: "Env_manager"):
        self.mgr = mgr
        self.keep = 2 * max(mgr.n_steps) - 1     # moves whose longest window was still incomplete at the rollout's end
        self._tail = None      # (states [keep + 1], actions, rewards, dones, exploratories) of the previous rollout's end

    def reset(self):
        """Forget the tail (after ``mgr.reset()`` / ``change_hex_size``: the stream is no longer continuous)."""
        self._tail = None

    def assemble(self, res: RolloutResult):
        T = len(res.actions)
        if T < self.keep:
            raise ValueError("a rollout must be at least 2 * n_step - 1 = %d moves long" % self.keep)
        states = list(res.states)
        acts, rews = list(res.actions), list(res.rewards)
        dones, expl = list(res.dones), list(res.exploratories)
        emitted = None
        if self._tail is not None:
            t_states, t_acts, t_rews, t_dones, t_expl = self._tail
            # the tail's last observation IS this rollout's first one (same boards): keep the tail's copy for the prefix
            states = t_states[:-1] + states
            acts, rews, dones, expl = t_acts + acts, t_rews + rews, t_dones + dones, t_expl + expl
            # a shorter window (n_step below the maximum) starting in the first 2 (n_max - n_step) prefix moves was already
            # complete in the previous rollout
            emitted = {n: self.keep + 1 - 2 * n for n in self.mgr.n_steps}
        blocks = self.mgr.assemble_transitions(states[0], states[1:], acts, rews, dones, expl, _already_emitted=emitted)
        # next prefix: the last `keep` moves with their keep + 1 observations, snapshots copied out of the rollout's ring
        k = self.keep
        tail_states = []
        for st in states[-(k + 1):]:
            if isinstance(st, SnapObs) and st._owner is not None:
                cp = SnapObs.__new__(SnapObs)
                cp.__dict__.update(st.__dict__)
                cp._snap = tuple(t.clone() for t in st._snap)
                cp._owner = None
                cp._items = {}
                st = cp
            tail_states.append(st)
        self._tail = (tail_states, acts[-k:], rews[-k:], dones[-k:], expl[-k:])
        return blocks


def transition_coef(gamma, n_steps) -> np.ndarray:
    """The reward factors of ``Env_manager.assemble_transitions`` as a table ``[len(n_steps), 2 * max(n_steps)]`` (fp64, zero
    behind a window's end): row ``ni`` holds, for ``j`` in the window of ``n_steps[ni]``, sign * gamma^(j // 2) computed by
    the very expression used there, so the device assembly multiplies by the same bits."""
    n_steps = [int(n) for n in n_steps]
    out = np.zeros((len(n_steps), 2 * max(n_steps)), dtype=np.float64)
    for ni, n_step in enumerate(n_steps):
        w = 2 * n_step
        jj = np.arange(w)
        out[ni, :w] = ((-(jj % 2)) * 2 + 1) * (float(gamma) ** (jj // 2))
    return out


class DeviceTransitionFeed:
    """Rollout -> replay rings without the host: what ``run_end`` -> ``RolloutStitcher.assemble`` -> ``put_block`` do, on the
    device (``hexgnn_transitions_assemble`` + ``hexgnn_replay_store_dev``), with the same transitions, ring slots and bits.

        feed = DeviceTransitionFeed(rollout, maker_buffer, breaker_buffer)
        rollout.run_begin()                  # the first run; later ones: rollout.run_continue()
        feed.push()                          # issued behind the run; nothing is waited for
        ... GraphedUpdate.step() ...
        feed.settle()                        # (push() does it for the previous push) -> episode counters

    The feed keeps the history on the device: the last ``keep = 2 max(n_steps) - 1`` moves of the previous push in front of
    the run's ``T`` new ones (``keep + T + 1`` board snapshots), the per-side transition lists and the reward factors.
    ``push()`` copies the run's arrays behind the carried prefix, assembles, stores each side's list into its buffer (a
    graph with more directed edges than the buffer's draw buffers hold is never stored: such a transition is dropped and
    reported), raises the new leaves to the running maximum priority, moves the last ``keep`` moves to the front and starts a
    non-blocking copy of a small record to pinned memory.  ``settle()`` waits for that record and refreshes what the host
    mirrors: ``mgr._sizes`` / ``last_obs`` / creation times as ``run_end`` does, and the buffers' ``pos``, ``size``, graph
    sizes and sides.  At most one record is outstanding: ``push()`` settles the previous one first (its event completed an
    iteration ago), so the host runs at most one iteration ahead of the GPU.  A buffer's own host-side methods settle too."""

    def __init__(self, rollout: DeviceRollout, maker_buffer, breaker_buffer, edge_limit: int = None):
        """``edge_limit``: a tighter bound on the directed edges of a stored graph than the buffers' own (tests)."""
        mgr = rollout.mgr
        self.edge_limit = edge_limit
        self.rollout, self.mgr, self.bufs = rollout, mgr, (maker_buffer, breaker_buffer)
        self.n_steps = [int(n) for n in mgr.n_steps]
        if not self.n_steps or len(self.n_steps) > 8 or min(self.n_steps) < 1:
            raise ValueError("n_steps: 1 to 8 positive window lengths")
        self.keep = 2 * max(self.n_steps) - 1
        T, k, nv, W = rollout.T, mgr.num_envs, mgr._nv, mgr._words
        if T < self.keep:
            raise ValueError("a rollout must be at least 2 * n_step - 1 = %d moves long" % self.keep)
        # per push and side: T / 2 start moves, each with one window per n_step and env
        self.list_len = L = (T // 2) * len(self.n_steps) * k
        dev = mgr.device
        here = torch.device("cuda", dev.index if dev.index is not None else torch.cuda.current_device())
        if maker_buffer is breaker_buffer:
            raise ValueError("maker and breaker transitions go to two buffers")
        for buf in self.bufs:
            if not buf.prioritized:
                raise ValueError("the device store raises new transitions to the running maximum priority: prioritized=True")
            bd = buf.device
            if torch.device("cuda", bd.index if bd.index is not None else torch.cuda.current_device()) != here:
                raise ValueError("buffer on another device than the env manager")
            if buf.hex_size != mgr.hex_size:
                raise ValueError("buffer of hex_size %d, manager of hex_size %d" % (buf.hex_size, mgr.hex_size))
            if buf.capacity < L:
                raise ValueError("buffer capacity %d is below the %d transitions one push can store" % (buf.capacity, L))
        H = self.keep + T
        z = lambda *shape, dtype: torch.zeros(shape, dtype=dtype, device=dev)     # noqa: E731
        self.result, self.rank, self.expl = z(H, k, 5, dtype=torch.int32), z(H, k, dtype=torch.int32), z(H, k, dtype=torch.uint8)
        self.adj, self.alive = z(H + 1, k, nv, W, dtype=torch.int64), z(H + 1, k, nv, dtype=torch.uint8)
        kp = self.keep
        self._tail = (z(kp, k, 5, dtype=torch.int32), z(kp, k, dtype=torch.int32), z(kp, k, dtype=torch.uint8),
                      z(kp + 1, k, nv, W, dtype=torch.int64), z(kp + 1, k, nv, dtype=torch.uint8))
        self.sizes0 = z(k, 2, dtype=torch.int32)
        self.src_step, self.env, self.action = (z(2, L, dtype=torch.int32) for _ in range(3))
        self.next_step, self.reward, self.done = z(2, L, dtype=torch.int32), z(2, L, dtype=torch.float32), z(2, L, dtype=torch.uint8)
        self.count = z(2, dtype=torch.int32)
        self.leaves = torch.full((2, L), -1, dtype=torch.int32, device=dev)
        self._rec_len = 16 + 5 * L
        self.record = z(2 * self._rec_len + 3 * k, dtype=torch.int32)       # two store records | last sizes [k][2] | env_done [k]
        self._pinned = torch.zeros(self.record.numel(), dtype=torch.int32, pin_memory=True)
        self.coef_host = transition_coef(mgr.gamma, self.n_steps)
        self.coef = torch.from_numpy(self.coef_host).to(dev)
        self._n_steps_c = (C.c_int * len(self.n_steps))(*self.n_steps)
        self._start = mgr._snapshot_handle(mgr._base, 1)
        self._prefix, self._pending = False, None
        self._pushed_run, self._touch = 0, mgr._touch
        self.games = self.maker_wins = self.length_sum = 0      # episode counters over every settled push

    def reset(self):
        """Forget the carried moves (after ``mgr.reset()`` / a fresh ``run_begin``: the stream is no longer continuous).
        An outstanding record is settled first."""
        self.settle()
        self._prefix = False

    def push(self) -> None:
        ro, mgr, L = self.rollout, self.mgr, _lib.lib()
        if ro._run_no == 0 or ro._run_no == self._pushed_run:
            raise RuntimeError("push() stores the run issued last: issue one first (run_begin / run_continue)")
        if ro._mgr_touch != mgr._touch:
            raise RuntimeError("the manager was reset, resized or stepped after the run was issued")
        if self._prefix and (self._touch != mgr._touch or ro._run_no != self._pushed_run + 1):
            raise RuntimeError("the carried moves belong to another stream of play (the manager was reset, or a run was not "
                               "pushed): feed.reset() first")
        self.settle()
        limits = [buf._device_store_begin(self) for buf in self.bufs]
        if self.edge_limit is not None:
            limits = [min(int(self.edge_limit), v) for v in limits]
        T, k, kp = ro.T, mgr.num_envs, self.keep
        P = kp if self._prefix else 0
        H = P + T
        self.result[P:H].copy_(ro.result)
        self.rank[P:H].copy_(ro.rank)
        self.expl[P:H].copy_(ro.expl)
        self.adj[P:H + 1].copy_(ro.adj)
        self.alive[P:H + 1].copy_(ro.alive)
        start_maker = ro.start_side == "m"
        if P == 0:
            if ro._sizes0_host is not None:
                self.sizes0.copy_(torch.from_numpy(ro._sizes0_host.astype(np.int32)))
            else:
                self.sizes0.copy_(ro.sizes0_dev)
        side0 = start_maker if P % 2 == 0 else not start_maker
        st = ops._stream()
        call = _lib.TransitionsCall(
            struct_bytes=C.sizeof(_lib.TransitionsCall), H=H, P=P, k=k, n_count=len(self.n_steps),
            prune_exploratories=int(bool(mgr.prune_exploratories)), side0_maker=int(side0), list_len=self.list_len,
            coef_stride=self.coef_host.shape[1], n_steps=C.cast(self._n_steps_c, C.c_void_p), result=self.result.data_ptr(),
            rank=self.rank.data_ptr(), expl=self.expl.data_ptr(), coef=self.coef.data_ptr(), src_step=self.src_step.data_ptr(),
            env=self.env.data_ptr(), action=self.action.data_ptr(), reward=self.reward.data_ptr(),
            next_step=self.next_step.data_ptr(), done=self.done.data_ptr(), count=self.count.data_ptr())
        _lib.check(L.hexgnn_transitions_assemble(C.byref(call), st), "hexgnn_transitions_assemble")
        rl = self._rec_len
        for s, buf in enumerate(self.bufs):
            rec = self.record[s * rl:(s + 1) * rl]
            sc = _lib.StoreCall(
                struct_bytes=C.sizeof(_lib.StoreCall), capacity=buf.capacity, nv=buf.nv, words=buf.words, list_len=self.list_len,
                side=1 - s, edge_limit=limits[s], H=H, P=P, k=k, start_nodes=int(mgr._base_sizes[0, 0]),
                start_edges=int(mgr._base_sizes[0, 1]), count=self.count[s:].data_ptr(), src_step=self.src_step[s].data_ptr(),
                env=self.env[s].data_ptr(), action=self.action[s].data_ptr(), reward=self.reward[s].data_ptr(),
                next_step=self.next_step[s].data_ptr(), done=self.done[s].data_ptr(), hist_adj=self.adj.data_ptr(),
                hist_alive=self.alive.data_ptr(), result=self.result.data_ptr(), sizes0=self.sizes0.data_ptr(),
                start_adj=self._start[0].data_ptr(), start_alive=self._start[1].data_ptr(), adj=buf.adj.data_ptr(),
                alive=buf.alive.data_ptr(), side_bytes=buf.side.data_ptr(), ring_action=buf.action.data_ptr(),
                ring_reward=buf.reward.data_ptr(), ring_done=buf.done.data_ptr(), sizes=buf.sizes_dev.data_ptr(),
                ring_words=buf._ring_words.data_ptr(), leaves=self.leaves[s].data_ptr(), record=rec.data_ptr(),
                env_done=self.record[2 * rl + 2 * k:].data_ptr() if s == 0 else None)
            _lib.check(L.hexgnn_replay_store_dev(C.byref(sc), st), "hexgnn_replay_store_dev")
            buf._tree_update_td(self.leaves[s], None)          # new transitions enter at the running maximum priority
        self.record[2 * rl:2 * rl + 2 * k].view(k, 2).copy_(self.result[H - 1, :, 2:4])
        # next prefix: the last `keep` moves with their keep + 1 observations (through scratch: the ranges may overlap)
        self.sizes0.copy_(self.result[H - kp - 1, :, 2:4])
        for hist, tail, n in zip((self.result, self.rank, self.expl, self.adj, self.alive), self._tail, (kp, kp, kp, kp + 1, kp + 1)):
            lo = H - kp
            tail.copy_(hist[lo:lo + n])
            hist[:n].copy_(tail)
        self._pinned.copy_(self.record, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self._prefix, self._pushed_run, self._touch, ro._open = True, ro._run_no, mgr._touch, False
        self._pending = (ev, ro._run_no, mgr._touch, P)
        for buf in self.bufs:
            buf._device_stores.append(self)

    def settle(self):
        """Consume the outstanding record, if any: refresh the manager's and the buffers' host mirrors, raise ``ValueError``
        for an illegal action (as ``run_end``) and ``RuntimeError`` when transitions were dropped by the edge limit, and
        return the push's episode counters ``{"games", "maker_wins", "length_sum"}`` (None without an outstanding push)."""
        if self._pending is None:
            return None
        ev, run_no, touch, P = self._pending
        ev.synchronize()
        rec = self._pinned.numpy().copy()
        self._pending = None
        mgr, ro, k, rl, L = self.mgr, self.rollout, self.mgr.num_envs, self._rec_len, self.list_len
        dropped = 0
        for s, buf in enumerate(self.bufs):
            buf._device_stores.remove(self)
            r = rec[s * rl:(s + 1) * rl]
            buf._device_store_settle(r[:16], r[16:16 + L], r[16 + L:].reshape(L, 4), 1 - s)
            dropped += int(r[2])
        head = rec[:16]
        # (not when the host has reset / stepped the boards since, or run_end has read this run or a later one: its sizes are newer)
        if touch == mgr._touch and ro._settled_run < run_no:
            mgr._sizes = rec[2 * rl:2 * rl + 2 * k].reshape(k, 2).astype(np.int64)
            mgr.last_obs = None
            now = time.perf_counter()
            for i in np.nonzero(rec[2 * rl + 2 * k:2 * rl + 3 * k])[0]:
                mgr._creation_time[i] = now
            ro._settled_run = run_no
        out = {"games": int(head[5]), "maker_wins": int(head[6]), "length_sum": int(head[7])}
        self.games += out["games"]
        self.maker_wins += out["maker_wins"]
        self.length_sum += out["length_sum"]
        if head[8]:
            t, i = divmod(int(head[8]) - 1, k)
            raise ValueError("illegal action at step %d for env %d" % (t, i))
        if dropped:
            raise RuntimeError("%d transitions were dropped: a graph of %d directed edges exceeds what the replay buffers' draw "
                               "buffers hold per graph (the sizes are recorded: GraphedUpdate makes larger ones on its next step)"
                               % (dropped, max(int(rec[4]), int(rec[rl + 4]))))
        return out


class _EnvView:
    """Read-only stand-in for the per-env ``Hex_game`` objects of the reference's ``Env_manager.envs``."""

    def __init__(self, mgr, idx):
        self._m, self._i = mgr, idx

    @property
    def onturn(self):
        return self._m.global_onturn

    @property
    def not_onturn(self):
        return "b" if self._m.global_onturn == "m" else "m"

    @property
    def total_num_moves(self):
        return int(self._m._state()["total_moves"][self._i])

    @property
    def creation_time(self):
        return self._m._creation_time[self._i]

    def get_actions(self):
        return self._m.get_valid_actions()[self._i]


class Env_manager:
    last_obs: ObsList

    def __init__(self, num_envs, hex_size, gamma=1, n_steps=[1], prune_exploratories=True, cnn_rep=False,
                 cnn_hex_size=5, gao_mode=False, border_fill=True, device=None):
        if cnn_rep:
            raise NotImplementedError("cnn_rep=True (CNN planes) is outside the accelerated hot path")
        self.num_envs = num_envs
        self.gamma = gamma
        self.global_onturn = "m"
        self.n_steps = n_steps
        self.prune_exploratories = prune_exploratories
        self.cnn_rep = cnn_rep
        self.gao_mode = gao_mode
        self.border_fill = border_fill
        self.cnn_hex_size = cnn_hex_size
        self.record_snapshots = True     # keep the 2 KB/env board snapshot with every observation (replay storage)
        self.device = torch.device(device if device is not None else "cuda")
        if self.device.type != "cuda":
            raise _lib.HexGnnError("Env_manager runs only on the MI355X HIP path (no CPU fallback)")
        self._h = None
        self._base = None
        self.change_hex_size(hex_size)

    # ---- handles ---------------------------------------------------------------------------------------
    def _destroy(self):
        L = _lib.lib()
        for name in ("_h", "_base"):
            h = getattr(self, name, None)
            if h:
                L.hexgnn_env_destroy(h)
                setattr(self, name, None)

    def __del__(self):
        try:
            self._destroy()
        except Exception:
            pass

    def change_hex_size(self, new_size):
        L = _lib.lib()
        self._destroy()
        self._touch = getattr(self, "_touch", 0) + 1      # the boards changed under any rollout in flight (DeviceRollout.run_continue)
        self.hex_size = new_size
        self.global_onturn = "m"
        with torch.cuda.device(self.device):
            h, hb = C.c_void_p(), C.c_void_p()
            _lib.check(L.hexgnn_env_create(self.num_envs, new_size, C.byref(h)), "hexgnn_env_create")
            _lib.check(L.hexgnn_env_create(1, new_size, C.byref(hb)), "hexgnn_env_create")
        self._h, self._base = h, hb
        self._nv = L.hexgnn_env_num_vertices(h)
        self._words = L.hexgnn_env_words(h)
        nv, n = self._nv, new_size
        e_start = 2 * (2 * n + (n - 2) * (n - 1) + n * (n - 1) + (n - 1) ** 2)
        self._sizes = np.tile(np.array([[nv, e_start]], dtype=np.int64), (self.num_envs, 1))
        self._base_sizes = np.array([[nv, e_start]], dtype=np.int64)
        self._creation_time = [time.perf_counter()] * self.num_envs
        self.envs = [_EnvView(self, i) for i in range(self.num_envs)]
        self.base_game = None
        self.last_obs = None

    # ---- observation -----------------------------------------------------------------------------------
    def _snapshot_handle(self, h, k):
        L = _lib.lib()
        dev = self.device
        adj = torch.empty((k, self._nv, self._words), dtype=torch.int64, device=dev)
        alive = torch.empty((k, self._nv), dtype=torch.uint8, device=dev)
        mt = torch.empty(k, dtype=torch.int32, device=dev)
        tm = torch.empty(k, dtype=torch.int32, device=dev)
        _lib.check(L.hexgnn_env_export(h, adj.data_ptr(), alive.data_ptr(), mt.data_ptr(), tm.data_ptr(), None, None,
                                       ops._stream()), "hexgnn_env_export")
        return adj, alive

    def _observe_handle(self, h, sizes, is_maker) -> ObsList:
        k = sizes.shape[0]
        t = ObsTarget.exact(sizes, self.device)
        t.observe_env(h)
        snap = self._snapshot_handle(h, k) if self.record_snapshots else None
        return ObsList(t.x, t.edge_local, t.edge_global, t.backmap, t.batch_vec, t.node_off_host.tolist(),
                       t.edge_off_host.tolist(), t.gs, is_maker, int(sizes[:, 0].max()) if k else 0, snap)

    @property
    def starting_obs(self) -> Data:
        """Fresh ``Data`` of the start position with maker to move (multi_env_manager.py:41-49)."""
        obs = self._observe_handle(self._base, self._base_sizes, True)
        d = obs[0]
        out = Data(x=d.x.clone(), edge_index=d.edge_index.clone(), backmap=d.backmap.clone())
        out._hex_src = (obs, 0)
        return out

    def observe(self) -> ObsList:
        self.last_obs = self._observe_handle(self._h, self._sizes, self.global_onturn == "m")
        return self.last_obs

    # ---- actions ---------------------------------------------------------------------------------------
    @staticmethod
    def validate_actions(states, actions: List[int]):
        """Node rank -> vertex id through each state's backmap (multi_env_manager.py:62-64)."""
        if isinstance(states, ObsList):
            idx = torch.as_tensor([int(a) for a in actions], dtype=torch.long, device=states.x.device)
            base = torch.as_tensor(states.node_off[:-1], dtype=torch.long, device=states.x.device)
            return states.backmap[base + idx].tolist()
        return [state.backmap[action].item() for state, action in zip(states, actions)]

    def select_actions(self, q: torch.Tensor, states: "ObsList" = None, eps: float = 0.0, generator=None,
                       temperature: float = None):
        """Device-side acting: epsilon-greedy over each env's non-terminal nodes given the model output for the batched
        observation (``Q`` or ``advantages_only`` values).  Returns ``(vertex_actions int32 [num_envs] on the device --
        ready for ``step`` --, node ranks, exploratory flags)``; nothing is copied to the host.

        With a ``temperature`` every env's move is instead one draw from softmax(q / temperature) over its non-terminal nodes
        (GN0/RainbowDQN/evaluate_elo.py:267-273; 0 = the first maximum), from one uniform per env out of ``generator``;
        ``eps`` must then be 0, no move counts as exploratory, and ``self.sample_status`` (int32 [1] on the device) is
        non-zero when some env's values held a NaN."""
        states = states if states is not None else self.last_obs
        dev = self.device
        k = len(states)
        if states._ptr is None:
            states._ptr = torch.tensor(states.node_off, dtype=torch.long, device=dev)
        gptr = states._ptr.to(torch.int32)
        qf = q.reshape(-1).float().contiguous()
        vert = torch.empty(k, dtype=torch.int32, device=dev)
        rank = torch.empty(k, dtype=torch.int32, device=dev)
        if temperature is not None:
            temperature = float(temperature)
            if eps != 0 or not temperature >= 0.0 or temperature == float("inf"):
                raise ValueError("temperature sampling takes eps == 0 and a finite temperature >= 0")
            u = torch.rand(k, dtype=torch.float32, device=dev, generator=generator)
            self.sample_status = torch.empty(1, dtype=torch.int32, device=dev)
            _lib.check(_lib.lib().hexgnn_sample_actions(k, gptr.data_ptr(), qf.data_ptr(), states.backmap.data_ptr(),
                                                        2 if temperature > 0 else 0, temperature if temperature > 0 else 1.0,
                                                        u.data_ptr(), vert.data_ptr(), rank.data_ptr(),
                                                        self.sample_status.data_ptr(), ops._stream()),
                       "hexgnn_sample_actions")
            return vert, rank, torch.zeros(k, dtype=torch.bool, device=dev)
        expl = torch.empty(k, dtype=torch.uint8, device=dev)
        u = torch.rand((k, 2), dtype=torch.float32, device=dev, generator=generator) if eps > 0 else None
        _lib.check(_lib.lib().hexgnn_select_actions(k, gptr.data_ptr(), qf.data_ptr(), states.backmap.data_ptr(),
                                                    float(eps), u.data_ptr() if u is not None else None, vert.data_ptr(),
                                                    rank.data_ptr(), expl.data_ptr(), ops._stream()),
                   "hexgnn_select_actions")
        return vert, rank, expl.bool()

    def get_valid_actions(self) -> List[np.ndarray]:
        obs = self.last_obs if self.last_obs is not None else self.observe()
        bm = obs.backmap.cpu().numpy()
        return [bm[obs.node_off[i] + 2:obs.node_off[i + 1]] for i in range(self.num_envs)]

    def sample(self) -> np.ndarray:
        return np.array([np.random.choice(x) for x in self.get_valid_actions()])

    # ---- stepping --------------------------------------------------------------------------------------
    def step(self, actions) -> Tuple[ObsList, np.ndarray, np.ndarray, List[dict]]:
        L = _lib.lib()
        if torch.is_tensor(actions):
            act = actions.to(device=self.device, dtype=torch.int32).contiguous()
        else:
            act = torch.as_tensor(np.asarray([int(a) for a in actions], dtype=np.int32)).to(self.device)
        if act.numel() != self.num_envs:
            raise ValueError("expected %d actions" % self.num_envs)
        result = torch.empty((self.num_envs, 5), dtype=torch.int32, device=self.device)
        reset_maker = self.global_onturn == "b"      # finished envs restart on the side everyone moves to next
        self._touch += 1
        _lib.check(L.hexgnn_env_step(self._h, act.data_ptr(), 1, 1, int(reset_maker), result.data_ptr(), ops._stream()),
                   "hexgnn_env_step")
        res = result.cpu().numpy()
        if res[:, 4].any():
            bad = int(np.nonzero(res[:, 4])[0][0])
            raise ValueError("illegal action %d for env %d" % (int(act[bad]), bad))
        now = time.perf_counter()
        rewards = np.zeros(self.num_envs, dtype=float)
        dones = res[:, 0] >= 0
        infos = [{} for _ in range(self.num_envs)]
        mover = self.global_onturn
        for i in np.nonzero(dones)[0]:
            winner = "m" if res[i, 0] == 0 else "b"
            n = int(res[i, 1])
            infos[i]["episode_metrics"] = {
                "return": 1 if winner == "m" else -1,
                "discounted_return": float(1 * self.gamma ** n if winner == "m" else -1 * self.gamma ** n),
                "length": n,
                "time": now - self._creation_time[i],
            }
            rewards[i] = 1 if winner == mover else -1       # winner == env.not_onturn after the move
            self._creation_time[i] = now
        self.global_onturn = "m" if self.global_onturn == "b" else "b"
        self._sizes = res[:, 2:4].astype(np.int64)
        states = self.observe()
        return states, rewards, dones.astype(bool), infos

    # ---- positions -------------------------------------------------------------------------------------
    def _pack_stones(self, stones, counts=None):
        """``(int32 [num_envs][L] HEXGNN_STONE rows, int32 [num_envs] counts)`` as host arrays, L >= 1."""
        k = self.num_envs
        if isinstance(stones, np.ndarray) or torch.is_tensor(stones):
            arr = np.ascontiguousarray(stones.cpu().numpy() if torch.is_tensor(stones) else stones).astype(np.int32)
            if arr.ndim != 2 or arr.shape[0] != k or arr.shape[1] < 1:
                raise ValueError("a stone array has the shape [%d][L], L >= 1" % k)
            cnt = np.full(k, arr.shape[1], dtype=np.int32) if counts is None else np.asarray(counts, dtype=np.int32).reshape(-1)
            if cnt.shape[0] != k or (cnt < 0).any() or (cnt > arr.shape[1]).any():
                raise ValueError("counts: %d entries in 0 .. %d" % (k, arr.shape[1]))
            return arr, np.ascontiguousarray(cnt)
        if counts is not None:
            raise ValueError("counts go with a packed stone array")
        rows = [list(r) for r in stones]
        if len(rows) != k:
            raise ValueError("expected %d stone lists" % k)
        arr = np.zeros((k, max(1, max(len(r) for r in rows))), dtype=np.int32)
        for i, r in enumerate(rows):
            arr[i, :len(r)] = [_lib.stone(*s) for s in r]
        return arr, np.asarray([len(r) for r in rows], dtype=np.int32)

    def set_positions(self, stones, onturn="m", from_start=True, counts=None) -> ObsList:
        """Put a position on every env with ONE launch (``hexgnn_env_setup``) and observe it: the reference's
        ``make_move(v, force_color=..., remove_dead_and_captured=...)`` stone by stone
        (GN0/tests/test_models_on_long_range_task.py:20-30).  ``stones``: per env a sequence of ``(vertex, colour)`` or
        ``(vertex, colour, remove)`` with colour ``"m"`` / ``"b"`` (a forced stone: the side and the move count stay) or
        ``"turn"`` (the move of the side on turn); or an int32 ``[num_envs][L]`` array of ``_lib.stone`` values with ``counts``.
        ``from_start``: every env starts from ``Hex_game(size)``, maker to move as there; else the stones go on top of the
        current boards.  After its last stone every env has ``onturn`` to move, and so has ``global_onturn``: the batched
        model needs one side per batch.  ``ValueError`` names env and stone for an illegal stone (a terminal, an out-of-range
        or dead vertex) and for a stone behind the one that decided the game -- such an env is back at the start position --
        and is raised for a position that is decided after its last stone, which cannot be observed.  A latency path: one
        launch and one read-back of the result record; nobody has timed it."""
        if onturn not in ("m", "b"):
            raise ValueError("onturn must be \"m\" or \"b\"")
        arr, cnt = self._pack_stones(stones, counts)
        k, dev = self.num_envs, self.device
        st = torch.from_numpy(arr).to(dev)
        ct = torch.from_numpy(cnt).to(dev)
        result = torch.empty((k, 5), dtype=torch.int32, device=dev)
        applied = torch.empty(k, dtype=torch.int32, device=dev)
        call = _lib.SetupCall(struct_bytes=C.sizeof(_lib.SetupCall), max_stones=arr.shape[1], from_start=int(bool(from_start)),
                              maker_turn_start=1, maker_turn_after=int(onturn == "m"), stones=st.data_ptr(), count=ct.data_ptr(),
                              result=result.data_ptr(), applied=applied.data_ptr())
        self._touch += 1
        _lib.check(_lib.lib().hexgnn_env_setup(self._h, C.byref(call), ops._stream()), "hexgnn_env_setup")
        res = result.cpu().numpy()
        self.global_onturn = onturn
        self._sizes = res[:, 2:4].astype(np.int64)
        self.last_obs = None
        if from_start:
            self._creation_time = [time.perf_counter()] * k
        if res[:, 4].any():
            # an env with an error went back to the start position with the maker to move: give it everyone's side
            _lib.check(_lib.lib().hexgnn_env_set_maker_turn(self._h, int(onturn == "m"), ops._stream()),
                       "hexgnn_env_set_maker_turn")
            bad = int(np.nonzero(res[:, 4])[0][0])
            j = int(applied[bad])
            what = ("is not a live board vertex" if res[bad, 4] == 1 else "follows the stone that decided the game")
            raise ValueError("env %d, stone %d (vertex %d) %s" % (bad, j, int(arr[bad, j]) & 0xffff, what))
        if (res[:, 0] >= 0).any():
            bad = int(np.nonzero(res[:, 0] >= 0)[0][0])
            raise ValueError("env %d: the position is decided after its last stone (%s has won) and cannot be observed"
                             % (bad, "the maker" if res[bad, 0] == 0 else "the breaker"))
        return self.observe()

    def reset(self) -> ObsList:
        L = _lib.lib()
        self.global_onturn = "m"
        self._touch += 1
        _lib.check(L.hexgnn_env_reset(self._h, None, 1, None, ops._stream()), "hexgnn_env_reset")
        self._sizes = np.tile(self._base_sizes, (self.num_envs, 1))
        self._creation_time = [time.perf_counter()] * self.num_envs
        return self.observe()

    def _state_tensors(self):
        """Device copy of the full env state (boards, side, move counters, response sets)."""
        L = _lib.lib()
        dev = self.device
        k, nv = self.num_envs, self._nv
        t = dict(adj=torch.empty((k, nv, self._words), dtype=torch.int64, device=dev),
                 alive=torch.empty((k, nv), dtype=torch.uint8, device=dev),
                 mt=torch.empty(k, dtype=torch.int32, device=dev), tm=torch.empty(k, dtype=torch.int32, device=dev),
                 rm=torch.empty((k, nv), dtype=torch.int16, device=dev), rb=torch.empty((k, nv), dtype=torch.int16, device=dev))
        _lib.check(L.hexgnn_env_export(self._h, t["adj"].data_ptr(), t["alive"].data_ptr(), t["mt"].data_ptr(),
                                       t["tm"].data_ptr(), t["rm"].data_ptr(), t["rb"].data_ptr(), ops._stream()),
                   "hexgnn_env_export")
        t["sizes"], t["onturn"] = self._sizes.copy(), self.global_onturn
        return t

    def _restore_state_tensors(self, t):
        _lib.check(_lib.lib().hexgnn_env_import(self._h, t["adj"].data_ptr(), t["alive"].data_ptr(), t["mt"].data_ptr(),
                                               t["tm"].data_ptr(), t["rm"].data_ptr(), t["rb"].data_ptr(), ops._stream()),
                   "hexgnn_env_import")
        self._sizes, self.global_onturn = t["sizes"].copy(), t["onturn"]
        self._touch += 1
        self.last_obs = None

    # ---- raw state (tests, debugging) ------------------------------------------------------------------
    def _state(self):
        L = _lib.lib()
        dev = self.device
        adj = torch.empty((self.num_envs, self._nv, self._words), dtype=torch.int64, device=dev)
        alive = torch.empty((self.num_envs, self._nv), dtype=torch.uint8, device=dev)
        mt = torch.empty(self.num_envs, dtype=torch.int32, device=dev)
        tm = torch.empty(self.num_envs, dtype=torch.int32, device=dev)
        rm = torch.empty((self.num_envs, self._nv), dtype=torch.int16, device=dev)
        rb = torch.empty((self.num_envs, self._nv), dtype=torch.int16, device=dev)
        _lib.check(L.hexgnn_env_export(self._h, adj.data_ptr(), alive.data_ptr(), mt.data_ptr(), tm.data_ptr(),
                                       rm.data_ptr(), rb.data_ptr(), ops._stream()), "hexgnn_env_export")
        return dict(adj=adj.cpu().numpy().view(np.uint64), alive=alive.cpu().numpy(), maker_turn=mt.cpu().numpy(),
                    total_moves=tm.cpu().numpy(), resp_maker=rm.cpu().numpy(), resp_breaker=rb.cpu().numpy())

    # ---- transition assembly, array form (same semantics as get_transitions below, no per-transition objects) --
    def assemble_transitions(self, starting_states, state_history: list, action_history: list, reward_history: list,
                             done_history: list, exploratories_history: list, _already_emitted=None):
        """``get_transitions`` (multi_env_manager.py:113-165) vectorised over the envs: returns
        ``(maker_block, breaker_block)`` of ``TransitionBlock`` whose entries appear in exactly the order the list
        form emits them.  Histories may hold ``ObsList`` observations (states stay on the device as board snapshots)."""
        sh = list(state_history)
        sh.insert(0, starting_states)
        T = len(action_history)
        A = np.asarray([np.asarray(a, dtype=np.int64) for a in action_history]).reshape(T, -1)
        R = np.asarray(reward_history, dtype=np.float64).reshape(T, -1)
        D = np.asarray(done_history, dtype=bool).reshape(T, -1)
        X = np.asarray(exploratories_history, dtype=bool).reshape(T, -1)
        E = A.shape[1]
        ks = np.arange(E)
        out = {True: [], False: []}
        for i in range(T):
            start_state = sh[i]
            maker_side = start_state.is_maker if isinstance(start_state, ObsList) else bool(start_state[0].x[0, 2] == 1)
            for n_step in self.n_steps:
                if not len(sh) > i + 2 * n_step:
                    continue
                if _already_emitted is not None and i < _already_emitted.get(n_step, 0):
                    continue        # RolloutStitcher: this window was complete, and emitted, in the previous rollout
                w = 2 * n_step
                jj = np.arange(w)
                coef = ((-(jj % 2)) * 2 + 1) * (float(self.gamma) ** (jj // 2))          # sign * gamma^((j-i)//2)
                r = R[i:i + w] * coef[:, None]
                csum = np.cumsum(r, axis=0)                                                # reward through window step j
                d = D[i:i + w]
                first_done = np.where(d.any(0), d.argmax(0), w)                           # w = none
                if self.prune_exploratories:
                    x = X[i:i + w].copy()
                    x[0] = False                                                           # only j > i prunes
                    first_expl = np.where(x.any(0), x.argmax(0), w)
                else:
                    first_expl = np.full(E, w)
                terminal = (first_done < w) & (first_done <= first_expl)
                pruned = (first_expl < w) & (first_expl < first_done)
                full = ~terminal & ~pruned
                emit = terminal | full
                jend = np.where(terminal, first_done, w - 1)
                reward = csum[jend, ks]
                nxt = np.where(terminal, -1, i + w)
                sel = ks[emit]
                out[maker_side].append((np.full(sel.shape, i), sel, A[i, sel], reward[sel], nxt[sel], terminal[sel]))
        blocks = []
        start_obs = None
        for side in (True, False):
            if out[side]:
                cat = [np.concatenate(c) for c in zip(*out[side])]
            else:
                cat = [np.zeros(0, dtype=np.int64)] * 3 + [np.zeros(0)] + [np.zeros(0, dtype=np.int64), np.zeros(0, dtype=bool)]
            if start_obs is None and len(cat[1]) and (cat[4] < 0).any():
                start_obs = self._observe_handle(self._base, self._base_sizes, True)
            blocks.append(TransitionBlock(sh, start_obs, side, *cat))
        if start_obs is not None:
            for b in blocks:
                b.start_obs = start_obs
        return blocks[0], blocks[1]

    # ---- transition assembly, list form (the reference's return type) -----------------------------------------
    def get_transitions(self, starting_states, state_history: list, action_history: list, reward_history: list,
                        done_history: list, exploratories_history: list):
        """``(maker_transitions, breaker_transitions)``, each a list of ``(s, a, r, s', done)`` -- the reference's
        n-step, sign-alternating, gamma-discounted two-player transitions, an exploratory action after the first step
        pruning a transition (graph_game/multi_env_manager.py:113-165).  Built from ``assemble_transitions`` (the
        rewards, windows and emission order are computed once, vectorised over envs); this method only materialises the
        per-transition ``Data`` views the list API promises: ``backmap`` removed from the states, a fresh start
        observation with the side column set for terminal transitions."""
        blocks = self.assemble_transitions(starting_states, state_history, action_history, reward_history,
                                           done_history, exploratories_history)
        out = []
        for blk in blocks:
            lst = []
            for src, env, act, rew, nxt, done in zip(blk.src_step.tolist(), blk.env.tolist(), blk.action.tolist(),
                                                     blk.reward.tolist(), blk.next_step.tolist(), blk.done.tolist()):
                s_k = blk.obs_list[src][env]
                if hasattr(s_k, "backmap"):
                    s_k.__delattr__("backmap")
                assert act < len(s_k.x)
                if done:
                    s_next = self.starting_obs
                    s_next.__delattr__("backmap")
                    s_next.x[:, 2] = 1.0 if blk.maker_side else 0.0
                    ops.attach_hints(s_next.x, blk.maker_side)
                else:
                    s_next = blk.obs_list[nxt][env]
                    if hasattr(s_next, "backmap"):
                        s_next.__delattr__("backmap")
                lst.append((s_k, action_history[src][env], rew, s_next, bool(done)))
            out.append(lst)
        return out[0], out[1]
