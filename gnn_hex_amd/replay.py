"""Device-resident n-step replay for the RainbowDQN loop: transitions as produced by ``Env_manager.get_transitions``
are stored in HBM as fixed-size board-state snapshots (the env's adjacency bit matrix: 2 KB per Hex-11 state), sampled
uniformly or with proportional prioritisation (sum / min trees on the device, ``hexgnn_per_*``), and the sampled
states are rebuilt into ``Batch`` objects by the same observation kernel the env uses (``hexgnn_states_observe``) --
sorted CSR, side to move and largest graph size attached, no host-side collation.

The reference's buffer lives in the un-vendored submodule ``GN0/RainbowDQN/Rainbow`` (.gitmodules:1-4); only its flags
are known (README.md:5,7: ``--buffer_size=260000 --burnin=20000 --prioritized_er=True --prioritized_er_beta0=0.6
--n_step=2``).  PARITY UNPINNED: this class follows the published algorithm (oracle/replay_ref.py) and is checked
against that oracle; method names follow the upstream buffer (``put`` / ``sample`` / ``update_priorities``).
"""
from __future__ import annotations

import ctypes
import weakref
from typing import List, Optional

import numpy as np
import torch

from . import _lib, ops
from .data import Batch, block_groups, blocks_for_order, pack_groups, pack_order
from .observation import ObsTarget


def _pow2_at_least(n: int) -> int:
    p = 1
    while p < n:
        p *= 2
    return p


class GraphReplayBuffer:
    """Ring of ``capacity`` transitions ``(state, action, reward, next_state, done)`` for one side (the loop keeps one
    buffer for maker and one for breaker transitions, multi_env_manager.py:139)."""

    def __init__(self, capacity: int, hex_size: int, prioritized: bool = True, alpha: float = 0.5, eps: float = 1e-6,
                 burnin: int = 0, device="cuda", pack_blocks: bool = True, group_blocks: bool = False):
        """``pack_blocks`` (boards above 128 nodes, Hex-12 and larger, which run on the one-launch SAGE stack kernels): a draw is
        listed in ``data.pack_order`` order -- indices, weights, both batches, actions, rewards and done flags alike, the order of
        a random draw carries no meaning -- with the row-block tables attached, so that workgroups hold whole graphs or their own
        pieces of a large one instead of whatever a multiple of 128 rows cuts.

        ``group_blocks``: a draw with more rows than can be resident at once (256 Hex-13 boards: one launch per layer otherwise)
        is packed with ``data.pack_groups`` and both batches carry their table in groups of whole graphs, one launch per group
        (``hexgnn_sage_stack_call.group_starts``).  Off by default: see ``Batch.from_data_list``."""
        self.capacity, self.hex_size = int(capacity), int(hex_size)
        self.pack_blocks = bool(pack_blocks) and hex_size * hex_size + 2 > 128
        self.group_blocks = bool(group_blocks)
        self._max_blocks = None
        self.prioritized, self.alpha, self.eps, self.burnin = prioritized, float(alpha), float(eps), int(burnin)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.HexGnnError("GraphReplayBuffer lives in HBM (no CPU fallback)")
        nv = hex_size * hex_size + 2
        self.nv, self.words = nv, (nv + 63) // 64
        dev, C = self.device, self.capacity
        z = lambda *shape, dtype: torch.zeros(shape, dtype=dtype, device=dev)
        # states and next states share one array pair: slot i = state of transition i, slot C + i = its next state
        self.adj = z(2 * C, nv, self.words, dtype=torch.int64)
        self.alive = z(2 * C, nv, dtype=torch.uint8)
        self.side = z(2 * C, dtype=torch.uint8)
        self.action = z(C, dtype=torch.long)
        self.reward = z(C, dtype=torch.float32)
        self.done = z(C, dtype=torch.bool)
        self.n_nodes = np.zeros(2 * C, dtype=np.int64)      # host copies of the graph sizes (known when stored)
        self.n_edges = np.zeros(2 * C, dtype=np.int64)
        self.side_host = np.zeros(2 * C, dtype=np.uint8)    # host mirror of `side` (sampling needs it without a sync)
        self.pos, self.size = 0, 0
        self.cap2 = _pow2_at_least(C)
        self.sum_tree = torch.empty(2 * self.cap2, dtype=torch.float64, device=dev)
        self.min_tree = torch.empty(2 * self.cap2, dtype=torch.float64, device=dev)
        _lib.check(_lib.lib().hexgnn_per_init(self.cap2, self.sum_tree.data_ptr(), self.min_tree.data_ptr(), ops._stream()),
                   "hexgnn_per_init")
        self.max_priority = torch.ones((), dtype=torch.float64, device=dev)
        # device mirror of the graph sizes, [slot] = (nodes, directed edges) as int32 pairs: what a draw sized on the device
        # (sample_device) prefix-sums.  Written by put / put_block as ONE int64 word per slot (nodes | edges << 32).
        self.sizes_dev = z(2 * C, 2, dtype=torch.int32)
        self._sizes64 = self.sizes_dev.view(torch.int64).view(2 * C)
        self._sides = (set(), set())                      # movers' sides ever stored: of the states, of the next states
        n = self.hex_size
        self._e_start = 2 * (2 * n + (n - 2) * (n - 1) + n * (n - 1) + (n - 1) ** 2)      # directed edges of the start position
        self._max_edges, self._max_nodes = 0, 0           # largest graph ever stored (host-known: bounds of sample_device)
        self._draw_size = z(1, dtype=torch.int32)         # fill level and beta of the next device-side draw
        self._draw_beta = z(1, dtype=torch.float64)
        # device stores (multi_env_manager.DeviceTransitionFeed): the ring's (position, fill level) as device words once a feed
        # has stored here, the feeds whose record the host has not consumed yet, and the draw buffers handed out (weakly held:
        # the store's edge limit is the smallest of them)
        self._ring_words = None
        self._device_stores = []
        self._draw_ecaps = weakref.WeakSet()

    def __len__(self):
        self._settle()
        return self.size

    @property
    def burnedin(self) -> bool:
        self._settle()
        return self.size >= self.burnin

    # ---- stores issued on the device -----------------------------------------------------------------------
    def _settle(self) -> None:
        """Bring the host mirrors up to date with every device store issued so far (waits for their records).  Nothing to do
        for a buffer that never saw one."""
        while self._device_stores:
            self._device_stores[0].settle()

    def _sync_ring_words(self) -> None:
        """The host moved the ring (put / put_block): tell the device words.  The values travel as kernel arguments."""
        if self._ring_words is not None:
            self._ring_words[0:1].fill_(int(self.pos))
            self._ring_words[1:2].fill_(int(self.size))

    def _device_store_begin(self, feed) -> int:
        """A feed is about to store here: make the device words and return the edge limit of this store -- no slot may hold a
        graph with more directed edges than ANY draw buffer in use has columns per graph (``hexgnn_states_observe`` does not
        check), whatever the host's lagging ``_max_edges`` says."""
        self._settle()
        if self._ring_words is None:
            self._ring_words = torch.zeros(2, dtype=torch.int32, device=self.device)
            self._sync_ring_words()
        return min([self.edge_capacity()] + [b.e_cap for b in self._draw_ecaps])

    def _device_store_settle(self, head: np.ndarray, slots: np.ndarray, sizes: np.ndarray, side: int) -> None:
        """Host mirrors after one device store, from its record (``hexgnn_replay_store_dev``)."""
        C = self.capacity
        kept = slots >= 0
        sl = slots[kept].astype(np.int64)
        if len(sl):
            self.n_nodes[sl], self.n_edges[sl] = sizes[kept, 0], sizes[kept, 1]
            self.n_nodes[sl + C], self.n_edges[sl + C] = sizes[kept, 2], sizes[kept, 3]
            self.side_host[sl] = side
            self.side_host[sl + C] = side
            self._sides[0].add(int(side))
            self._sides[1].add(int(side))
        self.pos, self.size = int(head[10]), int(head[11])
        self._max_nodes, self._max_edges = max(self._max_nodes, int(head[3])), max(self._max_edges, int(head[4]))

    # ---- insertion ---------------------------------------------------------------------------------------
    @staticmethod
    def _source(d):
        src = getattr(d, "_hex_src", None)
        if src is None:
            raise ValueError("GraphReplayBuffer stores states observed by gnn_hex_amd.Env_manager (they carry the "
                             "board snapshot); got a Data object without one")
        return src

    def _store_states(self, datas, slots: np.ndarray):
        groups = {}
        for d, slot in zip(datas, slots):
            obs, i = self._source(d)
            g = groups.setdefault(id(obs), (obs, [], [], []))
            g[1].append(i)
            g[2].append(int(slot))
            hint = getattr(d.x, "_hex_is_maker", None)
            g[3].append(int(obs.is_maker if hint is None else hint))
            self.n_nodes[slot] = obs.node_off[i + 1] - obs.node_off[i]
            self.n_edges[slot] = obs.edge_off[i + 1] - obs.edge_off[i]
            self._sides[int(slot >= self.capacity)].add(g[3][-1])
        self._note_sizes(np.asarray(slots, dtype=np.int64))
        dev = self.device
        for obs, idx, slot, side in groups.values():
            it = torch.as_tensor(idx, dtype=torch.long, device=dev)
            st = torch.as_tensor(slot, dtype=torch.long, device=dev)
            snap_adj, snap_alive = obs.snapshot()
            self.adj[st] = snap_adj[it]
            self.alive[st] = snap_alive[it]
            self.side[st] = torch.as_tensor(side, dtype=torch.uint8, device=dev)
            self.side_host[np.asarray(slot, dtype=np.int64)] = np.asarray(side, dtype=np.uint8)

    def _note_sizes(self, slots: np.ndarray) -> None:
        if len(slots):
            self._max_nodes = max(self._max_nodes, int(self.n_nodes[slots].max()))
            self._max_edges = max(self._max_edges, int(self.n_edges[slots].max()))

    def _size_words(self, slots: np.ndarray) -> np.ndarray:
        """(nodes | edges << 32) of the given slots: the device mirror's int64 words."""
        return self.n_nodes[slots] | (self.n_edges[slots] << 32)

    def put(self, transitions: List[tuple]) -> None:
        """Append transitions ``(state, action, reward, next_state, done)`` as returned by
        ``Env_manager.get_transitions``; new entries get the running maximum priority."""
        self._settle()
        k = len(transitions)
        if k == 0:
            return
        if k > self.capacity:
            transitions = transitions[-self.capacity:]
            k = self.capacity
        C = self.capacity
        slots = (self.pos + np.arange(k)) % C
        self._store_states([t[0] for t in transitions], slots)
        self._store_states([t[3] for t in transitions], slots + C)
        dev = self.device
        st = torch.as_tensor(slots, dtype=torch.long, device=dev)
        words = torch.as_tensor(np.stack([self._size_words(slots), self._size_words(slots + C)]), device=dev)
        self._sizes64[st] = words[0]
        self._sizes64[st + C] = words[1]
        self.action[st] = torch.as_tensor([int(t[1]) for t in transitions], dtype=torch.long, device=dev)
        self.reward[st] = torch.as_tensor([float(t[2]) for t in transitions], dtype=torch.float32, device=dev)
        self.done[st] = torch.as_tensor([bool(t[4]) for t in transitions], dtype=torch.bool, device=dev)
        self.pos = int((self.pos + k) % C)
        self.size = min(C, self.size + k)
        self._sync_ring_words()
        if self.prioritized:
            self._tree_update_td(st, None)         # new transitions enter at the running maximum priority

    def _store_indexed(self, obs_list, start_obs, steps: np.ndarray, envs: np.ndarray, slots: np.ndarray, side: bool):
        """Copy board snapshots ``obs_list[steps[i]][envs[i]]`` (``steps[i] == -1``: the start position) into ring
        slots: the distinct observations' snapshots are concatenated once and all entries move in ONE indexed copy per
        array (a loop over the observations cost ~8 small launches each: 4 ms of host time per 16-move rollout block)."""
        dev = self.device
        rows = np.zeros(len(steps), dtype=np.int64)      # row of every entry inside the concatenated snapshots
        adjs, alives, off = [], [], 0
        for st in np.unique(steps):
            m = steps == st
            obs = start_obs if st < 0 else obs_list[int(st)]
            idx = np.zeros(int(m.sum()), dtype=np.int64) if st < 0 else envs[m]
            sl = slots[m]
            noff, eoff = np.asarray(obs.node_off), np.asarray(obs.edge_off)
            self.n_nodes[sl] = noff[idx + 1] - noff[idx]
            self.n_edges[sl] = eoff[idx + 1] - eoff[idx]
            snap_adj, snap_alive = obs.snapshot()
            adjs.append(snap_adj)
            alives.append(snap_alive)
            rows[m] = off + idx
            off += snap_adj.shape[0]
        if not adjs:
            return
        src = torch.from_numpy(rows).to(dev)
        dst = torch.from_numpy(np.ascontiguousarray(slots, dtype=np.int64)).to(dev)
        all_adj = adjs[0] if len(adjs) == 1 else torch.cat(adjs)
        all_alive = alives[0] if len(alives) == 1 else torch.cat(alives)
        self.adj.index_copy_(0, dst, all_adj.index_select(0, src))
        self.alive.index_copy_(0, dst, all_alive.index_select(0, src))
        self.side.index_fill_(0, dst, 1 if side else 0)
        self.side_host[slots] = 1 if side else 0

    def put_block(self, block) -> None:
        """Append a ``TransitionBlock`` from ``Env_manager.assemble_transitions`` (array form of ``put``)."""
        self._settle()
        k = len(block)
        if k == 0:
            return
        C = self.capacity
        src, env, act = block.src_step, block.env, block.action
        rew, nxt, done = block.reward, block.next_step, block.done
        if k > C:
            src, env, act, rew, nxt, done = (v[-C:] for v in (src, env, act, rew, nxt, done))
            k = C
        slots = (self.pos + np.arange(k)) % C
        # states into slots [0, C), next states into [C, 2C): one pass
        both = np.concatenate([slots, slots + C])
        self._store_indexed(block.obs_list, block.start_obs, np.concatenate([src, nxt]), np.concatenate([env, env]),
                            both, block.maker_side)
        nn, ne = self.n_nodes[both], self.n_edges[both]
        self._max_nodes, self._max_edges = max(self._max_nodes, int(nn.max())), max(self._max_edges, int(ne.max()))
        self._sides[0].add(int(bool(block.maker_side)))
        self._sides[1].add(int(bool(block.maker_side)))
        dev = self.device
        # slots | actions | done flags | reward bit patterns | the slots of states and next states | their graph sizes (the device
        # mirror's words: nodes | edges << 32) in ONE host->device copy; the mirror then takes one indexed copy
        stage = np.empty((8, k), dtype=np.int64)
        stage[0], stage[1], stage[2] = slots, act, done
        stage[3] = np.ascontiguousarray(rew, dtype=np.float32).view(np.int32)
        stage[4:6] = both.reshape(2, k)
        stage[6:8] = (nn | (ne << 32)).reshape(2, k)
        sd = torch.from_numpy(stage).to(dev)
        st = sd[0]
        self._sizes64.index_copy_(0, sd[4:6].view(-1), sd[6:8].view(-1))
        self.action.index_copy_(0, st, sd[1])
        self.done.index_copy_(0, st, sd[2].bool())
        self.reward.index_copy_(0, st, sd[3].int().view(torch.float32))
        self.pos = int((self.pos + k) % C)
        self.size = min(C, self.size + k)
        self._sync_ring_words()
        if self.prioritized:
            self._tree_update_td(st, None)         # new transitions enter at the running maximum priority

    # ---- sampling ----------------------------------------------------------------------------------------
    def _build_batch(self, slots_dev: torch.Tensor, slots_host: np.ndarray, starts=None) -> Batch:
        dev = self.device
        k = len(slots_host)
        t = ObsTarget.exact(np.stack([self.n_nodes[slots_host], self.n_edges[slots_host]], axis=1), dev, with_ptr=True)
        t.observe_states(self.hex_size, self.adj, self.alive, self.side, slots_dev.to(torch.int32))
        N, gs = t.gs.n, t.gs
        b = Batch()
        b.x, b.edge_index, b.batch, b.ptr = t.x, t.edge_global, t.batch_vec, t.ptr
        b._num_graphs = k
        if starts is not None and len(starts) - 1 <= self._max_blocks:
            gs.blocks = (torch.tensor(starts, dtype=torch.int32).to(dev, non_blocking=True), len(starts) - 1)
        elif starts is not None and self.group_blocks and -(-N // 128) > self._max_blocks:
            # more rows than can be resident at once: whole graphs in groups, one launch of the stack kernels each
            groups = block_groups(self.n_nodes[slots_host], starts, self._max_blocks)
            if groups is not None:
                gs.groups = (torch.tensor(starts, dtype=torch.int32).to(dev, non_blocking=True), len(starts) - 1,
                             tuple(groups), (ctypes.c_int * len(groups))(*groups))
        b.edge_index._hex_csr = gs
        return b

    def sample(self, batch_size: int, beta: Optional[float] = None, generator: Optional[torch.Generator] = None):
        """Returns ``(indices, weights, state, next_state, action, reward, done)`` (weights all one when the buffer is
        not prioritized), states as device ``Batch`` objects.  One device->host copy of the sampled indices is needed
        to size the batches (the graph sizes live on the host)."""
        return self.sample_end(self.sample_begin(batch_size, beta, generator))

    def sample_begin(self, batch_size: int, beta: Optional[float] = None, generator: Optional[torch.Generator] = None):
        """First half of ``sample``: draws the indices on the device (stream-ordered behind every priority update issued
        so far) and starts their copy to pinned host memory; returns a handle for ``sample_end``.  A loop with several
        buffers can begin the next buffer's draw before it waits for this one, so that the host builds one batch while
        the GPU still runs the previous update (examples/selfplay_train.py)."""
        self._settle()
        if self.size == 0:
            raise ValueError("empty buffer")
        dev = self.device
        if self.prioritized:
            u = torch.rand(batch_size, dtype=torch.float64, device=dev, generator=generator)
            idx = torch.empty(batch_size, dtype=torch.int32, device=dev)
            w = torch.empty(batch_size, dtype=torch.float32, device=dev)
            _lib.check(_lib.lib().hexgnn_per_sample(self.cap2, self.size, batch_size, float(beta if beta is not None else 0.4),
                                                    u.data_ptr(), self.sum_tree.data_ptr(), self.min_tree.data_ptr(),
                                                    idx.data_ptr(), w.data_ptr(), ops._stream()), "hexgnn_per_sample")
            idx = idx.long()
        else:
            idx = torch.randint(0, self.size, (batch_size,), device=dev, generator=generator)
            w = torch.ones(batch_size, dtype=torch.float32, device=dev)
        host = torch.empty(batch_size, dtype=torch.int64, pin_memory=True)
        host.copy_(idx, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        return (idx, w, host, ev, (self.pos, self.size))

    def sample_end(self, pending):
        idx, w, host_t, ev, stamp = pending
        if stamp != (self.pos, self.size):
            raise RuntimeError("transitions were stored between sample_begin and sample_end: the drawn slots may have been "
                               "overwritten")
        ev.synchronize()
        host = host_t.numpy().copy()
        batch_size = len(host)
        st_blocks = nx_blocks = None
        if self.pack_blocks and batch_size:
            self._max_blocks = ops.stack_block_budget(self.device)      # (a host-side query; changes with GradSync.enable_overlap)
            order, st_blocks = pack_order(self.n_nodes[host], max_blocks=self._max_blocks)
            if st_blocks is None and self.group_blocks and self._max_blocks > 0:
                order, st_blocks, _ = pack_groups(self.n_nodes[host], max_blocks=self._max_blocks)
            if st_blocks is not None:
                perm = np.asarray(order, dtype=np.int64)
                host = host[perm]
                pd = torch.from_numpy(perm).to(self.device, non_blocking=True)
                idx, w = idx[pd], w[pd]
                nx_blocks = blocks_for_order(self.n_nodes[host + self.capacity])      # (same order: fewer nodes per graph)
        state = self._build_batch(idx, host, st_blocks)
        nxt = self._build_batch(idx + self.capacity, host + self.capacity, nx_blocks)
        # all stored states of one buffer share the mover's side (maker / breaker buffers are separate)
        for b, slots in ((state, host), (nxt, host + self.capacity)):
            ops.attach_hints(b.x, bool(self.side_host[int(slots[0])]) if batch_size else True,
                             int(self.n_nodes[slots].max()) if batch_size else 0)
        return idx, w, state, nxt, self.action[idx], self.reward[idx], self.done[idx]

    # ---- sampling with sizes that never leave the device ---------------------------------------------------
    def mover_side(self):
        """``(states' side, next states' side)`` of everything stored so far (True = maker to move): a buffer holds one
        side's transitions (multi_env_manager.py:139), recorded on the host as they are stored.  ``ValueError`` for a buffer
        that has stored both sides, or none yet."""
        if not self._sides[0] or not self._sides[1]:
            raise ValueError("empty buffer")
        if len(self._sides[0]) != 1 or len(self._sides[1]) != 1:
            raise ValueError("this buffer has stored transitions of both sides: a draw sized on the device takes the side to "
                             "move from the host's record and needs one side per buffer (keep a maker and a breaker buffer)")
        return bool(next(iter(self._sides[0]))), bool(next(iter(self._sides[1])))

    def edge_capacity(self) -> int:
        """Edge columns per graph that new draw buffers get: half as many again as the largest graph stored so far has (at
        least the start position's).  A maker move joins the removed node's neighbours, so a mid-game graph can have MORE
        edges than the start position; the host knows every stored graph's size, checks it against the buffers before every
        draw, and ``GraphedUpdate`` makes larger ones when a stored graph outgrows them."""
        self._settle()
        return -(-3 * max(self._e_start, self._max_edges) // 2)

    def draw_buffers(self, batch_size: int) -> "DrawBuffers":
        """Static output storage for ``sample_device(batch_size, out=...)``: repeated draws then reuse the same memory (what a
        captured graph needs)."""
        if self.nv > 128:
            raise NotImplementedError("sample_device: boards above 128 nodes (Hex-12 and larger) run on the layer-major kernels, "
                                      "which walk every row of their buffers; use sample()")
        bufs = DrawBuffers(int(batch_size), self.nv, self.edge_capacity(), self.device)
        self._draw_ecaps.add(bufs)                 # (a device store keeps every graph within the smallest of these)
        return bufs

    def set_draw_params(self, beta: Optional[float] = None) -> None:
        """Refresh the two device words the next ``sample_device`` draws with -- the fill level and beta -- without a host
        wait.  Two one-element fills: their values travel as kernel arguments, so a host that runs several steps ahead of the
        GPU cannot overwrite a staging buffer the copy has not read yet.  ``sample_device`` calls this itself unless the
        stream is being captured (a captured draw must not bake the values in: ``GraphedUpdate.step`` calls it before every
        replay)."""
        if self._ring_words is not None:           # device stores: the fill level the store kernels left, not the host's (it lags)
            self._draw_size.copy_(self._ring_words[1:2])
        else:
            self._draw_size.fill_(int(self.size))
        self._draw_beta.fill_(float(beta if beta is not None else 0.4))

    def draw_offsets(self, slots32: torch.Tensor, shift: int, node_off: torch.Tensor, edge_off: torch.Tensor,
                     ptr: Optional[torch.Tensor] = None) -> None:
        """Exclusive prefix sums of the stored graph sizes of ``slots32 + shift`` (int32 device slots; shift 0 = states,
        ``capacity`` = next states) into ``node_off`` / ``edge_off`` (int32 [k + 1]) and ``ptr`` (int64 [k + 1]), on the
        device (``hexgnn_replay_offsets``)."""
        k = int(slots32.numel())
        if slots32.dtype != torch.int32 or not slots32.is_cuda or not slots32.is_contiguous():
            raise ValueError("slots32: a contiguous int32 device tensor")
        for t, dt in ((node_off, torch.int32), (edge_off, torch.int32), (ptr, torch.int64)):
            if t is not None and (t.dtype != dt or t.numel() != k + 1 or not t.is_cuda or not t.is_contiguous()):
                raise ValueError("node_off / edge_off: int32 [k + 1], ptr: int64 [k + 1], contiguous, on the device")
        _lib.check(_lib.lib().hexgnn_replay_offsets(k, slots32.data_ptr(), int(shift), 2 * self.capacity,
                                                    self.sizes_dev.data_ptr(), node_off.data_ptr(), edge_off.data_ptr(),
                                                    ptr.data_ptr() if ptr is not None else None, ops._stream()),
                   "hexgnn_replay_offsets")

    def sample_device(self, batch_size: int, beta: Optional[float] = None, generator: Optional[torch.Generator] = None,
                      out: Optional["DrawBuffers"] = None):
        """``sample`` without the host in the loop: the same ``(indices, weights, state, next_state, action, reward, done)``
        with equal draws (same generator state -> same slots and weights), but the drawn slots are never read back.  The graph
        sizes are gathered and prefix-summed on the device (``hexgnn_replay_offsets`` over the device mirror of the sizes), so
        both ``Batch`` objects are CAPACITY-sized: ``batch_size * nv`` rows and ``batch_size * edge_capacity()`` edge columns,
        of which the first ``ptr[-1]`` rows / ``edge_off[-1]`` columns are written and everything behind them is left as it
        was.  ``x._hex_live_rows`` carries the live row count as a 1-element int32 device tensor; the per-graph kernels work
        from ``ptr``, and ``ops.td_step`` hands the count to the one kernel that walks rows.  The other hints are as
        ``sample``'s (``_hex_is_maker`` from the sides recorded when the transitions were stored, ``_hex_max_nodes`` = nv,
        ``_hex_csr`` on ``edge_index``).  ``out``: static storage from ``draw_buffers`` (reused by every call; else fresh
        buffers per call).  Nothing here waits for the GPU, and the whole call can be captured in a HIP graph.

        Boards above 128 nodes raise ``NotImplementedError`` (their kernels walk all rows), and so does a buffer without
        prioritisation; a buffer that stored both sides raises ``ValueError``."""
        k = int(batch_size)
        if self.nv > 128:
            raise NotImplementedError("sample_device: boards above 128 nodes (Hex-12 and larger) run on the layer-major kernels, "
                                      "which walk every row of their buffers; use sample()")
        if not self.prioritized:
            raise NotImplementedError("sample_device draws from the priority trees (prioritized=True); use sample()")
        if self.size == 0:
            raise ValueError("empty buffer")
        if k < 1:
            raise ValueError("batch_size must be positive")
        sides = self.mover_side()
        bufs = out if out is not None else self.draw_buffers(k)
        if bufs.k != k or bufs.nv != self.nv or bufs.device != self.device:
            raise ValueError("out: draw buffers of another batch size, board or device")
        if bufs.e_cap < self._max_edges or self._max_nodes > self.nv:
            raise RuntimeError("a stored graph is larger than these draw buffers were sized for (%d edges, buffers hold %d per "
                               "graph): make new ones with draw_buffers()" % (self._max_edges, bufs.e_cap))
        L, C = _lib.lib(), self.capacity
        if not torch.cuda.is_current_stream_capturing():
            self.set_draw_params(beta)
        torch.rand(k, dtype=torch.float64, device=self.device, generator=generator, out=bufs.u)
        _lib.check(L.hexgnn_per_sample_dev(self.cap2, self._draw_size.data_ptr(), k, self._draw_beta.data_ptr(),
                                           bufs.u.data_ptr(), self.sum_tree.data_ptr(), self.min_tree.data_ptr(),
                                           bufs.idx32.data_ptr(), bufs.w.data_ptr(), ops._stream()), "hexgnn_per_sample_dev")
        torch.add(bufs.idx32, C, out=bufs.idx32_next)
        bufs.idx.copy_(bufs.idx32)
        batches = []
        for half, slots in ((bufs.state, bufs.idx32), (bufs.next, bufs.idx32_next)):
            self.draw_offsets(bufs.idx32, C if half is bufs.next else 0, half.node_off, half.edge_off, half.ptr)
            half.observe_states(self.hex_size, self.adj, self.alive, self.side, slots)
            b = Batch()
            # (the hints belong to this draw)
            b.x, b.edge_index = half.inputs(sides[1] if half is bufs.next else sides[0], self.nv, live_rows=True)
            b.batch, b.ptr = half.batch_vec, half.ptr
            b._num_graphs = k
            batches.append(b)
        torch.index_select(self.action, 0, bufs.idx, out=bufs.action)
        torch.index_select(self.reward, 0, bufs.idx, out=bufs.reward)
        torch.index_select(self.done, 0, bufs.idx, out=bufs.done)
        return bufs.idx, bufs.w, batches[0], batches[1], bufs.action, bufs.reward, bufs.done

    def update_priorities(self, indices: torch.Tensor, td_errors: torch.Tensor) -> None:
        """priority_i = |td_i| + eps (the running maximum is raised to the largest), leaf = priority^alpha: one launch."""
        if not self.prioritized:
            return
        idx = indices.to(device=self.device)
        if idx.dtype not in (torch.int32, torch.int64):
            idx = idx.long()
        idx = idx.contiguous().flatten()
        td = td_errors.detach().to(device=self.device, dtype=torch.float32).contiguous().flatten()
        if td.numel() != idx.numel():
            raise ValueError("indices and td_errors differ in length")
        self._tree_update_td(idx, td)

    def _tree_update_td(self, idx: torch.Tensor, td: Optional[torch.Tensor]):
        _lib.check(_lib.lib().hexgnn_per_update_td(self.cap2, int(idx.numel()), idx.data_ptr(),
                                                   64 if idx.dtype == torch.int64 else 32,
                                                   td.data_ptr() if td is not None else None, self.alpha, self.eps,
                                                   self.max_priority.data_ptr(), self.sum_tree.data_ptr(),
                                                   self.min_tree.data_ptr(), ops._stream()), "hexgnn_per_update_td")


class DrawBuffers:
    """Everything ``GraphReplayBuffer.sample_device`` writes, for one batch size (``GraphReplayBuffer.draw_buffers``)."""

    def __init__(self, k: int, nv: int, e_cap: int, dev):
        self.k, self.nv, self.e_cap, self.device = k, nv, e_cap, torch.device(dev)
        self.u = torch.empty(k, dtype=torch.float64, device=dev)
        self.idx32 = torch.empty(k, dtype=torch.int32, device=dev)
        self.idx32_next = torch.empty(k, dtype=torch.int32, device=dev)
        self.idx = torch.empty(k, dtype=torch.long, device=dev)
        self.w = torch.empty(k, dtype=torch.float32, device=dev)
        self.action = torch.empty(k, dtype=torch.long, device=dev)
        self.reward = torch.empty(k, dtype=torch.float32, device=dev)
        self.done = torch.empty(k, dtype=torch.bool, device=dev)
        # capacity-sized storage of the two batches, left as allocated: a draw writes the live rows and nothing behind them
        self.state = ObsTarget.capacity(k, nv, e_cap, dev, zeroed=False, with_ptr=True)
        self.next = ObsTarget.capacity(k, nv, e_cap, dev, zeroed=False, with_ptr=True)


class GraphedUpdate:
    """One DQN update of one replay buffer as a single object, with no host wait anywhere in it:

        draw (``sample_device``) -> ``ops.double_dqn_targets`` -> ``ops.td_step(sel = ptr[:-1] + action)`` ->
        ``optimizer.step()`` -> ``update_priorities``

    ``step(beta)`` refreshes the device-side fill level and beta of the draw and, with ``graph=True``, replays the sequence
    as ONE HIP graph (``graphs.GraphedStep``: one stream, a linear graph); with ``graph=False`` it issues the same sequence
    eagerly.  It returns the static ``(loss, td)`` tensors, overwritten by the next step.

    The optimizer goes INSIDE the capture when it is capturable (``optimizer.param_groups[0]["capturable"]``, e.g.
    ``torch.optim.Adam(..., fused=True, capturable=True)``); any other optimizer is issued eagerly right after the replay --
    still no host wait, the graph then ends with the priority update.  Everything the graph reads is read at replay time from
    storage that stays where it is: the weight packs are made from the parameters' own storage by every forward, so an
    in-place optimizer step, ``target.load_state_dict(online.state_dict())`` and ``put`` / ``put_block`` between steps are all
    seen by the next replay, and so are stores issued on the device (``multi_env_manager.DeviceTransitionFeed``: the draw then
    takes its fill level from the ring's device word, not from the host's ``size``, which lags until the store is settled).
    What moves storage -- ``grow_*``, ``.to()``, ``load_state_dict(assign=True)`` -- needs a new ``GraphedUpdate``, as it needs a
    new ``DeviceRollout``.

    The static buffers hold ``edge_capacity()`` edge columns per graph; when a stored graph outgrows them (the host knows
    every stored size) the next ``step`` makes larger buffers and captures again -- rare, the sizes are bounded by the board.

    Capturing runs the sequence once as a warm-up (the optimizer's state must exist before the capture); the parameters, the
    optimizer's state, the priority trees and the device's random generator are put back afterwards, in place, so
    construction changes nothing a run could see.  Draws use the device's default generator (``torch.manual_seed``).

    Scope: batches that take the fused per-graph kernels -- boards up to 128 nodes, hidden <= 112, exact fp32, no norm layers,
    no noisy head, the ``mlp`` value head.  Everything else raises ``NotImplementedError`` here; a buffer that stored both sides
    raises ``ValueError``."""

    def __init__(self, buffer: GraphReplayBuffer, online, target, optimizer, batch_size: int, gamma_n: float,
                 loss_fn: str = "mse", graph: bool = True):
        if ops.get_math() != "fp32":
            raise NotImplementedError("GraphedUpdate: set_math(\"f16x3\") is not supported (its weight-gradient GEMM walks rows by "
                                      "the host's count); use exact fp32")
        if loss_fn not in ("mse", "huber"):
            raise ValueError("loss_fn: \"mse\" or \"huber\"")
        self.buffer, self.online, self.target, self.optimizer = buffer, online, target, optimizer
        self.batch_size, self.gamma_n, self.loss_fn = int(batch_size), float(gamma_n), loss_fn
        buffer.draw_buffers(1)                                  # (NotImplementedError above 128 nodes)
        buffer.mover_side()                                     # (ValueError: empty, or both sides stored)
        for name, m in (("online", online), ("target", target)):
            entry = getattr(m, "_fused_entry", None)
            heads = [m._modules.get("maker_head"), m._modules.get("breaker_head")] if entry is not None else [None]
            for head in heads:
                ent = entry(head) if head is not None else None
                ok = ent is not None and ent[3][4] and not ent[3][5] and ent[2] is not None and \
                    ops.qnet_fused_supported(ent[3][0], ent[3][1], buffer.nv)
                if not ok:
                    raise NotImplementedError("GraphedUpdate: the %s model does not take the fused per-graph kernels (norm "
                                              "layers, a noisy head, hidden > 112, the two_headed family's linear value head, "
                                              "or set_fused(False)); every other path reads all rows of its buffers" % name)
        self.params = [p for p in online.parameters()]
        self._opt_inside = bool(graph) and all(g.get("capturable", False) for g in optimizer.param_groups)
        self._use_graph, self._graph = bool(graph), None
        self._loss = torch.zeros((), dtype=torch.float32, device=buffer.device)
        self._td = torch.zeros(self.batch_size, dtype=torch.float32, device=buffer.device)
        self._build()

    def _build(self):
        """Draw buffers for the largest graph stored so far (with headroom) and, with ``graph=True``, the capture over them.
        Runs again when a stored graph outgrows the buffers (``step``)."""
        self._graph = None                                      # (a previous capture's pool goes first)
        self.bufs = self.buffer.draw_buffers(self.batch_size)
        if self._use_graph:
            from .graphs import GraphedStep
            saved = self._save_state()
            self.buffer.set_draw_params(None)
            self._graph = GraphedStep(lambda: self._body(self._opt_inside), self.params, warmup=1)
            self._restore_state(saved)

    # -- construction leaves no trace ------------------------------------------------------------------
    def _save_state(self):
        buf = self.buffer
        opt = {p: {k: (v.clone() if torch.is_tensor(v) else v) for k, v in st.items()}
               for p, st in self.optimizer.state.items()}
        return ([p.detach().clone() for p in self.params], opt, buf.sum_tree.clone(), buf.min_tree.clone(),
                buf.max_priority.clone(), torch.cuda.get_rng_state(buf.device))

    def _restore_state(self, saved):
        params, opt, sum_tree, min_tree, max_priority, rng = saved
        buf = self.buffer
        with torch.no_grad():
            for p, v in zip(self.params, params):
                p.copy_(v)
            for p, st in self.optimizer.state.items():
                old = opt.get(p)
                for k, v in st.items():
                    if torch.is_tensor(v):                 # in place: the graph holds these addresses
                        if old is not None and k in old:
                            v.copy_(old[k])
                        else:
                            v.zero_()                      # state the warm-up created: back to its initial zeros
            buf.sum_tree.copy_(sum_tree)
            buf.min_tree.copy_(min_tree)
            buf.max_priority.copy_(max_priority)
        torch.cuda.set_rng_state(rng, buf.device)

    # -- the sequence ------------------------------------------------------------------------------------
    def _body(self, with_optimizer: bool, beta: Optional[float] = None):
        buf = self.buffer
        for p in self.params:
            p.grad = None
        idx, w, st, nx, act, rew, done = buf.sample_device(self.batch_size, beta, None, out=self.bufs)
        y, _ = ops.double_dqn_targets(self.online, self.target, nx.x, nx.edge_index, nx.batch, nx.ptr, rew, done, self.gamma_n)
        sel = st.ptr[:-1] + act
        loss, td, _ = ops.td_step(self.online, st.x, st.edge_index, st.batch, st.ptr, sel=sel, target=y, weights=w,
                                  loss_fn=self.loss_fn)
        if with_optimizer:
            self.optimizer.step()
        buf.update_priorities(idx, td)
        return loss, td

    def step(self, beta: Optional[float] = None):
        """One update; ``beta``: the importance-weight exponent of this draw (0.4 when None, as ``sample``)."""
        buf = self.buffer
        if buf.size == 0:
            raise ValueError("empty buffer")
        buf.mover_side()
        if self.bufs.e_cap < buf._max_edges:       # a stored graph outgrew the static buffers (host-known): larger ones, new capture
            self._build()
        if self._graph is not None:
            buf.set_draw_params(beta)
            out = self._graph.replay()
            if not self._opt_inside:
                self.optimizer.step()
            return out
        loss, td = self._body(True, beta)
        self._loss.copy_(loss)
        self._td.copy_(td)
        return self._loss, self._td
