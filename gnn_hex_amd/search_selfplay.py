"""Search self-play and the policy/value update on the device: the AlphaZero loop of the reference's CrazyAra engine
(cpp_hex/CrazyAra/rl/selfplay.cpp, rl/traindataexporter.cpp, rl_loop/trainer_agent_pytorch.py) between ``search.TreeSearch`` and
``torch_script_models.SAGE_torch_script``.

``SearchSampleBuffer``   the sample ring on the device: per sample the board snapshot (what ``hexgnn_states_observe`` takes), the
                         visit distribution over the board cells, the root's mean value, the game result z for the side to move.
``SearchSelfPlay``       one lock-step match with the search on both sides on ``DeviceArena``'s pieces.  Per ply: observe -> a
                         fresh tree (``reuse_tree=True``: the played move's subtree) and ``sims`` simulations with Dirichlet
                         noise on the root priors -> ``hexgnn_search_record`` (one sample per undecided game into the ring,
                         one move choice per game) -> ``hexgnn_arena_ply`` with those choices as ``forced`` -> offsets.
                         ``hexgnn_samples_finish`` labels the match's samples.
``PolicyValueUpdate``    forward, ``ops.PolicyValueLossFn`` (``hexgnn_pv_loss``: the reference's ``val_factor * MSE * B +
                         pol_factor * sum(-target * log_policy)`` with both gradients in one call), backward, optimizer step.

The rules are stated in include/hexgnn.h (the section behind hexgnn_search_*) and restated on the host in
tests/selfplay_oracle.py.  Scope: ``swap_allowed=False`` networks only; a move is drawn in proportion to the visit counts or is
the most visited one (no other temperature exponent, no temperature decay); one match at a time fills the ring's tail, and
batches are drawn between matches; updates are issued eagerly.  Tree reuse between plies (``reuse_tree=True``) is off by
default.  Not part of this: a captured update, transposition merging.  There is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib, ops
from .arena import PICK_GREEDY, ArenaResult, DeviceArena
from .data import Batch
from .observation import ObsTarget
from .search import SearchPlies, TreeSearch, check_round_arguments, tensor_arg


class SearchSampleBuffer:
    """A ring of ``capacity`` training samples of Hex ``hex_size`` on the device.  ``capacity >= num_games * hex_size ** 2`` of
    the matches that fill it: a whole match fits, so a match never overwrites its own samples.  Arrays by slot: ``policy``
    float32 [capacity, hex_size ** 2], ``root_q`` / ``z`` float32, ``adj`` int64 [capacity, nv, words], ``alive`` uint8
    [capacity, nv], ``side`` uint8 (1 = maker to move), ``sizes`` int32 (nodes, directed edges), ``meta`` int32 (game, ply).
    ``head`` int64 [1] counts the samples ever recorded, on the device; the host follows it at ``finish``.  Sample number i lives
    in slot ``i mod capacity``; the drawable samples are the numbers ``[_low, _head)``: the finished ones that no later sample
    has overwritten, whether that later sample was finished or discarded."""

    def __init__(self, capacity: int, hex_size: int, device=None):
        if int(hex_size) < 2 or int(hex_size) > 25 or int(capacity) < 1:
            raise ValueError("2 <= hex_size <= 25 and capacity >= 1")
        dev = torch.device("cuda" if device is None else device)
        if dev.type != "cuda":
            raise _lib.HexGnnError("SearchSampleBuffer lives on the device (no CPU fallback)")
        self.capacity, self.hex_size = int(capacity), int(hex_size)
        cells = self.cells = self.hex_size ** 2
        nv = self.nv = cells + 2
        self.words = (nv + 63) // 64
        cap = self.capacity
        self.policy = torch.zeros((cap, cells), dtype=torch.float32, device=dev)
        self.root_q = torch.zeros(cap, dtype=torch.float32, device=dev)
        self.z = torch.zeros(cap, dtype=torch.float32, device=dev)
        self.adj = torch.zeros((cap, nv, self.words), dtype=torch.int64, device=dev)
        self.alive = torch.zeros((cap, nv), dtype=torch.uint8, device=dev)
        self.side = torch.zeros(cap, dtype=torch.uint8, device=dev)
        self.sizes = torch.zeros((cap, 2), dtype=torch.int32, device=dev)
        self.meta = torch.zeros((cap, 2), dtype=torch.int32, device=dev)
        self.head = torch.zeros(1, dtype=torch.int64, device=dev)
        self.recorded = torch.zeros(1, dtype=torch.int32, device=dev)
        self._status = torch.zeros(1, dtype=torch.int32, device=dev)
        self.device = self._status.device
        self._head = 0                       # the samples finished so far: what the host knows of ``head``
        self._low = 0                        # the oldest sample number whose slot still holds it

    def __len__(self) -> int:
        return self._head - max(self._low, self._head - self.capacity)

    def record_call(self, ply: int, pick_mode: int, u, pick) -> "_lib.RecordCall":
        """The ``hexgnn_record_call`` of this ring for one ply."""
        return _lib.RecordCall(struct_bytes=C.sizeof(_lib.RecordCall), capacity=self.capacity, ply=int(ply),
                               pick_mode=int(pick_mode), head=self.head.data_ptr(), recorded=self.recorded.data_ptr(),
                               u=u.data_ptr() if u is not None else None, pick=pick.data_ptr(), policy=self.policy.data_ptr(),
                               root_q=self.root_q.data_ptr(), z=self.z.data_ptr(), adj=self.adj.data_ptr(),
                               alive=self.alive.data_ptr(), side=self.side.data_ptr(), sizes=self.sizes.data_ptr(),
                               meta=self.meta.data_ptr())

    def record(self, root_handle, search: TreeSearch, ply: int, pick_mode: int, u, pick, active=None) -> None:
        """``hexgnn_search_record``: one sample per recorded game behind ``head``, one move choice per game into ``pick``
        (int32 [G]); ``u``: float32 [G] uniforms for ``pick_mode`` 1."""
        G = search.num_games
        tensor_arg("pick", pick, torch.int32, G)               # (no device named: the callers pass their arena's tensors)
        tensor_arg("u", u, torch.float32, G, optional=True)
        active = tensor_arg("active", active, torch.int32, G, optional=True)
        if search.hex_size != self.hex_size:
            raise ValueError("the search plays Hex-%d, the ring holds Hex-%d" % (search.hex_size, self.hex_size))
        call = search._call(active=active)
        rec = self.record_call(ply, pick_mode, u, pick)
        _lib.check(_lib.lib().hexgnn_search_record(root_handle, C.byref(call), C.byref(rec), ops._stream()),
                   "hexgnn_search_record")

    def pending(self) -> int:
        """Samples recorded since the last ``finish`` (reads ``head``: synchronises)."""
        return int(self.head.item()) - self._head

    def finish(self, game: torch.Tensor) -> int:
        """Label the samples recorded since the last ``finish`` with the results in ``game`` (``hexgnn_arena_ply``'s int32
        [G, 4] record) and make them drawable.  Returns their number.  When one of their games is undecided, or they overran
        the ring, they are discarded instead (``discard_pending``) and ``HexGnnError`` is raised."""
        if game.dtype != torch.int32 or game.dim() != 2 or game.shape[1] != 4 or not game.is_contiguous():
            raise ValueError("game: hexgnn_arena_ply's contiguous int32 [G, 4] record")
        count = self.pending()
        if count > self.capacity:
            self.discard_pending()
            raise _lib.HexGnnError("%d samples in one match overran the ring of %d" % (count, self.capacity))
        _lib.check(_lib.lib().hexgnn_samples_finish(self._head % self.capacity, count, self.capacity, int(game.shape[0]),
                                                    self.meta.data_ptr(), self.side.data_ptr(), self.z.data_ptr(),
                                                    game.data_ptr(), self._status.data_ptr(), ops._stream()),
                   "hexgnn_samples_finish")
        try:
            self.status()
        except _lib.HexGnnError:
            self.discard_pending()
            raise
        self._head += count
        return count

    def discard_pending(self) -> None:
        """Forget the samples recorded since the last ``finish``: ``head`` goes back and their slots are written again.  Where
        they had wrapped onto finished samples, those are gone (their slots hold the discarded match's boards and z = 0): the
        drawable range shrinks past them, so ``sample`` never draws such a slot.  Reads ``head``: synchronises."""
        count = self.pending()
        if count > 0:
            self._low = min(self._head, max(self._low, self._head + count - self.capacity))
            self.head.fill_(self._head)

    def status(self) -> None:
        code = int(self._status.item())
        if code:
            self._status.zero_()
            raise _lib.HexGnnError("SearchSampleBuffer (status=%d): 32 = a sample of an undecided game was labelled NaN, "
                                   "64 = a graph of a batch did not match its log-policy rows or its slot" % code)

    def _slots_of(self, i: torch.Tensor) -> torch.Tensor:
        """The slots of the drawable samples number ``i`` in ``[0, len(self))``, oldest first."""
        return (i + (self._head - len(self))) % self.capacity

    def sample(self, batch_size: int, generator=None):
        """``(batch, index)``: ``batch_size`` slots drawn uniformly with replacement from the finished samples, as a device
        ``Batch`` (``x``, ``edge_index``, ``batch``, ``ptr``; plus ``node_off`` int32, ``backmap`` and ``samples`` = this ring for
        ``PolicyValueUpdate``), and the slots as int32 [batch_size] on the device.  Built as ``GraphReplayBuffer._build_batch``
        builds it, with one small read-back of the drawn sizes."""
        n = len(self)
        if n == 0:
            raise ValueError("empty buffer")
        idx = self._slots_of(torch.randint(0, n, (int(batch_size),), device=self.device, generator=generator))
        sizes = self.sizes[idx].cpu().numpy().astype(np.int64)
        index = idx.to(torch.int32)
        t = ObsTarget.exact(sizes, self.device, with_ptr=True)
        t.observe_states(self.hex_size, self.adj, self.alive, self.side, index)
        b = Batch()
        b.x, b.edge_index, b.batch, b.ptr = t.x, t.edge_global, t.batch_vec, t.ptr
        b._num_graphs = int(batch_size)
        b.edge_index._hex_csr = t.gs
        b.node_off, b.backmap, b.samples = t.node_off, t.backmap, self
        return b, index


class SearchSelfPlay(SearchPlies):
    """Lock-step self-play of ``num_games`` games of Hex ``hex_size`` with a ``sims``-simulation search on both sides, every
    searched position recorded into ``buffer``.  ``evaluator``: as ``SearchPlayer`` takes it.  ``root_noise = (eps, alpha)``:
    Dirichlet(alpha) noise mixed into the root priors with weight eps after the simulation that expands the root (None: no
    noise).  ``proportional_plies``: the plies of a match (0 ..) whose move is drawn in proportion to the visit counts; from
    there on the most visited move is played (None: every ply is drawn).  ``leaves`` / ``virtual_loss``: as ``TreeSearch`` takes
    them (``sims`` is then what is asked for, collisions included; ``sims > leaves``).  ``reuse_tree=True`` keeps the played
    move's subtree between plies (the reference's Reuse_Tree; ``search.SearchPlies``, shared with ``SearchPlayer``): the trees
    hold ``capacity`` simulations (default ``4 * sims``), are reset once per match and re-rooted after every ply; every ply adds
    ``sims`` new simulations, and a sample's visit distribution N / T includes the carried visits, as in the reference."""

    def __init__(self, hex_size: int, num_games: int, evaluator, sims: int, buffer: SearchSampleBuffer, c_puct: float = 1.5,
                 root_noise=(0.25, 0.2), proportional_plies=None, prior_temperature: float = 1.0, device=None, leaves: int = 1,
                 virtual_loss: int = 1, reuse_tree: bool = False, capacity=None):
        if not hasattr(evaluator, "evaluate"):
            raise TypeError("SearchSelfPlay takes an evaluator (PolicyValueEvaluator, QEvaluator, UniformEvaluator)")
        if int(sims) < 2:
            raise ValueError("sims >= 2: the first simulation only expands the root, and a root without a visit is no sample")
        check_round_arguments(sims, leaves, virtual_loss)
        if buffer.hex_size != int(hex_size) or buffer.capacity < int(num_games) * int(hex_size) ** 2:
            raise ValueError("the buffer holds Hex-%d and needs capacity >= num_games * hex_size ** 2" % buffer.hex_size)
        if root_noise is not None and (not 0.0 <= float(root_noise[0]) <= 1.0 or not float(root_noise[1]) > 0):
            raise ValueError("root_noise = (eps in [0, 1], alpha > 0) or None")
        SearchPlies.__init__(self, sims, reuse_tree, capacity)
        self.hex_size, self.num_games = int(hex_size), int(num_games)
        self.evaluator, self.buffer, self.root_noise = evaluator, buffer, root_noise
        self.proportional_plies = proportional_plies
        self.arena = DeviceArena(hex_size, num_games, device=device if device is not None else buffer.device, graph=False)
        dev = self.device = self.arena.device
        self.search = TreeSearch(hex_size, num_games, self.capacity, c_puct, prior_temperature, device=dev, leaves=leaves,
                                 virtual_loss=virtual_loss)
        self._zeros = torch.zeros(num_games * self.arena.mgr._nv, dtype=torch.float32, device=dev)
        self._u = torch.zeros(num_games, dtype=torch.float32, device=dev)

    def play(self, first: str = "m", generator=None):
        """One match from the start position, ``first`` ("m" / "b") to move.  Returns ``(ArenaResult, samples)``; the samples
        are labelled and drawable.  On an arena error the match's samples are discarded and ``ValueError`` is raised as
        ``DeviceArena.play`` raises it."""
        if first not in ("m", "b"):
            raise ValueError("first must be \"m\" or \"b\"")
        L, ar, s, buf = _lib.lib(), self.arena, self.search, self.buffer
        h, k, obs = ar.mgr._h, self.num_games, ar.obs
        maker = first == "m"
        ar._prepare(maker, None)
        buf.discard_pending()
        plies, live = 0, k
        self._match_begins(s)                                 # tree reuse: once per match; from here the subtrees are kept
        try:
            while live > 0:
                if plies >= ar.max_plies:
                    raise RuntimeError("%d games still undecided after %d plies of Hex-%d" % (live, plies, self.hex_size))
                obs.observe_env(h)
                active = ((ar.game[:, 0] < 0) & (ar.game[:, 3] == 0)).to(torch.int32)
                self._search_ply(s, h, self.evaluator, active, root_noise=self.root_noise, generator=generator)
                proportional = self.proportional_plies is None or plies < int(self.proportional_plies)
                if proportional:
                    torch.rand(k, generator=generator, out=self._u)
                buf.record(h, s, plies, 1 if proportional else 0, self._u if proportional else None, ar.forced, active)
                # every undecided game carries its move in `forced`: the pick mode is never used, a game that ends restarts on
                # the side everyone moves to next
                _lib.check(L.hexgnn_arena_ply(h, obs.node_off.data_ptr(), self._zeros.data_ptr(), obs.backmap.data_ptr(),
                                              PICK_GREEDY, 1.0, None, ar.forced.data_ptr(), int(not maker), ar.game.data_ptr(),
                                              ar.log[plies].data_ptr(), ar.result.data_ptr(), ar.live.data_ptr(),
                                              ops._stream()), "hexgnn_arena_ply")
                _lib.check(L.hexgnn_env_offsets(k, ar.result.data_ptr(), obs.node_off.data_ptr(), obs.edge_off.data_ptr(),
                                                ops._stream()), "hexgnn_env_offsets")
                self._ply_played(s, ar.log[plies])
                maker = not maker
                plies += 1
                live = int(ar.live.item())
            s.status()
        except Exception:
            buf.discard_pending()
            raise
        game = ar.game.cpu().numpy()
        moves = ar.log[:plies].cpu().numpy().T.copy()
        if game[:, 3].any():
            buf.discard_pending()
            g = int(np.nonzero(game[:, 3])[0][0])
            ply = int(game[g, 2])
            what = "illegal move %d" % int(moves[g, ply]) if game[g, 3] == 1 else "non-finite action values"
            raise ValueError("%s in game %d at ply %d" % (what, g, ply))
        pending, played = buf.pending(), int(game[:, 1].sum())
        if pending != played:                                 # before they become drawable
            buf.discard_pending()
            raise _lib.HexGnnError("%d samples for %d moves: a searched position went unrecorded" % (pending, played))
        samples = buf.finish(ar.game)
        used = int((moves >= 0).any(0).sum())
        res = ArenaResult(game[:, 0].astype(np.int8), game[:, 1].astype(np.int64), moves[:, :used].astype(np.int64), used)
        return res, samples


class PolicyValueUpdate:
    """The reference's policy/value update (rl_loop/trainer_agent_pytorch.py:245-275) of a ``SAGE_torch_script`` without the
    swap output on batches of ``SearchSampleBuffer.sample``: value target ``(1 - q_ratio) z + q_ratio root_q``
    (rl_loop/dataset_loader.py:74), loss ``val_factor * sum (value - target) ** 2 + pol_factor * sum(-policy_target *
    log_policy)`` over the batch.  Issued eagerly."""

    def __init__(self, model, optimizer, q_ratio: float = 0.0, val_factor: float = 1.0, pol_factor: float = 1.0):
        from .torch_script_models import SAGE_torch_script
        if not isinstance(model, SAGE_torch_script) or model.swap_allowed:
            raise NotImplementedError("PolicyValueUpdate takes a SAGE_torch_script with swap_allowed=False")
        if not 0.0 <= float(q_ratio) <= 1.0:
            raise ValueError("q_ratio in [0, 1]")
        self.model, self.optimizer = model, optimizer
        self.q_ratio, self.val_factor, self.pol_factor = float(q_ratio), float(val_factor), float(pol_factor)

    def loss(self, batch, index):
        """Forward and loss: ``(loss, per_graph [b, 4])`` with the autograd graph attached."""
        buf = batch.samples
        pi, value, _, out_ptr = self.model(batch.x, batch.edge_index, batch.batch, batch.ptr)
        return ops.PolicyValueLossFn.apply(pi, value, out_ptr, batch.node_off, batch.backmap, buf.policy, buf.z, buf.root_q,
                                           index, buf.hex_size, self.q_ratio, self.val_factor, self.pol_factor, buf._status)

    def step(self, batch, index):
        """One update.  Returns ``(loss, metrics)`` as device tensors: the loss and the batch means of the reference's four
        metrics (policy loss, value loss, policy accuracy, value sign accuracy; train_util.py:25-26)."""
        self.optimizer.zero_grad(set_to_none=True)
        loss, per_graph = self.loss(batch, index)
        loss.backward()
        self.optimizer.step()
        return loss.detach(), per_graph.mean(0)
