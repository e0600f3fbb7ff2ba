"""Batched PUCT tree search on the device: ``run_many_mcts`` of GN0/alpha_zero/MCTS.py as a closed device loop.

G trees for G games, one leaf per game per simulation, the leaves of all games through ONE evaluator call.  Per simulation:
``hexgnn_search_descend`` (select down the tree with the env kernels' move routine, store the leaf position into the search's own
leaf env) -> the leaf observation (``hexgnn_env_offsets`` / ``hexgnn_env_observe``, unchanged) -> the evaluator ->
``hexgnn_search_backup`` (expand the leaf with softmax(logit / T) priors, back its value up).  ``hexgnn_search_root`` reads the
root visit counts out in the layout of the root observation, so ``hexgnn_arena_ply`` picks from them like from any model's output.
The rule is restated in include/hexgnn.h and on the host in tests/search_oracle.py.  A tree, not the reference's hash-keyed DAG:
transpositions are not merged; no swap rule.  Tree reuse between plies is ``TreeSearch.advance`` (``hexgnn_search_advance``: the
played move's subtree becomes the tree) and ``SearchPlayer(reuse_tree=True)``; off by default.  ``TreeSearch(leaves=K)`` makes a
ROUND of K descents per game under a virtual loss (``hexgnn_search_round_descend`` / ``_backup``; the rule: include/hexgnn.h,
tests/search_round_oracle.py): K times fewer rounds, K times larger evaluator batches; ``leaves=1`` is a round of one descent
and issues the one-leaf calls.  Dirichlet noise on the root priors is ``TreeSearch.add_root_noise`` /
``simulate(root_noise=...)`` (``hexgnn_search_root_noise``); the self-play loop that uses it, the sample ring and the
policy/value update are gnn_hex_amd/search_selfplay.py.

``TreeSearch``             the trees, the leaf env and the simulation loop.
``SearchPlies``            what a searching player does per match and per ply (reset, simulate, tree reuse): the one copy behind
                           ``SearchPlayer`` and ``search_selfplay.SearchSelfPlay``.
``PolicyValueEvaluator``   leaves through a ``SAGE_torch_script`` policy / value network (the HexAra network).
``QEvaluator``             leaves through a ``get_pre_defined`` Q-network or a ``MonteCarloPlayer``: scores as logits, the maximum
                           score as value; one forward per side, so two per simulation.
``UniformEvaluator``       uniform priors, value 0: plain UCT on terminal results alone, no network.
``SearchPlayer``           a player for ``DeviceArena.play`` / ``Elo_handler.add_player(model=...)``.

There is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch

from . import _lib, ops
from .multi_env_manager import Env_manager
from .observation import ObsTarget, live_norm_of


def tree_layout(num_games: int, hex_size: int, max_sims: int, leaves=None):
    """The workspace of include/hexgnn.h as ``({name: (byte offset, dtype, shape)}, tree bytes, total bytes)``: the sections in
    the header's order, each aligned to 256 bytes; ``score`` and ``moves`` are scratch behind the tree.  ``leaves=K``: the
    workspace of a round of K leaves per game (``hexgnn_search_round_workspace_bytes``), which keeps every offset and adds
    ``inflight`` and ``round_moves`` at the end."""
    G, Cn, A = int(num_games), int(max_sims) + 1, int(hex_size) ** 2
    out, off, tree = {}, 0, 0
    extra = () if leaves is None else (("inflight", np.int32, (G, Cn, A)), ("round_moves", np.uint16, (G, int(leaves), A)))
    for name, dt, shape in (("ns", np.int32, (G, Cn)), ("ne", np.int32, (G, Cn)), ("cnt", np.int32, (G, 2)),
                            ("P", np.float32, (G, Cn, A)), ("W", np.float32, (G, Cn, A)), ("N", np.int32, (G, Cn, A)),
                            ("child", np.int32, (G, Cn, A)), ("vertex", np.uint16, (G, Cn, A)),
                            ("score", np.float32, (G, A)), ("moves", np.uint16, (G, A))) + extra:
        if name == "score":
            tree = off
        out[name] = (off, dt, shape)
        off += -(-int(np.prod(shape)) * np.dtype(dt).itemsize // 256) * 256
    return out, tree, off


def tensor_arg(name: str, t, dtype, shape=None, device=None, optional: bool = False, message=None):
    """The one check of a tensor argument of a kernel call, and its address: a contiguous ``dtype`` tensor of ``shape`` (an int:
    that many elements, a tuple: exactly that shape, None: any) on ``device`` (None: anywhere), else ``ValueError`` (with
    ``message`` in place of the description made from the arguments).  ``optional``: None is allowed and returned."""
    if t is None and optional:
        return None
    dims = () if shape is None else shape if isinstance(shape, tuple) else (shape,)
    if not (torch.is_tensor(t) and t.dtype == dtype and t.is_contiguous() and (device is None or t.device == device)
            and (shape is None or (tuple(t.shape) == shape if isinstance(shape, tuple) else t.numel() == shape))):
        raise ValueError(message or "%s: a contiguous %s%s tensor%s" % (
            name, str(dtype)[6:], " [%s]" % ", ".join(map(str, dims)) if dims else "", "" if device is None else " on %s" % (device,)))
    return t.data_ptr()


class TreeSearch:
    """``num_games`` search trees of at most ``max_sims`` simulations each over Hex ``hex_size`` positions.  Owns the leaf env,
    the tree workspace, the path / leaf record / status tensors and a capacity-sized leaf observation.  ``c_puct`` and
    ``temperature`` (of the prior's softmax) are the rule's two constants.  ``leaves=K > 1``: every round makes K descents per
    game under the integer ``virtual_loss`` and evaluates ``num_leaves = num_games * K`` leaves at once; ``path`` is then
    [G, K, max_sims + 1], ``leaf`` [G, K, 5], ``result`` [G * K, 5] and leaf (g, k) is game ``g * K + k`` of the leaf env.
    ``leaves=1`` (the default) issues the one-leaf calls with the one-leaf shapes, whatever ``virtual_loss`` says."""

    def __init__(self, hex_size: int, num_games: int, max_sims: int, c_puct: float = 1.5, temperature: float = 1.0, device=None,
                 leaves: int = 1, virtual_loss: int = 1):
        if num_games < 1 or not 1 <= int(max_sims) <= _lib.SEARCH_MAX_SIMS:
            raise ValueError("num_games >= 1 and 1 <= max_sims <= %d" % _lib.SEARCH_MAX_SIMS)
        if not (c_puct >= 0 and math.isfinite(c_puct)) or not (temperature > 0 and math.isfinite(temperature)):
            raise ValueError("c_puct is finite and >= 0, temperature finite and > 0")
        self.hex_size, self.num_games, self.max_sims = int(hex_size), int(num_games), int(max_sims)
        check_round_arguments(None, leaves, virtual_loss)
        self.c_puct, self.temperature = float(c_puct), float(temperature)
        K = self.leaves = int(leaves)
        self.virtual_loss = int(virtual_loss)
        self.num_leaves = int(num_games) * K                   # the games of the leaf env = the graphs of one evaluator call
        self._leaf_mgr = mgr = Env_manager(self.num_leaves, hex_size, device=device)     # the leaf env the search owns
        mgr.record_snapshots = False
        dev = self.device = mgr.device
        self.leaf_handle, self.nv = mgr._h, mgr._nv
        L = _lib.lib()
        if K == 1:
            self.workspace_bytes = int(L.hexgnn_search_workspace_bytes(num_games, hex_size, max_sims))
        else:
            self.workspace_bytes = int(L.hexgnn_search_round_workspace_bytes(num_games, hex_size, max_sims, K))
        if self.workspace_bytes == 0:
            raise _lib.HexGnnError("hexgnn_search_workspace_bytes refuses Hex-%d" % hex_size)
        self.workspace = torch.zeros(self.workspace_bytes, dtype=torch.uint8, device=dev)
        G = num_games
        per_game = (G,) if K == 1 else (G, K)
        self.path = torch.zeros(per_game + (max_sims + 1,), dtype=torch.int32, device=dev)
        self.leaf = torch.zeros(per_game + (_lib.SEARCH_REC,), dtype=torch.int32, device=dev)
        self.result = torch.zeros((G * K, 5), dtype=torch.int32, device=dev)
        self._status = torch.zeros(1, dtype=torch.int32, device=dev)
        dev = self.device = self._status.device               # with its index, as every tensor handed in carries it
        # The maker's rewiring can leave a position with MORE edges than the start position (Hex-7: 125 against 122 after one
        # move), and a search puts every game one maker move deep at once: the leaf observation holds twice the start
        # position's edges per game, and leaf_offsets() guards the total.
        self.e_max = 2 * int(mgr._base_sizes[0, 1])
        self.obs = ObsTarget.capacity(G * K, self.nv, self.e_max, dev, zeroed=True, tail_clear=True)
        self._remap = self._carried = None                     # advance()'s scratch and output, allocated on first use
        self.reset()

    # -- the kernel calls ------------------------------------------------------------------------------------
    def _call(self, **kw):
        return _lib.SearchCall(struct_bytes=C.sizeof(_lib.SearchCall), num_games=self.num_games, hex_size=self.hex_size,
                               max_sims=self.max_sims, c_puct=self.c_puct, temperature=self.temperature,
                               workspace=self.workspace.data_ptr(), workspace_bytes=self.workspace_bytes,
                               status=self._status.data_ptr(), path=self.path.data_ptr(), leaf=self.leaf.data_ptr(),
                               result=self.result.data_ptr(), **kw)

    def _round_call(self, round_leaves=None, **kw):
        return _lib.SearchRoundCall(struct_bytes=C.sizeof(_lib.SearchRoundCall), call=self._call(**kw), leaves=self.leaves,
                                    round_leaves=self.leaves if round_leaves is None else int(round_leaves),
                                    virtual_loss=self.virtual_loss)

    def _issue(self, what: str, *handles, round_leaves=None, **kw) -> None:
        """``hexgnn_search_<what>(*handles, _call(**kw))`` or, with ``leaves > 1``, ``hexgnn_search_round_<what>`` with
        ``_round_call(round_leaves, **kw)``: the one place that tells the two forms of descend and backup apart."""
        if self.leaves > 1:
            name, call = "hexgnn_search_round_" + what, self._round_call(round_leaves, **kw)
        else:
            name, call = "hexgnn_search_" + what, self._call(**kw)
        _lib.check(getattr(_lib.lib(), name)(*handles, C.byref(call), ops._stream()), name)

    def _section(self, name: str) -> torch.Tensor:
        """A device view of the section ``name`` of the workspace (``tree_layout``: ``ns``, ``cnt``, ...); nothing is copied."""
        off, dt, shape = self._layout()[name]
        view = self.workspace[off:off + int(np.prod(shape)) * np.dtype(dt).itemsize]
        return view.view(getattr(torch, np.dtype(dt).name)).view(shape)

    def _layout(self):
        return tree_layout(self.num_games, self.hex_size, self.max_sims, self.leaves if self.leaves > 1 else None)[0]

    def reset(self) -> None:
        """Every tree becomes one unexpanded root."""
        self._advanced = False                                 # no tree holds a carried subtree
        _lib.check(_lib.lib().hexgnn_search_reset(C.byref(self._call()), ops._stream()), "hexgnn_search_reset")

    def advance(self, moves, max_carry=None) -> torch.Tensor:
        """Tree reuse between plies (``hexgnn_search_advance``): every game's tree is re-rooted at the child of the root edge
        that carries ``moves[g]`` -- int32 [G] on the device, vertex ids (board cell + 2), negative: no move -- and the rest of
        the tree is dropped; the kept nodes are compacted onto slots 0, 1, .. in their old order.  A game without such a
        subtree, or whose subtree holds more than ``max_carry`` applied simulations (default ``max_sims``), gets a fresh tree as
        by ``reset()``.  With ``max_carry = max_sims - s`` the next ``s`` simulations fit.  Call it between searches only.
        Returns ``carried`` int32 [G] on the device (overwritten by the next call): the visit count Ns of each new root, 0 for
        a fresh tree.  Nothing is read back."""
        G = self.num_games
        moves = tensor_arg("moves", moves, torch.int32, G, self.device)
        max_carry = self.max_sims if max_carry is None else max_carry
        if int(max_carry) != max_carry or not 0 <= int(max_carry) <= self.max_sims:
            raise ValueError("max_carry is an integer in 0 .. max_sims = %d" % self.max_sims)
        if self._remap is None:
            self._remap = torch.empty((G, self.max_sims + 1), dtype=torch.int32, device=self.device)
            self._carried = torch.zeros(G, dtype=torch.int32, device=self.device)
        call = _lib.SearchAdvanceCall(struct_bytes=C.sizeof(_lib.SearchAdvanceCall), call=self._call(), moves=moves,
                                      max_carry=int(max_carry), remap=self._remap.data_ptr(), carried=self._carried.data_ptr())
        _lib.check(_lib.lib().hexgnn_search_advance(C.byref(call), ops._stream()), "hexgnn_search_advance")
        self._advanced = True
        return self._carried

    def root_expanded(self) -> torch.Tensor:
        """bool [G] on the device: the games whose root is expanded (``ns[:, 0] > 0``); nothing is read back."""
        return self._section("ns")[:, 0] > 0

    def descend(self, root_handle, active=None, round_leaves=None) -> None:
        """One descent per game (``leaves`` > 1: one round of ``round_leaves`` <= ``leaves`` descents per game, None: all of
        them) from the positions of ``root_handle`` (read only); ``active``: int32 [G] on the device, 0 = the game rests.
        Fills ``path``, ``leaf``, ``result`` and the leaf env."""
        active = tensor_arg("active", active, torch.int32, self.num_games, self.device, optional=True)
        if self.leaves == 1 and round_leaves not in (None, 1):
            raise ValueError("round_leaves belongs to a search with leaves > 1")
        self._issue("descend", root_handle, self.leaf_handle, round_leaves=round_leaves, active=active)

    def backup(self, logits, offsets, skip: int, value=None) -> None:
        """Expand and back up: ``logits`` float32 placed by the int32 ``offsets [num_leaves + 1]`` and ``skip`` (0 / 2),
        ``value`` float32 [num_leaves] or None (the maximum logit clamped to [-1, 1])."""
        both = "logits: contiguous float32; offsets: contiguous int32 [%d]" % (self.num_leaves + 1)
        logits = tensor_arg("logits", logits, torch.float32, message=both)
        offsets = tensor_arg("offsets", offsets, torch.int32, self.num_leaves + 1, message=both)
        value = tensor_arg("value", value, torch.float32, self.num_leaves, optional=True)
        self._issue("backup", skip=int(skip), logits=logits, offsets=offsets, value=value)

    def root(self, obs, boards: bool = False, fill: float = 0.0):
        """The read-out in the layout of the root observation ``obs`` (an ``ObsTarget`` or ``ObsList`` of the root env):
        ``scores`` float32 [N], the visit count of every legal move on rows 2.. of its graph and the root's mean value on the
        two terminal rows.  ``boards=True``: ``(scores, counts [G, hex_size ** 2], q [G, hex_size ** 2], best int32 [G])`` with
        ``fill`` on cells without an edge and ``best`` the most visited vertex (first maximum; -1: root not expanded)."""
        from .positions import _gptr32
        dev, G, cells = self.device, self.num_games, self.hex_size ** 2
        gptr = _gptr32(obs)
        scores = torch.zeros(int(obs.x.shape[0]), dtype=torch.float32, device=dev)
        counts = q = best = None
        if boards:
            counts = torch.empty((G, cells), dtype=torch.float32, device=dev)
            q = torch.empty((G, cells), dtype=torch.float32, device=dev)
            best = torch.empty(G, dtype=torch.int32, device=dev)
        call = self._call(fill=float(fill), gptr=gptr.data_ptr(), scores=scores.data_ptr(),
                          counts=counts.data_ptr() if boards else None, q=q.data_ptr() if boards else None,
                          best=best.data_ptr() if boards else None)
        _lib.check(_lib.lib().hexgnn_search_root(C.byref(call), ops._stream()), "hexgnn_search_root")
        return (scores, counts, q, best) if boards else scores

    # -- the loop -------------------------------------------------------------------------------------------
    def leaf_offsets(self) -> None:
        """The leaf observation's offsets from the sizes the last descent reported, on the device.  Should the leaves hold more
        edges than the observation has columns, the edge offsets become zeros -- every graph then lands inside the storage,
        the simulation evaluates garbage -- and bit 8 of the status word makes ``status()`` raise: nothing is written out of
        bounds and nothing is read back."""
        obs, k = self.obs, self.num_leaves
        _lib.check(_lib.lib().hexgnn_env_offsets(k, self.result.data_ptr(), obs.node_off.data_ptr(), obs.edge_off.data_ptr(),
                                                 ops._stream()), "hexgnn_env_offsets")
        over = obs.edge_off[k] > obs.E
        self._status.bitwise_or_(over.to(torch.int32) * 8)
        obs.edge_off.mul_((~over).to(torch.int32))

    def add_root_noise(self, eps: float, alpha: float, active=None, generator=None) -> torch.Tensor:
        """Dirichlet(alpha) noise on the priors of every expanded root (of the games with ``active[g] != 0``):
        ``P = (1 - eps) P + eps * noise / sum(noise)`` over the root's edges (``hexgnn_search_root_noise``; the reference's
        Dirichlet_Epsilon / Dirichlet_Alpha, main/options.cpp:49-53).  The Gamma(alpha) draws are ``torch._standard_gamma`` on
        the device from ``generator``; returned (float32 [G, hex_size ** 2]) so that a test can restate the rule."""
        if not 0.0 <= float(eps) <= 1.0 or not (alpha > 0 and math.isfinite(alpha)):
            raise ValueError("eps in [0, 1], alpha finite and > 0")
        G, A = self.num_games, self.hex_size ** 2
        noise = torch._standard_gamma(torch.full((G, A), float(alpha), dtype=torch.float32, device=self.device), generator=generator)
        self.apply_root_noise(eps, noise, active)
        return noise

    def apply_root_noise(self, eps: float, noise, active=None) -> None:
        """``hexgnn_search_root_noise`` with the caller's ``noise`` (contiguous float32 [G, hex_size ** 2] on the device)."""
        G, A = self.num_games, self.hex_size ** 2
        noise = tensor_arg("noise", noise, torch.float32, (G, A), self.device)
        call = self._call(active=tensor_arg("active", active, torch.int32, G, self.device, optional=True))
        _lib.check(_lib.lib().hexgnn_search_root_noise(C.byref(call), float(eps), noise, ops._stream()),
                   "hexgnn_search_root_noise")

    def simulate(self, root_handle, evaluator, sims: int, active=None, trace=None, root_noise=None, generator=None) -> None:
        """``sims`` simulations per game in ``ceil(sims / K)`` ROUNDS of ``min(K, sims left)`` descents per game, K = ``leaves``:
        descend -> ``evaluator.evaluate(self)`` -> backup; with ``leaves = 1`` a round is one simulation.  ``trace``: a list that
        receives per round a dict of host copies: ``path``, ``leaf``, ``logits``, ``offsets``, ``skip``, ``value`` (None: the
        maximum logit rule) and, with ``leaves > 1`` only, ``round_leaves``.  ``root_noise = (eps, alpha)``: ``add_root_noise``
        (draws from ``generator``) once, behind the first round of the call -- on a fresh tree the one that expands the root.
        After ``advance`` a root may be expanded already: such a game's priors are noised before the first round instead, the
        others behind it, once per game.  With ``leaves > 1`` a descent that ends on a leaf an earlier descent of its round
        already waits for is a COLLISION and applies nothing, so the simulations applied (``applied()``) are then FEWER than
        ``sims``: on a fresh tree the whole first round but its first descent."""
        noise_behind = self._root_noise_plan(root_noise, active, generator) if root_noise is not None else None
        K, left = self.leaves, int(sims)
        while left > 0:
            n = min(K, left)
            self.descend(root_handle, active, round_leaves=n)
            logits, offsets, skip, value = evaluator.evaluate(self)
            if trace is not None:
                rec = dict(path=self.path.cpu().numpy(), leaf=self.leaf.cpu().numpy(), logits=logits.cpu().numpy(),
                           offsets=offsets.cpu().numpy(), skip=skip, value=value.cpu().numpy() if value is not None else None)
                if K > 1:
                    rec["round_leaves"] = n
                trace.append(rec)
            self.backup(logits, offsets, skip, value)
            if noise_behind is not None:                       # once, behind the first round
                noise_behind()
                noise_behind = None
            left -= n

    def _root_noise_plan(self, root_noise, active, generator):
        """The root noise of one ``simulate`` call: what to run behind its first simulation (round).  Trees that ``reset()``
        made: ``add_root_noise`` there, one call under the caller's mask.  Trees that went through ``advance`` may have an
        expanded root already, whose priors are noised BEFORE the first simulation; the others follow behind it.  Both masks
        are built on the device from ``ns[:, 0]``, every game is noised once, from one draw."""
        eps, alpha = root_noise
        if not self._advanced:
            return lambda: self.add_root_noise(eps, alpha, active=active, generator=generator)
        expanded = self.root_expanded()
        on = expanded if active is None else expanded & (active != 0)
        off = ~expanded if active is None else ~expanded & (active != 0)
        behind = off.to(torch.int32)
        noise = self.add_root_noise(eps, alpha, active=on.to(torch.int32), generator=generator)
        return lambda: self.apply_root_noise(eps, noise, behind)

    def applied(self) -> torch.Tensor:
        """The simulations applied to every tree since ``reset``: int32 [G] on the device (LEAF and TERMINAL descents that
        were not dropped; with ``leaves > 1`` collisions make it smaller than what ``simulate`` was asked for)."""
        return self._section("cnt")[:, 1].clone()

    def status(self) -> None:
        """Raise if a call since the last check met a limit (reads the device word: synchronises).  The kinds of a descent in
        ``leaf[..., 0]``: 0 = LEAF, 1 = TERMINAL, 2 = SKIPPED, 3 = COLLISION (``leaves > 1`` only)."""
        code = int(self._status.item())
        if code:
            self._status.zero_()
            raise _lib.HexGnnError("TreeSearch (status=%d): 1 = a simulation beyond max_sims=%d was not run, 2 = a non-finite "
                                   "logit or value dropped a simulation, 4 = a leaf got fewer logits than it has legal moves, "
                                   "8 = the leaves held more edges than the leaf observation, 16 = root noise that is negative, not "
                                   "finite or sums to nothing was not applied" % (code, self.max_sims))

    def tree(self):
        """Host copies of the tree's arrays by name (``tree_layout``): for tests and inspection."""
        raw = self.workspace.cpu().numpy()
        return {name: raw[off:off + int(np.prod(shape)) * np.dtype(dt).itemsize].view(dt).reshape(shape).copy()
                for name, (off, dt, shape) in self._layout().items()}


class UniformEvaluator:
    """Uniform priors and value 0 at every leaf: plain UCT that learns from decided games alone.  No network, no observation."""

    def __init__(self):
        self._zeros = None

    def evaluate(self, search: TreeSearch):
        search.leaf_offsets()
        n = search.num_leaves * search.nv
        if self._zeros is None or self._zeros[0].numel() != n or self._zeros[0].device != search.device:
            self._zeros = (torch.zeros(n, dtype=torch.float32, device=search.device),
                           torch.zeros(search.num_leaves, dtype=torch.float32, device=search.device))
        return self._zeros[0], search.obs.node_off, 2, self._zeros[1]


class QEvaluator:
    """Leaves through a ``get_pre_defined`` Q-network or a ``MonteCarloPlayer``: the scores of a leaf's rows are its logits
    (``skip = 2``) and its value is their maximum over the legal rows, clamped to [-1, 1].  These evaluate one side per batch
    (models.py: the head is chosen once per call) and the leaves' sides are mixed, as in the reference (MCTS.py:213-230), so
    the capacity-sized leaf observation goes through the model once per side with the side as the hint, and every row takes
    the output of its own side (``x[:, 2]``): TWO forwards per simulation (per round, over all ``num_leaves`` leaves).  Models with a norm are refused: a whole-batch norm
    ties the graphs of a batch together."""

    def __init__(self, model_or_player, value: str = "max"):
        if value != "max":
            raise NotImplementedError("QEvaluator: value=\"max\" (max_a Q(s, a)) is the one rule")
        if not callable(model_or_player):
            raise TypeError("QEvaluator takes a model of get_pre_defined or a MonteCarloPlayer")
        if live_norm_of(model_or_player):
            raise NotImplementedError("QEvaluator: a whole-batch norm ties the leaves of a batch together")
        self.model = model_or_player

    def side_scores(self, search: TreeSearch, is_maker: bool) -> torch.Tensor:
        """The model's full Q of every row of the leaf observation with the batch declared ``is_maker``'s."""
        obs = search.obs
        x, ei = obs.inputs(is_maker, search.nv)
        with torch.no_grad():
            q = self.model(x, ei, obs.batch_vec, obs.node_off).reshape(-1)
        return q if q.dtype == torch.float32 else q.float()

    def evaluate(self, search: TreeSearch):
        search.leaf_offsets()
        obs = search.obs
        obs.observe_env(search.leaf_handle)
        if search.nv > 128:
            obs.clear_tail()
        qm, qb = self.side_scores(search, True), self.side_scores(search, False)
        q = torch.where(obs.x[:, 2] == 1, qm, qb).contiguous()
        return q, obs.node_off, 2, None


class PolicyValueEvaluator:
    """Leaves through a ``SAGE_torch_script`` policy / value network without the swap output: logits = its log-policy in its
    compacted layout (``skip = 0``), value = its tanh value.  The leaves' sides are mixed, which is this network's normal input.
    The leaf observation is built exact-sized from the sizes the descent reports: one small read-back per simulation (the
    model's own forward reads back as well)."""

    def __init__(self, model):
        from .torch_script_models import SAGE_torch_script
        if not isinstance(model, SAGE_torch_script) or model.swap_allowed:
            raise NotImplementedError("PolicyValueEvaluator takes a SAGE_torch_script with swap_allowed=False")
        self.model = model

    def evaluate(self, search: TreeSearch):
        sizes = search.result[:, 2:4].cpu().numpy().astype(np.int64)
        t = ObsTarget.exact(sizes, search.device, with_ptr=True)
        t.observe_env(search.leaf_handle)
        with torch.no_grad():
            pi, value, _, out_ptr = self.model(t.x, t.edge_global, t.batch_vec, t.ptr)
        return pi.float().contiguous(), out_ptr.to(torch.int32).contiguous(), 0, value.float().contiguous()


def check_round_arguments(sims, leaves, virtual_loss) -> None:
    """``leaves`` / ``virtual_loss`` of a player that searches ``sims`` simulations per move on a fresh tree: the ranges of
    ``TreeSearch`` (which checks them here, with ``sims=None``) and, with ``leaves > 1``, ``sims > leaves`` -- the first round
    of a fresh tree only expands the root (one LEAF, the rest collisions), and a root without a visit has no move to offer."""
    if int(leaves) != leaves or not 1 <= int(leaves) <= _lib.SEARCH_MAX_LEAVES:
        raise ValueError("leaves is an integer in 1 .. %d" % _lib.SEARCH_MAX_LEAVES)
    if int(virtual_loss) != virtual_loss or not 1 <= int(virtual_loss) <= _lib.SEARCH_MAX_VIRTUAL_LOSS:
        raise ValueError("virtual_loss is an integer in 1 .. %d" % _lib.SEARCH_MAX_VIRTUAL_LOSS)
    if sims is not None and int(leaves) > 1 and int(sims) <= int(leaves):
        raise ValueError("sims > leaves: the first round of a fresh tree only expands the root")


def check_reuse_arguments(sims, reuse_tree, capacity) -> int:
    """The simulations a player's trees hold: ``sims`` without tree reuse (``capacity`` must then be None), else ``capacity``
    (default ``4 * sims``, capped at the search's limit), which must reach ``sims``: the new simulations of a ply have to fit
    behind whatever was carried."""
    if not reuse_tree:
        if capacity is not None:
            raise ValueError("capacity belongs to reuse_tree=True")
        return int(sims)
    if capacity is None:
        capacity = min(4 * int(sims), _lib.SEARCH_MAX_SIMS)
    if int(capacity) != capacity or not int(sims) <= int(capacity) <= _lib.SEARCH_MAX_SIMS:
        raise ValueError("capacity is an integer in sims .. %d" % _lib.SEARCH_MAX_SIMS)
    return int(capacity)


class SearchPlies:
    """What a player that searches ``sims`` simulations per move does per match and per ply, the one copy behind ``SearchPlayer``
    and ``search_selfplay.SearchSelfPlay``.  Without ``reuse_tree``: a fresh tree before every search.  With it the trees hold
    ``capacity`` simulations (``check_reuse_arguments``), are reset once per match and re-rooted at the moves played after every
    ply (``TreeSearch.advance`` with ``max_carry = capacity - sims``, so the next search always fits), and ``on_carried`` -- an
    optional callable, set at any time -- receives each ``advance``'s ``carried`` tensor."""

    def __init__(self, sims: int, reuse_tree: bool = False, capacity=None):
        self.sims, self.reuse_tree = int(sims), bool(reuse_tree)
        self.capacity = check_reuse_arguments(sims, reuse_tree, capacity)
        self.on_carried = None

    def _match_begins(self, search) -> None:
        if self.reuse_tree and search is not None:             # (None: a player before its first search)
            search.reset()

    def _search_ply(self, search: TreeSearch, root_handle, evaluator, active, root_noise=None, generator=None) -> None:
        if not self.reuse_tree:
            search.reset()
        search.simulate(root_handle, evaluator, self.sims, active=active, root_noise=root_noise, generator=generator)

    def _ply_played(self, search, moves) -> None:
        if self.reuse_tree and search is not None:
            carried = search.advance(moves, max_carry=self.capacity - self.sims)
            if self.on_carried is not None:
                self.on_carried(carried)


class SearchPlayer(SearchPlies):
    """A player that searches ``sims`` simulations per move with a fresh tree per ply (``leaves`` / ``virtual_loss``: as
    ``TreeSearch`` takes them; the simulations asked for, collisions included).  ``DeviceArena.play`` (``graph=False``)
    hands it the root env, the root observation and the mask of undecided games; it answers with the root visit counts in the
    observation's row layout, from which ``hexgnn_arena_ply`` picks: the most visited move by first maximum at temperature 0,
    else a draw from softmax(count / T) -- NOT the count ** (1 / T) of AlphaZero's move selection.

    ``reuse_tree=True`` keeps the played move's subtree between plies (the reference's Reuse_Tree; ``SearchPlies``): the trees
    hold ``capacity`` simulations (default ``4 * sims``, at least ``sims``), ``search_scores`` runs ``sims`` NEW simulations on
    whatever tree is there, ``begin_match()`` resets the trees and ``observe_moves(moves)`` -- called by the arena after every
    ply, the player's own and the opponent's -- re-roots them at the moves played; a subtree above ``capacity - sims``, a move
    the tree does not hold and a resting game's -1 give a fresh tree."""

    def __init__(self, evaluator, sims: int, c_puct: float = 1.5, prior_temperature: float = 1.0, leaves: int = 1,
                 virtual_loss: int = 1, reuse_tree: bool = False, capacity=None):
        if not hasattr(evaluator, "evaluate"):
            raise TypeError("SearchPlayer takes an evaluator (PolicyValueEvaluator, QEvaluator, UniformEvaluator)")
        if int(sims) < 1:
            raise ValueError("sims must be positive")
        check_round_arguments(sims, leaves, virtual_loss)
        SearchPlies.__init__(self, sims, reuse_tree, capacity)
        self.evaluator, self.c_puct, self.prior_temperature = evaluator, float(c_puct), float(prior_temperature)
        self.leaves, self.virtual_loss = int(leaves), int(virtual_loss)
        self._search = None

    def search_for(self, env_handle, num_games: int, device) -> TreeSearch:
        nv = _lib.lib().hexgnn_env_num_vertices(env_handle)
        size = math.isqrt(nv - 2)
        s = self._search
        if s is None or (s.hex_size, s.num_games, s.device) != (size, num_games, torch.device(device)):
            s = self._search = TreeSearch(size, num_games, self.capacity, self.c_puct, self.prior_temperature, device=device,
                                          leaves=self.leaves, virtual_loss=self.virtual_loss)
        return s

    def search_scores(self, env_handle, obs, active) -> torch.Tensor:
        s = self.search_for(env_handle, obs.k, obs.x.device)
        self._search_ply(s, env_handle, self.evaluator, active)
        return s.root(obs)

    def begin_match(self) -> None:
        """Before ply 0 of a match: with ``reuse_tree`` every tree becomes one unexpanded root (otherwise nothing)."""
        self._match_begins(self._search)

    def observe_moves(self, moves) -> None:
        """After a ply: ``moves`` int32 [G] on the device, the vertex played in each game (-1: the game rests).  With
        ``reuse_tree`` the trees are re-rooted at these moves (otherwise nothing)."""
        self._ply_played(self._search, moves)

    def status(self) -> None:
        if self._search is not None:
            self._search.status()
