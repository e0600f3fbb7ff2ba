"""Monte-Carlo playout players: non-neural opponents of tunable strength that live on the device.

Flat Monte-Carlo with all-moves-as-first statistics (``hexgnn_playout_values``, gnn_hex_amd/csrc/playout.hip).  A random playout
of the Shannon node-switching game needs no move-by-move simulation: the side to move ends up owning a uniformly random
ceil(m / 2) of the m free vertices, and the maker wins iff the terminals are connected inside the maker's vertices.  Because the
subsets are exchangeable, "the mover wins | the mover owns v" is an unbiased estimate of "play v, then a random playout": one
batch of R playouts scores every move, and R is the strength dial.

``playout_values``     the scores of every node of a batched observation (and the value of every graph) from its CSR alone.
``MonteCarloPlayer``   the same as a player with the models' call form: it drops into ``DeviceArena``,
                       ``Elo_handler.add_player(model=...)``, ``Env_manager.select_actions`` and ``positions.board_values``.

The random numbers are a counter-based hash of (seed, counter, graph, playout, vertex): the integers are the same for every
mapping of the kernel, and tests/playout_oracle.py restates the rule on the host.  There is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib, ops

_STATUS = {}


def playout_status(device) -> torch.Tensor:
    """The int32 [1] device word ``playout_values`` reports into by default (bit 1: a graph above ``max_nodes`` rows got NaN
    scores; bit 2: a column index that leaves its graph was dropped).  One per device; never cleared by the kernel."""
    dev = torch.device(device)
    key = (dev.type, dev.index if dev.index is not None else torch.cuda.current_device())
    t = _STATUS.get(key)
    if t is None:
        t = _STATUS[key] = torch.zeros(1, dtype=torch.int32, device=dev)
    return t


def playout_values(x, edge_index, ptr, playouts, *, seed=0, counter=None, is_maker=None, tables=False, max_nodes=None,
                   status=None, out=None):
    """``(scores float32 [N], value float32 [b])`` of the batched observation ``x`` / ``edge_index`` with the int32 or int64
    node offsets ``ptr [b + 1]`` (None: one graph) from ``playouts`` random playouts per graph: ``scores[r]`` in [-1, 1] is
    (2 won - own) / own over the playouts in which the side to move owns node r, ``value[g]`` -- also the score of the graph's
    two terminal rows -- the same over all playouts.  With ``tables=True`` also ``(own, won) int32 [N, 2]`` and ``wins int32
    [b]``.

    The CSR comes from ``edge_index._hex_csr`` (the env builder's), else from ``ops.GraphStructure(edge_index, N)``; the side to
    move and the largest graph from ``is_maker`` / ``max_nodes``, else from ``ops.hints_of(x)``, else as the model derives them
    (``x[0, 2]``, the largest graph: host syncs, as there).  ``counter``: an int64 [1] device tensor the kernel reads (its low
    32 bits), None = 0; ``seed``: 32 bits.  Graphs above ``max_nodes`` (at most 640) rows get NaN and set bit 1 of ``status``
    (int32 [1] on the device, ``playout_status(device)`` by default).  ``out``: the scores tensor to write into (float32 [N],
    contiguous); rows behind ``ptr[b]`` of a capacity-sized observation are neither read nor written.  Everything runs on the
    current stream, nothing is read back, the call is capturable."""
    ops._require_cuda(x, "x")
    dev = x.device
    n = int(x.shape[0])
    hint_maker, hint_nodes = ops.hints_of(x)
    if is_maker is None:
        is_maker = hint_maker if hint_maker is not None else bool(x[0, 2] == 1)
    gptr, b = ops.graph_ptr(None, ptr, n, dev)
    if not gptr.is_contiguous():
        gptr = gptr.contiguous()
    if max_nodes is None:
        max_nodes = hint_nodes
    if max_nodes is None:
        max_nodes = int((gptr[1:] - gptr[:-1]).max()) if b > 0 else 2      # host sync (no size hint given)
    max_nodes = min(max(int(max_nodes), 2), _lib.PLAYOUT_MAX_NODES)
    gs = getattr(edge_index, "_hex_csr", None)
    if gs is None or gs.n != n:
        gs = ops.GraphStructure(edge_index, n)
    if out is None:
        scores = torch.empty(n, dtype=torch.float32, device=dev)
    else:
        scores = out
        if scores.dtype != torch.float32 or not scores.is_contiguous() or scores.numel() < n or scores.device != dev:
            raise ValueError("out: a contiguous float32 tensor of %d values on %s" % (n, dev))
    value = torch.empty(b, dtype=torch.float32, device=dev)
    tab = torch.empty((n, 2), dtype=torch.int32, device=dev) if tables else None
    wins = torch.empty(b, dtype=torch.int32, device=dev) if tables else None
    if status is None:
        status = playout_status(dev)
    if counter is not None and (counter.dtype != torch.int64 or counter.device != dev or counter.numel() < 1):
        raise ValueError("counter: an int64 [1] tensor on %s" % (dev,))
    rowptr, col = gs.rowptr, gs.col
    call = _lib.PlayoutCall(struct_bytes=C.sizeof(_lib.PlayoutCall), b=b, playouts=int(playouts), max_nodes=max_nodes,
                            maker_to_move=int(bool(is_maker)), seed=int(seed) & 0xFFFFFFFF, gptr=gptr.data_ptr(),
                            rowptr=rowptr.data_ptr(), col=col.data_ptr(),
                            counter=counter.data_ptr() if counter is not None else None, scores=scores.data_ptr(),
                            value=value.data_ptr(), tables=tab.data_ptr() if tables else None,
                            wins=wins.data_ptr() if tables else None, status=status.data_ptr())
    _lib.check(_lib.lib().hexgnn_playout_values(C.byref(call), ops._stream()), "hexgnn_playout_values")
    if tables:
        return scores, value, tab, wins
    return scores, value


class MonteCarloPlayer:
    """A playout player with the call form of the ``get_pre_defined`` models: ``player(x, edge_index, graph_indices, ptr,
    advantages_only=...)`` returns one score per node, higher = better for the side to move, so the greedy pick over a graph's
    non-terminal rows is its move.  ``playouts`` is the strength dial.

    The player owns an int64 counter on the device: every call reads it in the kernel and then advances it by one
    (``hexgnn_frames_add``, stream-ordered behind the read), so a replayed HIP graph draws fresh numbers on every replay.
    ``set_counter`` rewinds it (a game is then reproducible from ``seed``)."""

    def __init__(self, playouts: int = 256, seed: int = 0):
        if int(playouts) < 1:
            raise ValueError("playouts must be positive")
        self.playouts, self.seed = int(playouts), int(seed) & 0xFFFFFFFF
        self._counter = None          # made on the device of the first observation
        self._status = None
        self._start = 0

    def _words(self, dev):
        if self._counter is None or self._counter.device != dev:
            self._counter = torch.full((1,), self._start, dtype=torch.int64, device=dev)
            self._status = torch.zeros(1, dtype=torch.int32, device=dev)
        return self._counter, self._status

    def __call__(self, x, edge_index, graph_indices=None, ptr=None, advantages_only=False, **kw):
        dev = x.device
        counter, status = self._words(dev)
        if ptr is None and graph_indices is not None:
            ptr, _ = ops.graph_ptr(graph_indices, None, int(x.shape[0]), dev)
        scores, _ = playout_values(x, edge_index, ptr, self.playouts, seed=self.seed, counter=counter, status=status)
        _lib.check(_lib.lib().hexgnn_frames_add(counter.data_ptr(), 1, ops._stream()), "hexgnn_frames_add")
        return scores

    forward = __call__

    def set_counter(self, n: int) -> None:
        """Set the call counter (device word), e.g. to replay a match: captured graphs read the same word."""
        if n < 0:
            raise ValueError("a call count is not negative")
        self._start = int(n)
        if self._counter is not None:
            self._counter.fill_(int(n))

    def counter(self) -> int:
        """The calls counted so far (reads the device word: synchronises)."""
        return int(self._counter.item()) if self._counter is not None else self._start

    def status(self) -> None:
        """Raise if a call since the last check met a graph the kernel does not take (reads the device word: synchronises)."""
        code = int(self._status.item()) if self._status is not None else 0
        if code:
            self._status.zero_()
            raise _lib.HexGnnError("MonteCarloPlayer (status=%d): 1 = a graph above %d nodes got NaN scores, 2 = a column index "
                                   "outside its graph was dropped" % (code, _lib.PLAYOUT_MAX_NODES))

    def train(self, mode: bool = True):
        return self

    def eval(self):
        return self

    def to(self, *args, **kwargs):
        return self

    def parameters(self):
        return iter(())
