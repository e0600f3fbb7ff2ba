"""Positions that are not reached by playing turn by turn, and the model's output back on the board.

``Env_manager.set_positions`` puts a list of stones on every env in one launch (``hexgnn_env_setup``: forced-colour stones as the
reference's ``make_move(v, force_color=..., remove_dead_and_captured=...)``, graph_game/shannon_node_switching_game.py:80-116).
This module holds what sits around it:

``board_values``       ``Q[n]`` of a batched observation -> the ``hex_size ** 2`` board vector the reference's evaluation code reads
                       (``-5`` on occupied cells) and its arg-max cell (``hexgnn_board_values``;
                       GN0/tests/test_models_on_long_range_task.py:47-52, ``advantage_model_to_evaluater``).
``evaluate``           the model on an observation, then ``board_values``.
``replay_games``       ``ArenaResult.moves`` (or any move log) -> the position after every ply, from ONE set-up launch with its
                       snapshot outputs; ``positions_at(ply)`` observes them (what ``explore_sgf_game.py`` and
                       ``visualize_transitions.py`` step through on the host).
``long_range_stones``  the two positions per defender colour of the reference's long-range dependency task as stone lists.

These are latency paths: nobody has timed them, no performance is claimed and no test depends on a time.  There is no CPU
fallback.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib, ops
from ._lib import stone  # noqa: F401  (re-exported: the packing of one stone)
from .multi_env_manager import Env_manager, ObsList
from .observation import ObsTarget


def _gptr32(obs) -> torch.Tensor:
    """int32 [k + 1] node offsets of an observation on the device (an ``ObsList`` keeps them as a host list)."""
    if torch.is_tensor(obs.node_off):
        return obs.node_off
    g = getattr(obs, "_ptr32", None)
    if g is None:
        g = obs._ptr32 = torch.tensor(obs.node_off, dtype=torch.int32, device=obs.x.device)
    return g


def board_values(q: torch.Tensor, obs, hex_size: int, fill: float = -5.0):
    """``(board float32 [k, hex_size ** 2], best int32 [k])`` for the model output ``q`` (one value per node) of the batched
    observation ``obs`` (an ``ObsList`` or ``ObsTarget``): ``board[g]`` holds ``fill`` on every cell that is no node of graph g
    any more and ``q`` of the node elsewhere; ``best[g]`` is the cell of the first maximum over the graph's non-terminal nodes
    (``hexgnn_select_actions``' comparison), -1 when there is none.  Device tensors, nothing is read back."""
    k = len(obs) if isinstance(obs, ObsList) else obs.k
    dev = obs.x.device
    qf = q.reshape(-1)
    if qf.dtype != torch.float32 or not qf.is_contiguous():
        qf = qf.float().contiguous()
    if qf.numel() < obs.x.shape[0]:
        raise ValueError("q holds %d values, the observation %d nodes" % (qf.numel(), obs.x.shape[0]))
    board = torch.empty((k, hex_size * hex_size), dtype=torch.float32, device=dev)
    best = torch.empty(k, dtype=torch.int32, device=dev)
    _lib.check(_lib.lib().hexgnn_board_values(k, int(hex_size), _gptr32(obs).data_ptr(), qf.data_ptr(), obs.backmap.data_ptr(),
                                              float(fill), board.data_ptr(), best.data_ptr(), ops._stream()),
               "hexgnn_board_values")
    return board, best


def evaluate(model, obs: ObsList, hex_size: int, fill: float = -5.0):
    """``model(x, edge_index, batch, ptr)`` on the observation -- full Q, as ``advantage_model_to_evaluater`` asks for -- then
    ``board_values``.  Boards above 128 nodes take the model's layer-major path as any other batch does."""
    b = obs.to_batch()
    with torch.no_grad():
        q = model(b.x, b.edge_index, b.batch, b.ptr)
    return board_values(q, obs, hex_size, fill)


class ReplayedGames:
    """The positions of ``G`` replayed games: ``winner`` int8 [G] (-1 undecided, 0 maker, 1 breaker) and ``length`` int64 [G]
    from the set-up's result record (host arrays), ``sizes`` int64 [G, plies, 2] (nodes, directed edges; (0, 0) where a game
    holds no position), and the board snapshots on the device."""

    def __init__(self, hex_size, first, winner, length, sizes, adj, alive, side):
        self.hex_size, self.first = hex_size, first
        self.winner, self.length, self.sizes = winner, length, sizes
        self._adj, self._alive, self._side = adj, alive, side
        self.plies = sizes.shape[1]

    def positions_at(self, ply: int):
        """``(ObsList, game_index)``: the observation of every game that still holds a position after its move ``ply`` (the
        game is not decided there and had that many moves), and the games' indices (int64 host array).  All of them have the
        same side to move."""
        if not 0 <= ply < self.plies:
            raise IndexError("ply %d of %d" % (ply, self.plies))
        games = np.nonzero(self.sizes[:, ply, 0] > 0)[0]
        if len(games) == 0:
            raise ValueError("no game holds a position after ply %d: every game was decided by then" % ply)
        sizes = self.sizes[games, ply]
        dev = self._adj.device
        G, L = self.sizes.shape[:2]
        maker = (self.first == "m") == (ply % 2 == 1)      # `first` made move 0: the other side moves after it
        t = ObsTarget.exact(sizes, dev)
        nv, W = self._adj.shape[2:]
        slots = torch.from_numpy((games * L + ply).astype(np.int32)).to(dev)
        t.observe_states(self.hex_size, self._adj.view(G * L, nv, W), self._alive.view(G * L, nv), self._side.view(G * L), slots)
        obs = ObsList(t.x, t.edge_local, t.edge_global, t.backmap, t.batch_vec, t.node_off_host.tolist(),
                      t.edge_off_host.tolist(), t.gs, maker, int(sizes[:, 0].max()))
        return obs, games


def replay_games(hex_size: int, moves, first: str = "m", device=None) -> ReplayedGames:
    """Turn a move log -- ``ArenaResult.moves``: vertex ids ``[G][plies]`` in the order played, -1 behind a game's end -- back
    into positions.  Every entry becomes a stone of the side on turn with dead/captured removal, ``first`` moving at ply 0,
    and ONE ``hexgnn_env_setup`` launch with its snapshot outputs plays all games.  ``ValueError`` for a log that holds an
    illegal move or a move behind the deciding one."""
    if first not in ("m", "b"):
        raise ValueError("first must be \"m\" or \"b\"")
    mv = np.asarray(moves, dtype=np.int64)
    if mv.ndim != 2 or mv.shape[0] < 1:
        raise ValueError("moves has the shape [G][plies]")
    G, L = mv.shape[0], max(1, mv.shape[1])
    played = mv >= 0
    cnt = played.sum(1).astype(np.int32)
    if (played != (np.arange(mv.shape[1])[None, :] < cnt[:, None])).any():
        raise ValueError("a move log holds its -1 entries behind the game's last move only")
    if mv.max(initial=0) >= 65536:
        raise ValueError("a move is a vertex id")
    arr = np.zeros((G, L), dtype=np.int32)
    arr[:, :mv.shape[1]] = np.where(played, mv | (2 << 16) | (1 << 18), 0)
    mgr = Env_manager(G, hex_size, device=device)
    dev, nv, W = mgr.device, mgr._nv, mgr._words
    st, ct = torch.from_numpy(arr).to(dev), torch.from_numpy(cnt).to(dev)
    result = torch.empty((G, 5), dtype=torch.int32, device=dev)
    applied = torch.empty(G, dtype=torch.int32, device=dev)
    adj = torch.empty((G, L, nv, W), dtype=torch.int64, device=dev)
    alive = torch.empty((G, L, nv), dtype=torch.uint8, device=dev)
    side = torch.empty((G, L), dtype=torch.uint8, device=dev)
    sizes = torch.empty((G, L, 2), dtype=torch.int32, device=dev)
    call = _lib.SetupCall(struct_bytes=C.sizeof(_lib.SetupCall), max_stones=L, from_start=1, maker_turn_start=int(first == "m"),
                          maker_turn_after=-1, stones=st.data_ptr(), count=ct.data_ptr(), result=result.data_ptr(),
                          applied=applied.data_ptr(), adj_out=adj.data_ptr(), alive_out=alive.data_ptr(),
                          side_out=side.data_ptr(), sizes_out=sizes.data_ptr())
    _lib.check(_lib.lib().hexgnn_env_setup(mgr._h, C.byref(call), ops._stream()), "hexgnn_env_setup")
    res = result.cpu().numpy()
    if res[:, 4].any():
        g = int(np.nonzero(res[:, 4])[0][0])
        j = int(applied[g])
        raise ValueError("game %d, ply %d: %s" % (g, j, "illegal move %d" % int(mv[g, j]) if res[g, 4] == 1
                                                  else "a move behind the one that decided the game"))
    return ReplayedGames(hex_size, first, res[:, 0].astype(np.int8), res[:, 1].astype(np.int64),
                         sizes.cpu().numpy().astype(np.int64), adj, alive, side)


def long_range_stones(hex_size: int, defender: str):
    """``(negative, positive)``: the two positions of the long-range dependency task for one defender colour, as lists of
    ``(vertex, colour, False)`` stones -- forced colours, no dead/captured removal; the defender is to move
    (``set_positions(..., onturn=defender)``).

    Board cell ``(r, c)`` is vertex ``r * n + c + 2``.  The maker connects row 0 with row n - 1, the breaker column 0 with column
    n - 1.  Defender ``"m"`` owns every cell of row 1; defender ``"b"`` every cell of column 1 (the transposed picture).  In
    the maker's picture the attacker owns, for i = 2 .. n - 1, the two border cells ``(i, 0)`` and ``(i, n - 1)`` of row i, and for
    i = 1 .. n - 2 cell ``(0, i)`` of the border row next to the defender's: 4n - 6 stones.  The defender's row is cut off from
    its near border except through the two corner cells ``(0, 0)`` and ``(0, n - 1)``.  The positive position adds the attacker's
    stone on the far corner ``(0, n - 1)`` and a defender's stone in mid-board, cell ``(2 + (n - 2) // 2, n // 2)``: 4n - 4 stones,
    and board cell 0, a whole board away from the new stones, has become the defender's only way to its border."""
    n = int(hex_size)
    if n < 3:
        raise ValueError("the long-range positions need a board of 3 x 3 or more")
    if defender not in ("m", "b"):
        raise ValueError("defender must be \"m\" or \"b\"")
    attacker = "b" if defender == "m" else "m"

    def vertex(r, c):          # (r, c) in the maker's picture; the breaker's is its transpose
        return (r * n + c if defender == "m" else c * n + r) + 2

    line = [(vertex(1, c), defender, False) for c in range(n)]
    sides = [(vertex(r, c), attacker, False) for r in range(2, n) for c in (0, n - 1)]
    border = [(vertex(0, c), attacker, False) for c in range(1, n - 1)]
    negative = line + sides + border
    positive = negative + [(vertex(0, n - 1), attacker, False), (vertex(2 + (n - 2) // 2, n // 2), defender, False)]
    return negative, positive
