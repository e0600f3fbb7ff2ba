"""The one owner of a batched board observation on the device: its storage layout (``x [N,3]``, ``backmap``, ``batch_vec``,
both edge lists, the sorted CSR, the int32 offsets) and the two kernel calls that fill it (``hexgnn_env_observe`` from live
envs, ``hexgnn_states_observe`` from stored board snapshots).  ``Env_manager.observe`` and ``GraphReplayBuffer.sample`` build
an EXACT target per call; ``DeviceRollout``, ``DeviceArena`` and ``GraphReplayBuffer.sample_device`` keep a CAPACITY-sized
one whose offsets are rewritten on the device and whose rows behind the live total are stale.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib, ops


def prefix_offsets(nodes, edges) -> np.ndarray:
    """Graph sizes -> their exclusive prefix sums as the rows ``(node_off, edge_off)`` of one int64 array [2, k + 1]."""
    off = np.zeros((2, len(nodes) + 1), dtype=np.int64)
    np.cumsum(nodes, out=off[0, 1:])
    np.cumsum(edges, out=off[1, 1:])
    return off


class ObsTarget:
    """Storage of one batched observation of ``k`` graphs: ``N`` rows, ``E`` edge columns (what the kernels are told).
    ``node_off`` / ``edge_off``: int32 [k + 1] on the device, what the observe kernels place the graphs by; ``ptr``: the int64
    form of ``node_off`` for targets that asked for it; ``node_off_host`` / ``edge_off_host``: the int64 prefix sums an exact
    target was sized by.  Built by ``exact`` or ``capacity``."""

    __slots__ = ("k", "E", "x", "backmap", "batch_vec", "edge_local", "edge_global", "gs", "node_off", "edge_off", "ptr",
                 "node_off_host", "edge_off_host", "_iota")

    def __init__(self, k: int, N: int, E: int, dev, zeroed: bool):
        new = torch.zeros if zeroed else torch.empty
        self.k, self.E = k, E
        self.x = new((N, 3), dtype=torch.float32, device=dev)
        self.backmap = new(N, dtype=torch.long, device=dev)
        self.batch_vec = new(N, dtype=torch.long, device=dev)
        self.edge_local = new((2, E), dtype=torch.long, device=dev)
        self.edge_global = new((2, E), dtype=torch.long, device=dev)
        rowptr = new(N + 1, dtype=torch.int32, device=dev)
        col = new(max(E, 1), dtype=torch.int32, device=dev)
        invdeg = (torch.ones if zeroed else torch.empty)(max(N, 1), dtype=torch.float32, device=dev)
        self.gs = ops.GraphStructure.from_csr(N, E, rowptr, col, invdeg)
        self.ptr = self.node_off_host = self.edge_off_host = self._iota = None

    @classmethod
    def exact(cls, sizes: np.ndarray, device, with_ptr: bool = False) -> "ObsTarget":
        """Sized for the graphs of the host array ``sizes [k, 2]`` (nodes, directed edges); ``empty`` storage, both offset
        arrays in one host-to-device copy."""
        off = prefix_offsets(sizes[:, 0], sizes[:, 1])
        self = cls(sizes.shape[0], int(off[0, -1]), int(off[1, -1]), device, False)
        self.node_off_host, self.edge_off_host = off
        self.node_off, self.edge_off = torch.from_numpy(off.astype(np.int32)).to(device, non_blocking=True)
        if with_ptr:
            self.ptr = torch.from_numpy(off[0]).to(device, non_blocking=True)
        return self

    @classmethod
    def capacity(cls, k: int, nv: int, e_cap: int, device, zeroed: bool, with_ptr: bool = False,
                 tail_clear: bool = False) -> "ObsTarget":
        """``k * nv`` rows and ``k * e_cap`` edge columns; the offsets start as zeros and are set by ``set_offsets`` or by a
        kernel.  ``zeroed``: zeros (``invdeg`` ones) instead of ``empty`` storage.  ``tail_clear``: make what ``clear_tail``
        needs."""
        self = cls(k, k * nv, k * e_cap, device, zeroed)
        self.node_off = torch.zeros(k + 1, dtype=torch.int32, device=device)
        self.edge_off = torch.zeros(k + 1, dtype=torch.int32, device=device)
        if with_ptr:
            self.ptr = torch.zeros(k + 1, dtype=torch.int64, device=device)
        if tail_clear:
            self._iota = torch.arange(k * nv + 1, dtype=torch.int32, device=device)
        return self

    def set_offsets(self, sizes: np.ndarray) -> None:
        """Prefix sums of the host array ``sizes [k, 2]`` into the offsets of a capacity target, in place."""
        t = torch.from_numpy(prefix_offsets(sizes[:, 0], sizes[:, 1]).astype(np.int32)).to(self.x.device)
        self.node_off.copy_(t[0])
        self.edge_off.copy_(t[1])

    def _tail(self):
        """The argument tail both observe kernels share.  Without edges the edge pointers fall back to ``x``'s."""
        el, eg = (self.edge_local, self.edge_global) if self.E > 0 else (self.x, self.x)
        return (self.node_off.data_ptr(), self.edge_off.data_ptr(), self.E, self.x.data_ptr(), self.backmap.data_ptr(),
                el.data_ptr(), eg.data_ptr(), self.gs.rowptr.data_ptr(), self.gs.col.data_ptr(), self.gs.invdeg.data_ptr(),
                self.batch_vec.data_ptr(), ops._stream())

    def observe_env(self, handle) -> None:
        """The boards of the env handle's ``k`` envs, placed by the offsets."""
        _lib.check(_lib.lib().hexgnn_env_observe(handle, *self._tail()), "hexgnn_env_observe")

    def observe_states(self, hex_size: int, adj, alive, side, slots32) -> None:
        """The stored board snapshots ``adj`` / ``alive`` / ``side`` of the int32 device slots ``slots32 [k]``."""
        _lib.check(_lib.lib().hexgnn_states_observe(hex_size, self.k, adj.data_ptr(), alive.data_ptr(), side.data_ptr(),
                                                    slots32.data_ptr(), *self._tail()), "hexgnn_states_observe")

    def clear_tail(self) -> None:
        """Empty the CSR rows behind the live total.  The layer-major kernels (boards above 128 nodes, --norm=True) walk ALL
        rows of a capacity-sized target: rows past the current total must be empty, not whatever an earlier, larger
        observation left there (the row right behind the end marker otherwise shows a bogus degree of thousands: 146 us per
        layer launch)."""
        if self._iota is None:
            raise RuntimeError("clear_tail() needs a capacity target built with tail_clear=True")
        k, rowptr = self.k, self.gs.rowptr
        torch.where(self._iota > self.node_off[k], self.edge_off[k], rowptr, out=rowptr)

    def inputs(self, is_maker, max_nodes, live_rows: bool = False):
        """``(x, edge_index)`` for the model: fresh tensor objects per call over the same storage (the hints differ per side
        and per draw), with the hints, the CSR and, where asked, the live row count (int32 [1] on the device) attached."""
        x = self.x.view(self.x.shape)
        ei = self.edge_global.view(self.edge_global.shape)
        if live_rows:
            x._hex_live_rows = self.node_off[self.k:self.k + 1]
        ei._hex_csr = self.gs
        return ops.attach_hints(x, is_maker, max_nodes), ei


def live_norm_of(model) -> bool:
    """Does the model normalise over the live batch?  --norm=True normalises over all nodes of the current observation; a
    capacity-sized target's tail rows are stale once nodes have been removed, so the norm kernels take the live node total
    from the device-side prefix sums instead (``ops.live_rows``).  Only the whole-batch LayerNorm can."""
    norms = getattr(getattr(model, "gnn", None), "norms", None)
    if norms is not None and any(type(m).__name__ != "LayerNorm" for m in norms):
        raise NotImplementedError("capacity-sized observations support the whole-batch LayerNorm of --norm=True; per-channel "
                                  "CachedGraphNorm statistics need exact-size batches: use Env_manager.observe()/step()")
    return norms is not None


def acting_forward(model, obs: ObsTarget, is_maker: bool, nv: int, live_norm: bool):
    """The advantages of every node of a capacity-sized observation of boards with ``nv`` vertices."""
    if nv > 128 or live_norm:
        obs.clear_tail()
    x, ei = obs.inputs(is_maker, nv)
    with torch.no_grad(), ops.live_rows(obs.node_off[obs.k:obs.k + 1] if live_norm else None):
        return model(x, ei, obs.batch_vec, obs.node_off, advantages_only=True)
