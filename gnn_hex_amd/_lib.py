"""ctypes binding of libhexgnn.so (C ABI: include/hexgnn.h).

There is NO fallback: if the shared library is missing or a call fails, this raises.
torch is imported first on purpose: libhexgnn.so links libamdhip64.so.7 by soname, and loading
torch first makes the dynamic loader hand it the HIP runtime torch already uses, so streams and
device pointers are shared with torch's allocator.
"""
from __future__ import annotations

import ctypes as C
import os

import torch  # noqa: F401  (must precede CDLL, see module docstring)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libhexgnn.so")
_lib = None
ABI_VERSION = 8          # HEXGNN_ABI_VERSION of include/hexgnn.h this binding was written against

vp = C.c_void_p
ci = C.c_int
sz = C.c_size_t


def _fields(kind, names):
    return [(name, kind) for name in names.split()]


class QNetCall(C.Structure):
    """``hexgnn_qnet_call`` of include/hexgnn.h, field for field in its order (tests/test_qnet_call_host.py compares the two)."""
    _fields_ = (_fields(sz, "struct_bytes")
                + _fields(ci, "n b c_in hidden total_layers body_layers mode math x_stride need_backward acts_layer")
                + _fields(vp, "gptr rowptr col rowptr_t col_t invdeg x")
                + _fields(vp, "wl bl wr lin_w lin_b v0_w v0_b v1_w v1_b")
                + _fields(vp, "wpack acts saved workspace") + _fields(sz, "workspace_bytes")
                + _fields(vp, "q out_v status")
                + _fields(vp, "td_sel td_target td_weights") + _fields(ci, "td_loss_fn")
                + _fields(vp, "td_dq td_out td_loss_part td_loss")
                + _fields(vp, "dq d_out_v d_embeds flat offsets n_live"))


QNET_CALL_BYTES = C.sizeof(QNetCall)


class SageStackCall(C.Structure):
    """``hexgnn_sage_stack_call`` of include/hexgnn.h, field for field (tests/test_stack_call_host.py compares the two)."""
    _fields_ = (_fields(sz, "struct_bytes") + _fields(ci, "n c_in hidden num_layers x_stride need_backward flags")
                + _fields(vp, "rowptr col rowptr_t col_t invdeg x wl bl wr wpack acts saved workspace")
                + _fields(sz, "workspace_bytes")
                + _fields(vp, "block_starts") + _fields(ci, "num_blocks") + _fields(vp, "group_starts") + _fields(ci, "num_groups")
                + _fields(vp, "nw nb") + _fields(C.c_float, "eps") + _fields(vp, "pre stats norm_ws") + _fields(sz, "norm_ws_bytes")
                + _fields(vp, "n_live dy dx d_wl d_bl d_wr d_nw d_nb") + _fields(ci, "tap_layer") + _fields(vp, "tap_out"))


SAGE_STACK_CALL_BYTES = C.sizeof(SageStackCall)


class TransitionsCall(C.Structure):
    """``hexgnn_transitions_call`` of include/hexgnn.h, field for field (tests/test_device_store_host.py compares the two)."""
    _fields_ = (_fields(sz, "struct_bytes")
                + _fields(ci, "H P k n_count prune_exploratories side0_maker list_len coef_stride")
                + _fields(vp, "n_steps result rank expl coef src_step env action reward next_step done count"))


class StoreCall(C.Structure):
    """``hexgnn_store_call`` of include/hexgnn.h, field for field."""
    _fields_ = (_fields(sz, "struct_bytes")
                + _fields(ci, "capacity nv words list_len side edge_limit H P k start_nodes start_edges")
                + _fields(vp, "count src_step env action reward next_step done")
                + _fields(vp, "hist_adj hist_alive result sizes0 start_adj start_alive")
                + _fields(vp, "adj alive side_bytes ring_action ring_reward ring_done sizes ring_words leaves record env_done"))


class RolloutCall(C.Structure):
    """``hexgnn_rollout_call`` of include/hexgnn.h, field for field (tests/test_eps_schedule_host.py compares the two)."""
    _fields_ = (_fields(sz, "struct_bytes") + _fields(C.c_int64, "frame_add") + _fields(ci, "reset_maker_turn")
                + _fields(vp, "gptr q backmap u sched frames action_vertex action_rank exploratory result adj_out alive_out eps_out"))


class SetupCall(C.Structure):
    """``hexgnn_setup_call`` of include/hexgnn.h, field for field (tests/test_positions_host.py compares the two)."""
    _fields_ = (_fields(sz, "struct_bytes") + _fields(ci, "max_stones from_start maker_turn_start maker_turn_after")
                + _fields(vp, "stones count result applied adj_out alive_out side_out sizes_out"))


class PlayoutCall(C.Structure):
    """``hexgnn_playout_call`` of include/hexgnn.h, field for field (tests/test_playout_host.py compares the two)."""
    _fields_ = (_fields(sz, "struct_bytes") + _fields(ci, "b playouts max_nodes maker_to_move") + _fields(C.c_uint32, "seed")
                + _fields(vp, "gptr rowptr col counter scores value tables wins status"))


PLAYOUT_MAX_NODES = 640      # HEXGNN_PLAYOUT_MAX_NODES


class SearchCall(C.Structure):
    """``hexgnn_search_call`` of include/hexgnn.h, field for field (tests/test_search_host.py compares the two)."""
    _fields_ = (_fields(sz, "struct_bytes") + _fields(ci, "num_games hex_size max_sims skip")
                + _fields(C.c_float, "c_puct temperature fill") + _fields(vp, "workspace") + _fields(sz, "workspace_bytes")
                + _fields(vp, "status active path leaf result logits offsets value gptr scores counts q best"))


class SearchRoundCall(C.Structure):
    """``hexgnn_search_round_call`` of include/hexgnn.h, field for field (tests/test_search_round_host.py compares the two)."""
    _fields_ = (_fields(sz, "struct_bytes") + [("call", SearchCall)] + _fields(ci, "leaves round_leaves virtual_loss"))


class SearchAdvanceCall(C.Structure):
    """``hexgnn_search_advance_call`` of include/hexgnn.h, field for field (tests/test_search_reuse_host.py compares the two)."""
    _fields_ = (_fields(sz, "struct_bytes") + [("call", SearchCall)] + _fields(vp, "moves") + _fields(ci, "max_carry")
                + _fields(vp, "remap carried"))


class RecordCall(C.Structure):
    """``hexgnn_record_call`` of include/hexgnn.h, field for field (tests/test_search_selfplay_host.py compares the two)."""
    _fields_ = (_fields(sz, "struct_bytes") + _fields(ci, "capacity ply pick_mode")
                + _fields(vp, "head recorded u pick policy root_q z adj alive side sizes meta"))


class PVLossCall(C.Structure):
    """``hexgnn_pv_loss_call`` of include/hexgnn.h, field for field (tests/test_search_selfplay_host.py compares the two)."""
    _fields_ = (_fields(sz, "struct_bytes") + _fields(ci, "b n m hex_size capacity")
                + _fields(C.c_float, "q_ratio val_factor pol_factor")
                + _fields(vp, "logp out_ptr gptr backmap value policy z root_q index loss d_logp d_value per_graph status"))


SEARCH_MAX_SIMS = 65535                                       # HEXGNN_SEARCH_MAX_SIMS
SEARCH_REC = 5                                                # HEXGNN_SEARCH_REC: kind, side, path length, terminal value, moves
SEARCH_LEAF, SEARCH_TERMINAL, SEARCH_SKIPPED = 0, 1, 2        # HEXGNN_SEARCH_*
SEARCH_COLLISION = 3                                          # HEXGNN_SEARCH_COLLISION: a descent of a round of several leaves
SEARCH_MAX_LEAVES = 64                                        # HEXGNN_SEARCH_MAX_LEAVES
SEARCH_MAX_VIRTUAL_LOSS = 1024                                # HEXGNN_SEARCH_MAX_VIRTUAL_LOSS


STONE_COLOURS = {"b": 0, "m": 1, "turn": 2}      # HEXGNN_STONE's colour field


def stone(vertex: int, colour, remove: bool = False) -> int:
    """``HEXGNN_STONE(vertex, colour, remove)``; ``colour`` is "b", "m" or "turn" (or the field's number 0 / 1 / 2)."""
    c = STONE_COLOURS.get(colour) if isinstance(colour, str) else (int(colour) if colour in (0, 1, 2) else None)
    if c is None:
        raise ValueError("a stone's colour is \"m\", \"b\" or \"turn\", not %r" % (colour,))
    v = int(vertex)
    if not 0 <= v < 65536:
        raise ValueError("a stone's vertex id is 0 .. 65535, not %d" % v)
    return v | (c << 16) | (int(bool(remove)) << 18)


_SIGS = {
    "hexgnn_abi_version": (ci, []),
    "hexgnn_strerror": (C.c_char_p, [ci]),
    "hexgnn_last_hip_error": (ci, []),
    "hexgnn_padded_width": (ci, [ci]),
    "hexgnn_csr_workspace_bytes": (sz, [ci, ci]),
    "hexgnn_csr_build": (ci, [ci, ci, vp, vp, vp, vp, vp, vp, vp, vp, vp, sz, vp]),
    "hexgnn_csr_build_grouped": (ci, [ci, ci, ci, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
    "hexgnn_csr_build_grouped_pack": (ci, [ci, ci, ci, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, ci, ci, ci, vp, vp, vp, vp, vp]),
    "hexgnn_csr_build_grouped_pack_e": (ci, [ci, ci, ci, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, ci, ci, ci, vp, vp, vp, vp, vp]),
    "hexgnn_csr_build_grouped_pack_b": (ci, [ci, ci, ci, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, ci, ci, ci, vp, vp, vp, vp,
                                             vp, ci, vp]),
    "hexgnn_graph_ptr": (ci, [ci, ci, vp, vp, vp]),
    "hexgnn_sage_stack_pack_bytes": (sz, [ci, ci, ci]),
    "hexgnn_sage_stack_saved_bytes": (sz, [ci, ci, ci, ci]),
    "hexgnn_sage_stack_forward": (ci, [ci, ci, ci, ci, vp, vp, vp, vp, ci, vp, vp, vp, vp, vp, vp, ci, ci, vp]),
    "hexgnn_sage_stack_backward_workspace_bytes": (sz, [ci, ci, ci, ci]),
    "hexgnn_dw_slice_plan": (ci, [ci, ci, ci, ci, C.POINTER(ci), C.POINTER(ci)]),
    "hexgnn_sage_stack_backward": (ci, [ci, ci, ci, ci, vp, vp, vp, vp, vp, vp, ci, vp, vp, vp, vp, vp,
                                        vp, vp, vp, vp, sz, ci, vp]),
    "hexgnn_sage_stack_call_forward": (ci, [C.POINTER(SageStackCall), vp]),
    "hexgnn_sage_stack_call_backward": (ci, [C.POINTER(SageStackCall), vp]),
    "hexgnn_sage_norm_stack_forward": (ci, [ci, ci, ci, ci, vp, vp, vp, vp, ci, vp, vp, vp, vp, vp, C.c_float, vp, vp, vp, vp,
                                            vp, vp, sz, ci, vp]),
    "hexgnn_sage_norm_stack_backward_workspace_bytes": (sz, [ci, ci, ci, ci]),
    "hexgnn_sage_norm_stack_backward": (ci, [ci, ci, ci, ci, vp, vp, vp, vp, ci, vp, vp, vp, vp, vp, vp, C.c_float, vp, vp, vp,
                                             vp, vp, vp, vp, vp, sz, vp, sz, vp]),
    "hexgnn_head_saved_bytes": (sz, [ci, ci, ci]),
    "hexgnn_head_forward": (ci, [ci, ci, ci, ci, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
    "hexgnn_head_backward_workspace_bytes": (sz, [ci, ci, ci]),
    "hexgnn_head_backward": (ci, [ci, ci, ci, ci, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp,
                                  vp, sz, vp]),
    "hexgnn_graph_layernorm_workspace_bytes": (sz, [ci]),
    "hexgnn_graph_layernorm_forward": (ci, [ci, ci, vp, vp, vp, C.c_float, ci, vp, vp, vp, sz, vp]),
    "hexgnn_graph_layernorm_forward_live": (ci, [ci, vp, ci, vp, vp, vp, C.c_float, ci, vp, vp, vp, sz, vp]),
    "hexgnn_graph_layernorm_backward": (ci, [ci, ci, vp, vp, vp, vp, vp, C.c_float, ci, vp, vp, vp, vp, sz, vp]),
    "hexgnn_graph_colnorm_workspace_bytes": (sz, [ci]),
    "hexgnn_graph_colnorm_forward": (ci, [ci, ci, vp, vp, vp, vp, C.c_float, ci, ci, vp, vp, vp, sz, vp]),
    "hexgnn_graph_colnorm_backward": (ci, [ci, ci, vp, vp, vp, vp, vp, vp, C.c_float, ci, ci, vp, vp, vp, vp, vp, sz, vp]),
    "hexgnn_head_linear_saved_bytes": (sz, [ci, ci]),
    "hexgnn_head_linear_forward": (ci, [ci, ci, ci, ci, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
    "hexgnn_head_linear_backward_workspace_bytes": (sz, [ci, ci, ci]),
    "hexgnn_head_linear_backward": (ci, [ci, ci, ci, ci, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, sz, vp]),
    "hexgnn_sage_scalar_forward": (ci, [ci, ci, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
    "hexgnn_sage_scalar_backward_workspace_bytes": (sz, [ci, ci]),
    "hexgnn_sage_scalar_backward": (ci, [ci, ci, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, sz, vp]),
    "hexgnn_policy_log_softmax_forward": (ci, [ci, ci, vp, vp, ci, ci, vp, vp, vp, vp, vp, vp]),
    "hexgnn_policy_log_softmax_backward": (ci, [ci, ci, vp, vp, ci, ci, vp, vp, vp, vp, vp, vp]),
    "hexgnn_qnet_supported": (ci, [ci, ci, ci]),
    "hexgnn_qnet_csr_capacity": (ci, [ci]),
    "hexgnn_qnet_saved_bytes": (sz, [ci, ci, ci, ci, ci]),
    "hexgnn_qnet_forward": (ci, [ci, ci, ci, ci, ci, ci, vp, vp, vp, vp, vp, ci, vp, vp, vp, vp, vp, vp, vp, vp, vp,
                                 vp, vp, vp, ci, ci, ci, vp, vp, vp, vp]),
    "hexgnn_qnet_backward_workspace_bytes": (sz, [ci, ci, ci, ci, ci]),
    "hexgnn_qnet_backward": (ci, [ci, ci, ci, ci, ci, ci, ci, ci, vp, vp, vp, vp, vp, ci, vp, vp, vp, vp, vp, vp, vp, vp,
                                  vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, sz, vp, vp]),
    "hexgnn_qnet_backward_staged": (ci, [ci, ci, ci, ci, ci, ci, ci, ci, vp, vp, vp, vp, vp, ci, vp, vp, vp, vp, vp, vp, vp,
                                         vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, sz, vp, ci, ci, ci, vp]),
    "hexgnn_qnet_call_forward": (ci, [C.POINTER(QNetCall), ci, vp]),
    "hexgnn_qnet_call_backward": (ci, [C.POINTER(QNetCall), ci, ci, ci, vp]),
    "hexgnn_stack_status": (ci, [ci]),
    "hexgnn_stack_reserve_cus": (ci, [ci]),
    "hexgnn_stack_block_budget": (ci, []),
    "hexgnn_debug_stack_mode": (ci, [ci, C.c_uint]),
    "hexgnn_debug_occupy": (ci, [ci, ci, vp, sz, vp, vp]),
    "hexgnn_qnet_jobs_bytes": (sz, [ci, ci]),
    "hexgnn_qnet_multi_workspace_bytes": (sz, [ci, ci, ci, ci, ci, ci]),
    "hexgnn_qnet_forward_jobs": (ci, [ci, ci, vp, vp, ci, ci, ci, vp, vp, vp, vp, vp]),
    "hexgnn_qnet_forward_multi": (ci, [ci, ci, ci, ci, ci, ci, vp, vp, vp, vp, vp, ci, vp, vp, vp, vp, vp, vp]),
    "hexgnn_dqn_targets": (ci, [ci, vp, vp, vp, vp, vp, C.c_float, vp, vp, vp]),
    "hexgnn_env_create": (ci, [ci, ci, vp]),
    "hexgnn_env_destroy": (None, [vp]),
    "hexgnn_env_num_vertices": (ci, [vp]),
    "hexgnn_env_words": (ci, [vp]),
    "hexgnn_env_reset": (ci, [vp, vp, ci, vp, vp]),
    "hexgnn_env_set_maker_turn": (ci, [vp, ci, vp]),
    "hexgnn_env_step": (ci, [vp, vp, ci, ci, ci, vp, vp]),
    "hexgnn_env_observe": (ci, [vp, vp, vp, C.c_int64, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
    "hexgnn_env_export": (ci, [vp, vp, vp, vp, vp, vp, vp, vp]),
    "hexgnn_env_offsets": (ci, [ci, vp, vp, vp, vp]),
    "hexgnn_env_import": (ci, [vp, vp, vp, vp, vp, vp, vp, vp]),
    "hexgnn_states_observe": (ci, [ci, ci, vp, vp, vp, vp, vp, vp, C.c_int64, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
    "hexgnn_per_init": (ci, [ci, vp, vp, vp]),
    "hexgnn_per_update": (ci, [ci, ci, vp, vp, vp, vp, vp]),
    "hexgnn_per_update_td": (ci, [ci, ci, vp, ci, vp, C.c_double, C.c_double, vp, vp, vp, vp]),
    "hexgnn_per_sample": (ci, [ci, ci, ci, C.c_double, vp, vp, vp, vp, vp, vp]),
    "hexgnn_per_sample_dev": (ci, [ci, vp, ci, vp, vp, vp, vp, vp, vp, vp]),
    "hexgnn_replay_offsets": (ci, [ci, vp, ci, ci, vp, vp, vp, vp, vp]),
    "hexgnn_transitions_assemble": (ci, [C.POINTER(TransitionsCall), vp]),
    "hexgnn_replay_store_dev": (ci, [C.POINTER(StoreCall), vp]),
    "hexgnn_select_actions": (ci, [ci, vp, vp, vp, C.c_float, vp, vp, vp, vp, vp]),
    "hexgnn_sample_actions": (ci, [ci, vp, vp, vp, ci, C.c_float, vp, vp, vp, vp, vp]),
    "hexgnn_arena_ply": (ci, [vp, vp, vp, vp, ci, C.c_float, vp, vp, ci, vp, vp, vp, vp, vp]),
    "hexgnn_rollout_ply": (ci, [vp, C.POINTER(RolloutCall), vp]),
    "hexgnn_frames_add": (ci, [vp, C.c_int64, vp]),
    "hexgnn_env_setup": (ci, [vp, C.POINTER(SetupCall), vp]),
    "hexgnn_board_values": (ci, [ci, ci, vp, vp, vp, C.c_float, vp, vp, vp]),
    "hexgnn_playout_values": (ci, [C.POINTER(PlayoutCall), vp]),
    "hexgnn_search_workspace_bytes": (sz, [ci, ci, ci]),
    "hexgnn_search_reset": (ci, [C.POINTER(SearchCall), vp]),
    "hexgnn_search_descend": (ci, [vp, vp, C.POINTER(SearchCall), vp]),
    "hexgnn_search_backup": (ci, [C.POINTER(SearchCall), vp]),
    "hexgnn_search_root": (ci, [C.POINTER(SearchCall), vp]),
    "hexgnn_search_round_workspace_bytes": (sz, [ci, ci, ci, ci]),
    "hexgnn_search_round_descend": (ci, [vp, vp, C.POINTER(SearchRoundCall), vp]),
    "hexgnn_search_round_backup": (ci, [C.POINTER(SearchRoundCall), vp]),
    "hexgnn_search_advance": (ci, [C.POINTER(SearchAdvanceCall), vp]),
    "hexgnn_search_root_noise": (ci, [C.POINTER(SearchCall), C.c_float, vp, vp]),
    "hexgnn_search_record": (ci, [vp, C.POINTER(SearchCall), C.POINTER(RecordCall), vp]),
    "hexgnn_samples_finish": (ci, [ci, ci, ci, ci, vp, vp, vp, vp, vp, vp]),
    "hexgnn_pv_loss": (ci, [C.POINTER(PVLossCall), vp]),
    "hexgnn_td_loss_forward": (ci, [ci, ci, vp, vp, vp, vp, ci, vp, vp, vp]),
    "hexgnn_td_loss_backward": (ci, [ci, ci, vp, vp, vp, ci, vp, vp, vp]),
    "hexgnn_td_loss_forward_backward": (ci, [ci, ci, vp, vp, vp, vp, ci, vp, vp, vp, vp]),
    "hexgnn_profile_enable": (ci, [ci]),
    "hexgnn_profile_read": (ci, [vp, vp]),
    "hexgnn_pad_rows": (ci, [ci, ci, vp, ci, vp, vp]),
    "hexgnn_unpad_rows": (ci, [ci, ci, vp, vp, ci, vp]),
}


class HexGnnError(RuntimeError):
    pass


def lib():
    """Load libhexgnn.so once; raise loudly when it is absent (no CPU fallback exists)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise HexGnnError(
                "libhexgnn.so not found at %s -- build it with `make -C gnn_hex_amd/csrc` "
                "(or `python -c 'import __graft_entry__ as g; g.build()'`). "
                "gnn_hex_amd has no CPU/PyTorch fallback." % LIB_PATH)
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in _SIGS.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        if L.hexgnn_abi_version() != ABI_VERSION:
            raise HexGnnError("libhexgnn.so ABI version mismatch")
        _lib = L
    return _lib


def check(rc: int, what: str = "") -> None:
    if rc != 0:
        L = lib()
        msg = L.hexgnn_strerror(rc).decode()
        if rc == -4:
            msg += " (hipError_t %d)" % L.hexgnn_last_hip_error()
        raise HexGnnError("%s failed: %s" % (what or "hexgnn call", msg))


def exported_symbols():
    """Names every entry point include/hexgnn.h declares (used by the CPU-side ABI test)."""
    return sorted(_SIGS)
