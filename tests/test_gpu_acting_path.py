"""GPU: the self-play acting path -- observation in a capacity-sized target, advantages-only forward without a backward, the pick,
the captured rollout, the example program -- at the published widths, against float64 oracles.

Why: DESIGN.md 7.8 / 7.12 and profiles/graph_updates/selfplay_alternation.txt record ``ValueError: illegal action at step 0 for env
1`` in the first rollout of a fresh ``examples/selfplay_train.py`` process at the GNN-L recipe (Hex-11, 128 envs, 15 + 2 layers,
hidden 110, captured rollout), intermittent, on parent and child commits alike, cause not looked for.  No other test plays that
shape: every rollout test runs 3 layers of hidden 16 or 35 on 6 to 24 envs.

Shapes (``helpers.ACTING_SHAPES``; model ``modern_two_headed`` with 2 head layers, ``helpers.sharpen_``):
  L  Hex-11, 15 body layers, hidden 110: the published GNN-L (123-row start graphs, NT 7 with two pad columns, 17 layers);
  S  Hex-7, 10 body layers, hidden 35: GNN-S (NT 3 with pad columns, 51-row graphs: waves 4-7 own no rows);
  W  Hex-12, 3 body layers, hidden 110: 146 rows, the layer-major kernels over a capacity target with ``clear_tail``.

Positions of cases 1 and 2 (``helpers.acting_script``, from the C env oracle alone): six lock-stepped envs play a seeded script of
legal random moves, ended at the first even (maker to move) or odd (breaker) ply count at which the six graphs have six different
node counts and at least one env has been auto-reset; both properties are asserted in the test, on the oracle and on the device.
Weight seed per (shape, side): the first below ``helpers.SEEDS`` at which the float64 oracle alone has every ReLU input at least
``helpers.MARGIN`` (2^-16 of its tensor's rms) from zero and an advantage spread of at least 0.5 over the non-terminal rows of every
graph.  It is recorded below and evaluated again at every use.  At L NO seed below 400 has that margin on either batch (294 and 327
rows x 17 layers x 110 columns are half a million ReLU inputs; the largest margin of the 400 is 3.9e-6 on the maker's batch, 3.0e-6
on the breaker's, a full scan takes 23 s), so L takes the first seed that meets the spread condition and prints its margin.  Nothing
is lost for a forward: ReLU is continuous, an input within m of zero moves its output by at most m whichever way fp32 rounds it; the
margin matters where a mask gates a gradient, and the acting form has no backward.

Cases:
  1. ``observation.acting_forward`` over ``ObsTarget.capacity`` (DeviceRollout's arguments) observed at the start position first and
     then at the scripted one, ``x`` and ``invdeg`` behind the live total painted NaN: max |A - A64| <= max(3 x the fp32 CPU
     oracle's own distance, 5e-6 = ``helpers.QnetCases.CONST``) on the live rows, all finite, status word 0; L and S: the bits of the
     exact-size call on ``Batch.from_data_list(mgr.observe())``; the same bits with the library's scratch filled with 0xFF and with
     0x3F; the kernel form that ran (per-graph for L and S, layer-major for W; n = k nv, hidden) read off the call record.
  2. the pick on those advantages: ``hexgnn_select_actions`` (eps 0), ``hexgnn_rollout_ply`` under ``EpsSchedule(0, 0, 0)`` on a twin
     and the arena's greedy ``hexgnn_sample_actions`` agree; every vertex is >= 2, alive, ``backmap[node_off[g] + rank]``, and its A64
     is within 2 B of its graph's maximum (B: case 1's bound); eps 1: every env explores, 2 <= rank < n_g, ``hexgnn_env_step`` accepts
     every move.
  3. L, 128 envs, ``steps=2``, captured, with eps 0.0 and with ``EpsSchedule(0, 0, 0)``: the state after construction (boards, sizes,
     frame counter, offsets), then two runs bit-equal (vertices, ranks, result words, all three board snapshots) to an eager rollout
     on a twin and to the public step-by-step loop, all envs playing the same two moves, move 0 of each run within 2 B of the float64
     oracle's maximum on the oracle's own position; the first run again behind a large unrelated matmul.
  4. L, 128 envs, ``steps=16``, captured, eps 0.12 as a float and as ``EpsSchedule(0.12, 0.05, 100000)``: the move log replayed on
     ``RefGame`` per env (legal moves, winner, length, auto reset, node and edge counts), and for envs 0-3 and 124-127 every
     non-exploratory move judged by the mover's float64 oracle at the bar of test_gpu_arena.py (picked q64 >= max - 2e-4).  No
     Hex-11 game can end within 16 moves, so five more runs are replayed the same way (not judged) until games end and reset.
  5. ``examples/selfplay_train.py`` with the default GNN-L arguments in one fresh child process per test (last in the file): exit
     status 0 and the closing ``env frames/s`` line; a fault or a hang of the child ends the session.

Measured on the MI355X (each test prints its own figures; DESIGN.md 7.15 says what they mean for the step-0 failure):

  shape, side    live rows   max |A - A64|   fp32 oracle's own   bound
  L maker        294 / 738   4.08e-6         2.69e-6             8.07e-6
  L breaker      327 / 738   3.33e-6         2.15e-6             6.44e-6
  S maker        236 / 306   1.28e-6         8.89e-7             5e-6
  S breaker      222 / 306   1.37e-6         1.24e-6             5e-6
  W maker        491 / 876   1.12e-6         1.06e-6             5e-6
  W breaker      470 / 876   1.64e-6         1.66e-6             5e-6

Case 4: 114 (float) and 115 (schedule) judged plies, 8 of each with a float64 top-2 gap below 2e-4; 242 and 239 of the first run's
2048 moves exploratory; 194 and 195 games finished and reset over the six runs.  All 18 tests pass (13 s with the two child
processes of 4.2 s and 4.0 s): no defect was found, and no run showed the step-0 failure.

That the file bites -- two libraries with one in-bounds arithmetic change each, run once through this file:
  (i)  the per-graph kernel's advantage dot skips the last column tile in mode 2 (qnet_fwd_body.inc, ``t < NT - 1``): 7 fail, 11
       pass.  Case 1 on L and S, both sides: |A - A64| 0.50, 1.17, 0.56, 0.42 against bounds of 5e-6 .. 8.1e-6; case 2 on L breaker
       (graph 0: picked A64 0.3547, maximum 0.6477); case 4 both ways (run 0, env 1, step 5: picked q64 1.0974, maximum 1.1369).
       W passes (another kernel), and so do the bit comparisons: exact-size call, poisoned scratch, eager rollout and step-by-step
       loop all run the changed kernel -- only the oracle sees it.  Case 3 passes too: the changed advantages still have their
       maximum at the oracle's node in the two positions it judges.
  (ii) the layer-major head's advantage dot drops the last column tile (head.hip, ``s_w`` zero from column 96 on): 4 fail, 14 pass:
       cases 1 and 2 on W, both sides (|A - A64| 0.635 and 0.245 against 5e-6; picked A64 1.2914 against 1.3958, 1.3339 against
       1.4054).  Every L and S case passes.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from helpers import (ACTING_ENVS, ACTING_SHAPES, MARGIN, PoisonedTorch, QnetCases, abs_bound, acting_oracle, acting_script,
                     graph_spreads, model_args, oracle_batch)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
GREEDY = 0
CONST = QnetCases.CONST
K = ACTING_ENVS

# (shape, side) -> (script seed, plies, weight seed, is the ReLU margin attainable below SEEDS): what the searches of
# helpers.acting_script / acting_oracle found; evaluated again at every use, searched again where it no longer holds
RECORDED = {("L", "maker"): (0, 42, 1, False), ("L", "breaker"): (0, 41, 13, False),
            ("S", "maker"): (0, 16, 12, True), ("S", "breaker"): (0, 17, 9, True),
            ("W", "maker"): (0, 48, 7, True), ("W", "breaker"): (0, 49, 7, True)}
CASES = [(s, side) for s in ("L", "S", "W") for side in ("maker", "breaker")]

_cases, _positions, _models, _worst = {}, {}, {}, {}


# ---- the CPU side: positions, weights, oracles -----------------------------------------------------------------------------------

def _case(hexref, shape, side):
    """The scripted position of (shape, side) on the C env oracle and the model oracle's advantages on it, once per session."""
    key = (shape, side)
    if key not in _cases:
        size, body, hidden = ACTING_SHAPES[shape]
        script_seed, _plies, weight_seed, need_margin = RECORDED[key]
        maker = side == "maker"
        s = acting_script(hexref, size, odd=not maker, recorded=script_seed)
        games = s["ref"].envs
        nodes = [g.num_vertices() for g in games]
        # the properties the script was chosen for
        assert len(s["moves"]) % 2 == int(not maker) and all(g.maker_turn == maker for g in games)
        assert len(set(nodes)) == K and s["reset"].any() and not s["reset"].all(), (nodes, s["reset"])
        batch = oracle_batch(games)
        o = acting_oracle(body, hidden, batch, maker, recorded=weight_seed, need_margin=need_margin)
        assert o["ok"], "%s %s: %s" % (shape, side, o["text"])
        assert not need_margin or o["margin"] >= MARGIN
        assert min(graph_spreads(o["a64"], batch[3])) >= 0.5
        print("%s %s: script seed %d, %d plies, nodes %s, reset %s; weight seed %d; %s"
              % (shape, side, s["seed"], len(s["moves"]), nodes, s["reset"].astype(int).tolist(), o["seed"], o["text"]))
        _cases[key] = dict(script=s, nodes=nodes, batch=batch, oracle=o, maker=maker)
    return _cases[key]


def _hip_model(shape, ref):
    """The HIP model with the oracle's weights (one per oracle model)."""
    from gnn_hex_amd.models import get_pre_defined
    if id(ref) not in _models:
        _, body, hidden = ACTING_SHAPES[shape]
        hip = get_pre_defined("modern_two_headed", model_args(body, hidden))
        res = hip.load_state_dict(ref.state_dict())
        assert not res.missing_keys and not res.unexpected_keys
        _models[id(ref)] = (hip.cuda().eval(), ref)
    return _models[id(ref)][0]


def _bound(a32, a64):
    """B of the float64 rule: max(3 x the fp32 oracle's own distance, the constant)."""
    return max(3.0 * (a32.double() - a64).abs().max().item(), CONST)


# ---- the device side of cases 1 and 2: the scripted position inside a capacity-sized target -------------------------------------------

def _position(hexref, shape, side):
    from gnn_hex_amd.data import Batch
    from gnn_hex_amd.multi_env_manager import Env_manager
    from gnn_hex_amd.observation import ObsTarget
    key = (shape, side)
    if key in _positions:
        return _positions[key]
    c = _case(hexref, shape, side)
    size = ACTING_SHAPES[shape][0]
    mgr = Env_manager(K, size)
    mgr.reset()
    nv = mgr._nv
    # (DeviceRollout.__init__'s arguments for a model without norms)
    obs = ObsTarget.capacity(K, nv, int(mgr._base_sizes[0, 1]), mgr.device, zeroed=True, tail_clear=nv > 128)
    obs.set_offsets(mgr._sizes)
    obs.observe_env(mgr._h)                       # the start position first: the rows behind the later, smaller total are stale
    assert int(obs.node_off[K]) == K * nv
    reset = np.zeros(K, dtype=bool)
    for acts in c["script"]["moves"]:
        _, _, dones, _ = mgr.step(acts)
        reset |= dones
    assert reset.tolist() == c["script"]["reset"].tolist() and mgr._sizes[:, 0].tolist() == c["nodes"]
    assert (mgr.global_onturn == "m") == c["maker"]
    obs.set_offsets(mgr._sizes)
    obs.observe_env(mgr._h)
    N = int(mgr._sizes[:, 0].sum())
    assert 0 < N < K * nv and int(obs.node_off[K]) == N
    obs.x[N:] = float("nan")                      # (the integer arrays stay as the start observation left them)
    obs.gs.invdeg[N:] = float("nan")
    # the device's batch is the one the oracle evaluated
    x, ei, bv, ptr, bm = c["batch"]
    bt = Batch.from_data_list(mgr.observe())
    assert torch.equal(bt.x.cpu(), x) and torch.equal(bt.edge_index.cpu(), ei) and torch.equal(bt.ptr.cpu(), ptr)
    assert torch.equal(obs.x[:N].cpu(), x) and torch.equal(obs.backmap[:N].cpu(), bm)
    assert obs.node_off.cpu().tolist() == ptr.tolist()
    _positions[key] = dict(mgr=mgr, obs=obs, N=N, nv=nv, bt=bt, case=c)
    return _positions[key]


def _acting(p, hip):
    """``acting_forward`` on the position's capacity target: (advantages of ALL rows, the call record)."""
    from gnn_hex_amd import ops
    from gnn_hex_amd.observation import acting_forward
    adv = acting_forward(hip, p["obs"], p["case"]["maker"], p["nv"], False).reshape(-1)
    call = hip.__dict__["_fca"]
    assert isinstance(call, ops._QNetCall), "the direct fused call did not run"
    return adv, call


# ---- 1. acting_forward over a capacity-sized target --------------------------------------------------------------------------------

@pytest.mark.parametrize("shape,side", CASES, ids=["%s-%s" % c for c in CASES])
def test_acting_forward_over_a_capacity_target(hexref, shape, side, monkeypatch):
    from gnn_hex_amd import ops
    p = _position(hexref, shape, side)
    c, N, nv = p["case"], p["N"], p["nv"]
    o = c["oracle"]
    hidden = ACTING_SHAPES[shape][2]
    hip = _hip_model(shape, o["ref"])
    status = ops.sticky_status(p["mgr"].device)
    status.zero_()                                # (sticky: whatever an earlier test left there is not this test's)

    adv, call = _acting(p, hip)
    a = adv[:N].clone()
    # the kernel form that ran
    assert call.layered == (shape == "W") and call.dims[0] == K * nv and call.dims[1] == K and call.dims[3] == hidden
    assert call.dims[6] == 2 and adv.numel() == K * nv
    if shape != "W":
        assert call.desc.need_backward == 0 and call.desc.acts_layer == call.desc.body_layers - 1 and call.desc.mode == 2
        assert ops.qnet_fused_supported(2, hidden, nv)
    else:
        assert not ops.qnet_fused_supported(2, hidden, nv)

    # the float64 rule on the live rows
    assert torch.isfinite(a).all()
    tag = "%s %s" % (shape, side)
    e, e32 = abs_bound(tag, "A", a, o["a32"], o["a64"], CONST)
    assert int(status.item()) == 0
    w = _worst.setdefault(shape, [0.0, 0.0])
    w[0], w[1] = max(w[0], e), max(w[1], e32)
    print("%s: %d live rows of %d, |A - A64| %.3g (fp32 oracle %.3g, bound %.3g); worst of shape %s so far %.3g (%.3g)"
          % (tag, N, K * nv, e, e32, max(3 * e32, CONST), shape, w[0], w[1]))

    # the bits of the exact-size call (the per-graph kernel does the same work)
    if shape != "W":
        bt = p["bt"]
        with torch.no_grad():
            exact = hip(bt.x, bt.edge_index, bt.batch, bt.ptr, advantages_only=True).reshape(-1)
        ecall = hip.__dict__["_fca"]
        assert not ecall.layered and ecall.dims[0] == N
        assert torch.equal(exact, a), "%s: the capacity-sized call differs from the exact-size one by %.3g" \
            % (tag, (exact - a).abs().max().item())

    # nothing depends on what the scratch held
    for byte in (0xFF, 0x3F):
        stand_in = PoisonedTorch(byte)
        with monkeypatch.context() as mp:
            mp.setattr(ops, "torch", stand_in)
            again = _acting(p, hip)[0][:N].clone()
            torch.cuda.synchronize()
        assert stand_in.filled >= 1, "the scratch did not come through ops' torch.empty"
        assert torch.equal(again, a), "%s: scratch byte %#x changes the advantages by %.3g" \
            % (tag, byte, (again - a).abs().max().item())
    assert int(status.item()) == 0


# ---- 2. the pick on the model's own output --------------------------------------------------------------------------------------------

def _twin_of(mgr):
    from gnn_hex_amd.multi_env_manager import Env_manager
    twin = Env_manager(mgr.num_envs, mgr.hex_size)
    twin.reset()
    twin._restore_state_tensors(mgr._state_tensors())
    return twin


def _ints(k, dtype=torch.int32, fill=-9):
    return torch.full((k,), fill, dtype=dtype, device=DEV)


@pytest.mark.parametrize("shape,side", CASES, ids=["%s-%s" % c for c in CASES])
def test_pick_on_the_models_own_advantages(hexref, shape, side):
    from gnn_hex_amd import _lib, ops
    from gnn_hex_amd.multi_env_manager import EpsSchedule
    L = _lib.lib()
    p = _position(hexref, shape, side)
    c, mgr, obs, nv = p["case"], p["mgr"], p["obs"], p["nv"]
    o, maker = c["oracle"], c["maker"]
    q = _acting(p, _hip_model(shape, o["ref"]))[0].contiguous()
    gptr, backmap = obs.node_off, obs.backmap
    ptr = c["batch"][3].tolist()
    st = ops._stream()

    # greedy, three ways
    v_sel, r_sel, x_sel = _ints(K), _ints(K), _ints(K, torch.uint8, 9)
    _lib.check(L.hexgnn_select_actions(K, gptr.data_ptr(), q.data_ptr(), backmap.data_ptr(), 0.0, None, v_sel.data_ptr(),
                                       r_sel.data_ptr(), x_sel.data_ptr(), st), "hexgnn_select_actions")
    v_arena, r_arena, status = _ints(K), _ints(K), _ints(1, fill=99)
    _lib.check(L.hexgnn_sample_actions(K, gptr.data_ptr(), q.data_ptr(), backmap.data_ptr(), GREEDY, 1.0, None, v_arena.data_ptr(),
                                       r_arena.data_ptr(), status.data_ptr(), st), "hexgnn_sample_actions")
    twin = _twin_of(mgr)
    v_ply, r_ply, x_ply = _ints(K), _ints(K), _ints(K, torch.uint8, 9)
    result = torch.full((K, 5), -9, dtype=torch.int32, device=DEV)
    adj_out = torch.zeros((K, nv, mgr._words), dtype=torch.int64, device=DEV)
    alive_out = torch.zeros((K, nv), dtype=torch.uint8, device=DEV)
    u = torch.zeros((K, 2), dtype=torch.float32, device=DEV)
    frames = torch.zeros(1, dtype=torch.int64, device=DEV)
    sched = EpsSchedule(0.0, 0.0, 0)
    block = sched.to_device(DEV)
    call = _lib.RolloutCall(
        struct_bytes=C.sizeof(_lib.RolloutCall), frame_add=0, reset_maker_turn=int(not maker), gptr=gptr.data_ptr(), q=q.data_ptr(),
        backmap=backmap.data_ptr(), u=u.data_ptr(), sched=block.data_ptr(), frames=frames.data_ptr(),
        action_vertex=v_ply.data_ptr(), action_rank=r_ply.data_ptr(), exploratory=x_ply.data_ptr(), result=result.data_ptr(),
        adj_out=adj_out.data_ptr(), alive_out=alive_out.data_ptr(), eps_out=None)
    _lib.check(L.hexgnn_rollout_ply(twin._h, C.byref(call), st), "hexgnn_rollout_ply")
    assert torch.equal(r_sel, r_arena) and torch.equal(v_sel, v_arena) and int(status.item()) == 0
    assert torch.equal(r_sel, r_ply) and torch.equal(v_sel, v_ply)
    assert not x_sel.any() and not x_ply.any()
    assert not result[:, 4].any(), "the ply's own move was refused: %s" % result.tolist()

    alive = mgr._state()["alive"]
    bm = backmap.cpu()
    B = _bound(o["a32"], o["a64"])
    ranks, verts = r_sel.tolist(), v_sel.tolist()
    for g in range(K):
        r, v, n_g = ranks[g], verts[g], ptr[g + 1] - ptr[g]
        assert 2 <= r < n_g and v >= 2 and alive[g][v] == 1 and v == int(bm[ptr[g] + r]), (g, r, v)
        a64 = o["a64"][ptr[g] + 2:ptr[g + 1]]
        assert a64[r - 2].item() >= a64.max().item() - 2 * B, \
            "%s %s graph %d: picked A64 %.6f, max %.6f, B %.3g" % (shape, side, g, a64[r - 2].item(), a64.max().item(), B)

    # eps 1: every env explores, and the env accepts every move
    gen = torch.Generator().manual_seed(7)
    u1 = torch.rand((K, 2), generator=gen).to(DEV)
    _lib.check(L.hexgnn_select_actions(K, gptr.data_ptr(), q.data_ptr(), backmap.data_ptr(), 1.0, u1.data_ptr(), v_sel.data_ptr(),
                                       r_sel.data_ptr(), x_sel.data_ptr(), st), "hexgnn_select_actions")
    assert x_sel.all()
    for g, (r, v) in enumerate(zip(r_sel.tolist(), v_sel.tolist())):
        assert 2 <= r < ptr[g + 1] - ptr[g] and v == int(bm[ptr[g] + r]) and alive[g][v] == 1, (g, r, v)
    twin = _twin_of(mgr)
    _lib.check(L.hexgnn_env_step(twin._h, v_sel.data_ptr(), 1, 1, int(not maker), result.data_ptr(), st), "hexgnn_env_step")
    assert not result[:, 4].any()


# ---- 3. construction and first replays of a captured rollout at the self-play shape -------------------------------------------------

ENVS = 128


def _eps(kind, e, final=None, decay=0):
    from gnn_hex_amd.multi_env_manager import EpsSchedule
    return float(e) if kind == "float" else EpsSchedule(e, e if final is None else final, decay)


def _fresh(k=ENVS, size=11):
    from gnn_hex_amd.multi_env_manager import Env_manager
    mgr = Env_manager(k, size, gamma=0.97, n_steps=[2])
    mgr.reset()
    return mgr


def _rings(ro):
    """What a run leaves on the device: vertices, ranks, result words and all board snapshots, as copies."""
    return tuple(t.clone() for t in (ro.vert, ro.rank, ro.result, ro.adj, ro.alive))


def _same_rings(a, b, tag):
    for name, x, y in zip(("vertices", "ranks", "result words", "adjacency snapshots", "alive snapshots"), a, b):
        assert torch.equal(x, y), "%s: %s differ" % (tag, name)


def _judge_move(hexref, o, history, rank, tag):
    """Move ``rank`` at the position reached by ``history`` (vertices from the start) against the float64 oracle: within 2 B."""
    game = hexref.RefGame(11)
    for v in history:
        game.make_move(int(v), remove_dead_and_captured=True)
    x, ei, bv, ptr, bm = oracle_batch([game])
    with torch.no_grad():
        a64 = o["ref64"](x.double(), ei, bv, ptr, advantages_only=True).reshape(-1)
        a32 = o["ref"](x, ei, bv, ptr, advantages_only=True).reshape(-1)
    B = _bound(a32, a64)
    assert 2 <= rank < x.shape[0]
    top = a64[2:].max().item()
    assert a64[rank].item() >= top - 2 * B, "%s: picked A64 %.6f, max %.6f, B %.3g" % (tag, a64[rank].item(), top, B)
    return int(bm[rank])


@pytest.mark.parametrize("kind", ["float", "schedule"])
def test_captured_rollout_construction_and_first_replays(hexref, kind):
    from gnn_hex_amd.data import Batch
    from gnn_hex_amd.multi_env_manager import DeviceRollout
    from gnn_hex_amd.observation import prefix_offsets
    o = _case(hexref, "L", "maker")["oracle"]
    hip = _hip_model("L", o["ref"])
    a, twin, loop = _fresh(), _fresh(), _fresh()
    start_sizes = a._sizes.copy()
    assert start_sizes[:, 0].tolist() == [123] * ENVS
    ro = DeviceRollout(a, hip, steps=2, eps=_eps(kind, 0.0), graph=True)
    assert ro._graph is not None

    # after construction, before any run: the warm-up and the capture left nothing behind
    sa, sb = a._state(), twin._state()
    assert set(sa) == set(sb)
    for key in sa:
        assert np.array_equal(sa[key], sb[key]), "after construction: %s differs from a freshly reset manager's" % key
    assert np.array_equal(a._sizes, start_sizes) and a.global_onturn == "m" and ro.frames_issued == 0 and ro._run_no == 0
    if kind == "schedule":
        assert int(ro.frames.item()) == 0
    else:
        assert ro.frames is None
    ro.obs.set_offsets(a._sizes)
    want = prefix_offsets(start_sizes[:, 0], start_sizes[:, 1])
    assert np.array_equal(ro.obs.node_off.cpu().numpy(), want[0]) and np.array_equal(ro.obs.edge_off.cpu().numpy(), want[1])

    eager = DeviceRollout(twin, hip, steps=2, eps=_eps(kind, 0.0), graph=False)
    first, history = None, []
    obs = loop.observe()
    for run in range(2):                          # the second run starts from the first run's boards
        res = ro.run()                            # (raises on an error word)
        got = _rings(ro)
        assert not got[2][:, :, 4].any()
        eager.run()
        _same_rings(got, _rings(eager), "%s run %d, captured against eager" % (kind, run))
        if run == 0:
            first = got
        # the public step-by-step loop (tests/test_gpu_env.py::test_device_rollout_equals_step_by_step_loop)
        for t in range(2):
            bt = Batch.from_data_list(obs)
            with torch.no_grad():
                adv = hip(bt.x, bt.edge_index, bt.batch, bt.ptr, advantages_only=True)
            vert, rank, _ = loop.select_actions(adv, obs, eps=0.0)
            assert vert.cpu().tolist() == res.vertices[t].tolist(), "run %d step %d" % (run, t)
            assert rank.cpu().tolist() == res.actions[t].tolist()
            assert obs.node_off == res.states[t].node_off and obs.edge_off == res.states[t].edge_off
            assert torch.equal(obs.snapshot()[0], res.states[t].snapshot()[0])
            assert torch.equal(obs.snapshot()[1], res.states[t].snapshot()[1])
            obs, rew, dones, _ = loop.step(vert)
            assert rew.tolist() == res.rewards[t].tolist() and dones.tolist() == res.dones[t].tolist()
        # identical boards and weights: every env plays the same two moves
        assert (res.vertices == res.vertices[:, :1]).all() and (res.actions == res.actions[:, :1]).all()
        assert not res.exploratories.any() and not res.dones.any()
        # move 0 against the float64 oracle on the oracle's own position
        v0 = _judge_move(hexref, o, history, int(res.actions[0, 0]), "%s run %d move 0" % (kind, run))
        assert v0 == int(res.vertices[0, 0])
        history += [int(res.vertices[0, 0]), int(res.vertices[1, 0])]
        sa, sb = a._state(), loop._state()
        for key in ("adj", "alive", "maker_turn", "total_moves"):
            assert np.array_equal(sa[key], sb[key]), key
        assert (a._sizes == loop._sizes).all()
    if kind == "schedule":
        assert int(ro.frames.item()) == 2 * 2 * ENVS == ro.frames_issued

    # the first run again with something else queued first on the same stream
    b = _fresh()
    rq = DeviceRollout(b, hip, steps=2, eps=_eps(kind, 0.0), graph=True)
    junk = torch.randn(4096, 4096, device=DEV) @ torch.randn(4096, 4096, device=DEV)
    rq.run()
    assert junk.isfinite().all()
    _same_rings(_rings(rq), first, "%s: the first run behind a queued matmul" % kind)


# ---- 4. a 16-move rollout replayed on the oracle env ----------------------------------------------------------------------------------

JUDGED = [0, 1, 2, 3, ENVS - 4, ENVS - 3, ENVS - 2, ENVS - 1]
RUNS = 6


@pytest.mark.parametrize("kind", ["float", "schedule"])
def test_sixteen_moves_replayed_on_the_oracle_env(hexref, kind):
    from gnn_hex_amd.multi_env_manager import DeviceRollout
    o = _case(hexref, "L", "maker")["oracle"]
    hip = _hip_model("L", o["ref"])
    mgr = _fresh()
    T, size = 16, 11
    ro = DeviceRollout(mgr, hip, steps=T, eps=_eps(kind, 0.12, 0.05, 100000), graph=True)
    torch.manual_seed(16)
    games = [hexref.RefGame(size) for _ in range(ENVS)]
    judged = tight = explored = finished = 0
    for run in range(RUNS):                       # run 0 is the judged one; the later ones play on until games end and reset
        res = ro.run()
        words = ro.result.cpu().numpy()
        assert not words[:, :, 4].any()
        maker = True
        for t in range(T):
            sel = [i for i in JUDGED if not res.exploratories[t, i]] if run == 0 else []
            if sel:
                x, ei, bv, ptr, _ = oracle_batch([games[i] for i in sel])
                assert bool((x[:, 2] == (1.0 if maker else 0.0)).all())
                with torch.no_grad():
                    q64 = o["ref64"](x.double(), ei, bv, ptr, advantages_only=True).reshape(-1).numpy()
                ptr = ptr.tolist()
            for i in range(ENVS):
                g = games[i]
                v, rank = int(res.vertices[t, i]), int(res.actions[t, i])
                where = "run %d env %d step %d" % (run, i, t)
                assert g.maker_turn == maker, where
                assert v in g.get_actions().tolist(), "%s: illegal move %d" % (where, v)
                assert int(g.observe()[2][rank]) == v, "%s: rank %d is not vertex %d in the oracle's observation" % (where, rank, v)
                explored += bool(res.exploratories[t, i])
                if i in sel:
                    j = sel.index(i)
                    qa = q64[ptr[j] + 2:ptr[j + 1]]
                    assert qa[rank - 2] >= qa.max() - 2e-4, "%s: picked q64 %.6f, max %.6f" % (where, qa[rank - 2], qa.max())
                    judged += 1
                    if len(qa) > 1:
                        top = np.sort(qa)[-2:]
                        tight += bool(top[1] - top[0] < 2e-4)
                g.make_move(v, remove_dead_and_captured=True)
                w = g.who_won()
                assert int(words[t, i, 1]) == g.total_num_moves, "%s: move count" % where
                if w is not None:
                    finished += 1
                    assert int(words[t, i, 0]) == (0 if w == "m" else 1) and bool(res.dones[t, i]), where
                    assert res.infos[t][i]["episode_metrics"]["length"] == g.total_num_moves, where
                    g = games[i] = hexref.RefGame(size)        # auto reset, on the side everyone moves to next
                    g.maker_turn = not maker
                else:
                    assert int(words[t, i, 0]) == -1 and not res.dones[t, i], where
                assert (int(words[t, i, 2]), int(words[t, i, 3])) == (g.num_vertices(), 2 * g.num_edges()), "%s: sizes" % where
            maker = not maker
        if run == 0:
            assert judged > 0 and 0 < explored < T * ENVS
            print("eps as %s: %d plies of 8 envs judged by the float64 oracle, %d with a float64 top-2 gap below 2e-4; %d of %d "
                  "moves exploratory" % (kind, judged, tight, explored, T * ENVS))
    print("eps as %s: %d games finished and reset in %d runs of %d moves" % (kind, finished, RUNS, T))
    assert finished > 0, "no game ended: winner, length and auto reset were not exercised"
    # the boards the rollout left are the oracle's
    st = mgr._state()
    for i in range(ENVS):
        adj, alive = games[i].dump()
        assert np.array_equal(st["alive"][i], alive) and np.array_equal(st["adj"][i], adj), "env %d: final board" % i


# ---- 5. the example in a fresh process (last in the file) ------------------------------------------------------------------------------

def _example(extra, timeout):
    """One child process of examples/selfplay_train.py with the default GNN-L arguments.  No retry: an ``illegal action`` here is
    a finding to explain.  A fault, an abort or a hang of the child ends the session: nothing else starts on the GPU after it."""
    cmd = [sys.executable, os.path.join("examples", "selfplay_train.py"), "--iters", "2", "--warm", "1"] + extra
    try:
        r = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=timeout)
    except subprocess.TimeoutExpired as err:
        out = err.stdout.decode(errors="replace") if isinstance(err.stdout, bytes) else (err.stdout or "")
        pytest.exit("examples/selfplay_train.py %s did not end within %d s (a hang):\n%s"
                    % (" ".join(extra), timeout, out[-2000:]), returncode=1)
    if r.returncode < 0 or r.returncode in (124, 134, 137, 139):
        pytest.exit("examples/selfplay_train.py %s ended with status %d:\n%s" % (" ".join(extra), r.returncode, r.stdout[-2000:]),
                    returncode=1)
    assert r.returncode == 0, r.stdout[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert lines and "env frames/s" in lines[-1] and lines[-1].startswith("hex 11, 128 envs, GNN 15x110"), r.stdout[-3000:]
    print(lines[-1])


TIMEOUT_PLAIN, TIMEOUT_STORE = 50, 50      # ten times the measured 4.2 s and 4.0 s, rounded up to the next ten


def test_example_in_a_fresh_process():
    """``--iters 2 --warm 1``: 4.2 s measured on the parent commit (4.2 .. 4.5 s under pytest); the timeout, ten times that rounded up
    to the next ten seconds, is a guard against a hang, not a speed assertion."""
    _example([], timeout=TIMEOUT_PLAIN)


def test_example_with_device_store_and_schedule_in_a_fresh_process():
    """``--iters 2 --warm 1 --device-store --eps-schedule 0.12,0.05,100000``: 4.0 s measured on the parent commit (4.1 .. 4.5 s under
    pytest); the timeout as above."""
    _example(["--device-store", "--eps-schedule", "0.12,0.05,100000"], timeout=TIMEOUT_STORE)
