"""GPU: search self-play (gnn_hex_amd/csrc/search_selfplay.hip, gnn_hex_amd/search_selfplay.py, ops.PolicyValueLossFn) against
the host oracle of tests/selfplay_oracle.py.  Trees are grown with the synthetic evaluator on real positions (test_gpu_search.Rig,
teacher-forced, so the oracle tree is checked on the way) and the expectations are computed from the DEVICE tree read back with
TreeSearch.tree(): the integers are exact and no share of cases needs leaving out.  Then the end-to-end loop: a self-play match
whose samples are the replayed positions, a training run on one batch, and a search player after training.
Boards: Hex-2 with 3 games (the smallest trees), Hex-3 with 1 (a single game), Hex-5 with 70 (ranks cross a 64-lane trip), Hex-9
with 3 (81 edges: more than 64 lanes), Hex-12 with 3 (nv > 128, three words), Hex-14 with 3 (four words, 196 edges) and Hex-16
with 2 (five words: the run-time word count; 256 edges, exactly four lane trips); 12 simulations each."""
import numpy as np
import pytest
import torch

import selfplay_oracle as spo
import test_gpu_search as tgs
from helpers import rel_bound

pytestmark = pytest.mark.gpu

DEV = "cuda"
GUARD = 4096
CASES = [(2, 3), (3, 1), (5, 70), (9, 3), (12, 3), (14, 3), (16, 2)]
SIMS = 12
POISON = 77
_RIGS = {}


def grown(hexref, size, G, sims=SIMS):
    """The case's rig after ``sims`` simulations, built once; tests leave its tree as they found it."""
    key = (size, G, sims)
    if key not in _RIGS:
        rig = tgs.Rig(hexref, size, G, sims)
        for s in range(sims):
            rig.sim(s, tgs._synthetic(size), check_env=False)
        rig.compare_trees()
        _RIGS[key] = rig
    return _RIGS[key]


def poisoned_buffer(capacity, size):
    """A SearchSampleBuffer whose arrays are POISON everywhere and are each followed by a poisoned guard."""
    from gnn_hex_amd.search_selfplay import SearchSampleBuffer
    buf = SearchSampleBuffer(capacity, size, DEV)
    buf._guards = {}
    for name in ("policy", "root_q", "z", "adj", "alive", "side", "sizes", "meta"):
        t = getattr(buf, name)
        big = torch.full((t.numel() + GUARD,), POISON, dtype=t.dtype, device=DEV)
        setattr(buf, name, big[:t.numel()].view(t.shape))
        buf._guards[name] = big
    return buf


def guards_intact(buf):
    for name, big in buf._guards.items():
        assert (big[getattr(buf, name).numel():] == POISON).all(), "the guard behind %s was written" % name


def set_head(buf, value):
    buf.head.fill_(value)
    buf._head = value


def ring(buf):
    return {n: getattr(buf, n).cpu().numpy() for n in ("policy", "root_q", "z", "adj", "alive", "side", "sizes", "meta")}


# ---- root noise -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size,G", CASES)
def test_root_noise(hexref, size, G):
    rig = grown(hexref, size, G)
    sr, A = rig.search, size * size
    ws = sr.workspace_bytes
    save = rig.big[:ws].clone()

    def restore():
        rig.big[:ws].copy_(save)               # the workspace alone: the guard behind it keeps whatever a call left there

    def noise_call(eps, nz_t, act_t):
        sr.apply_root_noise(eps, nz_t, act_t)
        assert (rig.big[ws:] == 0xA5).all(), "the guard behind the workspace was written"

    t0 = sr.tree()
    gen = torch.Generator(device=DEV)
    gen.manual_seed(100 + size)
    noise = torch._standard_gamma(torch.full((G, A), 0.2, dtype=torch.float32, device=DEV), generator=gen)
    noise = noise.clamp_min(1e-6).contiguous()          # a Gamma(0.2) draw can underflow to 0: keep every row's sum positive
    nz = noise.cpu().numpy()
    act = [int(g != 1) for g in range(G)]
    active = torch.tensor(act, dtype=torch.int32, device=DEV)
    worst = 0.0

    def others_untouched(t1):
        for name in ("ns", "ne", "cnt", "W", "N", "child", "vertex"):
            assert np.array_equal(t0[name], t1[name]), name
        assert t0["P"][:, 1:].tobytes() == t1["P"][:, 1:].tobytes(), "a prior below the root changed"

    for eps in (0.25, 0.0, 1.0):
        restore()
        noise_call(eps, noise, active)
        t1 = sr.tree()
        others_untouched(t1)
        for g in range(G):
            ne = int(t0["ne"][g, 0])
            p0, p1 = t0["P"][g, 0], t1["P"][g, 0]
            assert p0[ne:].tobytes() == p1[ne:].tobytes()
            if not act[g] or eps == 0.0:
                assert p0.tobytes() == p1.tobytes(), "Hex-%d game %d eps %g: the priors changed" % (size, g, eps)
                continue
            want = spo.root_noise64(p0[:ne], nz[g, :ne], eps)
            rel = float((np.abs(p1[:ne].astype(np.float64) - want) / want).max())
            worst = max(worst, rel)
            assert rel <= 1e-6, "Hex-%d game %d eps %g: P off by %.3g relative" % (size, g, eps, rel)
            if eps == 1.0:
                assert abs(p1[:ne].astype(np.float64).sum() - 1) <= 1e-5
        assert int(sr._status.item()) == 0
    print("Hex-%d G=%d: root noise worst relative error %.3g" % (size, G, worst))
    # refused noise: a zero row, a NaN entry, a negative entry, an infinite entry -- the game's priors stay, bit 16 is set
    for kind in range(4):
        g = kind % G
        ne = int(t0["ne"][g, 0])
        bad = noise.clone()
        if kind == 0:
            bad[g, :ne] = 0.0
        else:
            bad[g, ne // 2] = (float("nan"), -0.5, float("inf"))[kind - 1]
        restore()
        noise_call(0.25, bad, None)
        t1 = sr.tree()
        others_untouched(t1)
        assert t0["P"][g, 0].tobytes() == t1["P"][g, 0].tobytes(), "kind %d: refused noise changed the priors" % kind
        for h in range(G):
            if h != g and int(t0["ne"][h, 0]) > 1:          # (a single edge keeps its prior of 1 under any noise)
                assert t0["P"][h, 0].tobytes() != t1["P"][h, 0].tobytes(), "kind %d: game %d got no noise" % (kind, h)
        assert int(sr._status.item()) == 16
        sr._status.zero_()
    # entries behind the root's edges are never read
    g = G - 1
    ne = int(t0["ne"][g, 0])
    if ne < A:
        bad = noise.clone()
        bad[g, ne:] = float("nan")
        restore()
        noise_call(0.25, noise, None)
        want = sr.tree()["P"]
        restore()
        noise_call(0.25, bad, None)
        assert sr.tree()["P"].tobytes() == want.tobytes() and int(sr._status.item()) == 0
    # an unexpanded root is left alone
    sr.reset()
    before = rig.big.clone()
    noise_call(0.25, noise, None)
    assert torch.equal(rig.big, before) and int(sr._status.item()) == 0
    restore()
    assert (rig.big[ws:] == 0xA5).all(), "the guard behind the workspace was written"
    with pytest.raises(ValueError):
        sr.add_root_noise(1.5, 0.2)
    rig.finish()


def test_add_root_noise_draws_gamma(hexref):
    """TreeSearch.add_root_noise: the draws it returns are the ones it applied, and simulate(root_noise=...) applies them once,
    behind the simulation that expands the root."""
    from gnn_hex_amd.search import UniformEvaluator
    rig = grown(hexref, 5, 70)
    sr = rig.search
    save = rig.big[:sr.workspace_bytes].clone()
    gen = torch.Generator(device=DEV)
    gen.manual_seed(9)
    t0 = sr.tree()
    noise = sr.add_root_noise(0.25, 0.2, generator=gen).cpu().numpy()
    status = int(sr._status.item())          # a row of Gamma(0.2) draws may underflow to zeros: then the game is refused
    sr._status.zero_()
    t1 = sr.tree()
    assert noise.shape == (70, 25) and (noise >= 0).all() and status in (0, 16)
    for g in range(70):
        ne = int(t0["ne"][g, 0])
        want = spo.root_noise64(t0["P"][g, 0, :ne], noise[g, :ne], 0.25)
        if want is None:
            assert t0["P"][g, 0].tobytes() == t1["P"][g, 0].tobytes() and status == 16
        else:
            assert (np.abs(t1["P"][g, 0, :ne] - want) / want).max() <= 1e-6
    sr.reset()
    sr.simulate(rig.mgr._h, UniformEvaluator(), 3, root_noise=(0.5, 0.3), generator=gen)
    sr._status.zero_()
    t2 = sr.tree()
    ne = int(t2["ne"][0, 0])
    assert ne == 25 and len(np.unique(t2["P"][0, 0, :ne])) > 1, "uniform priors stayed uniform: no noise was applied"
    assert abs(float(t2["P"][0, 0, :ne].astype(np.float64).sum()) - 1) <= 1e-5
    assert all(len(np.unique(t2["P"][0, n, :int(t2["ne"][0, n])])) == 1 for n in (1, 2)), "noise below the root"
    rig.big[:sr.workspace_bytes].copy_(save)       # (the workspace alone: the guard keeps what the calls left)
    rig.finish()


# ---- record -----------------------------------------------------------------------------------------------------------
def check_record(rig, buf, before, head, ply, mode, u, act, pick):
    """One hexgnn_search_record call's outputs against the device tree."""
    sr, size, G = rig.search, rig.size, rig.G
    A, cap = size * size, buf.capacity
    t = sr.tree()
    after = ring(buf)
    obs = rig.mgr.observe()
    scores = sr.root(obs).cpu().numpy()
    rank, written = 0, set()
    for g in range(G):
        ns, ne = int(t["ns"][g, 0]), int(t["ne"][g, 0])
        what = "Hex-%d game %d mode %d" % (size, g, mode)
        if not act[g] or ns < 2:
            assert pick[g] == -1, what
            continue
        slot = (head + rank) % cap
        rank += 1
        written.add(slot)
        N, moves = t["N"][g, 0, :ne], t["vertex"][g, 0, :ne].astype(np.int64)
        assert int(N.sum()) == ns - 1
        row = spo.visit_policy(moves, N, A)
        assert after["policy"][slot].tobytes() == row.tobytes(), "%s: the policy row is not N / T bit for bit" % what
        assert abs(float(after["policy"][slot].astype(np.float64).sum()) - 1) <= 1e-6, what
        want_q = scores[obs.node_off[g]]
        assert after["root_q"][slot].tobytes() == want_q.tobytes(), "%s: root_q %r, TreeSearch.root %r" % (what, after["root_q"][slot], want_q)
        assert np.array_equal(after["adj"][slot], rig.root_before[0][g]), "%s: adjacency" % what
        assert np.array_equal(after["alive"][slot], rig.root_before[1][g]), "%s: alive" % what
        assert after["side"][slot] == rig.root_before[2][g], what
        game = rig.games[g]
        assert tuple(after["sizes"][slot]) == (game.num_vertices(), 2 * game.num_edges()), what
        assert tuple(after["meta"][slot]) == (g, ply) and after["z"][slot] == 0, what
        e = spo.proportional_pick(N, u[g]) if mode == 1 else spo.greedy_pick(N)
        assert pick[g] == moves[e], "%s: pick %d, oracle %d (N %s, u %r)" % (what, pick[g], moves[e], N, u[g])
        if mode == 0:
            assert pick[g] == rig.trees[g].best()
    for name in after:                                       # every other slot is as it was
        rest = np.array([s not in written for s in range(cap)])
        assert np.array_equal(after[name][rest], before[name][rest]), "%s: a slot that holds no sample was written" % name
    assert int(buf.head.item()) == head + rank and int(buf.recorded.item()) == rank
    guards_intact(buf)
    return rank


@pytest.mark.parametrize("size,G", CASES)
def test_record(hexref, size, G):
    rig = grown(hexref, size, G)
    sr, A = rig.search, size * size
    cap = G * A
    buf = poisoned_buffer(cap, size)
    gen = torch.Generator(device=DEV)
    gen.manual_seed(7 * size)
    pick = torch.full((G,), -5, dtype=torch.int32, device=DEV)
    every_second = [int(g % 2 == 0) for g in range(G)]
    total = 0
    last_u = float(np.nextafter(np.float32(1), np.float32(0)))
    # (head, ply, mode, u, active): seeded uniforms with every second game resting; the greedy pick; a head that wraps the ring;
    # the two edge values of u
    plan = [(3, 0, 1, torch.rand(G, generator=gen, device=DEV), every_second),
            (3 + cap, 4, 0, None, None),
            (cap - 1, 7, 1, torch.rand(G, generator=gen, device=DEV), None),
            (2 * cap - 1, 8, 1, torch.zeros(G, device=DEV), None),
            (5, 9, 1, torch.full((G,), last_u, device=DEV), None)]
    for head, ply, mode, u, act in plan:
        set_head(buf, head)
        before = ring(buf)
        active = torch.tensor(act, dtype=torch.int32, device=DEV) if act is not None else None
        buf.record(rig.mgr._h, sr, ply, mode, u, pick, active)
        uh = u.cpu().numpy() if u is not None else np.zeros(G, np.float32)
        got = check_record(rig, buf, before, head, ply, mode, uh, act if act is not None else [1] * G, pick.cpu().numpy())
        assert got == (sum(act) if act is not None else G)
        total += got
    # u = 0 lands on the first visited edge, the largest fp32 below 1 on the last
    t = sr.tree()
    for g in range(G):
        ne = int(t["ne"][g, 0])
        visited = np.nonzero(t["N"][g, 0, :ne])[0]
        assert int(pick[g]) == int(t["vertex"][g, 0, visited[-1]])
    assert total > 0
    rig.finish()


def test_record_without_a_visit_records_nothing(hexref):
    """One simulation only expands the root (T = 0), and a reset tree has no root: neither is a sample, in either pick mode."""
    rig = grown(hexref, 5, 3, sims=1)
    sr = rig.search
    buf = poisoned_buffer(75, 5)
    pick = torch.full((3,), -5, dtype=torch.int32, device=DEV)
    u = torch.full((3,), 0.5, device=DEV)
    save = rig.big[:sr.workspace_bytes].clone()
    for tree in ("expanded", "reset"):
        if tree == "reset":
            sr.reset()
        ns = sr.tree()["ns"][:, 0]
        assert (ns == (1 if tree == "expanded" else 0)).all()
        for mode in (0, 1):
            set_head(buf, 11)
            before = ring(buf)
            pick.fill_(-5)
            buf.record(rig.mgr._h, sr, 0, mode, u, pick)
            after = ring(buf)
            assert (pick.cpu().numpy() == -1).all(), (tree, mode)
            assert int(buf.head.item()) == 11 and int(buf.recorded.item()) == 0, (tree, mode)
            assert all(np.array_equal(before[n], after[n]) for n in before), (tree, mode)
    rig.big[:sr.workspace_bytes].copy_(save)
    assert (sr.tree()["ns"][:, 0] == 1).all()
    guards_intact(buf)
    rig.finish()


# ---- finish -----------------------------------------------------------------------------------------------------------
def test_samples_finish():
    from gnn_hex_amd import _lib
    buf = poisoned_buffer(20, 3)
    game = torch.tensor([[0, 5, 5, 0], [1, 4, 4, 0], [-1, 0, 3, 0]], dtype=torch.int32, device=DEV)
    # slots 18, 19, 0, 1, 2, 3: games 0, 0, 1, 1, 2, 0 with sides 1, 0, 1, 0, 1, 1
    slots, games, sides = [18, 19, 0, 1, 2, 3], [0, 0, 1, 1, 2, 0], [1, 0, 1, 0, 1, 1]
    for s, g, sd in zip(slots, games, sides):
        buf.meta[s, 0], buf.meta[s, 1], buf.side[s] = g, s, sd
    set_head(buf, 38)
    buf.head.fill_(44)
    with pytest.raises(_lib.HexGnnError, match="undecided"):
        buf.finish(game)
    z = buf.z.cpu().numpy()
    want = {18: 1.0, 19: -1.0, 0: -1.0, 1: 1.0, 3: 1.0}
    for s, v in want.items():
        assert z[s] == v == spo.z_label(int(game[games[slots.index(s)], 0]), sides[slots.index(s)]), "slot %d" % s
    assert np.isnan(z[2])
    rest = np.array([s not in slots for s in range(20)])
    assert (z[rest] == POISON).all(), "a slot outside the range was labelled"
    # the refused samples are discarded, and with them the six older samples whose slots they took: samples 24 .. 37 are left,
    # in slots 4 .. 17
    assert buf._head == 38 and buf.pending() == 0 and len(buf) == 14 and int(buf._status.item()) == 0
    assert buf._slots_of(torch.arange(14, device=DEV)).tolist() == list(range(4, 18))
    # a game index that leaves the record is an undecided game as well
    buf.meta[4, 0] = 3
    set_head(buf, 44)
    buf.head.fill_(45)
    with pytest.raises(_lib.HexGnnError):
        buf.finish(game)
    assert np.isnan(float(buf.z[4])) and float(buf.z[5]) == POISON
    buf.head.fill_(50)
    buf.discard_pending()
    assert buf.pending() == 0
    guards_intact(buf)


# ---- loss -------------------------------------------------------------------------------------------------------------
def loss_case(b, seed, size=12, cap=97):
    """b graphs of 3 .. 146 observation rows on Hex-12 cells, log-softmaxed random logits, ring targets with zeros."""
    rng = np.random.default_rng(seed)
    cells = size * size
    nrows = rng.integers(3, 147, b)
    nrows[0], nrows[-1] = 3, 146
    if b > 2:
        nrows[1] = 66 + 2                                     # one lane trip and two rows
    gptr = np.concatenate([[0], np.cumsum(nrows)]).astype(np.int32)
    out_ptr = np.concatenate([[0], np.cumsum(nrows - 2)]).astype(np.int64)
    backmap = np.zeros(gptr[-1], dtype=np.int64)
    index = rng.choice(cap, b, replace=b > cap).astype(np.int32)
    policy = rng.random((cap, cells)).astype(np.float32)     # junk everywhere: only a graph's own cells are read
    logp, target = [], []
    for g in range(b):
        k = int(nrows[g] - 2)
        mine = np.sort(rng.choice(cells, k, replace=False))
        backmap[gptr[g]:gptr[g] + 2] = (0, 1)
        backmap[gptr[g] + 2:gptr[g + 1]] = mine + 2
        t = rng.random(k) * (rng.random(k) < 0.5)
        t[int(rng.integers(0, k))] += 0.25
        if g % 3 == 1 and k >= 4:                              # first-index ties of the target's maximum
            t[[1, 3]] = t.max() + 0.5
        t = (t / t.sum()).astype(np.float32)
        policy[index[g], mine] = t
        lg = rng.standard_normal(k) * 2
        if g % 3 == 2 and k >= 4:                              # and of the log-policy's
            lg[[0, 2]] = lg.max() + 1.0
        lp = torch.log_softmax(torch.from_numpy(lg.astype(np.float32)), 0).numpy()
        logp.append(lp)
        target.append(t)
    value = np.tanh(rng.standard_normal(b)).astype(np.float32)
    z = np.full(cap, np.nan, dtype=np.float32)
    root_q = np.full(cap, np.nan, dtype=np.float32)
    z[index] = rng.choice([-1.0, 1.0], b)
    root_q[index] = np.tanh(rng.standard_normal(b))
    return dict(b=b, size=size, cap=cap, gptr=gptr, out_ptr=out_ptr, backmap=backmap, index=index, policy=policy, logp=logp,
                target=target, value=value, z=z, root_q=root_q)


def run_loss(c, q_ratio, vf, pf, out_ptr=None, backmap=None):
    from gnn_hex_amd import ops
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)       # noqa: E731
    logp = d(np.concatenate(c["logp"])).requires_grad_()
    value = d(c["value"]).requires_grad_()
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    loss, per = ops.PolicyValueLossFn.apply(logp, value, d(c["out_ptr"] if out_ptr is None else out_ptr), d(c["gptr"]),
                                            d(c["backmap"] if backmap is None else backmap), d(c["policy"]), d(c["z"]),
                                            d(c["root_q"]), d(c["index"]), c["size"], q_ratio, vf, pf, status)
    loss.backward()
    return loss.detach().cpu(), per.cpu(), logp.grad.cpu(), value.grad.cpu(), int(status.item())


def torch32(c, q_ratio, vf, pf):
    """torch's fp32 evaluation of the reference expression (CPU): loss, ce and se per graph, both gradients."""
    logp = [torch.from_numpy(l).requires_grad_() for l in c["logp"]]
    value = torch.from_numpy(c["value"]).requires_grad_()
    z, rq = torch.from_numpy(c["z"][c["index"]]), torch.from_numpy(c["root_q"][c["index"]])
    y = (1 - q_ratio) * z + q_ratio * rq
    ce = torch.stack([torch.sum(-torch.from_numpy(t) * l) for t, l in zip(c["target"], logp)])
    se = (value - y) ** 2
    loss = vf * torch.nn.MSELoss()(value, y) * c["b"] + pf * ce.sum()
    loss.backward()
    return loss.detach(), ce.detach(), se.detach(), torch.cat([l.grad for l in logp]), value.grad


@pytest.mark.parametrize("b", [1, 3, 70])
@pytest.mark.parametrize("q_ratio,vf,pf", [(0.0, 1.0, 1.0), (0.5, 0.01, 0.99)])
def test_pv_loss(b, q_ratio, vf, pf):
    c = loss_case(b, 40 + b)
    tag = "b=%d q_ratio=%g" % (b, q_ratio)
    loss, per, d_logp, d_value, status = run_loss(c, q_ratio, vf, pf)
    idx = c["index"]
    l64, per64, dl64, dv64 = spo.pv_loss(c["logp"], c["target"], c["value"], c["z"][idx], c["root_q"][idx], q_ratio, vf, pf)
    l32, ce32, se32, dl32, dv32 = torch32(c, q_ratio, vf, pf)
    t64 = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float64))     # noqa: E731
    assert status == 0
    figures = [rel_bound(tag, "loss", loss.reshape(1), l32.reshape(1), t64([l64])),
               rel_bound(tag, "ce", per[:, 0], ce32, t64(per64[:, 0])),
               rel_bound(tag, "se", per[:, 1], se32, t64(per64[:, 1])),
               rel_bound(tag, "d_logp", d_logp, dl32, t64(dl64)),
               rel_bound(tag, "d_value", d_value, dv32, t64(dv64))]
    print("%s: (kernel, torch fp32) relative to float64: %s" % (tag, ["%.2g / %.2g" % f for f in figures]))
    assert np.array_equal(per[:, 2].numpy(), per64[:, 2]), "%s: policy argmax hits" % tag
    assert np.array_equal(per[:, 3].numpy(), per64[:, 3]), "%s: value sign hits" % tag
    # the same inputs, the same bits
    again = run_loss(c, q_ratio, vf, pf)
    for a, bb in zip((loss, per, d_logp, d_value), again[:4]):
        assert a.numpy().tobytes() == bb.numpy().tobytes(), "%s: two runs differ" % tag
    # the incoming scalar scales both gradients
    from gnn_hex_amd import ops
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)       # noqa: E731
    lp, v = d(np.concatenate(c["logp"])).requires_grad_(), d(c["value"]).requires_grad_()
    out = ops.PolicyValueLossFn.apply(lp, v, d(c["out_ptr"]), d(c["gptr"]), d(c["backmap"]), d(c["policy"]), d(c["z"]),
                                      d(c["root_q"]), d(c["index"]), c["size"], q_ratio, vf, pf,
                                      torch.zeros(1, dtype=torch.int32, device=DEV))
    (out[0] * 3.0).backward()
    assert torch.equal(lp.grad.cpu(), d_logp * 3.0) and torch.equal(v.grad.cpu(), d_value * 3.0)


def test_pv_loss_guards():
    c = loss_case(3, 5)
    base = run_loss(c, 0.0, 1.0, 1.0)
    # graph 1's rows disagree with out_ptr (graph 0's then do as well): bit 64, zeros for both, graph 2 as before
    bad_ptr = c["out_ptr"].copy()
    bad_ptr[1] += 1
    loss, per, d_logp, d_value, status = run_loss(c, 0.0, 1.0, 1.0, out_ptr=bad_ptr)
    assert status == 64
    assert (per[:2] == 0).all() and (d_value[:2] == 0).all() and (d_logp[:c["out_ptr"][2]] == 0).all()
    assert torch.equal(per[2], base[1][2]) and d_value[2] == base[3][2]
    assert torch.equal(d_logp[c["out_ptr"][2]:], base[2][c["out_ptr"][2]:])
    assert abs(float(loss) - float(base[1][2, 0] + base[1][2, 1])) <= 1e-6 * abs(float(loss))
    # a slot outside the ring: the same guard
    far = dict(c, index=np.array([c["index"][0], c["cap"], c["index"][2]], dtype=np.int32))
    far["z"], far["root_q"] = c["z"], c["root_q"]
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)       # noqa: E731
    from gnn_hex_amd import ops
    status_t = torch.zeros(1, dtype=torch.int32, device=DEV)
    _, per2 = ops.PolicyValueLossFn.apply(d(np.concatenate(c["logp"])), d(c["value"]), d(c["out_ptr"]), d(c["gptr"]),
                                          d(c["backmap"]), d(c["policy"]), d(c["z"]), d(c["root_q"]), d(far["index"]), c["size"],
                                          0.0, 1.0, 1.0, status_t)
    assert int(status_t.item()) == 64 and (per2[1] == 0).all() and torch.equal(per2[0].cpu(), base[1][0])
    # tensors the kernel would misread are refused before the call
    args = [d(np.concatenate(c["logp"])), d(c["value"]), d(c["out_ptr"]), d(c["gptr"]), d(c["backmap"]), d(c["policy"]),
            d(c["z"]), d(c["root_q"]), d(c["index"]), c["size"], 0.0, 1.0, 1.0, status_t]
    for pos, wrong in ((6, args[6].double()), (7, args[7][:-1]), (6, torch.stack([args[6], args[6]], 1)[:, 0]),
                       (4, torch.stack([args[4], args[4]], 1)[:, 0]), (13, status_t.long()), (7, args[7].cpu())):
        broken = list(args)
        broken[pos] = wrong
        with pytest.raises(ValueError):
            ops.PolicyValueLossFn.apply(*broken)
    # a row whose cell lies outside the board contributes nothing: the row of graph 2 with the lowest log-policy
    g = 2
    j = int(np.argmin(c["logp"][g]))
    bm = c["backmap"].copy()
    bm[c["gptr"][g] + 2 + j] = c["size"] ** 2 + 2 + 5
    loss3, per3, d_logp3, _, status3 = run_loss(c, 0.0, 1.0, 1.0, backmap=bm)
    tg = [t.copy() for t in c["target"]]
    tg[g][j] = 0
    idx = c["index"]
    _, per64, dl64, _ = spo.pv_loss(c["logp"], tg, c["value"], c["z"][idx], c["root_q"][idx], 0.0, 1.0, 1.0)
    assert status3 == 0 and d_logp3[c["out_ptr"][g] + j] == 0
    assert abs(float(per3[g, 0]) - per64[g, 0]) <= 1e-5 * abs(per64[g, 0])
    assert np.allclose(d_logp3.numpy(), dl64, rtol=1e-6, atol=0)


# ---- end to end -------------------------------------------------------------------------------------------------------
def _start_state(size):
    from gnn_hex_amd.multi_env_manager import Env_manager
    mgr = Env_manager(1, size)
    got = tgs._export(mgr._h, 1, size * size + 2, mgr._words)
    return got[0][0], got[1][0]


def check_match(buf, res, count, size, first, head0=0):
    """The match's samples against the replayed move log: positions, sides, legal support, labels."""
    from gnn_hex_amd.positions import replay_games
    rep = replay_games(size, res.moves, first=first, device=DEV)
    adj, alive, side = rep._adj.cpu().numpy(), rep._alive.cpu().numpy(), rep._side.cpu().numpy()
    adj0, alive0 = _start_state(size)
    r = ring(buf)
    assert count == int(res.length.sum()) and np.array_equal(rep.winner, res.winner) and np.array_equal(rep.length, res.length)
    seen = set()
    for i in range(count):
        slot = (head0 + i) % buf.capacity
        g, ply = (int(v) for v in r["meta"][slot])
        assert (g, ply) not in seen and ply < res.length[g]
        seen.add((g, ply))
        what = "game %d ply %d" % (g, ply)
        if ply == 0:
            assert np.array_equal(r["adj"][slot], adj0) and np.array_equal(r["alive"][slot], alive0), what
            assert r["side"][slot] == int(first == "m"), what
        else:
            assert np.array_equal(r["adj"][slot], adj[g, ply - 1]) and np.array_equal(r["alive"][slot], alive[g, ply - 1]), what
            assert r["side"][slot] == side[g, ply - 1], what
            assert tuple(r["sizes"][slot]) == tuple(rep.sizes[g, ply - 1]), what
        pol = r["policy"][slot]
        assert abs(float(pol.astype(np.float64).sum()) - 1) <= 1e-6, what
        legal = r["alive"][slot][2:] == 1
        assert (pol[~legal] == 0).all(), "%s: the policy puts weight on a cell that is not legal" % what
        assert pol[int(res.moves[g, ply]) - 2] > 0, "%s: the move played was never visited" % what
        assert r["z"][slot] == spo.z_label(int(res.winner[g]), int(r["side"][slot])), what
        assert -1 <= r["root_q"][slot] <= 1
    assert len(seen) == count


def test_selfplay_match_records_the_replayed_positions():
    from gnn_hex_amd.search import UniformEvaluator
    from gnn_hex_amd.search_selfplay import SearchSelfPlay
    size, G = 4, 6
    buf = poisoned_buffer(G * size * size, size)
    sp = SearchSelfPlay(size, G, UniformEvaluator(), 8, buf, proportional_plies=4)
    gen = torch.Generator(device=DEV)
    gen.manual_seed(21)
    res, count = sp.play(first="m", generator=gen)
    assert set(res.winner.tolist()) <= {0, 1} and len(buf) == count
    check_match(buf, res, count, size, "m")
    # a second match, the breaker first, behind a head five slots short of the ring's end: it wraps; the same seed plays the
    # same match again
    head0 = 2 * buf.capacity - 5
    set_head(buf, head0)
    res2, count2 = sp.play(first="b", generator=gen)
    assert len(buf) == buf.capacity and count2 > 5 and buf._head == head0 + count2
    check_match(buf, res2, count2, size, "b", head0=head0)
    guards_intact(buf)
    # an aborted match of seven samples on the full ring: the seven oldest samples are gone, and no draw lands on their slots
    buf.head.fill_(buf._head + 7)
    buf.discard_pending()
    spoiled = {(buf._head + i) % buf.capacity for i in range(7)}
    assert len(buf) == buf.capacity - 7 and buf.pending() == 0
    batch, index = buf.sample(512, generator=gen)
    drawn = set(index.tolist())
    assert not (drawn & spoiled) and len(drawn) > buf.capacity // 2 and batch.ptr.numel() == 513
    res4, count4 = sp.play(first="m", generator=gen)         # the next match goes where the aborted one went
    assert len(buf) == buf.capacity and count4 > 7
    check_match(buf, res4, count4, size, "m", head0=buf._head - count4)
    gen.manual_seed(21)
    buf2 = poisoned_buffer(G * size * size, size)
    res3, count3 = SearchSelfPlay(size, G, UniformEvaluator(), 8, buf2, proportional_plies=4).play(first="m", generator=gen)
    assert count3 == count and np.array_equal(res3.moves, res.moves)
    with pytest.raises(ValueError):
        SearchSelfPlay(size, G, UniformEvaluator(), 1, buf)
    with pytest.raises(ValueError):
        SearchSelfPlay(size, G + 1, UniformEvaluator(), 8, buf)


def test_training_on_a_matchs_samples_and_playing_on():
    from gnn_hex_amd.arena import DeviceArena
    from gnn_hex_amd.positions import replay_games
    from gnn_hex_amd.search import PolicyValueEvaluator, SearchPlayer
    from gnn_hex_amd.search_selfplay import PolicyValueUpdate, SearchSampleBuffer, SearchSelfPlay
    from gnn_hex_amd.torch_script_models import SAGE_torch_script
    size, G = 4, 6
    torch.manual_seed(3)
    model = SAGE_torch_script(16, 3, 1, 1).to(DEV)
    buf = SearchSampleBuffer(G * size * size, size, DEV)
    gen = torch.Generator(device=DEV)
    gen.manual_seed(4)
    model.eval()
    res, count = SearchSelfPlay(size, G, PolicyValueEvaluator(model), 8, buf).play(generator=gen)
    check_match(buf, res, count, size, "m")
    batch, index = buf.sample(16, generator=gen)
    assert index.dtype == torch.int32 and int(index.max()) < count
    model.train()
    opt = torch.optim.Adam(model.parameters(), lr=3e-3)
    upd = PolicyValueUpdate(model, opt, q_ratio=0.15, val_factor=1.0, pol_factor=1.0)
    # the forward: a log-policy that sums to one per graph; the kernel's loss against the same expression in plain torch ops
    model.zero_grad()
    pi, value, _, out_ptr = model(batch.x, batch.edge_index, batch.batch, batch.ptr)
    ptr = out_ptr.cpu().numpy()
    for g in range(16):
        assert abs(float(pi.detach()[ptr[g]:ptr[g + 1]].double().exp().sum()) - 1) <= 1e-5
    loss, per = upd.loss(batch, index)
    loss.backward()
    names = [n for n, p in model.named_parameters() if p.grad is not None]
    grads = [p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None]
    assert names and all(torch.isfinite(g).all() for g in grads) and torch.isfinite(loss)

    def plain(dtype):
        """The same expression in plain torch ops on the same batch: the loss and the parameter gradients."""
        model.zero_grad()
        pi, value, _, out_ptr = model(batch.x, batch.edge_index, batch.batch, batch.ptr)
        rows = torch.cat([torch.arange(int(batch.node_off[g]) + 2, int(batch.node_off[g + 1]), device=DEV) for g in range(16)])
        cells = batch.backmap[rows] - 2
        graph = torch.repeat_interleave(torch.arange(16, device=DEV), (out_ptr[1:] - out_ptr[:-1]))
        target = buf.policy[index.long()[graph], cells].to(dtype)
        y = ((1 - 0.15) * buf.z[index.long()].to(dtype) + 0.15 * buf.root_q[index.long()].to(dtype))
        total = torch.nn.MSELoss()(value.to(dtype), y) * 16 + torch.sum(-target * pi.to(dtype))
        total.backward()
        return total.detach(), [p.grad.detach().clone().cpu() for n, p in model.named_parameters() if p.grad is not None]

    l32, g32 = plain(torch.float32)
    l64, g64 = plain(torch.float64)
    rel_bound("training", "loss", loss.reshape(1), l32.reshape(1).cpu(), l64.reshape(1).cpu().double())
    assert len(g32) == len(grads)
    for n, g, a32, a64 in zip(names, grads, g32, g64):
        rel_bound("training", n, g, a32, a64.double())
    # 20 Adam steps on that one batch
    first, metrics = upd.step(batch, index)
    for _ in range(19):
        last, metrics = upd.step(batch, index)
    first, last = float(first), float(last)
    print("policy/value loss on one batch of 16: %.4f -> %.4f after 20 Adam steps; metrics %s" % (first, last, metrics.tolist()))
    assert np.isfinite(last) and last < first
    assert metrics.shape == (4,) and 0 <= float(metrics[2]) <= 1 and 0 <= float(metrics[3]) <= 1
    buf.status()
    # the trained network still plays a match to the end
    model.eval()
    player = SearchPlayer(PolicyValueEvaluator(model), 8)
    out = DeviceArena(size, G, graph=False).play(player, "random", first="m")
    player.status()
    assert set(out.winner.tolist()) <= {0, 1} and (out.length >= 2).all()      # (captures can decide Hex-4 in three moves)
    rep = replay_games(size, out.moves, first="m", device=DEV)
    assert np.array_equal(rep.winner, out.winner) and np.array_equal(rep.length, out.length)
