"""GPU: the entry points gnn_hex_amd/search.py and search_selfplay.py issue, call for call.  ``_lib.check`` is wrapped and its second
argument -- the entry point's name -- recorded.  The expected sequences are literal.  They were recorded from the separate
one-leaf loop, round loop and per-ply code of the commit that introduced tree reuse, which is the reference here: the one
``TreeSearch.simulate`` loop, the one call path behind ``descend`` / ``backup`` and the one per-ply protocol (``SearchPlies``) of
``SearchPlayer`` and ``SearchSelfPlay.play`` must issue the same calls in the same order -- with ``leaves = 1`` never a round
call.  Hex-3, two games, ``UniformEvaluator``, 5 simulations; ``leaves = 2`` makes rounds of 2, 2 and 1 descents."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
SIMS = 5


def _rounds(descend, backup, n, noise_behind=None, noise_before=False):
    """``n`` rounds of descend -> the leaf offsets of ``UniformEvaluator`` -> backup, written out; the root noise behind round
    ``noise_behind`` and / or before the first."""
    out = ["hexgnn_search_root_noise"] if noise_before else []
    for i in range(n):
        out += [descend, "hexgnn_env_offsets", backup]
        if i == noise_behind:
            out.append("hexgnn_search_root_noise")
    return out


ONE = ("hexgnn_search_descend", "hexgnn_search_backup")
ROUND = ("hexgnn_search_round_descend", "hexgnn_search_round_backup")
# simulate(): with the noise on a fresh tree, without it, with it after an advance (carried roots before, new roots behind)
SIMULATE = {
    1: dict(noise_fresh=["hexgnn_search_descend", "hexgnn_env_offsets", "hexgnn_search_backup", "hexgnn_search_root_noise",
                         "hexgnn_search_descend", "hexgnn_env_offsets", "hexgnn_search_backup",
                         "hexgnn_search_descend", "hexgnn_env_offsets", "hexgnn_search_backup",
                         "hexgnn_search_descend", "hexgnn_env_offsets", "hexgnn_search_backup",
                         "hexgnn_search_descend", "hexgnn_env_offsets", "hexgnn_search_backup"],
            plain_fresh=_rounds(*ONE, 5),
            noise_advanced=["hexgnn_search_root_noise",
                            "hexgnn_search_descend", "hexgnn_env_offsets", "hexgnn_search_backup", "hexgnn_search_root_noise",
                            "hexgnn_search_descend", "hexgnn_env_offsets", "hexgnn_search_backup",
                            "hexgnn_search_descend", "hexgnn_env_offsets", "hexgnn_search_backup",
                            "hexgnn_search_descend", "hexgnn_env_offsets", "hexgnn_search_backup",
                            "hexgnn_search_descend", "hexgnn_env_offsets", "hexgnn_search_backup"],
            round_leaves=[None] * 5),
    2: dict(noise_fresh=["hexgnn_search_round_descend", "hexgnn_env_offsets", "hexgnn_search_round_backup", "hexgnn_search_root_noise",
                         "hexgnn_search_round_descend", "hexgnn_env_offsets", "hexgnn_search_round_backup",
                         "hexgnn_search_round_descend", "hexgnn_env_offsets", "hexgnn_search_round_backup"],
            plain_fresh=_rounds(*ROUND, 3),
            noise_advanced=["hexgnn_search_root_noise",
                            "hexgnn_search_round_descend", "hexgnn_env_offsets", "hexgnn_search_round_backup", "hexgnn_search_root_noise",
                            "hexgnn_search_round_descend", "hexgnn_env_offsets", "hexgnn_search_round_backup",
                            "hexgnn_search_round_descend", "hexgnn_env_offsets", "hexgnn_search_round_backup"],
            round_leaves=[2, 2, 1]),
}
# one ply of a SearchPlayer: begin_match() + search_scores() | observe_moves()
PLAYER = {
    False: (["hexgnn_search_reset"] + _rounds(*ONE, 5) + ["hexgnn_search_root"], []),
    True: (["hexgnn_search_reset"] + _rounds(*ONE, 5) + ["hexgnn_search_root"], ["hexgnn_search_advance"]),
}
# SearchSelfPlay.play() on Hex-3, whose first move decides the game: a match of one ply
SELFPLAY = {
    False: ["hexgnn_env_reset", "hexgnn_env_observe", "hexgnn_search_reset"] + _rounds(*ONE, 5, noise_behind=0)
           + ["hexgnn_search_record", "hexgnn_arena_ply", "hexgnn_env_offsets", "hexgnn_samples_finish"],
    True: ["hexgnn_env_reset", "hexgnn_search_reset", "hexgnn_env_observe"] + _rounds(*ONE, 5, noise_behind=0)
          + ["hexgnn_search_record", "hexgnn_arena_ply", "hexgnn_env_offsets", "hexgnn_search_advance", "hexgnn_samples_finish"],
}


@pytest.fixture
def calls(monkeypatch):
    """The names handed to ``_lib.check`` since the last ``take()``."""
    from gnn_hex_amd import _lib
    names, check = [], _lib.check

    def recording(rc, what=""):
        names.append(what)
        return check(rc, what)

    def take():
        got = list(names)
        del names[:]
        return got

    monkeypatch.setattr(_lib, "check", recording)
    return take


def test_the_literal_lists_say_what_they_are_meant_to():
    """The lists above, against their description: no round call with one leaf, only round calls with two."""
    for key in ("noise_fresh", "plain_fresh", "noise_advanced"):
        assert not any("round" in n for n in SIMULATE[1][key]) and SIMULATE[1][key].count("hexgnn_search_descend") == 5
        assert not any(n in ONE for n in SIMULATE[2][key]) and SIMULATE[2][key].count("hexgnn_search_round_descend") == 3
    assert SIMULATE[1]["noise_fresh"] == _rounds(*ONE, 5, noise_behind=0)
    assert SIMULATE[1]["noise_advanced"] == _rounds(*ONE, 5, noise_behind=0, noise_before=True)
    assert SIMULATE[2]["noise_fresh"] == _rounds(*ROUND, 3, noise_behind=0)
    assert SIMULATE[2]["noise_advanced"] == _rounds(*ROUND, 3, noise_behind=0, noise_before=True)


@pytest.mark.parametrize("K", [1, 2])
def test_simulate_issues_the_same_calls(calls, K):
    from gnn_hex_amd.multi_env_manager import Env_manager
    from gnn_hex_amd.search import TreeSearch, UniformEvaluator
    want = SIMULATE[K]
    mgr = Env_manager(2, 3)
    mgr.record_snapshots = False
    sr, ev = TreeSearch(3, 2, 16, leaves=K), UniformEvaluator()
    gen = torch.Generator(device=DEV).manual_seed(1)
    calls()

    def run(**kw):
        trace = []
        sr.simulate(mgr._h, ev, SIMS, trace=trace, **kw)
        got = calls()
        assert [d.get("round_leaves") for d in trace] == want["round_leaves"]
        assert all(("round_leaves" in d) == (K > 1) for d in trace), "the key belongs to leaves > 1 alone"
        assert all(sorted(set(d) - {"round_leaves"}) == ["leaf", "logits", "offsets", "path", "skip", "value"] for d in trace)
        return got

    assert run(root_noise=(0.25, 0.3), generator=gen) == want["noise_fresh"]
    sr.reset()
    calls()
    assert run() == want["plain_fresh"]
    best = sr.root(mgr.observe(), boards=True)[3]
    sr.advance(best)
    mgr.step(best)
    calls()
    assert run(root_noise=(0.25, 0.3), generator=gen) == want["noise_advanced"]
    sr.status()


@pytest.mark.parametrize("reuse_tree", [False, True])
def test_the_players_issue_the_same_calls(calls, reuse_tree):
    from gnn_hex_amd.arena import DeviceArena
    from gnn_hex_amd.search import SearchPlayer, UniformEvaluator
    from gnn_hex_amd.search_selfplay import SearchSampleBuffer, SearchSelfPlay
    ar = DeviceArena(3, 2, graph=False)
    mgr, obs = ar.mgr, ar.obs
    ar._prepare(True, None)
    obs.observe_env(mgr._h)
    active = torch.ones(2, dtype=torch.int32, device=DEV)
    player = SearchPlayer(UniformEvaluator(), SIMS, reuse_tree=reuse_tree)
    player.search_for(mgr._h, 2, obs.x.device)                # the trees exist: begin_match() has something to reset
    calls()
    player.begin_match()
    player.search_scores(mgr._h, obs, active)
    searched = calls()
    best = player._search.root(obs, boards=True)[3]
    calls()
    player.observe_moves(best)
    assert (searched, calls()) == PLAYER[reuse_tree]
    player.status()

    buf = SearchSampleBuffer(2 * 9, 3, DEV)
    sp = SearchSelfPlay(3, 2, UniformEvaluator(), SIMS, buf, root_noise=(0.25, 0.3), reuse_tree=reuse_tree)
    gen = torch.Generator(device=DEV).manual_seed(2)
    calls()
    res, samples = sp.play("m", generator=gen)
    assert res.plies == 1 and samples == 2
    assert calls() == SELFPLAY[reuse_tree]
