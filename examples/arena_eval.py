"""Play a match between two Q-networks on the device and print its statistics and speed.

    python examples/arena_eval.py --hex-size 11 --layers 15 --hidden 110            # two random-init (sharpened) GNN-L
    python examples/arena_eval.py --hex-size 7 --checkpoint a.pt b.pt --games 56     # two RainbowDQN checkpoints
    python examples/arena_eval.py --hex-size 11 --layers 15 --hidden 110 --compare 3 # arena vs the step loop, alternating
    python examples/arena_eval.py --hex-size 7 --checkpoint a.pt b.pt --mc 16,64,256  # rate model A on a ladder of playout players
    python examples/arena_eval.py --hex-size 7 --layers 10 --hidden 35 --search 32    # the model with a 32-simulation search vs itself

The match is ``gnn_hex_amd.arena.Elo_handler.play_some_games``: two legs over the shuffled unique opening moves, the first
model always playing maker.  ``--step-loop`` plays the same match with the calls that existed before the arena did
(``Env_manager.observe`` -> model -> ``select_actions`` -> ``step``, one read-back per ply, the first finish of every env
counted), which is what a user had to write by hand; at temperature 0 both give the same statistics.

``--mc R[,R...]`` rates the first model against a ladder of Monte-Carlo playout players (``gnn_hex_amd.playouts.MonteCarloPlayer``,
R playouts per move) beside ``random``: the ladder is rated first, from ``random`` = 0 upwards by each rung's match against the
rung below, then the model gets its performance rating against all of them.

``--search SIMS`` plays the first model behind a PUCT tree search (``gnn_hex_amd.search.SearchPlayer`` over ``QEvaluator``, SIMS
simulations per move, a fresh tree per ply; ``--reuse-tree``: the played move's subtree is kept) against the same model's greedy
play, as maker and as breaker.
"""
import argparse
import os
import random
import sys
import time
from argparse import Namespace

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import gnn_hex_amd  # noqa: E402,F401  (before the first device call: see gnn_hex_amd/graphs.py)
from gnn_hex_amd import _lib, ops  # noqa: E402
from gnn_hex_amd.arena import Elo_handler  # noqa: E402
from gnn_hex_amd.models import get_pre_defined  # noqa: E402
from gnn_hex_amd.multi_env_manager import Env_manager  # noqa: E402


def sharpen_(model, alpha=0.8, beta=0.5, gain=2.0, vscale=0.02):
    """A freshly initialised deep mean-aggregating stack over-smooths (all advantages equal to 1e-5): make every hidden SAGE
    layer a high-pass filter so that random-init models play distinguishable moves (the transformation the tests use)."""
    with torch.no_grad():
        sd = dict(model.named_parameters())
        for k, p in sd.items():
            if k.endswith("lin_r.weight") and p.shape[1] > 2:
                p.mul_(gain)
                sd[k.replace("lin_r", "lin_l")].mul_(beta * gain).add_(p, alpha=-alpha)
            if "value_head.layers.0.weight" in k:
                p.mul_(vscale)
    return model


def make_models(args):
    if args.checkpoint:
        models = []
        for path in args.checkpoint:
            stuff = torch.load(path, map_location="cuda", weights_only=False)
            m = get_pre_defined(args.model, stuff["args"]).cuda()
            m.load_state_dict(stuff["state_dict"])
            if stuff.get("cache") is not None:
                m.import_norm_cache(*stuff["cache"])
            models.append(m.eval())
        return models
    margs = Namespace(num_layers=args.layers, hidden_channels=args.hidden, norm=False, noisy_dqn=False, noisy_sigma0=0.5,
                      num_head_layers=2)
    models = []
    for seed in (args.seed, args.seed + 1):
        torch.manual_seed(seed)
        models.append(sharpen_(get_pre_defined(args.model, margs)).cuda().eval())
    return models


def step_loop_leg(mgr, maker_model, breaker_model, first, openings):
    """One leg with the per-ply host loop: (maker wins, breaker wins, plies)."""
    k = mgr.num_envs
    mgr.reset()
    if first == "b":
        _lib.check(_lib.lib().hexgnn_env_set_maker_turn(mgr._h, 0, ops._stream()), "hexgnn_env_set_maker_turn")
        mgr.global_onturn = "b"
    obs = mgr.observe()
    winner = np.full(k, -1)
    plies = 0
    while (winner < 0).any():
        if plies == 0:
            acts = torch.as_tensor(np.asarray(openings, dtype=np.int32)).cuda()
        else:
            model = maker_model if mgr.global_onturn == "m" else breaker_model
            b = obs.to_batch()
            with torch.no_grad():
                adv = model(b.x, b.edge_index, b.batch, b.ptr, advantages_only=True)
            acts, _, _ = mgr.select_actions(adv, obs)
        obs, _, done, infos = mgr.step(acts)
        plies += 1
        for i in np.nonzero(done)[0]:
            if winner[i] < 0:                       # the env restarts and plays on: only its first game counts
                winner[i] = 0 if infos[i]["episode_metrics"]["return"] == 1 else 1
    return int((winner == 0).sum()), int((winner == 1).sum()), plies


def play_match(args, handler, models, mgrs, step_loop):
    """(statistics, games, plies, seconds) of ``args.matches`` two-leg matches (the same match every time)."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    games = plies = 0
    for _ in range(args.matches):
        wins, g, p = play_one(args, handler, models, mgrs, step_loop)
        games, plies = games + g, plies + p
    torch.cuda.synchronize()
    return wins, games, plies, time.perf_counter() - t0


def play_one(args, handler, models, mgrs, step_loop):
    random.seed(args.seed)
    per_leg, openings = handler._match_plan(args.games, False)
    if step_loop:
        if per_leg not in mgrs:
            mgrs[per_leg] = Env_manager(per_leg, args.hex_size)
            mgrs[per_leg].record_snapshots = False
        wins, plies = {"A": 0, "B": 0}, 0
        for leg, first in enumerate(("m", "b")):
            m, b, p = step_loop_leg(mgrs[per_leg], models[0], models[1], first, openings[leg])
            wins["A"] += m
            wins["B"] += b
            plies += p
    else:
        arena = handler._arena(per_leg)
        wins, plies = {"A": 0, "B": 0}, 0
        for leg, first in enumerate(("m", "b")):
            res = arena.play(models[0], models[1], first=first, openings=openings[leg], temperature=args.temperature)
            wins["A"] += res.maker_wins
            wins["B"] += res.breaker_wins
            plies += res.plies
    return wins, 2 * per_leg, plies


def rate_on_ladder(args, handler, model):
    """``--mc``: the rating table of ``random``, the playout players and the model."""
    from gnn_hex_amd.playouts import MonteCarloPlayer
    rungs = sorted({int(r) for r in args.mc.split(",")})
    handler.add_player("random", model="random", simple=True, set_rating=0, rating_fixed=True, uses_empty_model=False)
    below = "random"
    for i, r in enumerate(rungs):
        name = "mc%d" % r
        handler.add_player(name, model=MonteCarloPlayer(r, seed=args.seed + i), uses_empty_model=False)
        stats = [handler.play_some_games(name, below, args.games, 0, progress=True),
                 handler.play_some_games(below, name, args.games, 0, progress=True)]
        handler.score_some_statistics(stats)            # an unrated player gets its performance rating
        handler.players[name]["rating_fixed"] = True
        below = name
    handler.add_player("model", model=model, uses_empty_model=False)
    stats = []
    for name in ["random"] + ["mc%d" % r for r in rungs]:
        stats.append(handler.play_some_games("model", name, args.games, args.temperature, progress=True))
        stats.append(handler.play_some_games(name, "model", args.games, args.temperature, progress=True))
    handler.score_some_statistics(stats)
    for name, rating in handler.get_rating_table()[1]:
        print("%-10s %8.1f" % (name, rating))


def search_match(args, handler, model):
    """``--search``: the model searching ``SIMS`` simulations per move (``QEvaluator`` -> ``SearchPlayer``) against the same
    model playing its greedy move, both ways round."""
    from gnn_hex_amd.search import QEvaluator, SearchPlayer
    handler.add_player("search%d" % args.search, model=SearchPlayer(QEvaluator(model), args.search, leaves=args.leaves,
                                                                   virtual_loss=args.virtual_loss, reuse_tree=args.reuse_tree),
                       uses_empty_model=False)
    handler.add_player("greedy", model=model, uses_empty_model=False)
    for maker, breaker in (("search%d" % args.search, "greedy"), ("greedy", "search%d" % args.search)):
        t0 = time.perf_counter()
        wins = handler.play_some_games(maker, breaker, args.games, args.temperature, progress=True)
        torch.cuda.synchronize()
        print("%s (maker) vs %s: %s in %.2f s" % (maker, breaker, wins, time.perf_counter() - t0), flush=True)


def report(tag, wins, games, plies, dt):
    print("%-9s %s  %d games in %.3f s: %.1f games/s, %.1f plies/s" % (tag, wins, games, dt, games / dt, plies / dt), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--hex-size", type=int, default=11)
    ap.add_argument("--games", type=int, default=None, help="games of the match (default and cap: n (n + 1))")
    ap.add_argument("--model", default="modern_two_headed")
    ap.add_argument("--layers", type=int, default=15)
    ap.add_argument("--hidden", type=int, default=110)
    ap.add_argument("--checkpoint", nargs=2, metavar=("A", "B"), help="two RainbowDQN checkpoints instead of random-init models")
    ap.add_argument("--temperature", type=float, default=0.0)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--step-loop", action="store_true", help="play with observe / model / select_actions / step instead")
    ap.add_argument("--compare", type=int, default=0, metavar="N",
                    help="after a warm-up match of each, alternate arena and step loop N times and print every timing")
    ap.add_argument("--mc", default=None, metavar="R[,R...]",
                    help="rate the first model against Monte-Carlo playout players of R playouts per move, beside random")
    ap.add_argument("--search", type=int, default=0, metavar="SIMS",
                    help="play the first model with a PUCT search of SIMS simulations per move against its own greedy play")
    ap.add_argument("--leaves", type=int, default=1,
                    help="--search: leaves per game per round under virtual loss (1: one leaf per round; else < SIMS)")
    ap.add_argument("--virtual-loss", type=int, default=1, help="--search: the virtual loss of a round of several leaves")
    ap.add_argument("--reuse-tree", action="store_true",
                    help="--search: keep the played move's subtree between plies (SIMS new simulations per move on top of it)")
    ap.add_argument("--matches", type=int, default=1, help="matches per timed window (a window should last a good part of a second)")
    ap.add_argument("--repeat", type=int, default=1, help="timed windows to play (the first one includes graph capture)")
    args = ap.parse_args()
    if (args.step_loop or args.compare) and args.temperature != 0:
        ap.error("the step loop has no temperature sampling: use --temperature 0")
    models = make_models(args)
    handler = Elo_handler(args.hex_size)
    mgrs = {}
    if args.mc:
        rate_on_ladder(args, handler, models[0])
        return
    if args.search:
        search_match(args, handler, models[0])
        return
    if args.compare:
        for step_loop in (False, True):
            report("warm-up", *play_match(args, handler, models, mgrs, step_loop))
        times = {False: [], True: []}
        stats = {}
        for _ in range(args.compare):
            for step_loop in (False, True):
                wins, games, plies, dt = play_match(args, handler, models, mgrs, step_loop)
                report("step-loop" if step_loop else "arena", wins, games, plies, dt)
                times[step_loop].append((games / dt, plies / dt))
                stats[step_loop] = wins
        for step_loop in (False, True):
            g = sorted(t[0] for t in times[step_loop])
            p = sorted(t[1] for t in times[step_loop])
            print("%-9s games/s median %.1f (min %.1f, max %.1f); plies/s median %.1f (min %.1f, max %.1f)"
                  % ("step-loop" if step_loop else "arena", g[len(g) // 2], g[0], g[-1], p[len(p) // 2], p[0], p[-1]))
        print("same statistics: %s" % (stats[False] == stats[True]))
        return
    for r in range(args.repeat):
        report("step-loop" if args.step_loop else "arena", *play_match(args, handler, models, mgrs, args.step_loop))


if __name__ == "__main__":
    main()
