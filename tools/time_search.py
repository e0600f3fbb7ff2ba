"""Time the batched PUCT tree search (gnn_hex_amd/search.py, csrc/search.hip) beside the plain forward of the same model.

    python tools/time_search.py                      # GNN-S Hex-7, GNN-L Hex-11, HexAra Hex-11; G = 32 / 128, 16 / 64 sims
    python tools/time_search.py --games 32 --sims 16 --arena-games 0
    python tools/time_search.py --leaves 1,2,4,8,16          # rounds of K leaves per game under virtual loss, equal total simulations

Part 1: per model, game count G and simulation count S, ``TreeSearch.simulate`` of S simulations from G start positions (a fresh
tree per call): simulations per second (G * S per call), microseconds per simulation round (one leaf per game), and the plain
forward of the same model on G start positions as the yardstick (one forward; ``QEvaluator`` runs two per round, one per side).
``--leaves K[,K...]``: ``TreeSearch(leaves=K, virtual_loss=--virtual-loss)``, the same S simulations ASKED FOR in ceil(S / K)
rounds; the rate counts the simulations asked for, and ``applied`` is the share of them that were applied (collisions are not).
Every point is warmed up once and then timed by the synchronised host clock over ``--repeats`` calls: the loop reads sizes back
and is host-driven, so device events alone would miss what bounds it.
Part 2: ``DeviceArena(graph=False)`` games per second of a ``SearchPlayer`` (as maker) against the built-in random player.
``--reuse``: tree reuse between plies.  Part 1 adds, behind every point, one ``TreeSearch.advance`` by the most visited move on
the tree that point built (the workspace restored before every call, each call timed alone by the synchronised host clock, the
median of ``--advance-repeats`` calls), to stand beside the us per round.  Part 2 plays every player a second time as
``SearchPlayer(reuse_tree=True)`` at equal new simulations per move and prints the mean of carried / sims over the advances of
the timed matches (all games of every ply played, both the own and the opponent's moves; a resting game counts as 0).
"""
import argparse
import os
import sys
import time
from argparse import Namespace

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import gnn_hex_amd  # noqa: E402,F401  (before the first device call: see gnn_hex_amd/graphs.py)
from gnn_hex_amd.arena import DeviceArena  # noqa: E402
from gnn_hex_amd.models import get_pre_defined  # noqa: E402
from gnn_hex_amd.multi_env_manager import Env_manager  # noqa: E402
from gnn_hex_amd.search import PolicyValueEvaluator, QEvaluator, SearchPlayer, TreeSearch  # noqa: E402
from gnn_hex_amd.torch_script_models import get_current_model  # noqa: E402


def q_net(layers, hidden, seed):
    margs = Namespace(num_layers=layers, hidden_channels=hidden, norm=False, noisy_dqn=False, noisy_sigma0=0.5, num_head_layers=2)
    torch.manual_seed(seed)
    return get_pre_defined("modern_two_headed", margs).cuda().eval()


def host_timed(fn, repeats):
    """Seconds per call of ``fn`` by the synchronised host clock, after one warm-up call."""
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(repeats):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / repeats


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--games", default="32,128")
    ap.add_argument("--sims", default="16,64")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--arena-games", type=int, default=32, help="games per arena match (0: skip part 2)")
    ap.add_argument("--arena-sims", type=int, default=16)
    ap.add_argument("--leaves", default="1", help="leaves per game per round, a list (1: the one-leaf search)")
    ap.add_argument("--virtual-loss", type=int, default=1)
    ap.add_argument("--models", default="0,1,2", help="which of the three models to time")
    ap.add_argument("--reuse", action="store_true", help="time TreeSearch.advance and a SearchPlayer(reuse_tree=True)")
    ap.add_argument("--advance-repeats", type=int, default=9)
    args = ap.parse_args()
    torch.manual_seed(0)
    models = [("GNN-S 10 x 35", 7, q_net(10, 35, 0), QEvaluator), ("GNN-L 15 x 110", 11, q_net(15, 110, 1), QEvaluator),
              ("HexAra 60, 15+2+2", 11, get_current_model().cuda().eval(), PolicyValueEvaluator)]
    models = [models[int(v)] for v in args.models.split(",")]
    leaves = [int(v) for v in args.leaves.split(",")]
    print("TreeSearch.simulate from start positions, a fresh tree per call; forward = one plain forward of the model on G positions")
    for name, size, model, make in models:
        ev = make(model)
        for G in (int(v) for v in args.games.split(",")):
            mgr = Env_manager(G, size)
            mgr.record_snapshots = False
            bt = mgr.observe().to_batch()
            with torch.no_grad():
                fwd = host_timed(lambda: model(bt.x, bt.edge_index, bt.batch, bt.ptr), 20)
            for S in (int(v) for v in args.sims.split(",")):
                for K in leaves:
                    search = TreeSearch(size, G, S, leaves=K, virtual_loss=args.virtual_loss)

                    def run():
                        search.reset()
                        search.simulate(mgr._h, ev, S)

                    sec = host_timed(run, args.repeats)
                    applied = float(search.applied().float().mean()) / S
                    search.status()
                    rounds = -(-S // K)
                    print("%-18s Hex-%-2d G %3d sims %3d leaves %2d  %9.0f sims/s  %8.1f us/round  applied %.2f  forward %7.1f us  "
                          "(round / forward %.1f)" % (name, size, G, S, K, G * S / sec, 1e6 * sec / rounds, applied, 1e6 * fwd,
                                                      sec / rounds / fwd), flush=True)
                    if args.reuse:
                        best = search.root(mgr.observe(), boards=True)[3]
                        saved, took = search.workspace.clone(), []
                        for _ in range(args.advance_repeats + 1):
                            search.workspace.copy_(saved)
                            torch.cuda.synchronize()
                            t0 = time.perf_counter()
                            carried = search.advance(best)
                            torch.cuda.synchronize()
                            took.append(time.perf_counter() - t0)
                        kept = search.tree()["cnt"][:, 0]
                        print("%-18s Hex-%-2d G %3d sims %3d leaves %2d  advance %7.1f us (median of %d, first call %.1f us)  carried "
                              "%.1f, kept %.1f of %d nodes  (advance / round %.2f)" % (
                                  name, size, G, S, K, 1e6 * sorted(took[1:])[len(took[1:]) // 2], len(took) - 1, 1e6 * took[0],
                                  float(carried.float().mean()), float(kept.mean()), S + 1,
                                  sorted(took[1:])[len(took[1:]) // 2] / (sec / rounds)), flush=True)
    if args.arena_games > 0:
        G, S = args.arena_games, args.arena_sims
        print("DeviceArena(size, %d, graph=False): SearchPlayer(%d sims) as maker against \"random\", both first movers" % (G, S))
        for name, size, model, make, K, reuse in [m + (K, r) for m in models for K in leaves if K == 1 or K < S
                                                  for r in ((False, True) if args.reuse else (False,))]:
            arena = DeviceArena(size, G, graph=False)
            player = SearchPlayer(make(model), S, leaves=K, virtual_loss=args.virtual_loss, reuse_tree=reuse)
            shares = []
            arena.play(player, "random", first="m")          # first use
            player.on_carried = lambda c: shares.append(c.float().mean())
            torch.cuda.synchronize()
            t0, won, plies = time.perf_counter(), 0, 0
            for first in ("m", "b"):
                res = arena.play(player, "random", first=first)
                won, plies = won + res.maker_wins, plies + res.plies
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            player.status()
            tail = "  reuse: carried / sims %.2f over %d advances" % (float(torch.stack(shares).mean()) / S, len(shares)) if reuse else ""
            print("%-18s Hex-%-2d leaves %2d  %6.2f games/s  %6.1f plies/s  won %d of %d%s" % (name, size, K, 2 * G / dt, plies / dt, won,
                                                                                          2 * G, tail), flush=True)


if __name__ == "__main__":
    main()
