"""Train the HexAra policy/value network from its own search: self-play match, k updates, repeat.

    python examples/search_selfplay_train.py                                   # Hex-5, 32 games, 16 simulations, small net
    python examples/search_selfplay_train.py --hex-size 7 --games 64 --sims 32 --hidden 60 --layers 15 --iterations 50

Every iteration plays one lock-step match with the search on both sides (``gnn_hex_amd.search_selfplay.SearchSelfPlay``:
Dirichlet noise on the root priors, the first ``--proportional-plies`` moves drawn in proportion to the visit counts), which
records one sample per move into the device ring, and then makes ``--updates`` policy/value updates on batches drawn from the
ring (``PolicyValueUpdate``).  Every ``--eval-every`` iterations the current network's ``SearchPlayer`` plays an arena match
against the built-in random player, as maker and as breaker.
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import gnn_hex_amd  # noqa: E402,F401  (before the first device call: see gnn_hex_amd/graphs.py)
from gnn_hex_amd.arena import DeviceArena  # noqa: E402
from gnn_hex_amd.search import PolicyValueEvaluator, SearchPlayer  # noqa: E402
from gnn_hex_amd.search_selfplay import PolicyValueUpdate, SearchSampleBuffer, SearchSelfPlay  # noqa: E402
from gnn_hex_amd.torch_script_models import SAGE_torch_script  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--hex-size", type=int, default=5)
    ap.add_argument("--games", type=int, default=32, help="games per self-play match")
    ap.add_argument("--sims", type=int, default=16, help="simulations per move")
    ap.add_argument("--hidden", type=int, default=32)
    ap.add_argument("--layers", type=int, default=4)
    ap.add_argument("--head-layers", type=int, default=2)
    ap.add_argument("--iterations", type=int, default=10)
    ap.add_argument("--updates", type=int, default=8, help="updates per iteration")
    ap.add_argument("--batch-size", type=int, default=64)
    ap.add_argument("--matches-kept", type=int, default=8, help="the ring holds this many whole matches")
    ap.add_argument("--lr", type=float, default=1e-3)
    ap.add_argument("--q-ratio", type=float, default=0.15, help="rl_loop/train_config.py: q_value_ratio")
    ap.add_argument("--val-factor", type=float, default=1.0)
    ap.add_argument("--pol-factor", type=float, default=1.0)
    ap.add_argument("--dirichlet-eps", type=float, default=0.25)
    ap.add_argument("--dirichlet-alpha", type=float, default=0.2)
    ap.add_argument("--proportional-plies", type=int, default=None, help="default: every move is drawn")
    ap.add_argument("--c-puct", type=float, default=1.5)
    ap.add_argument("--leaves", type=int, default=1, help="leaves per game per search round under virtual loss (< --sims)")
    ap.add_argument("--virtual-loss", type=int, default=1)
    ap.add_argument("--reuse-tree", action="store_true",
                    help="keep the played move's subtree between plies, in self-play and in the evaluation player")
    ap.add_argument("--eval-every", type=int, default=5)
    ap.add_argument("--eval-games", type=int, default=16)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    torch.manual_seed(args.seed)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(args.seed)
    size = args.hex_size
    model = SAGE_torch_script(args.hidden, args.layers, args.head_layers, args.head_layers).cuda()
    optimizer = torch.optim.Adam(model.parameters(), lr=args.lr)
    buf = SearchSampleBuffer(args.matches_kept * args.games * size * size, size, "cuda")
    noise = (args.dirichlet_eps, args.dirichlet_alpha) if args.dirichlet_eps > 0 else None
    selfplay = SearchSelfPlay(size, args.games, PolicyValueEvaluator(model), args.sims, buf, c_puct=args.c_puct,
                              root_noise=noise, proportional_plies=args.proportional_plies, leaves=args.leaves,
                              virtual_loss=args.virtual_loss, reuse_tree=args.reuse_tree)
    update = PolicyValueUpdate(model, optimizer, q_ratio=args.q_ratio, val_factor=args.val_factor, pol_factor=args.pol_factor)
    arena = DeviceArena(size, args.eval_games, graph=False)
    player = SearchPlayer(PolicyValueEvaluator(model), args.sims, c_puct=args.c_puct, leaves=args.leaves,
                          virtual_loss=args.virtual_loss, reuse_tree=args.reuse_tree)
    for it in range(1, args.iterations + 1):
        model.eval()
        t0 = time.perf_counter()
        res, samples = selfplay.play(first="m" if it % 2 else "b", generator=gen)
        t1 = time.perf_counter()
        model.train()
        for _ in range(args.updates):
            batch, index = buf.sample(args.batch_size, generator=gen)
            loss, metrics = update.step(batch, index)
        loss, metrics = float(loss) / args.batch_size, metrics.tolist()
        t2 = time.perf_counter()
        print("iteration %3d: %4d samples in %.2f s (maker won %d of %d, mean length %.1f), ring %d; %d updates in %.2f s: "
              "loss %.4f, policy loss %.4f, value loss %.4f, policy acc %.2f, value sign acc %.2f"
              % (it, samples, t1 - t0, res.maker_wins, args.games, float(res.length.mean()), len(buf), args.updates, t2 - t1,
                 loss, metrics[0], metrics[1], metrics[2], metrics[3]), flush=True)
        if args.eval_every > 0 and it % args.eval_every == 0:
            model.eval()
            won = arena.play(player, "random", first="m").maker_wins + arena.play("random", player, first="m").breaker_wins
            player.status()
            print("              search player (%d simulations) against random: won %d of %d" % (args.sims, won, 2 * args.eval_games),
                  flush=True)


if __name__ == "__main__":
    main()
