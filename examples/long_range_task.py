"""The long-range dependency task of the reference (GN0/tests/test_models_on_long_range_task.py) on the device.

    python examples/long_range_task.py --min 5 --max 13                                   # a random-init model
    python examples/long_range_task.py --min 8 --max 25 --checkpoint CKPT --model modern_two_headed

Per board size and defender colour the task builds two positions out of forced-colour stones
(``gnn_hex_amd.positions.long_range_stones``).  In the negative one board cell 0 is no better than its neighbours for the
defender; in the positive one two stones a whole board away have made it the only move that keeps the defender connected.  The
model is evaluated once per colour -- both positions in one batch of two envs: ``Env_manager.set_positions`` +
``positions.evaluate`` -- and the arg-max of its board-indexed output is checked.  The printed fail list is the reference's:
``"{n}_{m|b}_false_positive"`` when the negative position's arg-max is cell 0, ``"{n}_{m|b}_false_negative"`` when the positive
position's is not.  A random-init model fails about everywhere; the published GNN-L checkpoint is what the table is about.
This is a latency path: nothing here is timed.
"""
import argparse
import os
import sys
from argparse import Namespace

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import gnn_hex_amd  # noqa: E402,F401  (before the first device call: see gnn_hex_amd/graphs.py)
from gnn_hex_amd.models import get_pre_defined  # noqa: E402
from gnn_hex_amd.multi_env_manager import Env_manager  # noqa: E402
from gnn_hex_amd.positions import evaluate, long_range_stones  # noqa: E402


def make_model(args):
    if args.checkpoint:
        stuff = torch.load(args.checkpoint, map_location="cuda", weights_only=False)
        model = get_pre_defined(args.model, stuff["args"]).cuda()
        model.load_state_dict(stuff["state_dict"])
        if stuff.get("cache") is not None:
            model.import_norm_cache(*stuff["cache"])
        return model.eval()
    margs = Namespace(num_layers=args.layers, hidden_channels=args.hidden, norm=False, noisy_dqn=False, noisy_sigma0=0.5,
                      num_head_layers=2)
    torch.manual_seed(args.seed)
    return get_pre_defined(args.model, margs).cuda().eval()


def long_range_fails(model, min_hex_size=5, max_hex_size=13, device=None):
    """The reference's ``test_on_long_range_tasks(model, cnn_mode=False, ...)``: the list of failed cases."""
    fails = []
    for n in range(min_hex_size, max_hex_size + 1):
        mgr = Env_manager(2, n, device=device)
        mgr.record_snapshots = False
        for defender in ("m", "b"):
            obs = mgr.set_positions(long_range_stones(n, defender), onturn=defender)
            _, best = evaluate(model, obs, n)
            negative, positive = best.tolist()
            if negative == 0:
                fails.append("%d_%s_false_positive" % (n, defender))
            if positive != 0:
                fails.append("%d_%s_false_negative" % (n, defender))
    return fails


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--min", type=int, default=5, help="smallest board size")
    ap.add_argument("--max", type=int, default=25, help="largest board size (25 at the most)")
    ap.add_argument("--checkpoint", help="a RainbowDQN checkpoint instead of a random-init model")
    ap.add_argument("--model", default="modern_two_headed")
    ap.add_argument("--layers", type=int, default=15)
    ap.add_argument("--hidden", type=int, default=110)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    if not 3 <= args.min <= args.max <= 25:
        ap.error("board sizes: 3 <= --min <= --max <= 25")
    fails = long_range_fails(make_model(args), args.min, args.max)
    cases = 4 * (args.max - args.min + 1)
    print("Mistakes: %s" % fails)
    print("%d of %d cases failed" % (len(fails), cases))


if __name__ == "__main__":
    main()
