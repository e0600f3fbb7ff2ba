"""Time search self-play and the policy/value update (gnn_hex_amd/search_selfplay.py) beside the plain forward of the same model.

    python tools/time_search_selfplay.py                    # HexAra 60, 15+2+2 on Hex-7 and Hex-11; G = 32 / 128; 16 simulations
    python tools/time_search_selfplay.py --sizes 7 --games 32 --repeats 1
    python tools/time_search_selfplay.py --sizes 11 --games 128 --leaves 4     # rounds of 4 leaves per game under virtual loss

Per board size and game count G: one ``SearchSelfPlay.play`` match (samples per second, plies), then ``--updates``
``PolicyValueUpdate.step`` calls on batches of G samples drawn from that match (updates per second, ``sample`` included), and one
plain no-grad forward of the model on G start positions as the yardstick.  Everything is warmed up once and timed by the
synchronised host clock: the loop reads sizes back and is host-driven, so device events alone would miss what bounds it.
``--reuse``: ``SearchSelfPlay(reuse_tree=True)`` at equal new simulations per move; the line gains the mean of carried / sims
over the advances of the timed matches (all games of every ply, a resting game counts as 0).
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import gnn_hex_amd  # noqa: E402,F401  (before the first device call: see gnn_hex_amd/graphs.py)
from gnn_hex_amd.multi_env_manager import Env_manager  # noqa: E402
from gnn_hex_amd.search import PolicyValueEvaluator  # noqa: E402
from gnn_hex_amd.search_selfplay import PolicyValueUpdate, SearchSampleBuffer, SearchSelfPlay  # noqa: E402
from gnn_hex_amd.torch_script_models import get_current_model  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", default="7,11")
    ap.add_argument("--games", default="32,128")
    ap.add_argument("--sims", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=1, help="timed matches per point")
    ap.add_argument("--updates", type=int, default=10)
    ap.add_argument("--leaves", type=int, default=1, help="leaves per game per round (1: the one-leaf search; else < --sims)")
    ap.add_argument("--virtual-loss", type=int, default=1)
    ap.add_argument("--reuse", action="store_true", help="keep the played move's subtree between plies")
    args = ap.parse_args()
    torch.manual_seed(0)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(0)
    print("HexAra 60, 15+2+2; %d simulations per move, %d leaves per round; forward = one plain forward of the model on G start "
          "positions" % (args.sims, args.leaves))
    for size in (int(v) for v in args.sizes.split(",")):
        model = get_current_model().cuda()
        opt = torch.optim.Adam(model.parameters(), lr=1e-4)
        upd = PolicyValueUpdate(model, opt, q_ratio=0.15)
        for G in (int(v) for v in args.games.split(",")):
            mgr = Env_manager(G, size)
            mgr.record_snapshots = False
            bt = mgr.observe().to_batch()
            model.eval()
            with torch.no_grad():
                model(bt.x, bt.edge_index, bt.batch, bt.ptr)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(20):
                    model(bt.x, bt.edge_index, bt.batch, bt.ptr)
                torch.cuda.synchronize()
                fwd = (time.perf_counter() - t0) / 20
            buf = SearchSampleBuffer(G * size * size, size, "cuda")
            sp = SearchSelfPlay(size, G, PolicyValueEvaluator(model), args.sims, buf, leaves=args.leaves,
                                virtual_loss=args.virtual_loss, reuse_tree=args.reuse)
            shares = []
            sp.play(generator=gen)                          # first use
            if args.reuse:
                sp.on_carried = lambda c: shares.append(c.float().mean())
            torch.cuda.synchronize()
            t0, samples, plies = time.perf_counter(), 0, 0
            for r in range(args.repeats):
                res, n = sp.play(first="b" if r % 2 else "m", generator=gen)
                samples, plies = samples + n, plies + res.plies
            torch.cuda.synchronize()
            play = time.perf_counter() - t0
            model.train()
            upd.step(*buf.sample(G, generator=gen))         # first use
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.updates):
                upd.step(*buf.sample(G, generator=gen))
            torch.cuda.synchronize()
            step = (time.perf_counter() - t0) / args.updates
            tail = "  reuse: carried / sims %.2f" % (float(torch.stack(shares).mean()) / args.sims) if shares else ""
            print("Hex-%-2d G %3d  self-play %8.1f samples/s (%d samples, %d plies, %.2f s)  update of %3d graphs %6.1f /s "
                  "(%.2f ms)  forward %7.1f us%s" % (size, G, samples / play, samples, plies, play, G, 1 / step, 1e3 * step,
                                                     1e6 * fwd, tail), flush=True)


if __name__ == "__main__":
    main()
