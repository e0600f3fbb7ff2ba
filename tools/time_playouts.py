"""Time the Monte-Carlo playout player (gnn_hex_amd/playouts.py, csrc/playout.hip) beside the GNN-L forward of the same run.

    python tools/time_playouts.py                      # b = 128, R = 256: Hex-5 / 11 / 13 start positions, then arena games/s
    python tools/time_playouts.py --playouts 64 --arena-size 7

Part 1: ``playout_values`` over ``b`` start positions per board size: microseconds per call and playouts per second, and the
advantages-only forward of a random-init GNN-L (modern_two_headed, 15 layers, hidden 110) on the same observation as the
yardstick.  Every point is warmed up and then timed with device events over at least ``--seconds`` of back-to-back calls.
Part 2: ``DeviceArena`` games per second of (A) the playout player as maker against the GNN-L player and (B) the GNN-L player
against itself, the two variants alternated ``--rounds`` times in one process after a warm-up (graph capture) of each.
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
from gnn_hex_amd.playouts import MonteCarloPlayer, playout_values  # noqa: E402


def timed(fn, seconds, warmup=10):
    """(microseconds per call, calls) of ``fn`` over at least ``seconds`` of device time, by device events."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    calls, total_ms, batch = 0, 0.0, 20
    while total_ms < 1000.0 * seconds:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(batch):
            fn()
        b.record()
        b.synchronize()
        total_ms += a.elapsed_time(b)
        calls += batch
        batch = min(4 * batch, 2000)
    return 1000.0 * total_ms / calls, calls


def gnn_l(seed):
    margs = Namespace(num_layers=15, hidden_channels=110, norm=False, noisy_dqn=False, noisy_sigma0=0.5, num_head_layers=2)
    torch.manual_seed(seed)
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    from arena_eval import sharpen_
    return sharpen_(get_pre_defined("modern_two_headed", margs)).cuda().eval()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--playouts", type=int, default=256)
    ap.add_argument("--sizes", default="5,11,13")
    ap.add_argument("--seconds", type=float, default=1.0, help="device time per point, at least")
    ap.add_argument("--arena-size", type=int, default=11)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    b, R = args.batch, args.playouts
    model = gnn_l(0)
    print("playout_values, b = %d start positions, R = %d; GNN-L = modern_two_headed 15 x 110, advantages only" % (b, R))
    for size in (int(s) for s in args.sizes.split(",")):
        mgr = Env_manager(b, size)
        mgr.record_snapshots = False
        bt = mgr.observe().to_batch()
        counter = torch.zeros(1, dtype=torch.int64, device="cuda")
        us, calls = timed(lambda: playout_values(bt.x, bt.edge_index, bt.ptr, R, counter=counter), args.seconds)
        with torch.no_grad():
            us_m, calls_m = timed(lambda: model(bt.x, bt.edge_index, bt.batch, bt.ptr, advantages_only=True), args.seconds)
        print("Hex-%-2d (%3d nodes)  playouts %8.1f us/call  %7.2f M playouts/s  (%d calls)   GNN-L forward %8.1f us/call (%d calls)"
              % (size, size * size + 2, us, b * R / us, calls, us_m, calls_m), flush=True)
    size = args.arena_size
    arena = DeviceArena(size, b)
    openings = [2 + (7 * i) % (size * size) for i in range(b)]
    variants = {"mc%d-vs-gnn" % R: (MonteCarloPlayer(R, seed=1), model), "gnn-vs-gnn": (model, gnn_l(1))}

    def window(players):
        """Play matches (both first movers) for at least ``--seconds``: (games/s, plies/s) by the synchronised host clock."""
        torch.cuda.synchronize()
        t0, games, plies = time.perf_counter(), 0, 0
        while time.perf_counter() - t0 < args.seconds:
            for first in ("m", "b"):
                res = arena.play(players[0], players[1], first=first, openings=openings)
                games, plies = games + b, plies + res.plies
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        return games / dt, plies / dt

    print("DeviceArena(%d, %d), greedy, fixed openings, both first movers per match" % (size, b))
    for name, players in variants.items():
        window(players)                                  # graph capture and first use
    for r in range(args.rounds):
        for name, players in variants.items():
            g, p = window(players)
            print("round %d  %-14s %8.1f games/s  %8.1f plies/s" % (r, name, g, p), flush=True)


if __name__ == "__main__":
    main()
