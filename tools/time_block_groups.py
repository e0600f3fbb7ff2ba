"""Eager training step (forward, TD loss, backward) of GNN-L (15 x 110) on a uniform Hex-13 batch of 256 graphs, start boards and
mid-game boards: the batch whose block table (512 blocks for start boards) exceeds one resident set of workgroups.

    python tools/time_block_groups.py [--root DIR] [--graphs 256] [--windows 5] [--seconds 2.0] [--pack]

Each board set is timed over ``--windows`` windows of at least ``--seconds`` each, every window ending in a device synchronise;
the median and min..max of the windows' per-step times are printed, with the launch form the collation chose.  ``--root`` is the
checkout whose ``gnn_hex_amd`` is imported (default: the one this file lies in).  Only ``Batch.from_data_list`` and
``ops.td_step`` are used (``groups=True`` where the collation knows it), so the script also runs against a build of a commit
without block groups, where the same batch takes one launch per layer: run the two alternately for a comparison."""
import argparse
import inspect
import os
import statistics
import sys
import time

import torch

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def data_list(kind, graphs, dev):
    """``graphs`` Hex-13 positions as single-graph Data objects (the collation's input)."""
    from gnn_hex_amd.data import Data
    from helpers import batch_tensors
    x, ei, _, ptr = batch_tensors(kind, [13] * graphs, maker=True)
    p = ptr.tolist()
    owner = torch.bucketize(ei[0], ptr[1:], right=True)
    cnt = torch.bincount(owner, minlength=graphs).tolist()
    assert bool((owner[1:] >= owner[:-1]).all())                 # edges grouped by graph, in graph order
    out, e0 = [], 0
    for g in range(graphs):
        d = Data(x=x[p[g]:p[g + 1]].to(dev), edge_index=(ei[:, e0:e0 + cnt[g]] - p[g]).to(dev))
        d.x._hex_is_maker = True
        out.append(d)
        e0 += cnt[g]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=HERE)
    ap.add_argument("--graphs", type=int, default=256)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--seconds", type=float, default=2.0)
    ap.add_argument("--pack", action="store_true", help="collate with pack=True (a replay draw) instead of the caller's order")
    args = ap.parse_args()
    if args.windows < 5 or args.seconds < 2.0:
        ap.error("at least 5 windows of at least 2 s")
    root = os.path.abspath(args.root)
    sys.path.insert(0, os.path.join(HERE, "tests"))
    sys.path.insert(0, HERE)                     # (oracle/: the board generator)
    sys.path.insert(0, root)
    import gnn_hex_amd
    from gnn_hex_amd import ops
    from gnn_hex_amd.data import Batch
    from helpers import make_pair, sel_and_targets
    assert os.path.abspath(os.path.dirname(os.path.dirname(gnn_hex_amd.__file__))) == root
    dev = torch.device("cuda:0")
    hip, _ = make_pair(15, 110, seed=0, device=dev)
    params = list(hip.parameters())
    print("root %s  graphs %d  pack %s" % (root, args.graphs, args.pack), flush=True)
    for kind, name in (("D0", "start boards"), ("D1", "mid-game boards")):
        kw = {"groups": True} if "groups" in inspect.signature(Batch.from_data_list).parameters else {}
        bt = Batch.from_data_list(data_list(kind, args.graphs, dev), pack=args.pack, **kw)
        sel, tgt = sel_and_targets(bt.ptr.cpu(), seed=1)
        sel, tgt = sel.to(dev), tgt.to(dev)
        blk, grp = getattr(bt.edge_index, "_hex_blocks", None), getattr(bt.edge_index, "_hex_block_groups", None)
        form = "table of %d blocks" % blk[1] if blk is not None else \
            ("%d blocks in groups %s" % (grp[1], list(grp[2])) if grp is not None else "no table")

        def step():
            for p in params:
                p.grad = None
            return ops.td_step(hip, bt.x, bt.edge_index, bt.batch, bt.ptr, sel=sel, target=tgt)[0]

        for _ in range(20):
            loss = step()
        torch.cuda.synchronize()
        assert bool(torch.isfinite(loss).all())
        per_step = []
        for _ in range(args.windows):
            steps, t0 = 0, time.perf_counter()
            while True:
                for _ in range(10):
                    step()
                steps += 10
                if time.perf_counter() - t0 >= args.seconds:
                    break
            torch.cuda.synchronize()
            per_step.append((time.perf_counter() - t0) / steps * 1e3)
        print("%-16s n=%-6d %-44s step median %.3f ms  (min %.3f .. max %.3f, %d windows)"
              % (name, int(bt.x.shape[0]), form, statistics.median(per_step), min(per_step), max(per_step), len(per_step)),
              flush=True)


if __name__ == "__main__":
    main()
