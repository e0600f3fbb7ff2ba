#!/usr/bin/env python
"""Double-DQN targets: the fused call (ops.double_dqn_targets: both networks in one load-balanced forward launch + one target
launch) against the plain sequence (two model calls, ops.greedy_nodes, the torch expression -- the call's own fallback), and
ops.multi_forward([model]) against the plain model call, on seeded mid-game batches ("D1") of the tests' helpers.

    python tools/time_dqn_targets.py [--window 2.0] [--repeats 5] [--only NAME]

Per configuration: both variants are warmed up, then alternate in the same process; a window runs calls back to back for at
least --window seconds and ends in a device synchronise (host clock around it); --repeats windows per variant; median and
spread (min .. max) of the time per call.  The outputs of the two variants are compared bit for bit first.  One JSON line per
configuration at the end."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from helpers import batch_tensors, make_pair  # noqa: E402
from gnn_hex_amd import ops  # noqa: E402

GAMMA_N = 0.97 ** 2
CONFIGS = [      # (name, body layers, hidden, board sizes, what)
    ("GNN-L Hex-11 B=256 D1", 15, 110, [11] * 256, "targets"),
    ("GNN-S Hex-7 B=256 D1", 10, 35, [7] * 256, "targets"),
    ("GNN-L Hex-5..11 mix B=256 D1", 15, 110, ([5, 6, 7, 8, 9, 10, 11] * 37)[:256], "targets"),
    ("GNN-L Hex-11 B=768 D1, one model", 15, 110, [11] * 768, "single"),
]


def device_batch(sizes):
    x, ei, batch, ptr = batch_tensors("D1", sizes)
    xd, eid = x.cuda(), ei.cuda()
    ops.attach_hints(xd, True, int((ptr[1:] - ptr[:-1]).max()))      # what a replay buffer knows on the host
    eid._hex_grouped = True
    return xd, eid, batch.cuda(), ptr.cuda()


def window(fn, seconds):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    calls = 0
    while True:
        for _ in range(10):
            fn()
        calls += 10
        if time.perf_counter() - t0 >= seconds:
            break
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=2.0)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--only", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    out = []
    for name, layers, hidden, sizes, what in CONFIGS:
        if args.only and args.only not in name:
            continue
        online = make_pair(layers, hidden, seed=0)[0]
        target = make_pair(layers, hidden, seed=1)[0]
        dev = device_batch(sizes)
        b = len(sizes)
        gen = torch.Generator().manual_seed(3)
        r = (torch.rand(b, generator=gen) * 2 - 1).cuda()
        d = (torch.rand(b, generator=gen) < 0.2).cuda()
        if what == "targets":
            def fused():
                return ops.double_dqn_targets(online, target, *dev, r, d, GAMMA_N)

            def plain():
                with torch.no_grad():
                    q_on = online(*dev)
                    q_tg = target(*dev)
                    a2 = ops.greedy_nodes(q_on, dev[3])
                    return r + GAMMA_N * q_tg[a2] * (~d).float(), a2
            assert ops._multi_plan([online, target], *dev) is not None, "the fused form does not apply to this configuration"
        else:
            def fused():
                return tuple(ops.multi_forward([online], *dev))

            def plain():
                with torch.no_grad():
                    return (online(*dev),)
        for _ in range(5):          # warm-up of both variants (code objects, allocator)
            f, p = fused(), plain()
        torch.cuda.synchronize()
        assert all(torch.equal(u, v) for u, v in zip(f, p)), "fused and plain results differ"
        tf, tp = [], []
        for _ in range(args.repeats):      # alternating windows
            tf.append(window(fused, args.window))
            tp.append(window(plain, args.window))
        rec = {"config": name, "window_s": args.window, "repeats": args.repeats,
               "fused_us": [round(1e6 * v, 1) for v in tf], "plain_us": [round(1e6 * v, 1) for v in tp],
               "fused_median_us": round(1e6 * statistics.median(tf), 1), "plain_median_us": round(1e6 * statistics.median(tp), 1),
               "ratio_plain_over_fused": round(statistics.median(tp) / statistics.median(tf), 3)}
        print("%-36s fused %8.1f us (%.1f .. %.1f)   plain %8.1f us (%.1f .. %.1f)   plain / fused %.3f"
              % (name, rec["fused_median_us"], 1e6 * min(tf), 1e6 * max(tf), rec["plain_median_us"], 1e6 * min(tp), 1e6 * max(tp),
                 rec["ratio_plain_over_fused"]), flush=True)
        out.append(rec)
    for rec in out:
        print(json.dumps(rec))


if __name__ == "__main__":
    main()
