#!/usr/bin/env python
"""A complete RainbowDQN-style self-play loop on the HIP path (what GN0/RainbowDQN's train.py does with the reference
pieces, README.md:5,7 flags): 128 parallel Hex-11 envs, eps-greedy acting with the online network, n-step (2) transitions
into two prioritized replay rings (maker / breaker), double-DQN targets from a target network, importance-weighted MSE,
Adam, priority updates.  Everything between two prints stays on the GPU except one read-back per 16-move rollout -- and with
--device-store not even that: the transitions are assembled and stored on the device, and the host reads one small pinned
record per iteration, an iteration late.

    python examples/selfplay_train.py --iters 50

The reference's training script itself lives in an un-vendored submodule and is not rebuilt; this file shows how its loop
maps onto the drop-in API and measures end-to-end frames/s and updates/s."""
import argparse
import copy
import os
import sys
import time
from argparse import Namespace

os.environ.setdefault("DEBUG_CLR_GRAPH_PACKET_CAPTURE", "0")      # gnn_hex_amd/graphs.py
import torch  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gnn_hex_amd import ops  # noqa: E402
from gnn_hex_amd.models import get_pre_defined  # noqa: E402
from gnn_hex_amd.multi_env_manager import (DeviceRollout, DeviceTransitionFeed, Env_manager, EpsSchedule,  # noqa: E402
                                           RolloutStitcher)
from gnn_hex_amd.replay import GraphedUpdate, GraphReplayBuffer  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hex-size", type=int, default=11)
    ap.add_argument("--envs", type=int, default=128)
    ap.add_argument("--layers", type=int, default=15)
    ap.add_argument("--hidden", type=int, default=110)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warm", type=int, default=5, help="untimed iterations first (graph capture, first launches, allocator)")
    ap.add_argument("--rollout", type=int, default=16, help="moves per env between updates")
    ap.add_argument("--updates", type=int, default=2, help="gradient steps per side and iteration")
    ap.add_argument("--math", default="fp32", choices=["fp32", "f16x3"])
    ap.add_argument("--no-graph", action="store_true")
    ap.add_argument("--async-rollout", action="store_true",
                    help="issue the next rollout before this iteration's updates: the GPU plays while the host prepares "
                         "the update batches; the actor's weights are then one iteration (4 updates) old")
    ap.add_argument("--graph-updates", action="store_true",
                    help="every update as ONE HIP graph per side (replay.GraphedUpdate): the draw is sized on the device, so "
                         "the host neither waits for the drawn slots nor issues the update's launches one by one "
                         "(fp32 only; with --no-graph the same sequence is issued eagerly, still without a host wait)")
    ap.add_argument("--device-store", action="store_true",
                    help="assemble the n-step transitions and store them in the replay rings on the device "
                         "(multi_env_manager.DeviceTransitionFeed): no run_end, no host assembly, no put_block; every run "
                         "continues the previous one on the device.  Implies --graph-updates")
    ap.add_argument("--eps-schedule", metavar="INIT,FINAL,DECAY_FRAMES", default=None,
                    help="the recipe's exploration schedule (--init_eps=0.12 --final_eps=0.05 --eps_decay_frames=100000 is "
                         "0.12,0.05,100000): epsilon is computed on the device per ply (multi_env_manager.EpsSchedule), so it "
                         "decays under the one captured rollout and with --device-store.  Default: a fixed epsilon of 0.12")
    args = ap.parse_args()
    schedule = None
    if args.eps_schedule is not None:
        try:
            e0, e1, decay = args.eps_schedule.split(",")
            schedule = EpsSchedule(float(e0), float(e1), int(decay))
        except ValueError as err:
            ap.error("--eps-schedule INIT,FINAL,DECAY_FRAMES: %s" % err)
    if args.device_store:
        if args.async_rollout:
            ap.error("--device-store issues rollout, store and updates in stream order: there is no host work to hide "
                     "behind --async-rollout")
        args.graph_updates = True
    ops.set_math(args.math)
    gamma, n_step = 0.97, 2
    margs = Namespace(num_layers=args.layers, hidden_channels=args.hidden, norm=False, noisy_dqn=False, noisy_sigma0=0.5,
                      num_head_layers=2)
    torch.manual_seed(0)
    q_net = get_pre_defined("modern_two_headed", margs).cuda()
    target_net = copy.deepcopy(q_net)
    # one launch for all 66 parameter tensors; capturable (step counts on the device) when it runs inside the updates' graphs
    opt = torch.optim.Adam(q_net.parameters(), lr=4e-4, fused=True, capturable=args.graph_updates)
    graphed = {}                       # --graph-updates: side -> GraphedUpdate, built when its buffer first holds a batch
    mgr = Env_manager(args.envs, args.hex_size, gamma=gamma, n_steps=[n_step])
    mgr.reset()
    cap = 65536
    bufs = {True: GraphReplayBuffer(cap, args.hex_size, prioritized=True, alpha=0.5),
            False: GraphReplayBuffer(cap, args.hex_size, prioritized=True, alpha=0.5)}
    rollout = DeviceRollout(mgr, q_net, steps=args.rollout, eps=schedule if schedule is not None else 0.12, graph=not args.no_graph)
    stitch = RolloutStitcher(mgr)      # carries the last 2 * n_step moves of a rollout into the next assembly
    feed = DeviceTransitionFeed(rollout, bufs[True], bufs[False]) if args.device_store else None
    frames = updates = games = games0 = 0
    last_loss = float("nan")
    t0 = time.perf_counter()
    ahead = None
    for it in range(-args.warm, args.iters):
        if it == 0:       # start of the timed part
            torch.cuda.synchronize()
            frames = updates = games = 0
            if feed is not None:
                feed.settle()         # (outside the timed part: the games of the untimed iterations are all counted now)
                games0 = feed.games
            t0 = time.perf_counter()
        frames += args.envs * args.rollout
        if feed is not None:
            # rollout, assembly, store: issued, never waited for.  push() consumes the PREVIOUS push's record (pinned, long
            # complete), which is what the sizes below are: the host runs at most one iteration ahead of the GPU
            if it == -args.warm:
                rollout.run_begin()
            else:
                rollout.run_continue()
            feed.push()
        else:
            res = rollout.run_end(ahead) if ahead is not None else rollout.run()
            games += int(res.dones.sum())
            mb, bb = stitch.assemble(res)
            bufs[True].put_block(mb)
            bufs[False].put_block(bb)
        # Updates alternate between the two buffers, and a buffer's next draw (stream-ordered behind its own priority
        # update) is started right after its update is issued: while the host waits for those indices and builds that
        # batch, the GPU runs the OTHER buffer's update.
        # (device store: the settled size, one push old, once a side's update exists -- len() would wait for this push's record)
        sides = [sd for sd in (True, False) if (bufs[sd].size if feed is not None and sd in graphed else len(bufs[sd])) >= args.batch]
        pending = {} if args.graph_updates else {sd: bufs[sd].sample_begin(args.batch, beta=0.6) for sd in sides}
        # (after put_block: the run overwrites the snapshot ring; after the first draws: they need not wait for the rollout)
        ahead = rollout.run_begin() if args.async_rollout else None
        for k in range(args.updates):
            for side in sides:
                buf = bufs[side]
                if args.graph_updates:
                    if side not in graphed:
                        graphed[side] = GraphedUpdate(buf, q_net, target_net, opt, args.batch, gamma ** n_step, "mse",
                                                      graph=not args.no_graph)
                    last_loss, _ = graphed[side].step(beta=0.6)
                    updates += 1
                    continue
                idx, w, s, s2, act, r, d = buf.sample_end(pending[side])
                # double DQN: argmax of the online net over each next state's non-terminal nodes, target net's value there --
                # both networks in one forward launch, y = r + gamma^n * q_tg[argmax] * (~d).float() formed by one more
                y, _ = ops.double_dqn_targets(q_net, target_net, s2.x, s2.edge_index, s2.batch, s2.ptr, r, d, gamma ** n_step)
                q = q_net(s.x, s.edge_index, s.batch, s.ptr)
                loss, td = ops.td_loss(q, s.ptr[:-1] + act.long(), y, w, "mse")
                opt.zero_grad(set_to_none=True)
                ops.backward(loss)
                opt.step()
                buf.update_priorities(idx, td.abs() + 1e-3)
                if k + 1 < args.updates:
                    pending[side] = buf.sample_begin(args.batch, beta=0.6)
                updates += 1
                last_loss = loss.detach()
        if (it + 1) % 10 == 0 and it >= 0:
            target_net.load_state_dict(q_net.state_dict())
            if schedule is not None:      # the host's own frame count: nothing is read back
                print("iteration %d: %d env frames issued, epsilon %.5f"
                      % (it + 1, rollout.frames_issued, schedule.value(rollout.frames_issued)))
    if ahead is not None:
        rollout.run_end(ahead)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    if feed is not None:
        feed.settle()
        games = feed.games - games0
    print("hex %d, %d envs, GNN %dx%d, math %s%s%s%s: %.0f env frames/s, %.1f updates/s (batch %d), %d games finished, last loss %.4f"
          % (args.hex_size, args.envs, args.layers, args.hidden, args.math, ", rollout one iteration ahead" if args.async_rollout else "",
             (", device store" if args.device_store else ", graphed updates") if args.graph_updates else "",
             ", eps schedule %s" % args.eps_schedule if schedule is not None else "", frames / dt, updates / dt, args.batch, games,
             float(last_loss)))


if __name__ == "__main__":
    main()
