"""DuelingNetwork fold (profiles/dueling.md): event timing of the per-stage DQN update (DQNLearner.optimise_, config 2, batch 512)
with a plain HipApproximator and with a DuelingApproximator, for 4->128->2 (two layers), 4->128->128->2 and 4->256->256->2, and of the
fold / unfold launches alone -- each series after a settle phase of untimed calls, as blocks whose median and
range are printed.

    python tools/dueling_time.py [--tree DIR] [--blocks 7] [--reps 500] [--sync-freq 100] [--trace]

--tree DIR: time another checkout of this project (built there), e.g. the parent commit for the baseline of the plain update; a
tree without DuelingApproximator gets the plain update only.  One process times one tree: to compare two, alternate processes.
--sync-freq 1: every update is a sync step (one more fold launch for the target).
--trace: few repetitions and no settle phase, for a run under `rocprofv3 --kernel-trace --stats`.
One JSON line per network, times in microseconds per call; the first line stamps the device and the tree."""
import argparse
import json
import os
import statistics
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--blocks", type=int, default=7)
ap.add_argument("--reps", type=int, default=500)
ap.add_argument("--sync-freq", type=int, default=100)
ap.add_argument("--trace", action="store_true")
args = ap.parse_args()
tree = os.path.abspath(args.tree)
sys.path.insert(0, tree)
sys.path.insert(0, os.path.join(tree, "reinforcementlearning.jl_amd"))

import torch  # noqa: E402

import rlhip as rl  # noqa: E402

assert os.path.abspath(rl.__file__).startswith(tree), rl.__file__
assert torch.cuda.is_available(), "a timing needs the GPU"
HAS_DUELING = hasattr(rl, "DuelingApproximator")
SETTLE_S = 0.0 if args.trace else 0.3
BATCH = 512
if args.trace:
    args.blocks, args.reps = 1, 200


def ring(n=4096, cap=64, pushes=80):
    env = rl.CartPoleEnv(n, seed=3)
    tr = rl.CircularArraySARTSTraces(capacity=cap, n_env=n, obs_dim=4)
    tr.push_state_(env.state())
    g = torch.Generator().manual_seed(0)
    for _ in range(pushes):
        a = torch.randint(0, 2, (n,), generator=g, dtype=torch.int32).cuda()
        env.act0_(a)
        tr.push_transition_(env.state(), a, env.reward(), env._done)
    return tr


def timed(f):
    """-> (median, min, max) microseconds per call over `blocks` event-timed blocks of `reps` calls, behind a settle phase"""
    t_end = time.perf_counter() + SETTLE_S
    while True:
        for _ in range(16):
            f()
        torch.cuda.synchronize()
        if time.perf_counter() >= t_end:
            break
    us = []
    for _ in range(args.blocks):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(args.reps):
            f()
        e.record()
        torch.cuda.synchronize()
        us.append(s.elapsed_time(e) / args.reps * 1e3)
    return [round(statistics.median(us), 2), round(min(us), 2), round(max(us), 2)]


def update(tr, cls, layers, h):
    net = cls(4, h, 2, seed=1, layers=layers)
    L = rl.DQNLearner(rl.TargetNetwork(net, sync_freq=args.sync_freq), batchsize=BATCH, min_replay_history=1, seed=1)
    traj = rl.Trajectory(tr)
    traj.controller.on_insert_(10 ** 9)
    return lambda: L.optimise_(traj)


props = torch.cuda.get_device_properties(0)
print(json.dumps(dict(device=props.name, cus=props.multi_processor_count, torch=torch.__version__, hip=torch.version.hip, tree=tree,
                      has_dueling=HAS_DUELING, batch=BATCH, sync_freq=args.sync_freq, blocks=args.blocks, reps=args.reps,
                      settle_s=SETTLE_S, columns="[median, min, max] us")), flush=True)
tr = ring()
for layers, h in ((2, 128), (3, 128), (3, 256)):
    row = dict(layers=layers, h=h)
    row["update_plain"] = timed(update(tr, rl.HipApproximator, layers, h))
    if HAS_DUELING:
        from rlhip import dqn

        net = rl.DuelingApproximator(4, h, 2, seed=1, layers=layers)
        g, gd = torch.zeros_like(net.params), torch.zeros_like(net.dueling_params)
        row["fold"] = timed(lambda: dqn.fold_dueling(net.dueling_params, net.params, 4, h, 2, layers))
        row["unfold"] = timed(lambda: dqn.unfold_dueling_grad(g, gd, 4, h, 2, layers))
        row["update_dueling"] = timed(update(tr, rl.DuelingApproximator, layers, h))
        row["update_plain_again"] = timed(update(tr, rl.HipApproximator, layers, h))
    print(json.dumps(row), flush=True)
