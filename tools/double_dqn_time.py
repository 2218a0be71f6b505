"""Double DQN (profiles/double_dqn.md): event timing of the fold launch alone, of DQNLearner.optimise_ with and without
double_dqn, and (two-layer rows, profiles/fold_stages.md) of rlhip_dqn_sample_fold_f32 -- draw + 3-step window + Double DQN target in
one launch -- through the C ABI on outputs allocated once, each series after a settle phase of untimed calls, as blocks whose median and range are printed.

    python tools/double_dqn_time.py [--tree DIR] [--blocks 7] [--reps 500] [--trace]

--tree DIR: time another checkout of this project (built there), e.g. the parent commit for the baseline of the plain update; a
tree without DoubleTargetFold gets the plain update only.  One process times one tree: to compare two, alternate processes.
--trace: few repetitions and no settle phase, for a run under `rocprofv3 --kernel-trace --stats`.
One JSON line per (layers, hidden, batch), times in microseconds per call; the first line stamps the device and the tree."""
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
ap.add_argument("--trace", action="store_true")
args = ap.parse_args()
tree = os.path.abspath(args.tree)
sys.path.insert(0, tree)
sys.path.insert(0, os.path.join(tree, "reinforcementlearning.jl_amd"))

import torch  # noqa: E402

import rlhip as rl  # noqa: E402

assert os.path.abspath(rl.__file__).startswith(tree), rl.__file__
assert torch.cuda.is_available(), "a timing needs the GPU"
HAS_FOLD = hasattr(rl, "DoubleTargetFold")
HAS_SAMPLE_FOLD = hasattr(rl._lib.lib, "rlhip_dqn_sample_fold_f32")
SETTLE_S = 0.0 if args.trace else 0.3
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


def update(tr, layers, h, batch, **kw):
    net = rl.HipApproximator(4, h, 2, seed=1, layers=layers)
    L = rl.DQNLearner(rl.TargetNetwork(net, sync_freq=100), batchsize=batch, min_replay_history=1, seed=1, **kw)
    traj = rl.Trajectory(tr)
    traj.controller.on_insert_(10 ** 9)
    return lambda: L.optimise_(traj)


def sample_fold(tr, h, batch, n_step=3):
    import ctypes as C

    from rlhip._lib import call
    from rlhip.ops import ptr, stream_ptr

    net = rl.HipApproximator(4, h, 2, seed=1)
    tn = rl.TargetNetwork(net, sync_freq=100)
    folded = rl.CircularArraySARTSTraces(capacity=1, n_env=batch, obs_dim=4)
    idx, iota = (torch.empty(batch, dtype=torch.int64, device="cuda") for _ in range(2))

    def f(_keep=(net, tn, folded, idx, iota)):
        call("rlhip_dqn_sample_fold_f32", C.byref(tr.rb), batch, n_step, 1, 0.99, 1, 0, h, 2, 0, ptr(net.params), ptr(tn.target),
             C.byref(folded.rb), ptr(idx), ptr(iota), stream_ptr())

    return f


props = torch.cuda.get_device_properties(0)
print(json.dumps(dict(device=props.name, cus=props.multi_processor_count, torch=torch.__version__, hip=torch.version.hip, tree=tree,
                      has_fold=HAS_FOLD, has_sample_fold=HAS_SAMPLE_FOLD, blocks=args.blocks, reps=args.reps, settle_s=SETTLE_S, columns="[median, min, max] us")), flush=True)
tr = ring()
for layers, h in ((2, 128), (3, 128), (3, 256)):
    for batch in (512, 4096):
        row = dict(layers=layers, h=h, batch=batch)
        row["update_plain"] = timed(update(tr, layers, h, batch))
        if HAS_FOLD:
            net = rl.HipApproximator(4, h, 2, seed=1, layers=layers)
            tn = rl.TargetNetwork(net, sync_freq=100)
            idx = tr.sample_indices(batch, 1, 0)
            fold = rl.DoubleTargetFold()
            row["fold"] = timed(lambda: fold.fold(tr, idx, net, tn.target, tn.target_packed, 0.99))
            row["update_double"] = timed(update(tr, layers, h, batch, double_dqn=True))
            row["update_plain_again"] = timed(update(tr, layers, h, batch))
        if HAS_SAMPLE_FOLD and layers == 2:
            row["sample_fold"] = timed(sample_fold(tr, h, batch))
        print(json.dumps(row), flush=True)
