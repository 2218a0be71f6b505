"""Prioritized n-step replay (profiles/per_nstep.md): event timing of rlhip_per_sample_fold_nstep_f32 against the two launches it
replaces (rlhip_ring_sample_prioritized -> rlhip_ring_fold_nstep; both through the C ABI on outputs allocated once) and of
DQNLearner.optimise_ on prioritized traces with n_step = 3 against the 1-step prioritized learner, each series after a settle phase
of untimed calls, as blocks whose median and range are printed.  The method of tools/double_dqn_time.py.

    python tools/per_nstep_time.py [--tree DIR] [--label TEXT] [--blocks 7] [--reps 500] [--envs 4096] [--batch 512] [--n-step 3]

--tree DIR: time another checkout of this project (built there), e.g. the parent commit for the 1-step prioritized baseline; a tree
without rlhip_per_sample_fold_nstep_f32 gets that baseline only.  One process times one tree: to compare two, alternate processes.
One JSON line per series, times in microseconds per call; the first line stamps the device, the tree (relative to the working
directory) and --label, a free text that names the commit of that tree."""
import argparse
import json
import os
import statistics
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--label", default="")
ap.add_argument("--blocks", type=int, default=7)
ap.add_argument("--reps", type=int, default=500)
ap.add_argument("--envs", type=int, default=4096)
ap.add_argument("--batch", type=int, default=512)
ap.add_argument("--n-step", type=int, default=3)
args = ap.parse_args()
tree = os.path.abspath(args.tree)
sys.path.insert(0, tree)
sys.path.insert(0, os.path.join(tree, "reinforcementlearning.jl_amd"))

import torch  # noqa: E402

import rlhip as rl  # noqa: E402

assert os.path.abspath(rl.__file__).startswith(tree), rl.__file__
assert torch.cuda.is_available(), "a timing needs the GPU"
HAS_FUSED = hasattr(rl._lib.lib, "rlhip_per_sample_fold_nstep_f32") and hasattr(rl.NStepBatchSampler, "sample_fold_prioritized")
SETTLE_S = 0.3


def ring(n_step, cap=64, pushes=80):
    n = args.envs
    env = rl.CartPoleEnv(n, seed=3)
    kw = dict(n_step=n_step) if n_step > 1 else {}
    tr = rl.CircularPrioritizedTraces(capacity=cap, n_env=n, obs_dim=4, **kw)
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


def update(tr, layers=2, h=128, **kw):
    net = rl.HipApproximator(4, h, 2, seed=1, layers=layers)
    L = rl.DQNLearner(rl.TargetNetwork(net, sync_freq=100), batchsize=args.batch, min_replay_history=1, seed=1, per_beta=0.4, **kw)
    traj = rl.Trajectory(tr)
    traj.controller.on_insert_(10 ** 9)
    return lambda: L.optimise_(traj)


def draw_and_fold(tr, n):
    """(fused, two launches): both through the C ABI on outputs allocated ONCE, so that the series differ by the launches alone"""
    import ctypes as C

    from rlhip._lib import call
    from rlhip.ops import ptr, stream_ptr

    b, dev = args.batch, tr.state.device
    idx, key = torch.empty(b, dtype=torch.int64, device=dev), torch.empty(b, dtype=torch.int64, device=dev)
    prio, iota = torch.empty(b, dtype=torch.float32, device=dev), torch.empty(b, dtype=torch.int64, device=dev)
    folded = rl.CircularArraySARTSTraces(capacity=1, n_env=b, obs_dim=tr.obs_dim, device=dev)
    keep = (idx, key, prio, iota, folded)

    def fused(_keep=keep):
        call("rlhip_per_sample_fold_nstep_f32", C.byref(tr.rb), ptr(tr.priorities), b, n, 0.99, 1, 0, ptr(idx), ptr(key), ptr(prio),
             C.byref(folded.rb), ptr(iota), stream_ptr())

    def two(_keep=keep):
        call("rlhip_ring_sample_prioritized", C.byref(tr.rb), ptr(tr.priorities), b, 1, 0, ptr(idx), ptr(key), ptr(prio), stream_ptr())
        call("rlhip_ring_fold_nstep", C.byref(tr.rb), ptr(idx), b, n, 0.99, C.byref(folded.rb), ptr(iota), stream_ptr())

    return fused, two


props = torch.cuda.get_device_properties(0)
print(json.dumps(dict(device=props.name, cus=props.multi_processor_count, torch=torch.__version__, hip=torch.version.hip,
                      tree=os.path.relpath(tree), label=args.label, has_fused=HAS_FUSED, envs=args.envs, batch=args.batch, n_step=args.n_step, blocks=args.blocks, reps=args.reps,
                      settle_s=SETTLE_S, columns="[median, min, max] us")), flush=True)
print(json.dumps(dict(series="update_1step_prioritized", us=timed(update(ring(1))))), flush=True)
if HAS_FUSED:
    n = args.n_step
    tr = ring(n)
    fused, two = draw_and_fold(tr, n)
    # A / B / A: the first series again at the end shows how far the machine moved meanwhile
    print(json.dumps(dict(series="fused_draw_fold", us=timed(fused))), flush=True)
    print(json.dumps(dict(series="two_launches", us=timed(two))), flush=True)
    print(json.dumps(dict(series="fused_draw_fold_again", us=timed(fused))), flush=True)
    print(json.dumps(dict(series="update_nstep_prioritized", us=timed(update(tr, n_step=n)))), flush=True)
    print(json.dumps(dict(series="update_nstep_prioritized_double", us=timed(update(tr, n_step=n, double_dqn=True)))), flush=True)
print(json.dumps(dict(series="update_1step_prioritized_again", us=timed(update(ring(1))))), flush=True)
