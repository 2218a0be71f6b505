"""The fused prioritized vec-step (profiles/per_fused_step.md), two measurements in one process.

A. microseconds per vec-step of `rlhip.run` (the per-stage loop, unchanged by the fused step) against `rlhip.run_fused_dqn_prioritized`
   on two identically built agents: 4096-env CartPole, 4 -> 128 -> 2, capacity 256 (2^20 leaves), beta = 0.4; batch 32 / 512 x
   n_step 1 / 3 x Double DQN off / on, and the 4 -> 128 -> 128 -> 2 net at batch 512.  Host clock around a whole run that ends in a
   device synchronise; both forms warmed with --warmup vec-steps, then --rounds alternations of --steps vec-steps each.
B. rlhip_per_writeback_f32 against rlhip_per_priority_f32 + rlhip_sumtree_update on a 2^20-leaf tree, 32 / 512 / 4096 keys, HIP
   events round blocks of --reps back-to-back calls, --alternations times in the order one launch, two launches, one launch again.
The spread of a form against itself comes first in every line: for A the range of the rounds of one form, for B the median distance
between the two one-launch blocks of an alternation.  One JSON line per row, times in microseconds.

    python tools/per_step_time.py [--only A|B|T] [--steps 500] [--rounds 4] [--warmup 200] [--alternations 300] [--reps 20]

--only T: nothing is timed -- the fused loop alone (batch 512, n_step 3, Double DQN) for --steps vec-steps, to be run under
`rocprofv3 --kernel-trace --stats -- python tools/per_step_time.py --only T` for the kernel list of one vec-step."""
import argparse
import json
import os
import statistics
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--only", default="")
ap.add_argument("--steps", type=int, default=500)
ap.add_argument("--rounds", type=int, default=4)
ap.add_argument("--warmup", type=int, default=200)
ap.add_argument("--alternations", type=int, default=300)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--envs", type=int, default=4096)
ap.add_argument("--capacity", type=int, default=256)
args = ap.parse_args()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "reinforcementlearning.jl_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import rlhip as rl  # noqa: E402

assert torch.cuda.is_available(), "a timing needs the GPU"


def agent(layers, batch, n_step, double):
    n = args.envs
    env = rl.HipVecEnv("cartpole", n, seed=4, continuous=False)
    net = rl.HipApproximator(env.odim, 128, 2, seed=4, layers=layers)
    learner = rl.DQNLearner(rl.TargetNetwork(net, sync_freq=100), batchsize=batch, min_replay_history=4 * n, seed=4, max_grad_norm=1.0,
                            n_step=n_step, double_dqn=double, per_beta=0.4)
    policy = rl.QBasedPolicy(learner, rl.EpsilonGreedyExplorer(0.05, kind="exp", decay_steps=1000, seed=4))
    traces = rl.CircularPrioritizedTraces(capacity=args.capacity, n_env=n, obs_dim=env.odim, n_step=n_step)
    return rl.Agent(policy, rl.Trajectory(traces)), env


def timed_run(loop, ag, env, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    loop(ag, env, rl.StopAfterNSteps(steps))
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e6


def measurement_a():
    rows = [(2, b, n, d) for b in (32, 512) for n in (1, 3) for d in (False, True)] + [(3, 512, 1, False)]
    for layers, batch, n_step, double in rows:
        forms = {"per_stage": (rl.run,) + agent(layers, batch, n_step, double),
                 "fused": (rl.run_fused_dqn_prioritized,) + agent(layers, batch, n_step, double)}
        for loop, ag, env in forms.values():
            timed_run(loop, ag, env, args.warmup)
        us = {k: [] for k in forms}
        for _ in range(args.rounds):
            for k, (loop, ag, env) in forms.items():
                us[k].append(round(timed_run(loop, ag, env, args.steps), 2))
        same = torch.equal(forms["per_stage"][1].policy.learner.approximator.network.params,
                           forms["fused"][1].policy.learner.approximator.network.params)
        med = {k: statistics.median(v) for k, v in us.items()}
        print(json.dumps(dict(measurement="A", layers=layers, batch=batch, n_step=n_step, double=double,
                              spread_same_form_us={k: round(max(v) - min(v), 2) for k, v in us.items()}, rounds_us=us,
                              median_us={k: round(v, 2) for k, v in med.items()}, factor=round(med["per_stage"] / med["fused"], 2),
                              timed_steps_per_form=args.rounds * args.steps, params_bit_identical=same)), flush=True)


def measurement_b():
    from rlhip._lib import call
    from rlhip.ops import ptr, stream_ptr

    n_leaves = 1 << 20
    tree = torch.zeros(int(rl._lib.lib.rlhip_sumtree_nodes(n_leaves)), dtype=torch.float32, device="cuda")
    s = stream_ptr()
    call("rlhip_sumtree_fill_range", ptr(tree), n_leaves, 0, n_leaves, 1.0, s)
    rng = np.random.default_rng(0)
    for n in (32, 512, 4096):
        key = torch.as_tensor(rng.integers(0, n_leaves, n), device="cuda")
        td = torch.as_tensor(rng.standard_normal(n).astype(np.float32), device="cuda")
        out = torch.empty_like(td)

        def one():
            call("rlhip_per_writeback_f32", ptr(tree), n_leaves, ptr(key), ptr(td), n, 1e-6, 0.6, ptr(out), s)

        def two():
            call("rlhip_per_priority_f32", ptr(td), n, 1e-6, 0.6, ptr(out), s)
            call("rlhip_sumtree_update", ptr(tree), n_leaves, ptr(key), ptr(out), n, s)

        def block(f):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.reps):
                f()
            b.record()
            b.synchronize()
            return a.elapsed_time(b) / args.reps * 1e3

        for f in (one, two) * 20:  # warm both shapes
            block(f)
        t1, t2, t1b = [], [], []
        for _ in range(args.alternations):
            t1.append(block(one))
            t2.append(block(two))
            t1b.append(block(one))
        r = lambda x: round(x, 2)  # noqa: E731
        print(json.dumps(dict(measurement="B", keys=n, leaves=n_leaves, alternations=args.alternations, calls_per_block=args.reps,
                              spread_same_form_us=r(statistics.median(abs(a - b) for a, b in zip(t1, t1b))),
                              one_launch_us=dict(median=r(statistics.median(t1 + t1b)), min=r(min(t1 + t1b))),
                              two_launches_us=dict(median=r(statistics.median(t2)), min=r(min(t2))),
                              gain_us=r(statistics.median(t2) - statistics.median(t1 + t1b)))), flush=True)


props = torch.cuda.get_device_properties(0)
print(json.dumps(dict(device=props.name, cus=props.multi_processor_count, torch=torch.__version__, hip=torch.version.hip, envs=args.envs,
                      capacity=args.capacity, steps=args.steps, rounds=args.rounds, warmup=args.warmup)), flush=True)
if args.only == "T":
    ag, env = agent(2, 512, 3, True)
    rl.run_fused_dqn_prioritized(ag, env, rl.StopAfterNSteps(args.steps))
    torch.cuda.synchronize()
    print(json.dumps(dict(trace="fused loop only", vec_steps=args.steps, updates=ag.policy.learner.n_updates)), flush=True)
if args.only in ("", "B"):
    measurement_b()
if args.only in ("", "A"):
    measurement_a()
