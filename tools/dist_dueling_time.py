"""Dueling distributional heads (profiles/dist_dueling.md): device-event timings, the protocol of tools/noisy_time.py

  fold      rlhip_noisy_dueling_fold_f32 (both nets) and rlhip_noisy_dueling_unfold_grad_f32 against their two-launch compositions,
            ALTERNATED block by block, at (4, 128, 2, 51) and (4, 256, 4, 51)
  plan      rlhip_noisy_c51_dueling_plan_f32 at n = 4096 against rlhip_noisy_c51_plan_f32 (CartPole: 4 -> 128 -> 2 x 51)
  update    one RainbowLearner update at batch 32 / 512 / 4096 over the two new approximators against plain and noisy C51
  learn     --learn STEPS: CartPole, 4096 envs, noisy + dueling + prioritized + 3-step + Double DQN, eps = 0; mean episode length per
            250 vec-steps

    python tools/dist_dueling_time.py [--blocks 5] [--reps 100] [--only plan] [--learn 1250]

Every series runs behind a settle phase of untimed calls; a figure is [median, min, max] microseconds per call over the blocks.
One JSON line per series; the first line stamps the device."""
import argparse
import json
import os
import statistics
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--blocks", type=int, default=5)
ap.add_argument("--reps", type=int, default=100)
ap.add_argument("--only", default="")
ap.add_argument("--learn", type=int, default=0)
args = ap.parse_args()
tree = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, tree)
sys.path.insert(0, os.path.join(tree, "reinforcementlearning.jl_amd"))

import torch  # noqa: E402

import rlhip as rl  # noqa: E402
from rlhip import ops  # noqa: E402

assert torch.cuda.is_available(), "a timing needs the GPU"
SETTLE_S = 0.3


def settle(fs):
    t_end = time.perf_counter() + SETTLE_S
    while time.perf_counter() < t_end:
        for f in fs:
            for _ in range(16):
                f()
        torch.cuda.synchronize()


def block(f):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(args.reps):
        f()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / args.reps * 1e3


def alternated(**fs):
    settle(list(fs.values()))
    us = {k: [] for k in fs}
    for _ in range(args.blocks):
        for k, f in fs.items():
            us[k].append(block(f))
    return {k: [round(statistics.median(v), 2), round(min(v), 2), round(max(v), 2)] for k, v in us.items()}


props = torch.cuda.get_device_properties(0)
print(json.dumps(dict(device=props.name, cus=props.multi_processor_count, torch=torch.__version__, hip=torch.version.hip, blocks=args.blocks,
                      reps=args.reps, settle_s=SETTLE_S, plan_tile=rl.noisy_plan_tile(), columns="[median, min, max] us per call")), flush=True)
g = torch.Generator().manual_seed(0)
NS, H, NA, K = 4, 128, 2, 51

if args.only in ("", "fold"):
    for ns, h, na, k in ((4, 128, 2, 51), (4, 256, 4, 51)):
        rows, shape = (1 + na) * k, (ns, h, na, k)
        nd, ne = ops.mlp2_nparams(ns, h, rows), ops.mlp2_nparams(ns, h, na * k)
        n1, n2, gr = (torch.randn(n, generator=g).cuda() for n in (2 * nd, 2 * nd, ne))
        e1, e2, m1, m2, gm = (torch.empty(n, device="cuda") for n in (ne, ne, nd, nd, nd))
        gn = torch.empty(2 * nd, device="cuda")

        def two_fold():
            ops.noisy_fold(n1, m1, ns, h, rows, 3, 9, n2, m2)
            ops.dist_dueling_fold(m1, e1, *shape, m2, e2)

        def two_unfold():
            ops.noisy_unfold_grad(ops.dist_dueling_unfold_grad(gr, gm, *shape), gn, ns, h, rows, 3, 9)

        row = alternated(fused_fold=lambda: ops.noisy_dueling_fold(n1, e1, *shape, 3, 9, n2, e2), two_launch_fold=two_fold,
                         fused_unfold=lambda: ops.noisy_dueling_unfold_grad(gr, gn, *shape, 3, 9), two_launch_unfold=two_unfold,
                         plain_dueling_fold=lambda: ops.dist_dueling_fold(m1, e1, *shape, m2, e2))
        print(json.dumps(dict(series="fold", ns=ns, h=h, na=na, K=k, **row)), flush=True)

if args.only in ("", "plan"):
    n = 4096
    x = torch.randn((NS, n), generator=g).cuda()
    duel, noisy = rl.noisy_init(NS, H, (1 + NA) * K, 1), rl.noisy_init(NS, H, NA * K, 1)
    a1, q1, a2, q2 = (torch.empty(s, dtype=d, device="cuda") for s, d in ((n, torch.int32), ((NA, n), torch.float32)) * 2)
    row = alternated(noisy_dueling_plan=lambda: rl.noisy_c51_dueling_plan(duel, NS, H, NA, K, 0, 0.0, 200.0, x, 0.0, 5, 0, 3, a1, q1),
                     noisy_c51_plan=lambda: rl.noisy_c51_plan(noisy, NS, H, NA, K, 0, 0.0, 200.0, x, 0.0, 5, 0, 3, a2, q2))
    print(json.dumps(dict(series="plan", ns=NS, h=H, na=NA, n_atoms=K, n=n, **row)), flush=True)

if args.only in ("", "update"):
    for bsz in (32, 512, 4096):
        n_env, cap = 4096, 16
        env = rl.CartPoleEnv(n_env, seed=3)
        mk = lambda net: rl.RainbowLearner(rl.TargetNetwork(net, sync_freq=100), NA, n_atoms=K, v_min=0.0, v_max=200.0, batchsize=bsz,  # noqa: E731
                                           min_replay_history=1, seed=1)
        ls = dict(noisy_dueling_update=mk(rl.NoisyDuelingApproximator(NS, H, NA, K, seed=1)),
                  noisy_dueling_two_launch_update=mk(rl.NoisyDuelingApproximator(NS, H, NA, K, seed=1, fused=False)),
                  dueling_update=mk(rl.DistDuelingApproximator(NS, H, NA, K, seed=1)),
                  noisy_update=mk(rl.NoisyApproximator(NS, H, NA * K, seed=1)), c51_update=mk(rl.HipApproximator(NS, H, NA * K, seed=1)))
        tr = rl.CircularArraySARTSTraces(cap, n_env, NS)
        pol = rl.RandomPolicy(env.action_space(), seed=3)
        tr.push_state_(env.state())
        for _ in range(20):
            act = pol.plan_(env)
            env.act_(act)
            tr.push_transition_(env.state(), (act - 1).to(torch.int32), env.reward(), env._done)
        row = alternated(**{name: (lambda l=l: l._update_(tr, False)) for name, l in ls.items()})
        print(json.dumps(dict(series="update", ns=NS, h=H, na=NA, n_atoms=K, batch=bsz, **row)), flush=True)

if args.learn:
    n, chunk = 4096, 250
    env = rl.CartPoleEnv(n, seed=5)
    learner = rl.RainbowLearner(rl.TargetNetwork(rl.NoisyDuelingApproximator(4, 128, 2, 51, seed=5), sync_freq=100), 2, n_atoms=51, v_min=0.0,
                                v_max=200.0, batchsize=512, min_replay_history=n, seed=5, n_step=3, double_dqn=True, per_beta=0.4)
    tr = rl.CircularPrioritizedTraces(256, n, 4, n_step=3)
    agent = rl.Agent(rl.QBasedPolicy(learner, rl.EpsilonGreedyExplorer(0.0, seed=5)), rl.Trajectory(tr))
    curve, t0 = [], time.perf_counter()
    for _ in range(args.learn // chunk):
        rl.run(agent, env, rl.StopAfterNSteps(chunk))
        term = tr.gather(torch.arange(len(tr) * n, device="cuda"))[3]
        curve.append(round(len(tr) * n / max(1.0, float(term.sum())), 1))
    print(json.dumps(dict(series="learn", eps=0.0, form="noisy + dueling + prioritized + 3-step + Double DQN", vec_steps=args.learn,
                          ep_len_per_250_vec_steps=curve, updates=learner.n_updates, seconds=round(time.perf_counter() - t0, 2))), flush=True)
