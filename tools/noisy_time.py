"""NoisyDense networks (profiles/noisy.md): device-event timings, the protocol of tools/iqn_time.py

  plan      rlhip_noisy_c51_plan_f32 at n = 4096 (CartPole: 4 -> 128 -> 2 x 51) against rlhip_c51_plan_f32, ALTERNATED block by block
  fold      rlhip_noisy_fold_f32 (both nets) + rlhip_noisy_unfold_grad_f32 against the same arithmetic in torch on staged factor vectors,
            at the three shapes of tests/test_gpu_noisy.py
  update    one RainbowLearner update at batch 32 / 512 / 4096 over a NoisyApproximator against the plain C51 update on the same ring
  learn     --learn STEPS: the CartPole curve of tests/test_gpu_noisy.py, mean episode length per 250 vec-steps

    python tools/noisy_time.py [--blocks 5] [--reps 100] [--only plan] [--learn 2500]

Every series runs behind a settle phase of untimed calls; a figure is [median, min, max] microseconds per call over the blocks.
One JSON line per series; the first line stamps the device and the plan kernel's tile."""
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

if args.only in ("", "plan"):
    n = 4096
    x = torch.randn((NS, n), generator=g).cuda()
    noisy = rl.noisy_init(NS, H, NA * K, 1)
    plain = ops.mlp2_init(NS, H, NA * K, 1, 0)
    a1, q1, a2, q2 = (torch.empty(s, dtype=d, device="cuda") for s, d in ((n, torch.int32), ((NA, n), torch.float32)) * 2)
    row = alternated(noisy_c51_plan=lambda: rl.noisy_c51_plan(noisy, NS, H, NA, K, 0, 0.0, 200.0, x, 0.0, 5, 0, 3, a1, q1),
                     c51_plan=lambda: rl.c51_plan(plain, NS, H, NA, K, 0, 0.0, 200.0, x, 0.0, 5, 0, 3, a2, q2))
    print(json.dumps(dict(series="plan", ns=NS, h=H, na=NA, n_atoms=K, n=n, **row)), flush=True)

if args.only in ("", "fold"):
    for ns, h, M in ((2, 4, 2), (4, 128, 102), (16, 256, 256)):
        np_ = rl.noisy_nparams(ns, h, M) // 2
        n1, n2, gr = (torch.randn(k, generator=g).cuda() for k in (2 * np_, 2 * np_, np_))
        e1, e2, gn = torch.empty(np_, device="cuda"), torch.empty(np_, device="cuda"), torch.empty(2 * np_, device="cuda")
        a, b, c, d = (torch.randn(k, generator=g).cuda() for k in (ns, h, h, M))  # torch gets its factors for free

        def torch_fold_unfold():
            xi = torch.cat([torch.outer(a, b).reshape(-1), b, torch.outer(c, d).reshape(-1), d])
            o1, o2 = torch.addcmul(n1[:np_], n1[np_:], xi), torch.addcmul(n2[:np_], n2[np_:], xi)
            return o1, o2, torch.cat([gr, gr * xi])

        def fold_unfold():
            ops.noisy_fold(n1, e1, ns, h, M, 3, 9, n2, e2)
            ops.noisy_unfold_grad(gr, gn, ns, h, M, 3, 9)

        row = alternated(fold_plus_unfold=fold_unfold, fold=lambda: ops.noisy_fold(n1, e1, ns, h, M, 3, 9, n2, e2), torch_same_arithmetic=torch_fold_unfold)
        print(json.dumps(dict(series="fold", ns=ns, h=h, M=M, **row)), flush=True)

if args.only in ("", "update"):
    for bsz in (32, 512, 4096):
        n_env, cap = 4096, 16
        env = rl.CartPoleEnv(n_env, seed=3)
        mk = lambda net: rl.RainbowLearner(rl.TargetNetwork(net, sync_freq=100), NA, n_atoms=K, v_min=0.0, v_max=200.0, batchsize=bsz,  # noqa: E731
                                           min_replay_history=1, seed=1)
        noisy_l, plain_l = mk(rl.NoisyApproximator(NS, H, NA * K, seed=1)), mk(rl.HipApproximator(NS, H, NA * K, seed=1))
        tr = rl.CircularArraySARTSTraces(cap, n_env, NS)
        pol = rl.RandomPolicy(env.action_space(), seed=3)
        tr.push_state_(env.state())
        for _ in range(20):
            act = pol.plan_(env)
            env.act_(act)
            tr.push_transition_(env.state(), (act - 1).to(torch.int32), env.reward(), env._done)
        row = alternated(noisy_update=lambda: noisy_l._update_(tr, False), c51_update=lambda: plain_l._update_(tr, False))
        print(json.dumps(dict(series="update", ns=NS, h=H, na=NA, n_atoms=K, batch=bsz, **row)), flush=True)

if args.learn:
    n, chunk = 4096, 250
    env = rl.CartPoleEnv(n, seed=5)
    learner = rl.RainbowLearner(rl.TargetNetwork(rl.NoisyApproximator(4, 128, 2 * 51, seed=5), sync_freq=100), 2, n_atoms=51, v_min=0.0, v_max=200.0,
                                batchsize=512, min_replay_history=n, seed=5)
    tr = rl.CircularArraySARTSTraces(256, n, 4)
    agent = rl.Agent(rl.QBasedPolicy(learner, rl.EpsilonGreedyExplorer(0.0, seed=5)), rl.Trajectory(tr))
    curve, t0 = [], time.perf_counter()
    for _ in range(args.learn // chunk):
        rl.run(agent, env, rl.StopAfterNSteps(chunk))
        term = tr.gather(torch.arange(len(tr) * n, device="cuda"))[3]
        curve.append(round(len(tr) * n / max(1.0, float(term.sum())), 1))
    print(json.dumps(dict(series="learn", eps=0.0, vec_steps=args.learn, ep_len_per_250_vec_steps=curve, updates=learner.n_updates,
                          seconds=round(time.perf_counter() - t0, 2))), flush=True)
