"""The quantile-regression (QR-DQN) learner (profiles/qrdqn.md): device-event timings, the protocol of tools/c51_time.py

  plan      rlhip_qrdqn_plan_f32 at n = 4096 (CartPole: 4 -> 128 -> 2 x 51) against rlhip_qrdqn_forward_f32 followed by
            rlhip_eps_greedy_select_f32, ALTERNATED block by block in this process
  update    one QRDQNLearner update at batch 32 / 512 / 4096 for 4 -> 128 -> 2 x 51, launch by launch (draw, gather, gradient + fold,
            clip + Adam) and as a whole (with the target sync)
  baseline  the same update in torch Float32 autograd with torch.optim.Adam (the gathered batch handed over, not timed)

    python tools/qrdqn_time.py [--blocks 5] [--reps 100]

Every series runs behind a settle phase of untimed calls; a figure is [median, min, max] microseconds per call over the blocks.
One JSON line per series; the first line stamps the device.  (The C51 figures to compare with come from tools/c51_time.py in the same
session on the same device.)"""
import argparse
import json
import os
import statistics
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--blocks", type=int, default=5)
ap.add_argument("--reps", type=int, default=100)
args = ap.parse_args()
tree = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, tree)
sys.path.insert(0, os.path.join(tree, "reinforcementlearning.jl_amd"))

import torch  # noqa: E402

import rlhip as rl  # noqa: E402
from rlhip import ops, qrdqn  # noqa: E402

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
    """the versions timed in turn, block by block -> {name: [median, min, max]}"""
    settle(list(fs.values()))
    us = {k: [] for k in fs}
    for _ in range(args.blocks):
        for k, f in fs.items():
            us[k].append(block(f))
    return {k: [round(statistics.median(v), 2), round(min(v), 2), round(max(v), 2)] for k, v in us.items()}


props = torch.cuda.get_device_properties(0)
print(json.dumps(dict(device=props.name, cus=props.multi_processor_count, torch=torch.__version__, hip=torch.version.hip, blocks=args.blocks,
                      reps=args.reps, settle_s=SETTLE_S, columns="[median, min, max] us per call")), flush=True)
g = torch.Generator().manual_seed(0)
NS, H, NA, N, KAPPA = 4, 128, 2, 51, 1.0

# ------------------------------------------------------------------------------------------------------------------- plan
n = 4096
x = torch.randn((NS, n), generator=g).cuda()
params = ops.mlp2_init(NS, H, NA * N, 1, 0)
a1, q1 = torch.empty(n, dtype=torch.int32, device="cuda"), torch.empty((NA, n), device="cuda")
q2 = torch.empty((NA, n), device="cuda")


def fused():
    qrdqn.qrdqn_plan(params, NS, H, NA, N, 0, x, 0.1, 5, 0, 3, a1, q1)


def two():
    qrdqn.qrdqn_forward(params, NS, H, NA, N, 0, x, q2)
    ops.eps_greedy_select(q2, 0.1, 5, 3, 0)


print(json.dumps(dict(series="plan", ns=NS, h=H, na=NA, n_quantiles=N, n=n, **alternated(qrdqn_plan=fused, forward_then_select=two))), flush=True)


# ----------------------------------------------------------------------------------------------------------------- update
def torch_update(learner, batch):
    """the update of include/rlhip.h in torch Float32 autograd on a gathered batch, Adam from torch.optim"""
    s, a, r, t, sn = batch[:5]
    b = a.numel()
    cont = 1.0 - t.float()
    net_p = learner.approximator.network.params.clone().requires_grad_(True)
    targ = learner.approximator.target.clone()
    opt = torch.optim.Adam([net_p], lr=1e-3)
    tau = ((2.0 * torch.arange(N, device="cuda") + 1.0) / (2.0 * N))[None, :, None]
    cols = torch.arange(b, device="cuda")
    al = a.long()

    def net(p, xx):
        W1, b1 = p[:H * NS].view(NS, H), p[H * NS:H * NS + H]
        W2, b2 = p[H * NS + H:H * NS + H + NA * N * H].view(H, NA * N), p[H * NS + H + NA * N * H:]
        return (torch.relu(xx.T @ W1 + b1) @ W2 + b2).view(b, NA, N)

    def f():
        with torch.no_grad():
            tht = net(targ, sn)
            T = r[:, None] + 0.99 * cont[:, None] * tht[cols, tht.mean(2).argmax(1)]
        opt.zero_grad(set_to_none=True)
        u = T[:, None, :] - net(net_p, s)[cols, al][:, :, None]  # (b, k, j)
        au = u.abs()
        hub = torch.where(au <= KAPPA, 0.5 * u * u, KAPPA * (au - 0.5 * KAPPA)) / KAPPA
        ((tau - (u < 0).float()).abs() * hub).sum(1).mean(1).mean().backward()
        opt.step()

    return f


for b in (32, 512, 4096):
    n_env, cap = 4096, 16
    env = rl.CartPoleEnv(n_env, seed=3)
    net = rl.HipApproximator(NS, H, NA * N, seed=1)
    learner = rl.QRDQNLearner(rl.TargetNetwork(net, sync_freq=100), NA, n_quantiles=N, kappa=KAPPA, batchsize=b, min_replay_history=1, seed=1)
    tr = rl.CircularArraySARTSTraces(cap, n_env, NS)
    pol = rl.RandomPolicy(env.action_space(), seed=3)
    tr.push_state_(env.state())
    for _ in range(20):
        a = pol.plan_(env)
        env.act_(a)
        tr.push_transition_(env.state(), (a - 1).to(torch.int32), env.reward(), env._done)
    idx = tr.sample_indices(b, 1, 0)
    batch = tr.gather(idx) + (None,)
    tn = learner.approximator

    def draw():
        tr.sample_indices(b, 1, 0)

    def gather():
        tr.gather(idx)

    def gradient():
        s, a_, r, t, sn, _ = batch
        qrdqn.qrdqn_grad_batch(NS, H, NA, N, 0, KAPPA, net.params, tn.target, s, a_, r, t, sn, 0.99, None, None, False, learner.workspace,
                               learner.grad, learner.loss, learner.ql)

    def clip_adam():
        net.optimise_(learner.grad)

    def update():
        learner._update_(tr, False)

    row = alternated(draw=draw, gather=gather, gradient=gradient, clip_adam=clip_adam, update=update, torch_autograd_f32=torch_update(learner, batch))
    print(json.dumps(dict(series="update", ns=NS, h=H, na=NA, n_quantiles=N, batch=b, **row)), flush=True)
