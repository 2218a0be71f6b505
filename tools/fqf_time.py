"""The FQF learner (profiles/fqf.md): device-event timings, the protocol of tools/iqn_time.py

  plan      rlhip_fqf_plan_f32 at n = 4096, N = 32 (CartPole: 4 -> 128, n_cos = 64, 2 actions) against rlhip_iqn_plan_f32 at K = 32,
            ALTERNATED block by block in this process
  update    one FQFLearner update at batch 32 / 512 / 4096 with N = 32: the gradient entry alone and the whole update, against the same
            update in torch Float32 autograd with torch.optim.Adam on both vectors (the gathered batch handed over) and against one
            IQNLearner update at N = N' = 32 on the same ring

    python tools/fqf_time.py [--blocks 5] [--reps 100]

Every series runs behind a settle phase of untimed calls; a figure is [median, min, max] microseconds per call over the blocks.
One JSON line per series; the first line stamps the device."""
import argparse
import json
import math
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
from rlhip import fqf, iqn  # noqa: E402

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
NS, H, NA, NC, N, KAPPA = 4, 128, 2, 64, 32, 1.0

# ------------------------------------------------------------------------------------------------------------------- plan
n = 4096
x = torch.randn((NS, n), generator=g).cuda()
fnet = rl.FQFApproximator(NS, H, NA, N, NC, seed=1)
a1, q1, a2, q2 = (torch.empty(n, dtype=torch.int32, device="cuda"), torch.empty((NA, n), device="cuda"), torch.empty(n, dtype=torch.int32, device="cuda"),
                  torch.empty((NA, n), device="cuda"))


def fqf_plan():
    fqf.fqf_plan(fnet.params, fnet.frac_params, NS, H, NA, NC, N, 0, x, 0.1, 5, 0, 3, a1, q1)


def iqn_plan():
    iqn.iqn_plan(fnet.params, NS, H, NA, NC, N, 0, x, 0.1, 5, 0, 3, a2, q2)


print(json.dumps(dict(series="plan", ns=NS, h=H, na=NA, n_cos=NC, N=N, n=n, **alternated(fqf_plan=fqf_plan, iqn_plan_K32=iqn_plan))), flush=True)


# ----------------------------------------------------------------------------------------------------------------- update
def torch_update(learner, batch):
    """the update of include/rlhip.h in torch Float32 autograd on a gathered batch, Adam from torch.optim on both vectors"""
    s, a, r, t, sn = batch[:5]
    b = a.numel()
    cont = 1.0 - t.float()
    net = learner.approximator.network
    net_p, frac_p = net.params.clone().requires_grad_(True), net.frac_params.clone().requires_grad_(True)
    targ = learner.approximator.target.clone()
    opt, fopt = torch.optim.Adam([net_p], lr=1e-3), torch.optim.Adam([frac_p], lr=1e-5)
    cols, al = torch.arange(b, device="cuda"), a.long()
    e = math.pi * torch.arange(1, NC + 1, device="cuda", dtype=torch.float32)
    o = [H * NS, H, H * NC, H, NA * H]

    def psi_of(p, xx):
        return torch.relu(xx.T @ p[:H * NS].view(NS, H) + p[H * NS:H * NS + H])

    def net_at(p, psi, tau):  # psi (b, h), tau (b, L) -> (b, L, na)
        _, _, Wp, bp, W2, b2 = torch.split(p, o + [NA])
        phi = torch.relu(torch.cos(tau[:, :, None] * e) @ Wp.view(NC, H) + bp)
        return (psi[:, None, :] * phi) @ W2.view(H, NA) + b2

    def f():
        psi = psi_of(net_p, s)
        q = torch.softmax(psi.detach() @ frac_p[:N * H].view(H, N) + frac_p[N * H:], 1)
        tau = torch.cat([torch.zeros((b, 1), device="cuda"), q.cumsum(1)], 1)
        that, d = (0.5 * (tau[:, 1:] + tau[:, :-1])).detach(), (tau[:, 1:] - tau[:, :-1]).detach()
        with torch.no_grad():
            tht = net_at(targ, psi_of(targ, sn), that)
            T = r[:, None] + 0.99 * cont[:, None] * tht[cols, :, (d[:, :, None] * tht).sum(1).argmax(1)]
        opt.zero_grad(set_to_none=True)
        fopt.zero_grad(set_to_none=True)
        th = net_at(net_p, psi, that)[cols, :, al]
        u = T[:, None, :] - th[:, :, None]  # (b, n, j)
        au = u.abs()
        hub = torch.where(au <= KAPPA, 0.5 * u * u, KAPPA * (au - 0.5 * KAPPA)) / KAPPA
        ((that[:, :, None] - (u < 0).float()).abs() * hub).sum(1).mean(1).mean().backward()
        with torch.no_grad():
            gf = 2.0 * net_at(net_p, psi, tau[:, 1:-1])[cols, :, al] - th[:, 1:] - th[:, :-1]
        (gf * tau[:, 1:-1]).sum(1).mean().backward()
        opt.step()
        fopt.step()

    return f


for b in (32, 512, 4096):
    n_env, cap = 4096, 16
    env = rl.CartPoleEnv(n_env, seed=3)
    net = rl.FQFApproximator(NS, H, NA, N, NC, seed=1)
    learner = rl.FQFLearner(rl.TargetNetwork(net, sync_freq=100), NA, N, NC, kappa=KAPPA, batchsize=b, min_replay_history=1, seed=1)
    il = rl.IQNLearner(rl.TargetNetwork(rl.IQNApproximator(NS, H, NA, NC, seed=1), sync_freq=100), NA, N=N, N_target=N, K=N, kappa=KAPPA,
                       batchsize=b, min_replay_history=1, seed=1)
    tr = rl.CircularArraySARTSTraces(cap, n_env, NS)
    pol = rl.RandomPolicy(env.action_space(), seed=3)
    tr.push_state_(env.state())
    for _ in range(20):
        a = pol.plan_(env)
        env.act_(a)
        tr.push_transition_(env.state(), (a - 1).to(torch.int32), env.reward(), env._done)
    batch = tr.gather(tr.sample_indices(b, 1, 0)) + (None,)
    tn = learner.approximator

    def gradient():
        s, a_, r, t, sn, _ = batch
        fqf.fqf_grad_batch(NS, H, NA, NC, N, 0, KAPPA, 0.0, net.params, tn.target, net.frac_params, s, a_, r, t, sn, 0.99, None, None, False,
                           learner.workspace, learner.grad, net.frac_grad, learner.loss, learner.ql)

    def update():
        learner._update_(tr, False)

    def iqn_update():
        il._update_(tr, False)

    row = alternated(gradient=gradient, update=update, iqn_update_N32=iqn_update, torch_autograd_f32=torch_update(learner, batch))
    print(json.dumps(dict(series="update", ns=NS, h=H, na=NA, n_cos=NC, N=N, batch=b, **row)), flush=True)
