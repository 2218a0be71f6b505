"""TD3 / DDPG with two hidden layers (profiles/td3_mlp3.md): device-event timings, in the shape of tools/td3_time.py, of

  plan      rlhip_td3_mlp3_plan_f32 at n = 4096 (Pendulum: 3 -> h -> h -> 1, h = 64 / 256) beside the two-layer rlhip_td3_plan_f32
  update    one TD3Policy(layers = 3) update at batch 64 / 512 / 4096, h = 64 / 256, launch by launch (critic launches + fold, actor launch
            + fold) and as a whole with policy_freq = 1, beside the two-layer kernels at the same h, ALTERNATED block by block
  baseline  the same three-layer update in torch Float32 autograd with torch.optim.Adam (noise and batch handed over, not timed)

    python tools/td3_mlp3_time.py [--blocks 7] [--reps 200]

Every series runs behind a settle phase of untimed calls; a figure is [median, min, max] microseconds per call over the blocks.
One JSON line per series; the first line stamps the device."""
import argparse
import json
import os
import statistics
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--blocks", type=int, default=7)
ap.add_argument("--reps", type=int, default=200)
args = ap.parse_args()
tree = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, tree)
sys.path.insert(0, os.path.join(tree, "reinforcementlearning.jl_amd"))

import torch  # noqa: E402

import rlhip as rl  # noqa: E402
from rlhip import td3  # noqa: E402

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
NS, SCALE = 3, 2.0


def filled(h, b, layers, n_env=4096, cap=16, pushes=20):
    env = rl.PendulumEnv(n_env, seed=3)
    pol = rl.TD3Policy(env, hidden=h, batchsize=b, update_after=1, seed=1, policy_freq=1, layers=layers)
    tr = rl.CircularArraySARTSTraces(cap, n_env, NS, action_dtype=torch.float32)
    tr.push_state_(env.state())
    for _ in range(pushes):
        a = pol.plan_(env)
        env.act_(a)
        tr.push_transition_(env.state(), a, env.reward(), env._done)
    return pol, tr, env


def torch_update(pol, tr, b):
    """the three-layer update of include/rlhip.h in torch Float32 autograd on a gathered batch, Adam from torch.optim, policy_freq = 1"""
    h = pol.hidden
    s, a, r, t, sn = tr.gather(tr.sample_indices(b, 2, 0))
    cont = 1.0 - t.float()
    e = (0.2 * torch.randn(b, generator=g)).clamp_(-0.5, 0.5).cuda()
    actor, crit = pol.actor.clone().requires_grad_(True), pol.critics.clone().requires_grad_(True)
    at, ct = pol.actor_target.clone(), pol.critic_targets.clone()
    oa, oc = torch.optim.Adam([actor], lr=3e-3), torch.optim.Adam([crit], lr=3e-3)
    nq = (NS + 1) * h + h + h * h + 2 * h + 1

    def net(p, ni, xx):
        o = h * ni + h
        a1 = torch.relu(xx.T @ p[:h * ni].view(ni, h) + p[h * ni:o])
        a2 = torch.relu(a1 @ p[o:o + h * h].view(h, h) + p[o + h * h:o + h * h + h])
        return a2 @ p[o + h * h + h:o + h * h + 2 * h] + p[o + h * h + 2 * h]

    def f():
        with torch.no_grad():
            xn = torch.cat([sn, (SCALE * torch.tanh(net(at, NS, sn)) + e).clamp(-SCALE, SCALE)[None, :]])
            y = r + 0.99 * cont * torch.minimum(net(ct[:nq], NS + 1, xn), net(ct[nq:], NS + 1, xn))
        xx = torch.cat([s, a[None, :]])
        oc.zero_grad(set_to_none=True)
        (((net(crit[:nq], NS + 1, xx) - y) ** 2).mean() + ((net(crit[nq:], NS + 1, xx) - y) ** 2).mean()).backward()
        oc.step()
        oa.zero_grad(set_to_none=True)
        (-net(crit.detach()[:nq], NS + 1, torch.cat([s, (SCALE * torch.tanh(net(actor, NS, s)))[None, :]])).mean()).backward()
        oa.step()
        with torch.no_grad():
            at.mul_(0.995).add_(actor, alpha=0.005)
            ct.mul_(0.995).add_(crit, alpha=0.005)

    return f


for h in (64, 256):
    pols = {L: filled(h, 64, L) for L in (2, 3)}
    a1 = torch.empty(4096, device="cuda")
    plan = lambda L: lambda: td3.td3_plan(pols[L][0].actor, NS, h, 0, pols[L][2].state(), SCALE, 0.1, -SCALE, SCALE, 5, 0, 3, action=a1, layers=L)  # noqa: E731
    print(json.dumps(dict(series="plan", ns=NS, h=h, n=4096, **alternated(mlp3_plan=plan(3), mlp2_plan=plan(2)))), flush=True)
    for b in (64, 512, 4096):
        fs = {}
        for L, tag in ((3, "mlp3"), (2, "mlp2")):
            pol, tr, _ = filled(h, b, L)
            idx = tr.sample_indices(b, 2, 0)

            def critic_grad(pol=pol, tr=tr, idx=idx, L=L):
                td3.td3_critic_grad(tr, h, 0, 2, pol.actor_target, pol.critics, pol.critic_targets, idx, 0.99, SCALE, 0.2, 0.5, -SCALE, SCALE, 2, 0,
                                    pol.workspace.t, pol.critic_grad, pol.critic_loss, layers=L)

            def actor_grad(pol=pol, tr=tr, idx=idx, L=L):
                td3.td3_actor_grad(tr, h, 0, pol.actor, pol.critics, idx, SCALE, pol.workspace.t, pol.actor_grad, pol.actor_stats, layers=L)

            fs.update({f"{tag}_critic_grad": critic_grad, f"{tag}_actor_grad": actor_grad, f"{tag}_update": lambda pol=pol, tr=tr: pol.update_(tr)})
            if L == 3:
                fs["torch_autograd_f32"] = torch_update(pol, tr, b)
        print(json.dumps(dict(series="update", ns=NS, h=h, batch=b, **alternated(**fs))), flush=True)
