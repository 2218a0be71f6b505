"""Soft Actor-Critic (profiles/sac.md): device-event timings of

  plan      rlhip_sac_plan_f32 at n = 4096 (Pendulum: 3 -> h -> 2, h = 64 / 256) against the three launches it replaces
            (rlhip_mlp2_forward_f32 -> a torch softplus -> rlhip_gaussian_head_sample_f32), ALTERNATED block by block in this process
  update    one SACPolicy update at batch 64 / 512 / 4096, h = 64 / 256, launch by launch (draw, critic gradient + fold, Adam over
            [Q1 | Q2], actor gradient + fold with the alpha step, Adam over the actor, Polyak) and as a whole
  baseline  the same update in torch Float32 autograd with torch.optim.Adam (the draws and the batch handed over, not timed)

    python tools/sac_time.py [--blocks 7] [--reps 200]

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
ap.add_argument("--blocks", type=int, default=7)
ap.add_argument("--reps", type=int, default=200)
args = ap.parse_args()
tree = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, tree)
sys.path.insert(0, os.path.join(tree, "reinforcementlearning.jl_amd"))

import torch  # noqa: E402

import rlhip as rl  # noqa: E402
from rlhip import ops, sac  # noqa: E402
from rlhip._lib import call  # noqa: E402
from rlhip.ops import ptr, stream_ptr  # noqa: E402

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

# ------------------------------------------------------------------------------------------------------------------- plan
n = 4096
x = torch.randn((NS, n), generator=g).cuda()
for h in (64, 256):
    actor = ops.mlp2_init(NS, h, 2, 1, 0)
    a1, lp1 = torch.empty(n, device="cuda"), torch.empty(n, device="cuda")
    out2, a2, lp2 = torch.empty((2, n), device="cuda"), torch.empty(n, device="cuda"), torch.empty(n, device="cuda")

    def fused():
        sac.sac_plan(actor, NS, h, 0, x, 0.0, math.inf, SCALE, 5, 0, 3, action=a1, logp=lp1)

    def three():
        call("rlhip_mlp2_forward_f32", ptr(actor), NS, h, 2, 0, ptr(x), n, ptr(out2), stream_ptr())
        raw = torch.nn.functional.softplus(out2[1])
        call("rlhip_gaussian_head_sample_f32", ptr(out2[0]), ptr(raw), 1, n, 1, 0.0, math.inf, 1, 1, 5, 0, 3, ptr(a2), ptr(lp2), stream_ptr())

    row = alternated(sac_plan=fused, forward_softplus_head=three)
    print(json.dumps(dict(series="plan", ns=NS, h=h, n=n, **row)), flush=True)


# ----------------------------------------------------------------------------------------------------------------- update
def filled_policy(h, b, n_env=4096, cap=16, pushes=20):
    env = rl.PendulumEnv(n_env, seed=3)
    pol = rl.SACPolicy(env, hidden=h, batchsize=b, update_after=1, seed=1)
    tr = rl.CircularArraySARTSTraces(cap, n_env, NS, action_dtype=torch.float32)
    tr.push_state_(env.state())
    for _ in range(pushes):
        a = pol.plan_(env)
        env.act_(a)
        tr.push_transition_(env.state(), a, env.reward(), env._done)
    return pol, tr


def torch_update(pol, tr, b):
    """the update of include/rlhip.h in torch Float32 autograd on a gathered batch, Adam from torch.optim"""
    h = pol.hidden
    s, a, r, t, sn = tr.gather(tr.sample_indices(b, 2, 0))
    cont = 1.0 - t.float()
    eps0, eps1 = torch.randn(b, generator=g).cuda(), torch.randn(b, generator=g).cuda()
    actor, crit = pol.actor.clone().requires_grad_(True), pol.critics.clone().requires_grad_(True)
    targ, alpha = pol.targets.clone(), pol.alpha.clone()
    oa, oc = torch.optim.Adam([actor], lr=3e-3), torch.optim.Adam([crit], lr=3e-3)
    nq = (NS + 1) * h + 2 * h + 1

    def net(p, ni, no, xx):
        W1, b1 = p[:h * ni].view(ni, h), p[h * ni:h * ni + h]
        W2, b2 = p[h * ni + h:h * ni + h + no * h].view(h, no), p[h * ni + h + no * h:]
        return torch.relu(xx.T @ W1 + b1) @ W2 + b2

    def head(p, st, eps):
        o = net(p, NS, 2, st)
        mu, sg = o[:, 0], torch.nn.functional.softplus(o[:, 1])
        z = mu + sg * eps
        zz = (z - mu) / (sg + 1e-8)
        lp = -(zz * zz + math.log(2 * math.pi)) / 2 - torch.log(sg + 1e-8) - 2 * (math.log(2.0) - z - torch.nn.functional.softplus(-2 * z))
        return SCALE * torch.tanh(z), lp

    def f():
        with torch.no_grad():
            un, lpn = head(actor, sn, eps0)
            xn = torch.cat([sn, un[None, :]])
            y = r + 0.99 * cont * (torch.minimum(net(targ[:nq], NS + 1, 1, xn)[:, 0], net(targ[nq:], NS + 1, 1, xn)[:, 0]) - alpha * lpn)
        xx = torch.cat([s, a[None, :]])
        oc.zero_grad(set_to_none=True)
        (((net(crit[:nq], NS + 1, 1, xx)[:, 0] - y) ** 2).mean() + ((net(crit[nq:], NS + 1, 1, xx)[:, 0] - y) ** 2).mean()).backward()
        oc.step()
        u, lp = head(actor, s, eps1)
        xa = torch.cat([s, u[None, :]])
        cd = crit.detach()
        oa.zero_grad(set_to_none=True)
        (alpha * lp - torch.minimum(net(cd[:nq], NS + 1, 1, xa)[:, 0], net(cd[nq:], NS + 1, 1, xa)[:, 0])).mean().backward()
        oa.step()
        with torch.no_grad():
            alpha.sub_(3e-3 * (-lp.mean() - (-1.0)))
            targ.mul_(0.995).add_(cd, alpha=0.005)

    return f


for h in (64, 256):
    for b in (64, 512, 4096):
        pol, tr = filled_policy(h, b)
        idx = tr.sample_indices(b, 2, 0)
        ws = pol.workspace.t

        def draw():
            tr.sample_indices(b, 2, 0)

        def critic_grad():
            sac.sac_critic_grad(tr, h, 0, pol.actor, pol.critics, pol.targets, idx, pol.alpha, 0.99, 0.0, math.inf, SCALE, 2, 0, ws,
                                pol.critic_grad, pol.critic_loss)

        def actor_grad():
            sac.sac_actor_grad(tr, h, 0, pol.actor, pol.critics, idx, pol.alpha, 0.0, math.inf, SCALE, 2, 0, 3e-3, -1.0, pol.alpha, ws,
                               pol.actor_grad, pol.actor_stats)

        def adam_critics():
            pol.critic_opt.step_(pol.critics, pol.critic_grad, 0.0)

        def adam_actor():
            pol.actor_opt.step_(pol.actor, pol.actor_grad, 0.0)

        def polyak():
            ops.polyak_(pol.targets, pol.critics, 0.995)

        def update():
            pol.update_(tr)

        row = alternated(draw=draw, critic_grad=critic_grad, adam_critics=adam_critics, actor_grad=actor_grad, adam_actor=adam_actor,
                         polyak=polyak, update=update, torch_autograd_f32=torch_update(pol, tr, b))
        print(json.dumps(dict(series="update", ns=NS, h=h, batch=b, **row)), flush=True)
