"""SAC with two hidden layers (profiles/sac_mlp3.md): device-event timings, in the shape of tools/td3_mlp3_time.py, of
  plan      rlhip_sac_mlp3_plan_f32 at n = 4096 (Pendulum: 3 -> h -> h -> 2, h = 64 / 256)
  update    one SACPolicy(layers = 3) update at batch 64 / 512 / 4096, h = 64 / 256, beside TD3Policy(layers = 3), the two-layer
            SACPolicy (h = 64) and the same update in torch Float32 autograd with torch.optim.Adam (draws and batch handed over)
Each figure is the median over `--blocks` blocks of the mean of `--reps` back-to-back calls, in microseconds; one JSON line per row.

    python tools/sac_mlp3_time.py [--blocks 7] [--reps 200]
"""
import argparse
import json
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "reinforcementlearning.jl_amd")]
import rlhip as rl  # noqa: E402
from rlhip import sac  # noqa: E402

NS, N_ENV, CAP = 3, 64, 1024


def timed(f, blocks, reps):
    for _ in range(10):
        f()
    out = []
    for _ in range(blocks):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            f()
        b.record()
        torch.cuda.synchronize()
        out.append(1e3 * a.elapsed_time(b) / reps)
    return round(statistics.median(out), 2)


def filled_traces():
    tr = rl.CircularArraySARTSTraces(CAP, N_ENV, NS, action_dtype=torch.float32)
    g = torch.Generator(device="cuda").manual_seed(1)
    r = lambda *s: torch.randn(*s, device="cuda", generator=g)  # noqa: E731
    tr.push_state_(r(NS, N_ENV))
    for _ in range(CAP):
        tr.push_transition_(r(NS, N_ENV), r(N_ENV).clamp(-2, 2), r(N_ENV), (r(N_ENV) > 1.5).to(torch.uint8))
    return tr


def torch_update(h, batch):
    """the same update (critic step, actor step with the alpha step, Polyak) in torch Float32 autograd"""
    mlp = lambda ni, no: torch.nn.Sequential(torch.nn.Linear(ni, h), torch.nn.ReLU(), torch.nn.Linear(h, h), torch.nn.ReLU(),  # noqa: E731
                                             torch.nn.Linear(h, no)).cuda()
    actor, q, qt = mlp(NS, 2), [mlp(NS + 1, 1) for _ in range(2)], [mlp(NS + 1, 1) for _ in range(2)]
    oa = torch.optim.Adam(actor.parameters(), lr=3e-3)
    oq = torch.optim.Adam([p for m in q for p in m.parameters()], lr=3e-3)
    alpha = torch.tensor(0.2, device="cuda")
    s, sn, a, r, cont = (torch.randn(batch, k, device="cuda") for k in (NS, NS, 1, 1, 1))
    e0, e1 = torch.randn(batch, 1, device="cuda"), torch.randn(batch, 1, device="cuda")
    sp = torch.nn.functional.softplus

    def head(x, eps):
        o = actor(x)
        mu, sg = o[:, :1], sp(o[:, 1:])
        z = mu + sg * eps
        return 2.0 * torch.tanh(z), -((z - mu) / sg) ** 2 / 2 - torch.log(sg) - 0.9189385 - 2 * (math.log(2) - z - sp(-2 * z))

    def update():
        nonlocal alpha
        with torch.no_grad():
            un, lpn = head(sn, e0)
            xn = torch.cat([sn, un], 1)
            y = r + 0.99 * cont * (torch.minimum(qt[0](xn), qt[1](xn)) - alpha * lpn)
        x = torch.cat([s, a], 1)
        oq.zero_grad()
        (((q[0](x) - y) ** 2).mean() + ((q[1](x) - y) ** 2).mean()).backward()
        oq.step()
        u, lp = head(s, e1)
        xa = torch.cat([s, u], 1)
        oa.zero_grad()
        (alpha * lp - torch.minimum(q[0](xa), q[1](xa))).mean().backward()
        oa.step()
        alpha = alpha - 3e-3 * (-lp.detach().mean() + 1.0)
        with torch.no_grad():
            for m, mt in zip(q, qt):
                for p, pt in zip(m.parameters(), mt.parameters()):
                    pt.mul_(0.995).add_(p, alpha=0.005)

    return update


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--reps", type=int, default=200)
    a = ap.parse_args()
    env, tr = rl.PendulumEnv(N_ENV, seed=1), filled_traces()
    for h in (64, 256):
        actor = rl.SACPolicy(env, hidden=h, layers=3).actor
        obs, out = torch.randn(NS, 4096, device="cuda"), torch.empty(4096, device="cuda")
        f = lambda: sac.sac_plan(actor, NS, h, 0, obs, 0.0, math.inf, 2.0, 5, 0, 3, action=out, layers=3)  # noqa: E731
        print(json.dumps(dict(series="plan", h=h, n=4096, sac_mlp3_us=timed(f, a.blocks, a.reps))), flush=True)
    for h in (64, 256):
        for batch in (64, 512, 4096):
            idx = torch.randint(0, CAP * N_ENV, (batch,), device="cuda")
            row = dict(series="update", h=h, batch=batch)
            pols = dict(sac_mlp3=rl.SACPolicy(env, hidden=h, batchsize=batch, layers=3), td3_mlp3=rl.TD3Policy(env, hidden=h, batchsize=batch, layers=3))
            if h == 64:
                pols["sac_mlp2"] = rl.SACPolicy(env, hidden=h, batchsize=batch)
            for k, pol in pols.items():
                row[k + "_us"] = timed(lambda: pol.update_(tr, idx), a.blocks, a.reps)
            row["torch_autograd_us"] = timed(torch_update(h, batch), a.blocks, max(10, a.reps // 4))
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
