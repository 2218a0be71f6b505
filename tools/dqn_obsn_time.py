"""DQN on observations of 5..16 components (profiles/dqn_obsn.md): device-event timings of

  plan      rlhip_dqn_plan_obsn_f32 at n = 4096, 6 -> 128 -> 3, against the two launches it replaces (rlhip_mlp2_forward_f32 ->
            rlhip_eps_greedy_select_f32), the two versions ALTERNATED block by block inside this process
  gradient  rlhip_dqn_grad_batch_f32 at batch 32 / 512 / 4096 for 6 -> 128 -> 3 and 16 -> 256 -> 3; beside it, for context,
            rlhip_dqn_grad_idx_f32 at ns = 4 with the same hidden width and batch (the nearest shipped kernel; it gathers from a
            record ring inside the launch) and Float32 torch autograd of the same loss
  update    one whole DQNLearner.optimise_ (draw + gather + gradient + clip / Adam) at batch 512 on a six-component frame ring,
            and the record-ring learner at ns = 4 beside it

    python tools/dqn_obsn_time.py [--blocks 7] [--reps 300]

Every series runs behind a settle phase of untimed calls; a figure is [median, min, max] microseconds per call over the blocks.
One JSON line per series; the first line stamps the device."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--blocks", type=int, default=7)
ap.add_argument("--reps", type=int, default=300)
args = ap.parse_args()
tree = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, tree)
sys.path.insert(0, os.path.join(tree, "reinforcementlearning.jl_amd"))

import torch  # noqa: E402

import rlhip as rl  # noqa: E402
from rlhip import dqn  # noqa: E402
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

# ------------------------------------------------------------------------------------------------------------------- plan
ns, h, na, n = 6, 128, 3, 4096
net = rl.HipApproximator(ns, h, na, seed=1)
x = torch.randn((ns, n), generator=g).cuda()
a1, q1 = torch.empty(n, dtype=torch.int32, device="cuda"), torch.empty((na, n), device="cuda")
a2, q2 = torch.empty_like(a1), torch.empty_like(q1)


def fused():
    call("rlhip_dqn_plan_obsn_f32", ptr(net.params), ns, h, na, 0, ptr(x), n, 0.1, 5, 0, 3, ptr(a1), ptr(q1), stream_ptr())


def pair():
    call("rlhip_mlp2_forward_f32", ptr(net.params), ns, h, na, 0, ptr(x), n, ptr(q2), stream_ptr())
    call("rlhip_eps_greedy_select_f32", ptr(q2), na, n, n, 1, None, 0.1, 0, 5, 0, 3, ptr(a2), stream_ptr())


row = alternated(plan_obsn=fused, forward_then_select=pair)
assert torch.equal(a1, a2) and torch.equal(q1, q2)
print(json.dumps(dict(series="plan", ns=ns, h=h, na=na, n=n, **row)), flush=True)


# --------------------------------------------------------------------------------------------------------------- gradient
def record_ring(n_env=4096, cap=16, pushes=20):
    env = rl.CartPoleEnv(n_env, seed=3)
    tr = rl.CircularArraySARTSTraces(capacity=cap, n_env=n_env, obs_dim=4)
    tr.push_state_(env.state())
    for _ in range(pushes):
        a = torch.randint(0, 2, (n_env,), generator=g, dtype=torch.int32).cuda()
        env.act0_(a)
        tr.push_transition_(env.state(), a, env.reward(), env._done)
    return tr


def torch_grad(ns, h, na, p, pt, s, a, r, t, sn, gamma):
    def net_(pp, xx):
        W1, b1 = pp[:h * ns].view(ns, h), pp[h * ns:h * ns + h]
        W2, b2 = pp[h * ns + h:h * ns + h + na * h].view(h, na), pp[h * ns + h + na * h:]
        return torch.relu(xx.T @ W1 + b1) @ W2 + b2

    P = p.clone().requires_grad_(True)
    af, cont = a.long()[:, None], 1.0 - t.float()

    def f():
        P.grad = None
        with torch.no_grad():
            y = r + gamma * cont * net_(pt, sn).max(1).values
        loss = torch.nn.functional.huber_loss(net_(P, s).gather(1, af)[:, 0], y, delta=1.0)
        loss.backward()

    return f


rec = record_ring()
for ns, h in ((6, 128), (16, 256)):
    na = 3
    net, net4 = rl.HipApproximator(ns, h, na, seed=1), rl.HipApproximator(4, h, na, seed=1)
    pt, pt4 = net.params.clone(), net4.params.clone()
    for b in (32, 512, 4096):
        s, sn = torch.randn((ns, b), generator=g).cuda(), torch.randn((ns, b), generator=g).cuda()
        a = torch.randint(0, na, (b,), generator=g, dtype=torch.int32).cuda()
        r, t = torch.randn(b, generator=g).cuda(), (torch.rand(b, generator=g) < 0.1).to(torch.uint8).cuda()
        ws = dqn.dqn_batch_workspace(ns, h, na, b)
        grad, loss, td = torch.empty_like(net.params), torch.empty(1, device="cuda"), torch.empty(b, device="cuda")
        ws4, grad4 = dqn.dqn_workspace(4, h, na, b), torch.empty_like(net4.params)
        idx = rec.sample_indices(b, 1, 0)

        def batch_form():
            dqn.dqn_grad_batch(ns, h, na, 0, net.params, pt, s, a, r, t, sn, 0.99, 1.0, None, None, False, ws, grad, loss, td)

        def ring_form_ns4():
            call("rlhip_dqn_grad_idx_f32", C.byref(rec.rb), h, na, 0, ptr(net4.params), ptr(pt4), b, ptr(idx), 0.99, 1.0, ptr(ws4), ptr(grad4),
                 ptr(loss), ptr(td), stream_ptr())

        row = alternated(grad_batch=batch_form, grad_idx_ns4=ring_form_ns4, torch_autograd_f32=torch_grad(ns, h, na, net.params, pt, s, a, r, t, sn, 0.99))
        print(json.dumps(dict(series="gradient", ns=ns, h=h, na=na, batch=b, **row)), flush=True)


# ----------------------------------------------------------------------------------------------------------------- update
def learner(traces, n_in, n_act, **kw):
    L = rl.DQNLearner(rl.TargetNetwork(rl.HipApproximator(n_in, 128, n_act, seed=1), sync_freq=100), batchsize=512, min_replay_history=1, seed=1, **kw)
    traj = rl.Trajectory(traces)
    traj.controller.on_insert_(10 ** 9)
    return lambda: L.optimise_(traj)


def frame_ring(cls=None, n_env=4096, cap=16, pushes=20, **kw):
    env = rl.AcrobotRK4Env(n_env, seed=3)
    tr = (cls or rl.CircularArraySARTSTraces)(cap, n_env, 6, **kw)
    tr.push_state_(env.state())
    for _ in range(pushes):
        a = torch.randint(0, 3, (n_env,), generator=g, dtype=torch.int32).cuda()
        env.act0_(a)
        tr.push_transition_(env.state(), a, env.reward(), env._done)
    return tr


row = alternated(update_obs6_uniform=learner(frame_ring(), 6, 3), update_obs4_record_ring=learner(rec, 4, 2),
                 update_obs6_nstep3=learner(frame_ring(), 6, 3, n_step=3),
                 update_obs6_per_nstep3=learner(frame_ring(rl.CircularPrioritizedFrameTraces, n_step=3), 6, 3, n_step=3, per_beta=0.4))
print(json.dumps(dict(series="update", batch=512, h=128, **row)), flush=True)
