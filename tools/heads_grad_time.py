"""Pullback kernels of the diagonal Gaussian heads (profiles/heads_grad.md): event timing of rlhip_gaussian_head_logp_bwd_f32 (the
SoftGaussianNetwork form, atanhf included), of rlhip_gaussian_head_sample_bwd_f32 (SoftGaussianNetwork with both cotangents, and
GaussianNetwork), of the forward sampling launch at the same shape -- what regenerating the draws costs is one forward's worth of
Philox + Box-Muller -- and of what a user runs without them: torch Float32 autograd (forward and backward) over the reference's
SoftGaussianNetwork formulas with a saved noise tensor, on the same device.  Each series runs after a settle phase of untimed calls, as
blocks of event-timed calls whose median and range are printed.

    python tools/heads_grad_time.py [--blocks 7] [--reps 50] [--torch-reps 3]

Fractions are of 8 TB/s against the algorithmic bytes, 4 (4 d + (d + 1) K) per state for both pullbacks: mu, raw_sigma, dmu and
draw_sigma (4 d), and per sample dlogp and d values of dact (sampling) or of the actions (evaluation).
One JSON line per shape, times in microseconds per call; the first line stamps the device."""
import argparse
import json
import math
import os
import statistics
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--blocks", type=int, default=7)
ap.add_argument("--reps", type=int, default=50)
ap.add_argument("--torch-reps", type=int, default=3)
args = ap.parse_args()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "reinforcementlearning.jl_amd"))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import rlhip  # noqa: E402,F401
from rlhip._lib import call  # noqa: E402
from rlhip.ops import ptr, stream_ptr  # noqa: E402

assert torch.cuda.is_available(), "a timing needs the GPU"
SETTLE_S = 0.3
PEAK = 8.0e12
SHAPES = [(1, 1 << 20, 1), (6, 1 << 20, 1), (6, 1 << 16, 16), (64, 1 << 16, 1)]
LO, HI = 0.2, 1.7


def settle(f):
    t_end = time.perf_counter() + SETTLE_S
    while True:
        f()
        torch.cuda.synchronize()
        if time.perf_counter() >= t_end:
            break


def block(f, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        f()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps * 1e3


def timed(f, reps=None, blocks=None):
    settle(f)
    us = [block(f, reps or args.reps) for _ in range(blocks or args.blocks)]
    return [round(statistics.median(us), 2), round(min(us), 2), round(max(us), 2)]


props = torch.cuda.get_device_properties(0)
print(json.dumps(dict(device=props.name, cus=props.multi_processor_count, torch=torch.__version__, hip=torch.version.hip,
                      blocks=args.blocks, reps=args.reps, torch_reps=args.torch_reps, settle_s=SETTLE_S,
                      columns="[median, min, max] us")), flush=True)
for d, n, K in SHAPES:
    g = torch.Generator(device="cuda").manual_seed(d)
    mu = torch.randn((n, d), device="cuda", generator=g)
    raw = F.softplus(torch.randn((n, d), device="cuda", generator=g))
    dlogp, dact = torch.randn((n, K), device="cuda", generator=g), torch.randn((n, K, d), device="cuda", generator=g)
    noise = torch.randn((n, K, d), device="cuda", generator=g)
    act, lp = torch.empty((n, K, d), device="cuda"), torch.empty((n, K), device="cuda")
    dmu, draw = torch.empty_like(mu), torch.empty_like(raw)

    def fwd_sample():
        call("rlhip_gaussian_head_sample_f32", ptr(mu), ptr(raw), d, n, K, LO, HI, 1, 1, 11, 5, 4, ptr(act), ptr(lp), stream_ptr())

    fwd_sample()                                                     # the evaluation pullback reads these actions

    def logp_bwd():
        call("rlhip_gaussian_head_logp_bwd_f32", ptr(mu), ptr(raw), ptr(act), ptr(dlogp), d, n, K, LO, HI, 1, 1, ptr(dmu), ptr(draw),
             stream_ptr())

    def sample_bwd_soft():
        call("rlhip_gaussian_head_sample_bwd_f32", ptr(mu), ptr(raw), d, n, K, LO, HI, 1, 1, 11, 5, 4, ptr(dact), ptr(dlogp), ptr(dmu),
             ptr(draw), stream_ptr())

    def sample_bwd_gaussian():
        call("rlhip_gaussian_head_sample_bwd_f32", ptr(mu), ptr(raw), d, n, K, LO, HI, 1, 0, 11, 5, 4, None, ptr(dlogp), ptr(dmu),
             ptr(draw), stream_ptr())

    # what a user runs today: the reference's SoftGaussianNetwork sampling call (networks.jl:153-160) in torch, noise kept in memory
    def torch_soft():
        m, r = mu.detach().requires_grad_(True), raw.detach().requires_grad_(True)
        sg = r.clamp(LO, HI).unsqueeze(1)
        z = m.unsqueeze(1) + sg * noise
        zz = (z - m.unsqueeze(1)) / (sg + 1e-8)
        nl = -(zz * zz + math.log(2 * math.pi)) / 2 - torch.log(sg + 1e-8)
        logp = (nl - 2 * (math.log(2.0) - z - F.softplus(-2 * z))).sum(2)
        torch.autograd.grad((logp * dlogp).sum() + (torch.tanh(z) * dact).sum(), (m, r))

    nbytes = 4 * (4 * d + (d + 1) * K) * n
    row = dict(d=d, n=n, K=K, bytes=nbytes)
    for name, f in (("logp_bwd_soft", logp_bwd), ("sample_bwd_soft", sample_bwd_soft), ("sample_bwd_gaussian", sample_bwd_gaussian),
                    ("forward_sample_soft", fwd_sample)):
        row[name] = timed(f)
    for name in ("logp_bwd_soft", "sample_bwd_soft"):
        row[name + "_fraction_of_8TBs"] = round(nbytes / (row[name][0] * 1e-6) / PEAK, 4)
    if d % 2 == 0:      # A/B in process: the pair kernel (the default for even d) against one lane per component, alternating; equal bits
        def unpaired(f):
            def run():
                os.environ["RLHIP_HEAD_GRAD_PAIR"] = "0"
                f()
                del os.environ["RLHIP_HEAD_GRAD_PAIR"]
            return run

        for name, f in (("sample_bwd_soft", sample_bwd_soft), ("sample_bwd_gaussian", sample_bwd_gaussian)):
            f()
            a = (dmu.clone(), draw.clone())
            unpaired(f)()
            assert torch.equal(a[0], dmu) and torch.equal(a[1], draw), f"{name}: the two variants differ"
            ab = [(timed(f, blocks=3), timed(unpaired(f), blocks=3)) for _ in range(2)]
            row[name + "_ab_pair_vs_single"] = ab
    row["torch_autograd_soft_sampling"] = timed(torch_soft, reps=args.torch_reps, blocks=3)
    print(json.dumps(row), flush=True)
    del mu, raw, dlogp, dact, noise, act, lp, dmu, draw
    torch.cuda.empty_cache()
