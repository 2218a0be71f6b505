"""CovGaussianNetwork head kernels (profiles/cov_heads.md): event timing of the fused sample + logp launch
(rlhip_cov_gaussian_head_sample_f32), of the (state, action) launch (rlhip_cov_gaussian_head_logp_f32) and of the composition the fused
sample call stands for -- rlhip_vec_to_tril_f32, the draws from the existing Gaussian head (mu = 0, sigma = 1), the product
mu + L eps as torch.baddbmm (the library has no stand-alone product) and rlhip_mvnormlogpdf_f32 -- on preallocated buffers in the
library's own layouts (no transposes).  Each series runs after a settle phase of untimed calls, as blocks of event-timed calls whose
median and range are printed; the A/B alternates fused and composed blocks in the same process.

    python tools/cov_heads_time.py [--blocks 7] [--reps 50]

Fractions are of 8 TB/s against the algorithmic bytes 4 ((da + nv) + (da + 1) K) per state.  One JSON line per shape, times in
microseconds per call; the first line stamps the device."""
import argparse
import json
import os
import statistics
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--blocks", type=int, default=7)
ap.add_argument("--reps", type=int, default=50)
args = ap.parse_args()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "reinforcementlearning.jl_amd"))

import torch  # noqa: E402

import rlhip  # noqa: E402,F401
from rlhip._lib import call  # noqa: E402
from rlhip.ops import ptr, stream_ptr  # noqa: E402

assert torch.cuda.is_available(), "a timing needs the GPU"
SETTLE_S = 0.3
PEAK = 8.0e12
SHAPES = [(1, 1 << 20, 1), (4, 1 << 20, 1), (10, 1 << 20, 1), (16, 1 << 20, 1), (4, 1 << 16, 16)]


def settle(fs):
    t_end = time.perf_counter() + SETTLE_S
    while True:
        for f in fs:
            for _ in range(4):
                f()
        torch.cuda.synchronize()
        if time.perf_counter() >= t_end:
            break


def block(f):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(args.reps):
        f()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / args.reps * 1e3


def stats(us):
    return [round(statistics.median(us), 2), round(min(us), 2), round(max(us), 2)]


def timed(f):
    settle([f])
    return stats([block(f) for _ in range(args.blocks)])


def alternating(fa, fb):
    settle([fa, fb])
    a, b = [], []
    for _ in range(args.blocks):
        a.append(block(fa))
        b.append(block(fb))
    return stats(a), stats(b)


props = torch.cuda.get_device_properties(0)
print(json.dumps(dict(device=props.name, cus=props.multi_processor_count, torch=torch.__version__, hip=torch.version.hip,
                      blocks=args.blocks, reps=args.reps, settle_s=SETTLE_S, columns="[median, min, max] us")), flush=True)
for da, n, K in SHAPES:
    nv = da * (da + 1) // 2
    g = torch.Generator(device="cuda").manual_seed(da)
    mu = torch.randn((n, da), device="cuda", generator=g)
    vec = torch.randn((n, nv), device="cuda", generator=g)
    act, lp = torch.empty((n, K, da), device="cuda"), torch.empty((n, K), device="cuda")
    L, eps, lp2 = torch.empty((n, da, da), device="cuda"), torch.empty((n, K, da), device="cuda"), torch.empty((n, K), device="cuda")
    zero, one = torch.zeros((n, da), device="cuda"), torch.ones((n, da), device="cuda")
    step = [0]

    def fused():
        step[0] += 1
        call("rlhip_cov_gaussian_head_sample_f32", ptr(mu), ptr(vec), da, n, K, 1, 0, step[0], ptr(act), ptr(lp), None, stream_ptr())

    def logp():
        call("rlhip_cov_gaussian_head_logp_f32", ptr(mu), ptr(vec), ptr(act), da, n, K, ptr(lp2), None, stream_ptr())

    def composed():
        step[0] += 1
        call("rlhip_vec_to_tril_f32", ptr(vec), da, n, ptr(L), stream_ptr())
        call("rlhip_gaussian_head_sample_f32", ptr(zero), ptr(one), da, n, K, 1.0, 1.0, 0, 0, 1, 0, step[0], ptr(eps), None, stream_ptr())
        z = torch.baddbmm(mu.unsqueeze(1), eps, L)          # z[i, j, r] = mu[i, r] + sum_c eps[i, j, c] L[i, c, r]
        call("rlhip_mvnormlogpdf_f32", ptr(mu), ptr(L), ptr(z), da, K, n, ptr(lp2), stream_ptr())

    byts = 4 * ((da + nv) + (da + 1) * K) * n
    row = dict(da=da, n=n, K=K, algorithmic_bytes=byts)
    row["fused_sample_logp"] = timed(fused)
    row["logp"] = timed(logp)
    row["fused_fraction_of_8TBs"] = round(byts / (row["fused_sample_logp"][0] * 1e-6) / PEAK, 4)
    row["logp_fraction_of_8TBs"] = round(byts / (row["logp"][0] * 1e-6) / PEAK, 4)
    row["ab_fused"], row["ab_composed"] = alternating(fused, composed)
    print(json.dumps(row), flush=True)
    del mu, vec, act, lp, L, eps, lp2, zero, one
    torch.cuda.empty_cache()
