"""Pullback kernels of the CovGaussianNetwork head (profiles/cov_heads_grad.md): event timing of the fused head pullback
(rlhip_cov_gaussian_head_logp_bwd_f32), of rlhip_mvnormkldivergence_bwd_f32 (all four outputs, and the dmu2 / dL2 pair an MPO step
asks for) and of the composition a user runs without them: torch Float32 autograd (forward and backward) over a dense L from
ops.vec_to_tril and torch.linalg.solve_triangular on the batch, on the same device.  Each series runs after a settle phase of untimed
calls, as blocks of event-timed calls whose median and range are printed.

    python tools/cov_heads_grad_time.py [--blocks 7] [--reps 50] [--torch-reps 3]

Fractions are of 8 TB/s against the algorithmic bytes: the head pullback reads mu, chol_vec, the actions and dlogp and writes dmu and
dvec, 4 (2 da + 2 nv + (da + 1) K) per state; the KL pullback reads and writes two means and two dense L, 4 (4 da + 4 da^2 + 1).
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

import rlhip  # noqa: E402,F401
from rlhip import ops  # noqa: E402
from rlhip._lib import call  # noqa: E402
from rlhip.ops import ptr, stream_ptr  # noqa: E402

assert torch.cuda.is_available(), "a timing needs the GPU"
SETTLE_S = 0.3
PEAK = 8.0e12
SHAPES = [(1, 1 << 20, 1), (4, 1 << 20, 1), (10, 1 << 20, 1), (16, 1 << 20, 1), (4, 1 << 16, 16)]


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
for da, n, K in SHAPES:
    nv = da * (da + 1) // 2
    g = torch.Generator(device="cuda").manual_seed(da)
    mu, mu2 = torch.randn((n, da), device="cuda", generator=g), torch.randn((n, da), device="cuda", generator=g)
    vec, vec2 = torch.randn((n, nv), device="cuda", generator=g), torch.randn((n, nv), device="cuda", generator=g)
    act = mu.unsqueeze(1) + 3 * torch.randn((n, K, da), device="cuda", generator=g)
    dlogp, dout = torch.randn((n, K), device="cuda", generator=g), torch.randn(n, device="cuda", generator=g)
    L1, L2 = ops.vec_to_tril(vec, da), ops.vec_to_tril(vec2, da)
    dmu, dvec = torch.empty_like(mu), torch.empty_like(vec)
    dmu1, dmu2, dL1, dL2 = torch.empty_like(mu), torch.empty_like(mu), torch.empty_like(L1), torch.empty_like(L2)

    def head_bwd():
        call("rlhip_cov_gaussian_head_logp_bwd_f32", ptr(mu), ptr(vec), ptr(act), ptr(dlogp), da, n, K, ptr(dmu), ptr(dvec),
             stream_ptr())

    def kl_bwd():
        call("rlhip_mvnormkldivergence_bwd_f32", ptr(mu), ptr(L1), ptr(mu2), ptr(L2), ptr(dout), da, n, ptr(dmu1), ptr(dL1), ptr(dmu2),
             ptr(dL2), stream_ptr())

    def kl_bwd_second():
        call("rlhip_mvnormkldivergence_bwd_f32", ptr(mu), ptr(L1), ptr(mu2), ptr(L2), ptr(dout), da, n, None, None, ptr(dmu2), ptr(dL2),
             stream_ptr())

    # what a user runs today: storage [state, column, row] -> matrices [state, row, column], then batched triangular solves
    def torch_head():
        m, Ls = mu.detach().requires_grad_(True), L1.detach().requires_grad_(True)
        L = torch.tril(Ls.transpose(1, 2))
        y = torch.linalg.solve_triangular(L, (act - m.unsqueeze(1)).transpose(1, 2), upper=False)
        lp = -((da * math.log(2 * math.pi) + 2 * torch.log(torch.diagonal(L, dim1=1, dim2=2)).sum(1)).unsqueeze(1) + (y * y).sum(1)) / 2
        torch.autograd.grad((lp * dlogp).sum(), (m, Ls))

    def torch_kl():
        m2, Ls2 = mu2.detach().requires_grad_(True), L2.detach().requires_grad_(True)
        A, B = torch.tril(L1.transpose(1, 2)), torch.tril(Ls2.transpose(1, 2))
        W = torch.linalg.solve_triangular(B, A, upper=False)
        q = torch.linalg.solve_triangular(B, (m2 - mu).unsqueeze(2), upper=False)
        logdet = 2 * torch.log(torch.diagonal(B, dim1=1, dim2=2)).sum(1) - 2 * torch.log(torch.diagonal(A, dim1=1, dim2=2)).sum(1)
        kl = (logdet - da + (W * W).sum((1, 2)) + (q * q).sum((1, 2))) / 2
        torch.autograd.grad((kl * dout).sum(), (m2, Ls2))

    head_bytes = 4 * (2 * da + 2 * nv + (da + 1) * K) * n
    kl_bytes = 4 * (4 * da + 4 * da * da + 1) * n
    row = dict(da=da, n=n, K=K, head_bytes=head_bytes, kl_bytes=kl_bytes)
    row["head_bwd"] = timed(head_bwd)
    row["head_bwd_fraction_of_8TBs"] = round(head_bytes / (row["head_bwd"][0] * 1e-6) / PEAK, 4)
    row["kl_bwd"] = timed(kl_bwd)
    row["kl_bwd_fraction_of_8TBs"] = round(kl_bytes / (row["kl_bwd"][0] * 1e-6) / PEAK, 4)
    row["kl_bwd_dmu2_dL2_only"] = timed(kl_bwd_second)
    row["torch_autograd_head"] = timed(torch_head, reps=args.torch_reps, blocks=3)
    row["torch_autograd_kl_second"] = timed(torch_kl, reps=args.torch_reps, blocks=3)
    print(json.dumps(row), flush=True)
    del mu, mu2, vec, vec2, act, dlogp, dout, L1, L2, dmu, dvec, dmu1, dmu2, dL1, dL2
    torch.cuda.empty_cache()
