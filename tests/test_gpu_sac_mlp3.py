"""The three-layer SAC kernels (csrc/sac_mlp3.hip) on the device against the Float64 model of tests/sac_mlp3_ref.py, teacher-forced on
the regenerated draws.  The cases (sac_mlp3_ref.CASES) change one axis at a time from ns 3, h 64, relu, batch 65; their records hold
terminal transitions, every case with more than one sample selects both critics, `clamp` has the sigma clamp active.

Bars     4 x the Float32 floor of the output: the distance of the SAME model in Float32 torch from its Float64 run, relative to
         max |reference|, computed here on the CPU -- never taken from the kernel -- and taken as the largest over the case list (the
         rule and the reasoning of tests/test_gpu_td3_mlp3.py).  sel_out must be equal.
Also     every launch twice, the same bytes; `alpha`: alpha_out aliasing alpha; tests/test_sac_mlp3_reference.py holds the Float32 and
         Float64 models to the same decisions on every case."""
import numpy as np
import pytest
import torch

import sac_mlp3_ref as R
import sac_ref
import td3_mlp3_ref as T
from heads_ref import F32, Q

pytestmark = pytest.mark.gpu
SEED, STEP = 77, 5
up = lambda x: torch.tensor(np.asarray(x), device="cuda")  # noqa: E731


@pytest.fixture(scope="module")
def dev():
    from test_gpu_sac_kernels import SacDevice

    return SacDevice()


@pytest.fixture(scope="module")
def model(dev):
    """name -> (case, records, draws, Float64 critic run, Float64 actor run), and the floor of every output over the cases"""
    runs, floor = {}, {}
    for name in R.CASES:
        c = R.build(name)
        rec, eps = T.records(c, c["idx"]), sac_ref.draw_pair(dev.sample, c["batch"], SEED + 1, STEP)
        rc, ra, fl, same = R.floors(c, rec, *eps)
        assert same, f"{name}: the Float32 and Float64 models decide differently"
        runs[name] = (c, rc, ra)
        floor = {k: max(v, floor.get(k, 0.0)) for k, v in fl.items()}
        print(f"sac_mlp3 {name}: Float32 floors " + ", ".join(f"{k} {v:.2e}" for k, v in fl.items()))
    return runs, floor


@pytest.mark.parametrize("name", list(R.CASES))
def test_both_gradients_against_the_float64_model(dev, model, name):
    from rlhip import _lib, sac

    (c, rc, ra), floor = model[0][name], model[1]
    B, tr, idx, h = c["batch"], dev.traces(c), up(c["idx"]), c["h"]
    if name.startswith("carry"):  # the partial rows stop growing one tile before this batch: a workgroup carries its second tile
        rows = lambda b: _lib.lib.rlhip_sac_mlp3_workspace_bytes(c["ns"], h, b) - 4 * b  # noqa: E731
        assert rows(B) == rows(B - 1) > rows(B - 33)
    args = (c["lo"], c["hi"], c["scale"], SEED + 1, STEP)

    def critic():
        y = torch.empty(B, device="cuda")
        g, l = sac.sac_critic_grad(tr, h, c["act"], up(c["actor"]), up(c["critics"]), up(c["targets"]), idx, up(F32([c["alpha"]])), c["gamma"],
                                   *args, y=y, layers=3)
        return [t.cpu().numpy() for t in (y, l, g)]

    def actor():
        alpha = up(F32([c["alpha"]]))
        out = alpha if c.get("alias") else torch.empty(1, device="cuda")
        sel, logp = torch.empty(B, dtype=torch.int32, device="cuda"), torch.empty(B, device="cuda")
        g, st = sac.sac_actor_grad(tr, h, c["act"], up(c["actor"]), up(c["critics"]), idx, alpha, *args, c["alpha_lr"], c["target_entropy"], out,
                                   sel=sel, logp=logp, layers=3)
        return [t.cpu().numpy() for t in (sel, logp, st, g, out)]

    (y, loss, cgrad), (sel, logp, stats, agrad, alpha) = critic(), actor()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(critic() + actor(), [y, loss, cgrad, sel, logp, stats, agrad, alpha])), "run to run"
    assert np.array_equal(sel, ra["sel"]), f"sel_out differs at {int((sel != ra['sel']).sum())} samples"
    errs = dict(y=T.rel(y, rc["y"]), closs=T.rel(loss, rc["loss"]), cgrad=T.rel(cgrad, rc["grad"]), logp=T.rel(logp, ra["logp"]),
                stats=T.rel(stats, ra["stats"]), agrad=T.rel(agrad, ra["grad"]), alpha=T.rel(alpha, ra["alpha_new"]))
    print(f"sac_mlp3 {name}: " + ", ".join(f"{k} {v:.2e} (bar {4 * floor[k]:.2e})" for k, v in errs.items()))
    assert all(np.isfinite(v) and v <= 4 * floor[k] for k, v in errs.items()), errs


@pytest.mark.parametrize("ns,h,act,base,lo,hi", [(2, 32, 0, 1000, 0.0, np.inf), (3, 96, 1, 2 ** 32 - 40, 0.6, 0.75), (4, 256, 0, 7, 0.0, np.inf)])
def test_plan_is_forward_then_head(dev, ns, h, act, base, lo, hi):
    """(the env ids of the second case wrap 2^32, and its sigma clamp is active)"""
    from rlhip import sac

    n, seed, step, scale = 77, 21, 9, 2.0  # three tiles, the last ragged
    rng = np.random.default_rng(ns * 1000 + h)
    p, obs = R._actor(rng, ns, h), rng.normal(0, 1, (ns, n)).astype(F32)
    a, lp, mu, rho, raw = (torch.empty(n, device="cuda") for _ in range(5))
    args = (up(p), ns, h, act, up(obs), lo, hi, scale, seed, base, step)
    sac.sac_plan(*args, action=a, logp=lp, mu=mu, rho=rho, raw_sigma=raw, layers=3)
    ref = {dt: R.mlp2o(torch.tensor(p, dtype=dt), ns, h, act, torch.tensor(obs, dtype=dt)).numpy() for dt in (torch.float64, torch.float32)}
    floor = T.rel(ref[torch.float32], ref[torch.float64])
    got = np.stack([mu.cpu().numpy(), rho.cpu().numpy()])
    assert T.rel(got, ref[torch.float64]) <= 4 * floor, "mu_out / rho_out against the Float64 model at 4 x its Float32 floor"
    sac_ref.within(raw.cpu().numpy(), sac_ref.softplus_q(Q(rho.cpu().numpy())), "raw_sigma_out")
    a_ref, lp_ref = dev.empty(n, 1, 1), dev.empty(n, 1)
    dev.call("rlhip_gaussian_head_sample_f32", dev.ptr(mu), dev.ptr(raw), 1, n, 1, float(lo), float(hi), 1, 1, seed, base, step, dev.ptr(a_ref),
             dev.ptr(lp_ref), dev.sp())
    assert torch.equal(a / scale, a_ref.reshape(-1)), "action_out / action_scale is not the head's action"
    assert torch.equal(lp.view(torch.int32), lp_ref.reshape(-1).view(torch.int32)), "logp_out is not the head's log-probability"
    if np.isfinite(hi):
        assert (raw < lo).any() and (raw > hi).any()
    a2, mu2 = torch.empty(n, device="cuda"), torch.empty(n, device="cuda")
    sac.sac_plan(*args, action=a2, layers=3)  # the nullable outputs
    det = sac.sac_plan(*args, deterministic=True, mu=mu2, layers=3)
    assert torch.equal(a2, a) and torch.equal(mu2, mu) and torch.equal(det, scale * torch.tanh(mu)), "deterministic: action_scale * tanhf(mu_out)"
