"""The three-layer TD3 / DDPG kernels (csrc/td3_mlp3.hip) on the device against the Float64 model of tests/td3_mlp3_ref.py,
teacher-forced on the launch's own noise_out.  The cases (td3_mlp3_ref.CASES) change one axis at a time from ns 3, h 64, relu, two
critics, batch 65; their records hold terminal transitions and an action box inside action_scale, so u' clamps on some samples.

Bars     4 x the Float32 floor of the output: the distance of the SAME model in Float32 torch from its Float64 run, relative to
         max |reference|, computed here on the CPU -- never taken from the kernel.  The floor of an output is its largest over the case
         list (the rule of tests/test_gpu_td3.py's FLOOR): one case's Float32 run can land on the Float64 value by chance (batch 1 is
         one rounding), which says nothing about the error of another order of the same sum.
Also     noise_out = clampj(target_noise * draw) on regenerated draws, bit for bit; every launch twice, the same bytes; tests/
         test_td3_mlp3_reference.py holds the Float32 and Float64 models to the same decisions on every case."""
import numpy as np
import pytest
import torch

import heads_grad_ref as G
import td3_mlp3_ref as R
from heads_ref import F32

pytestmark = pytest.mark.gpu
SEED, STEP = 77, 5
up = lambda x: torch.tensor(np.asarray(x), device="cuda")  # noqa: E731


@pytest.fixture(scope="module")
def dev():
    from test_gpu_sac_kernels import SacDevice

    return SacDevice()


@pytest.fixture(scope="module")
def model(dev):
    """name -> (case, records, clipped noise, Float64 critic run, Float64 actor run), and the floor of every output over the cases"""
    runs, floor = {}, {}
    for name in R.CASES:
        c = R.build(name)
        rec, e = R.records(c, c["idx"]), R.clipped(c, G.draws(dev.sample, 1, c["batch"], 1, SEED + 1, 0, STEP)[0, 0])
        rc, ra, fl, same = R.floors(c, rec, e)
        assert same, f"{name}: the Float32 and Float64 models decide differently"
        runs[name] = (c, rec, e, rc, ra)
        floor = {k: max(v, floor.get(k, 0.0)) for k, v in fl.items()}
        print(f"td3_mlp3 {name}: Float32 floors " + ", ".join(f"{k} {v:.2e}" for k, v in fl.items()))
    return runs, floor


@pytest.mark.parametrize("name", list(R.CASES))
def test_both_gradients_against_the_float64_model(dev, model, name):
    from rlhip import _lib, td3

    (c, rec, e, rc, ra), floor = model[0][name], model[1]
    B, tr, idx = c["batch"], dev.traces(c), up(c["idx"])
    if name == "carry":
        rows = lambda b: _lib.lib.rlhip_td3_mlp3_workspace_bytes(c["ns"], c["h"], c["nc"], b) - 4 * b  # noqa: E731
        assert rows(B) == rows(B - 1) > rows(B - 33), "a workgroup carries its second tile first at this batch"

    def critic():
        y, noise = torch.empty(B, device="cuda"), torch.empty(B, device="cuda")
        g, l = td3.td3_critic_grad(tr, c["h"], c["act"], c["nc"], up(c["actor_t"]), up(c["critics"]), up(c["targets"]), idx, c["gamma"],
                                   c["scale"], c["tn"], c["clip"], c["lo"], c["hi"], SEED + 1, STEP, y=y, noise=noise, layers=3)
        return [t.cpu().numpy() for t in (y, noise, l, g)]

    def actor():
        return [t.cpu().numpy() for t in td3.td3_actor_grad(tr, c["h"], c["act"], up(c["actor"]), up(c["critics"]), idx, c["scale"], layers=3)]

    (y, noise, loss, cgrad), (agrad, stats) = critic(), actor()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(critic() + actor(), [y, noise, loss, cgrad, agrad, stats])), "run to run"
    assert np.array_equal(noise, e), "noise_out is not clampj(target_noise * draw, -noise_clip, noise_clip)"
    errs = dict(y=R.rel(y, rc["y"]), closs=R.rel(loss, rc["loss"]), cgrad=R.rel(cgrad, rc["grad"]), stats=R.rel(stats, ra["stats"]),
                agrad=R.rel(agrad, ra["grad"]))
    print(f"td3_mlp3 {name}: " + ", ".join(f"{k} {v:.2e} (bar {4 * floor[k]:.2e})" for k, v in errs.items()))
    assert all(np.isfinite(v) and v <= 4 * floor[k] for k, v in errs.items()), errs


@pytest.mark.parametrize("ns,h,act,base", [(2, 32, 0, 1000), (3, 96, 1, 2 ** 32 - 40), (4, 256, 0, 7)])
def test_plan_is_forward_then_noise_and_clamp(dev, ns, h, act, base):
    """(the env ids of the second case wrap 2^32)"""
    from rlhip import td3

    n, seed, step, scale, sigma, lo, hi = 77, 21, 9, 2.0, 0.3, -1.5, 1.5  # three tiles, the last ragged
    rng = np.random.default_rng(ns * 1000 + h)
    p = R._net(rng, ns, h)
    obs = rng.normal(0, 1, (ns, n)).astype(F32)
    mu, args = torch.empty(n, device="cuda"), (up(p), ns, h, act, up(obs), scale)
    a = td3.td3_plan(*args, sigma, lo, hi, seed, base, step, mu=mu, layers=3)
    ref = {dt: R.mlp(torch.tensor(p, dtype=dt), ns, h, act, torch.tensor(obs, dtype=dt))[0].numpy() for dt in (torch.float64, torch.float32)}
    floor = R.rel(ref[torch.float32], ref[torch.float64])
    assert R.rel(mu.cpu().numpy(), ref[torch.float64]) <= 4 * floor, "mu_out against the Float64 model at 4 x its Float32 floor"
    t = scale * np.tanh(mu.cpu().numpy().astype(np.float64))
    draws = np.concatenate([G.draws(dev.sample, 1, k, 1, seed, b, step)[0, 0] for b, k in ((base, min(n, 2 ** 32 - base)), (0, max(0, n - (2 ** 32 - base)))) if k])
    want = np.clip(t + np.float64(F32(sigma)) * draws, lo, hi)
    # three Float32 roundings of values <= 4 (tanhf inside 2 ulp, the product, the sum): 4 x 2^-23 x 2 absolute
    assert np.abs(a.cpu().numpy() - want).max() <= 1e-6 and (np.abs(want) == hi).sum() > 0
    det = td3.td3_plan(*args, sigma, lo, hi, seed, base, step, deterministic=True, layers=3)
    assert torch.equal(det, (scale * torch.tanh(mu)).clamp(lo, hi)), "deterministic: clampj(action_scale * tanhf(mu_out)), exactly"
    assert torch.equal(det, td3.td3_plan(*args, 0.0, lo, hi, seed, base, step, layers=3)), "deterministic adds nothing"
