"""The TD3 / DDPG kernels (csrc/td3.hip) on the device against the Float64 model of tests/td3_ref.py, teacher-forced on the launch's own
noise_out.  One list of cases, each changing one axis of the base case (ns 3, h 64, relu, two critics, batch 64); `big` also widens
layer 1 of the critics (x 64), since 2 x 10^6 distinct pre-activations of unit width never all clear the margin below.

Bars     4 x FLOOR[output]: the largest distance over these cases of the SAME model in Float32 torch from its Float64 run, relative to
         max|reference| (measured on the CPU, profiles/td3.md) -- never taken from the kernel.
Margins  asserted on the reference alone, for every sample of every case (the seeds were walked on the CPU until they hold): every
         pre-activation, |Qt1 - Qt2|, and the distances of the unclipped noise and of u' from their clamp bounds stay above 1e-5.
Also     noise_out = clampj(target_noise * draw) on regenerated draws, bit for bit; every launch twice, the same bytes."""
import numpy as np
import pytest
import torch

import heads_grad_ref as G
import sac_cases as SC
import td3_ref as R
from heads_ref import F32

pytestmark = pytest.mark.gpu
SEED, STEP, BIG = 77, 5, 64 * 256 + 65  # BIG: every workgroup of the 256 carries a second tile, the last tile is partial
BASE = dict(ns=3, h=64, act=0, nc=2, batch=64, tn=0.2, clip=0.5, scale=2.0, lo=-2.0, hi=2.0, terminal=0.15, l1=4.0)
CASES = {"base": (dict(), 0), "ns2": (dict(ns=2), 0), "ns4": (dict(ns=4), 0), "tanh": (dict(act=1), 0), "h16": (dict(h=16), 0),
         "h48": (dict(h=48), 0), "h256": (dict(h=256), 1), "one-critic": (dict(nc=1), 0), "b1": (dict(batch=1), 0),
         "b63": (dict(batch=63), 0), "b65": (dict(batch=65), 1), "big": (dict(batch=BIG, l1=64.0), 2),
         "all-terminal": (dict(terminal=2.0), 0), "both-clamps": (dict(tn=1.0, clip=0.5, scale=1.0, lo=-0.6, hi=0.6), 0),
         "no-noise": (dict(tn=0.0), 0)}
FLOOR = dict(y=3.07e-7, closs=1.07e-7, cgrad=3.59e-7, stats=3.92e-7, agrad=5.0e-7)


def build(name, seed=None):
    kw, s0 = CASES[name]
    c = dict(BASE, name=name, gamma=0.99, **kw)
    rng = np.random.default_rng(1000 * (list(CASES).index(name) + 1) + (s0 if seed is None else seed))
    ns, h = c["ns"], c["h"]
    c["actor"], c["actor_t"] = SC._net(rng, ns, h, 1, 1.0, 4.0), SC._net(rng, ns, h, 1, 1.0, 4.0)
    c["critics"] = np.concatenate([SC._net(rng, ns + 1, h, 1, 1.0, c["l1"]) for _ in range(c["nc"])])
    c["targets"] = (c["critics"] + rng.normal(0, 0.02, c["critics"].shape)).astype(F32)
    c["S"] = rng.normal(0, 1, (SC.PUSHES + 1, ns, SC.N_ENV)).astype(F32)
    c["A"] = rng.uniform(-c["scale"], c["scale"], (SC.PUSHES, SC.N_ENV)).astype(F32)
    c["Rw"] = rng.normal(0, 1, (SC.PUSHES, SC.N_ENV)).astype(F32)
    c["T"] = (rng.uniform(size=(SC.PUSHES, SC.N_ENV)) < c["terminal"]).astype(np.uint8)
    c["idx"] = rng.integers(0, SC.CAP * SC.N_ENV, c["batch"]).astype(np.int64)
    return c


def records(c, idx):
    p, e = idx // SC.N_ENV + (SC.PUSHES - SC.CAP), idx % SC.N_ENV  # logical transition li is push li + (PUSHES - CAP)
    return (np.ascontiguousarray(c["S"][p, :, e].T), c["A"][p, e], c["Rw"][p, e], c["T"][p, e], np.ascontiguousarray(c["S"][p + 1, :, e].T))


def clipped(c, draws):
    raw = F32(c["tn"]) * draws
    return np.clip(raw, F32(-c["clip"]), F32(c["clip"])).astype(F32) if c["tn"] else np.zeros_like(draws)


def margin(c, rc, ra, draws):
    """the smallest distance of the reference from any decision of the update"""
    m = [np.abs(rc["z"]).min(), np.abs(ra["z"]).min(), np.abs(rc["u_raw"] - c["lo"]).min(), np.abs(rc["u_raw"] - c["hi"]).min()]
    if c["nc"] == 2:
        m.append(np.abs(rc["qt"][0] - rc["qt"][1]).min())
    if c["tn"]:
        m.append(np.abs(np.abs((F32(c["tn"]) * draws).astype(np.float64)) - c["clip"]).min())
    return float(min(m))


rel = lambda got, want: float(np.abs(np.asarray(got, np.float64) - want).max() / max(np.abs(want).max(), 1e-30))  # noqa: E731


@pytest.fixture(scope="module")
def dev():
    from test_gpu_sac_kernels import SacDevice

    return SacDevice()


@pytest.mark.parametrize("name", list(CASES))
def test_both_gradients_against_the_float64_model(dev, name):
    from rlhip import td3

    c = build(name)
    B, up = c["batch"], lambda x: torch.tensor(np.asarray(x), device="cuda")  # noqa: E731
    tr, idx, rec = dev.traces(c), up(c["idx"]), records(c, c["idx"])
    draws = G.draws(dev.sample, 1, B, 1, SEED + 1, 0, STEP)[0, 0]

    def critic():
        y, noise = torch.empty(B, device="cuda"), torch.empty(B, device="cuda")
        g, l = td3.td3_critic_grad(tr, c["h"], c["act"], c["nc"], up(c["actor_t"]), up(c["critics"]), up(c["targets"]), idx, c["gamma"],
                                   c["scale"], c["tn"], c["clip"], c["lo"], c["hi"], SEED + 1, STEP, y=y, noise=noise)
        return [t.cpu().numpy() for t in (y, noise, l, g)]

    def actor():
        return [t.cpu().numpy() for t in td3.td3_actor_grad(tr, c["h"], c["act"], up(c["actor"]), up(c["critics"]), idx, c["scale"])]

    (y, noise, loss, cgrad), (agrad, stats) = critic(), actor()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(critic() + actor(), [y, noise, loss, cgrad, agrad, stats])), "run to run"
    assert np.array_equal(noise, clipped(c, draws)), "noise_out is not clampj(target_noise * draw, -noise_clip, noise_clip)"
    rc, ra = R.critic(c, rec, noise), R.actor(c, rec)
    m = margin(c, rc, ra, draws)
    assert m > 1e-5, f"{name}: the reference sits {m:.2e} from a decision (pick another seed)"
    if name == "both-clamps":
        assert (np.abs(noise) == F32(c["clip"])).mean() > 0.1 and (np.abs(rc["u_raw"]) > c["hi"]).mean() > 0.1
    if name == "all-terminal":
        assert rec[3].all() and np.array_equal(y, rec[2])
    errs = dict(y=rel(y, rc["y"]), closs=rel(loss, rc["loss"]), cgrad=rel(cgrad, rc["grad"]), stats=rel(stats, ra["stats"]),
                agrad=rel(agrad, ra["grad"]))
    print(f"td3 {name}: margin {m:.2e}; " + ", ".join(f"{k} {v:.2e} (bar {4 * FLOOR[k]:.2e})" for k, v in errs.items()))
    assert all(np.isfinite(v) and v <= 4 * FLOOR[k] for k, v in errs.items()), errs


@pytest.mark.parametrize("ns,h,act", [(2, 16, 0), (3, 64, 1), (4, 256, 0)])
def test_plan_is_forward_then_noise_and_clamp(dev, ns, h, act):
    from rlhip import ops, td3

    n, seed, base, step, scale, sigma, lo, hi = 301, 21, 1000, 9, 2.0, 0.3, -1.5, 1.5  # five workgroups of one wave, the last ragged
    rng = np.random.default_rng(ns * 1000 + h)
    actor = torch.tensor(SC._net(rng, ns, h, 1, 4.0), device="cuda")
    obs = torch.tensor(rng.normal(0, 1, (ns, n)).astype(F32), device="cuda")
    mu = torch.empty(n, device="cuda")
    a = td3.td3_plan(actor, ns, h, act, obs, scale, sigma, lo, hi, seed, base, step, mu=mu)
    assert torch.equal(ops.mlp2_forward(actor, ns, h, 1, act, obs)[0], mu), "mu_out is not rlhip_mlp2_forward_f32's bytes"
    t = scale * np.tanh(mu.cpu().numpy().astype(np.float64))
    want = np.clip(t + np.float64(F32(sigma)) * G.draws(dev.sample, 1, n, 1, seed, base, step)[0, 0], lo, hi)
    # three Float32 roundings of values <= 4 (tanhf inside 2 ulp, the product, the sum): 4 x 2^-23 x 2 absolute
    assert np.abs(a.cpu().numpy() - want).max() <= 1e-6 and (np.abs(want) == hi).sum() > 0
    det = td3.td3_plan(actor, ns, h, act, obs, scale, sigma, lo, hi, seed, base, step, deterministic=True)
    assert np.abs(det.cpu().numpy() - np.clip(t, lo, hi)).max() <= 1e-6
    assert torch.equal(det, td3.td3_plan(actor, ns, h, act, obs, scale, 0.0, lo, hi, seed, base, step)), "deterministic adds nothing"
