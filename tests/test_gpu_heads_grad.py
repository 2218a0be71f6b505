"""The pullbacks of GaussianNetwork, SoftGaussianNetwork, normlogpdf and diagnormlogpdf on the device (csrc/heads_grad.hip) against the
model (tests/heads_grad_ref.py), through the C ABI and through rlhip/grad.py.  The sampling pullbacks and the identity-squash evaluation
pullback are exact Float32 replays and are compared bit for bit; the evaluation pullbacks that hold an atanhf lie within 2 x budget."""
import math

import numpy as np
import pytest
import torch

import heads_grad_ref as G
import heads_ref as H
from heads_ref import F32
from test_gpu_cov_heads import Device

pytestmark = pytest.mark.gpu
SENTINEL = 7.0
LO, HI = H.LO, H.HI
SEED, BASE, STEP = H.SEED, H.BASE, H.STEP


class HeadsDevice(Device):
    """the entry points of csrc/heads.hip / csrc/heads_grad.hip on numpy arrays in the reference's shapes; an output that is not asked
    for is handed over as NULL and its buffer, filled with a sentinel, is returned as it is"""

    def _outs(self, shapes, need):
        outs = [torch.full(s, SENTINEL, dtype=torch.float32, device="cuda") for s in shapes]
        return outs, [self.ptr(o) if w else None for o, w in zip(outs, need)]

    def sample(self, mu, raw, K, lo, hi, family, seed, base, step):
        """the forward entry, with the signature of tests/heads_ref.py's `impl.sample` -> a (d, K, n), lp (K, n)"""
        squash, soft = H.SQUASH_SOFT[family]
        d, n = mu.shape
        m, r, act, lp = self.up(mu), self.up(raw), self.empty(n, K, d), self.empty(n, K)
        self.call("rlhip_gaussian_head_sample_f32", self.ptr(m), self.ptr(r), d, n, K, float(lo), float(hi), squash, soft, seed, base, step,
                  self.ptr(act), self.ptr(lp), self.sp())
        return self.down(act), self.down(lp)

    def logp_bwd(self, family, mu, raw, a, g, lo, hi, need=(1, 1)):
        squash, soft = H.SQUASH_SOFT[family]
        d, K, n = a.shape
        ins = [self.up(t) for t in (mu, raw, a, g)]
        outs, ptrs = self._outs([(n, d), (n, d)], need)
        self.call("rlhip_gaussian_head_logp_bwd_f32", *(self.ptr(t) for t in ins), d, n, K, float(lo), float(hi), squash, soft, *ptrs,
                  self.sp())
        return [self.down(o) for o in outs]

    def sample_bwd(self, family, mu, raw, K, lo, hi, seed, base, step, g=None, dact=None, need=(1, 1)):
        squash, soft = H.SQUASH_SOFT[family]
        d, n = mu.shape
        m, r = self.up(mu), self.up(raw)
        tg, ta = (None if g is None else self.up(g)), (None if dact is None else self.up(dact))
        outs, ptrs = self._outs([(n, d), (n, d)], need)
        self.call("rlhip_gaussian_head_sample_bwd_f32", self.ptr(m), self.ptr(r), d, n, K, float(lo), float(hi), squash, soft, seed, base,
                  step, self.ptr(ta), self.ptr(tg), *ptrs, self.sp())
        return [self.down(o) for o in outs]

    def normlogpdf_bwd(self, mu, sigma, x, g, need=(1, 1, 1)):
        ins = [self.up(t) for t in (mu, sigma, x, g)]
        outs, ptrs = self._outs([tuple(ins[0].shape)] * 3, need)
        self.call("rlhip_normlogpdf_bwd_f32", *(self.ptr(t) for t in ins), mu.size, *ptrs, self.sp())
        return [self.down(o) for o in outs]

    def diagnormlogpdf_bwd(self, mu, sigma, x, g, need=(1, 1, 1)):
        d, n = mu.shape
        ins = [self.up(t) for t in (mu, sigma, x, g)]
        outs, ptrs = self._outs([(n, d)] * 3, need)
        self.call("rlhip_diagnormlogpdf_bwd_f32", *(self.ptr(t) for t in ins), d, n, *ptrs, self.sp())
        return [self.down(o) for o in outs]


@pytest.fixture(scope="module")
def dev():
    import rlhip  # noqa: F401
    return HeadsDevice()


def _show(res):
    print({k: (f"{v:.3g}" if isinstance(v, float) else v) for k, v in res.items()})
    return res


def check_sampling(dev, family, mu, raw, K, lo, hi, seed, base, step, tag):
    """the sampling pullback against the exact replay on the forward's own draws (and, soft, its own tanhf(z)): bit for bit, with every
    combination of the nullable cotangents -> (eps, the forward's actions)"""
    d, n = mu.shape
    eps = G.draws(dev.sample, d, n, K, seed, base, step)
    a, _ = dev.sample(mu, raw, K, lo, hi, family, seed, base, step)
    g, da = G.cotangent((K, n), 1), G.cotangent((d, K, n), 2)
    combos = ((g, da), (g, None), (None, da)) if family == "soft" else ((g, None),)
    for gg, dd in combos:
        got = dev.sample_bwd(family, mu, raw, K, lo, hi, seed, base, step, g=gg, dact=dd)
        want = G.sample_bwd(family, mu, raw, eps, lo, hi, g=gg, dact=dd, t=a if family == "soft" else None)
        for name, x, y in zip(("dmu", "draw_sigma"), got, want):
            assert G.same(x, y), f"sample {name} {tag} dlogp={gg is not None} dact={dd is not None}: {int((x != y).sum())} of {x.size} differ"
    return eps, a


def check_eval(dev, family, mu, raw, a, lo, hi, tag):
    """the (state, action) pullback at the actions a: exact elements bit for bit, the others within 2 x budget, non-finite patterns equal"""
    K, n = a.shape[1:]
    g = G.cotangent((K, n), 1)
    got = dev.logp_bwd(family, mu, raw, a, g, lo, hi)
    want = G.logp_bwd(family, mu, raw, a, g, lo, hi)
    res = [_show(G.judge_grad(x, c, e, tag=f"eval {name} {tag}")) for name, x, (c, e) in zip(("dmu", "draw_sigma"), got, want)]
    if family == "identity":
        assert all(r["exact"] + r["non_finite"] == r["n"] for r in res), tag
    return got, res


@pytest.mark.parametrize("family", H.FAMILIES)
@pytest.mark.parametrize("d,n,K", H.SHAPES)
def test_head_pullbacks_match_the_model(dev, family, d, n, K):
    """both head entries through the C ABI: the sampling forms and the identity evaluation bit for bit, tanh / soft evaluation within
    2 x budget; outputs not asked for keep the sentinel"""
    tag = f"{family} d={d} n={n} K={K}"
    mu, raw = H.inputs(d, n, seed=d)
    eps, a = check_sampling(dev, family, mu, raw, K, LO, HI, SEED, BASE, STEP, tag)
    full, _ = check_eval(dev, family, mu, raw, a, LO, HI, tag)
    g = G.cotangent((K, n), 1)
    if family == "identity":                                        # networks.jl tests :73-110: the two gradients are identical
        z = dev.sample_bwd(family, mu, raw, K, LO, HI, SEED, BASE, STEP, g=g)
        assert G.same(z[0], full[0]) and G.same(z[1], full[1]), tag
    sfull = dev.sample_bwd(family, mu, raw, K, LO, HI, SEED, BASE, STEP, g=g)
    for need in ((1, 0), (0, 1), (0, 0)):
        for run, ref in ((dev.logp_bwd(family, mu, raw, a, g, LO, HI, need=need), full),
                         (dev.sample_bwd(family, mu, raw, K, LO, HI, SEED, BASE, STEP, g=g, need=need), sfull)):
            for b in range(2):
                assert G.same(run[b], ref[b]) if need[b] else (run[b] == SENTINEL).all(), (tag, need, b)


@pytest.mark.parametrize("d,n,K", H.SHAPES)
def test_density_pullbacks_match_the_model(dev, d, n, K):
    mu, raw = H.inputs(d, n, seed=d)
    x = (mu + 2 * np.random.default_rng(d).normal(size=(d, n))).astype(F32)
    ge, gc = G.cotangent((d, n), 4), G.cotangent((n,), 3)
    for fn, ref, g in ((dev.normlogpdf_bwd, G.normlogpdf_bwd, ge), (dev.diagnormlogpdf_bwd, G.diagnormlogpdf_bwd, gc)):
        full = fn(mu, raw, x, g)
        for name, a, b in zip(("dmu", "dsigma", "dx"), full, ref(mu, raw, x, g)):
            assert G.same(a, b), f"{fn.__name__} {name} d={d} n={n}"
        for mask in range(7):
            need = [(mask >> b) & 1 for b in range(3)]
            for b, (got, want) in enumerate(zip(fn(mu, raw, x, g, need=need), full)):
                assert G.same(got, want) if need[b] else (got == SENTINEL).all(), (fn.__name__, need, b)


@pytest.mark.parametrize("family", H.FAMILIES)
@pytest.mark.parametrize("base,step,n", [(2 ** 32 - 2, 0, 300), (5, 2 ** 32 - 1, 64), (0xFFFFFFF0, 7, 257)])
def test_regenerated_draws_follow_the_counters(dev, family, base, step, n):
    """env_id_base + i wraps at 2^32, a non-zero step, n that is no multiple of 256; odd d with K > 1"""
    d, K = 3, 2
    mu, raw = H.inputs(d, n, seed=n)
    eps, _ = check_sampling(dev, family, mu, raw, K, LO, HI, SEED, base, step, f"{family} base={base} step={step} n={n}")
    other = G.draws(dev.sample, d, n, K, SEED, base, (step + 1) % 2 ** 32)
    assert not G.same(eps, other)


@pytest.mark.parametrize("name", sorted(H.edge_cases()))
@pytest.mark.parametrize("family", H.FAMILIES)
def test_edge_patterns(dev, family, name):
    """raw sigma at, below and above the clamp limits (+0 outside, the gradient passes at the limits), NaN sigma (passes), sigma = 0,
    min == max, saturating means (the evaluation point is a = +-1: the model's non-finite pattern), a subnormal prod(v)"""
    case = H.edge_cases()[name]
    mu, raw, lo, hi, K = case["mu"], case["raw"], case["lo"], case["hi"], case["K"]
    tag = f"{name} {family}"
    eps, a = check_sampling(dev, family, mu, raw, K, lo, hi, SEED, BASE, STEP, tag)
    g = G.cotangent((K, mu.shape[1]), 1)
    dmu, dsg = dev.sample_bwd(family, mu, raw, K, lo, hi, SEED, BASE, STEP, g=g)
    ok = G.passes(raw, lo, hi)
    assert not dsg[~ok].any() and not np.signbit(dsg[~ok]).any(), tag
    if name == "clamp_limits":
        at = (raw == F32(lo)) | (raw == F32(hi))
        assert at.sum() >= 8 and (dsg[at] != 0).all() and np.isfinite(dmu).all(), tag
    if name == "nan_sigma":
        assert np.array_equal(np.isnan(dmu), np.isnan(raw)) and np.array_equal(np.isnan(dsg), np.isnan(raw)), tag
    if name.startswith("sigma0") or name == "subnormal_prod":
        assert np.isfinite(dmu).all() and np.isfinite(dsg).all(), tag
    if name == "saturated":
        assert np.isfinite(dmu).all(), tag
    got, res = check_eval(dev, family, mu, raw, a, lo, hi, tag)
    if name == "saturated" and family != "identity":
        assert res[0]["non_finite"] == res[0]["n"] and not got[1].any(), tag          # raw = 1 is clamped to 0.05: dsg is +0 even there
    # the densities on the same sigma edges
    x, sg = a[:, 0, :], H.clamp(raw, lo, hi)
    for a_, b_ in zip(dev.normlogpdf_bwd(mu, sg, x, G.cotangent(mu.shape, 4)), G.normlogpdf_bwd(mu, sg, x, G.cotangent(mu.shape, 4))):
        assert G.same(a_, b_), tag
    for a_, b_ in zip(dev.diagnormlogpdf_bwd(mu, sg, x, g[0]), G.diagnormlogpdf_bwd(mu, sg, x, g[0])):
        assert G.same(a_, b_), tag


def test_non_finite_cotangent_at_a_clamped_component_gives_zero(dev):
    """draw_sigma is a select: a NaN / Inf dsg at a component outside [lo, hi] is +0, not NaN"""
    d, n, K = 3, 8, 2
    mu, raw = H.inputs(d, n, seed=3)
    raw[:, :4], raw[:, 4:], mu[1, :] = 0.05, 0.9, np.inf
    for family in H.FAMILIES:
        eps, a = check_sampling(dev, family, mu, raw, K, LO, HI, SEED, BASE, STEP, "inf mu " + family)
        dmu, dsg = dev.sample_bwd(family, mu, raw, K, LO, HI, SEED, BASE, STEP, g=G.cotangent((K, n), 1))
        assert not dsg[:, :4].any() and not np.signbit(dsg[:, :4]).any() and np.isnan(dsg[1, 4:]).all(), family


@pytest.mark.parametrize("d,n,K", H.SCALED_SHAPES)
def test_tanh_sampling_pullback_is_finite_where_the_saved_action_saturates(dev, d, n, K):
    mu, raw = H.inputs(d, n, seed=d, scale=3.0)
    for family in ("tanh", "soft"):
        tag = f"{family} d={d} n={n} K={K} mu x 3"
        eps, a = check_sampling(dev, family, mu, raw, K, LO, HI, SEED, BASE, STEP, tag)
        assert (np.abs(a) == 1).sum() >= 5
        for out in dev.sample_bwd(family, mu, raw, K, LO, HI, SEED, BASE, STEP, g=G.cotangent((K, n), 1)):
            assert np.isfinite(out).all(), tag
        got, res = check_eval(dev, family, mu, raw, a, LO, HI, tag)
        assert sum(r["non_finite"] for r in res) >= 2 and not np.isfinite(got[0]).all()


def test_k_sum_is_bit_identical_from_run_to_run(dev):
    d, n, K = 2, 1, 300
    mu, raw = H.inputs(d, n, seed=d)
    g, da = G.cotangent((K, n), 1), G.cotangent((d, K, n), 2)
    first = dev.sample_bwd("soft", mu, raw, K, LO, HI, SEED, BASE, STEP, g=g, dact=da)
    for _ in range(3):
        again = dev.sample_bwd("soft", mu, raw, K, LO, HI, SEED, BASE, STEP, g=g, dact=da)
        assert G.same(again[0], first[0]) and G.same(again[1], first[1])


@pytest.mark.parametrize("family", H.FAMILIES)
def test_pair_kernel_and_single_kernel_agree_on_even_d(dev, family, monkeypatch):
    """even d takes one lane per component pair (one Philox block for both draws); with the A/B hook of tools/heads_grad_time.py it
    takes the kernel odd d uses -- the same bits either way"""
    d, n, K = 6, 300, 3
    mu, raw = H.inputs(d, n, seed=d)
    kw = dict(g=G.cotangent((K, n), 1), dact=G.cotangent((d, K, n), 2) if family == "soft" else None)
    paired = dev.sample_bwd(family, mu, raw, K, LO, HI, SEED, BASE, STEP, **kw)
    monkeypatch.setenv("RLHIP_HEAD_GRAD_PAIR", "0")
    single = dev.sample_bwd(family, mu, raw, K, LO, HI, SEED, BASE, STEP, **kw)
    assert G.same(paired[0], single[0]) and G.same(paired[1], single[1])
    eps = G.draws(dev.sample, d, n, K, SEED, BASE, STEP)
    t = dev.sample(mu, raw, K, LO, HI, family, SEED, BASE, STEP)[0] if family == "soft" else None
    want = G.sample_bwd(family, mu, raw, eps, LO, HI, t=t, **kw)
    assert G.same(single[0], want[0]) and G.same(single[1], want[1])


def test_bad_arguments_launch_nothing(dev):
    """d = 0, 65, K = 0, NULL inputs, a dact for soft = 0, no cotangent: RLHIP_EINVAL, and the output buffers keep their contents"""
    from rlhip import _lib

    n, K = 4, 2
    out, src = torch.full((n * K * 65,), 7.0, device="cuda"), torch.full((n * K * 65,), 7.0, device="cuda")
    P, sp = dev.ptr, dev.sp
    for d in (0, 65):
        for name, args in (("rlhip_diagnormlogpdf_bwd_f32", (P(src), P(src), P(src), P(src), d, n, P(out), P(out), P(out), sp())),
                           ("rlhip_gaussian_head_logp_bwd_f32", (P(src), P(src), P(src), P(src), d, n, K, 0.0, 1.0, 0, 0, P(out), P(out), sp())),
                           ("rlhip_gaussian_head_sample_bwd_f32", (P(src), P(src), d, n, K, 0.0, 1.0, 0, 1, 1, 0, 0, P(src), P(src), P(out),
                                                                   P(out), sp()))):
            with pytest.raises(_lib.RLHipArgumentError, match="d must be in 1 ... 64"):
                dev.call(name, *args)
    with pytest.raises(_lib.RLHipArgumentError):
        dev.call("rlhip_gaussian_head_logp_bwd_f32", P(src), P(src), P(src), P(src), 3, n, 0, 0.0, 1.0, 0, 0, P(out), P(out), sp())
    with pytest.raises(_lib.RLHipArgumentError, match="dact must be NULL"):
        dev.call("rlhip_gaussian_head_sample_bwd_f32", P(src), P(src), 3, n, K, 0.0, 1.0, 1, 0, 1, 0, 0, P(src), P(src), P(out), P(out), sp())
    with pytest.raises(_lib.RLHipArgumentError, match="NULL"):
        dev.call("rlhip_gaussian_head_sample_bwd_f32", P(src), P(src), 3, n, K, 0.0, 1.0, 1, 1, 1, 0, 0, None, None, P(out), P(out), sp())
    with pytest.raises(_lib.RLHipArgumentError, match="NULL"):
        dev.call("rlhip_normlogpdf_bwd_f32", P(src), P(src), P(src), None, n, P(out), P(out), P(out), sp())
    dev.call("rlhip_gaussian_head_logp_bwd_f32", P(src), P(src), P(src), P(src), 3, 0, K, 0.0, 1.0, 0, 0, P(out), P(out), sp())
    dev.call("rlhip_gaussian_head_sample_bwd_f32", P(src), P(src), 3, 0, K, 0.0, 1.0, 0, 1, 1, 0, 0, P(src), P(src), P(out), P(out), sp())
    dev.call("rlhip_gaussian_head_sample_bwd_f32", P(src), P(src), 3, n, K, 0.0, 1.0, 0, 1, 1, 0, 0, P(src), P(src), None, None, sp())
    dev.call("rlhip_normlogpdf_bwd_f32", P(src), P(src), P(src), P(src), 0, P(out), P(out), P(out), sp())
    dev.call("rlhip_diagnormlogpdf_bwd_f32", P(src), P(src), P(src), P(src), 3, n, None, None, None, sp())
    torch.cuda.synchronize()
    assert (out == 7).all()


# ------------------------------------------------------------------------------------------------ rlhip/grad.py end to end
def _net(rl, family, lin_mu, lin_sg, keep, **kw):
    """a head over torch.nn.Linear sub-networks; `keep` receives the heads' outputs (d, n) of every call"""
    squash, soft = H.SQUASH_SOFT[family]

    def mu(s):
        keep["mu"] = lin_mu(s.t()).t()
        return keep["mu"]

    def sigma(s):
        keep["raw"] = torch.nn.functional.softplus(lin_sg(s.t())).t()
        return keep["raw"]

    if soft:
        return rl.SoftGaussianNetwork(mu=mu, sigma=sigma, min_sigma=LO, max_sigma=HI, **kw)
    return rl.GaussianNetwork(mu=mu, sigma=sigma, min_sigma=LO, max_sigma=HI, squash="tanh" if squash else "identity", **kw)


@pytest.mark.parametrize("family", H.FAMILIES)
def test_autograd_through_the_networks_on_the_device(dev, family):
    """torch.autograd.grad through the heads over torch.nn.Linear equals the ABI result; forward values with and without requires_grad
    are bit-identical, `step` advances alike, and only a SoftGaussianNetwork's actions require a gradient"""
    import rlhip

    soft = family == "soft"
    ns, d, n, K = 4, 5, 33, 3
    torch.manual_seed(3)
    lin_mu, lin_sg = torch.nn.Linear(ns, d).cuda(), torch.nn.Linear(ns, d).cuda()
    keep = {}
    live = _net(rlhip, family, lin_mu, lin_sg, keep, seed=SEED, env_id_base=BASE)
    plain = _net(rlhip, family, lin_mu, lin_sg, {}, seed=SEED, env_id_base=BASE)
    live.step = plain.step = STEP
    state = torch.tensor(np.random.default_rng(1).normal(size=(ns, 1, n)), dtype=torch.float32, device="cuda")
    g, da = G.cotangent((K, n), 1), G.cotangent((d, K, n), 2)
    tg, tda = torch.tensor(g, device="cuda"), torch.tensor(da, device="cuda")
    params = list(lin_mu.parameters()) + list(lin_sg.parameters())
    # action_samples
    with torch.no_grad():
        a0, lp0 = plain.sample(state, K)
    a1, lp1 = live.sample(state, K)
    assert torch.equal(a0, a1) and torch.equal(lp0, lp1) and live.step == plain.step == STEP + 1
    assert a1.requires_grad == soft and lp1.requires_grad and not a0.requires_grad
    loss = (lp1[0] * tg).sum() + ((a1 * tda).sum() if soft else 0.0)
    grads = torch.autograd.grad(loss, [keep["mu"], keep["raw"]] + params)
    mu, raw = keep["mu"].detach().cpu().numpy(), keep["raw"].detach().cpu().numpy()
    want = dev.sample_bwd(family, mu, raw, K, LO, HI, SEED, BASE, STEP, g=g, dact=da if soft else None)
    assert G.same(grads[0].cpu().numpy(), want[0]) and G.same(grads[1].cpu().numpy(), want[1])
    assert all(torch.isfinite(t).all() and t.abs().max() > 0 for t in grads[2:])
    # is_sampling = True: the log-probability, and (soft) the actions alone
    s2 = state[:, 0, :]
    with torch.no_grad():
        a0, lp0 = plain(s2, is_sampling=True, is_return_log_prob=True)
    a1, lp1 = live(s2, is_sampling=True, is_return_log_prob=True)
    assert torch.equal(a0, a1) and torch.equal(lp0, lp1) and a1.shape == (d, n) and lp1.shape == (1, n)
    grads = torch.autograd.grad(lp1.sum(), [keep["mu"], keep["raw"]])
    want = dev.sample_bwd(family, mu, raw, 1, LO, HI, SEED, BASE, STEP + 1, g=np.ones((1, n), F32))
    assert G.same(grads[0].cpu().numpy(), want[0]) and G.same(grads[1].cpu().numpy(), want[1])
    a1 = live(s2, is_sampling=True)
    with torch.no_grad():
        a0 = plain(s2, is_sampling=True)
    assert torch.equal(a0, a1) and a1.requires_grad == soft and live.step == plain.step == STEP + 3
    if soft:
        grads = torch.autograd.grad((a1 * tda[:, 0, :]).sum(), [keep["mu"], keep["raw"]])
        want = dev.sample_bwd(family, mu, raw, 1, LO, HI, SEED, BASE, STEP + 2, dact=da[:, :1, :])
        assert G.same(grads[0].cpu().numpy(), want[0]) and G.same(grads[1].cpu().numpy(), want[1])
    # (state, action)
    act = dev.sample(mu, raw, K, LO, HI, family, SEED, BASE, STEP)[0]
    ta = torch.tensor(act, device="cuda")
    with torch.no_grad():
        lp0 = plain(state, ta)
    lp1 = live(state, ta)
    assert torch.equal(lp0, lp1) and lp1.shape == (1, K, n) and live.step == STEP + 3
    grads = torch.autograd.grad((lp1[0] * tg).sum(), [keep["mu"], keep["raw"]])
    want = dev.logp_bwd(family, mu, raw, act, g, LO, HI)
    assert G.same(grads[0].cpu().numpy(), want[0]) and G.same(grads[1].cpu().numpy(), want[1])
    with pytest.raises(NotImplementedError, match="actions .* are data"):
        live(state, ta.clone().requires_grad_(True))


def test_density_functions_under_autograd_on_the_device(dev):
    from rlhip import ops

    d, n = 5, 33
    mu, raw = H.inputs(d, n, seed=d)
    x = (mu + 1).astype(F32)
    ge, gc = G.cotangent((d, n), 4), G.cotangent((n,), 3)
    for fn, bwd, g in ((ops.normlogpdf, dev.normlogpdf_bwd, ge), (ops.diagnormlogpdf, dev.diagnormlogpdf_bwd, gc)):
        ts = [dev.up(a).requires_grad_(True) for a in (mu, raw, x)]
        with torch.no_grad():
            plain = fn(*ts)
        out = fn(*ts)
        assert out.grad_fn is not None and torch.equal(out, plain)
        (out * dev.up(g)).sum().backward()
        for t, w in zip(ts, bwd(mu, raw, x, g)):
            assert G.same(dev.down(t.grad), w)


# ------------------------------------------------------------------------------------------------ an SAC-style actor trains
# loss = mean(0.2 logp - Q(a)) with the fixed critic Q(a) = -|a - a*|^2 over a SoftGaussianNetwork, d = 2, 256 states, 40 Adam steps at
# lr 0.05.  Three runs from the same weights on the same per-step draws (read back from the device through the identity trick):
# the device run through rlhip/grad.py, a float64 torch model on the CPU, and the same model in torch Float32 autograd on the CPU with no
# project code in it.  The bar on |device - float64| of the final loss is 10 x the gap |Float32 torch - float64| of that third run: the
# margin covers the kernel's different, stated rounding order compounding through Adam.  Measured once on one MI355X:
# profiles/heads_grad.md.
TRAIN_STEPS, TRAIN_LR, ALPHA = 40, 0.05, 0.2
A_STAR = (0.5, -0.3)
TRAIN_LO, TRAIN_HI = 0.05, 2.0


def _sac_loss_torch(ps, state, eps, dtype):
    """the reference's SoftGaussianNetwork sampling call (networks.jl:153-160) and the actor loss, in plain torch"""
    mu = state @ ps[0].t() + ps[1]
    raw = torch.nn.functional.softplus(state @ ps[2].t() + ps[3])
    sg = raw.clamp(TRAIN_LO, TRAIN_HI)
    z = mu + sg * eps
    zz = (z - mu) / (sg + 1e-8)
    nl = -(zz * zz + math.log(2.0 * math.pi)) / 2.0 - torch.log(sg + 1e-8)
    lp = (nl - 2.0 * (math.log(2.0) - z - torch.nn.functional.softplus(-2.0 * z))).sum(1)
    a = torch.tanh(z)
    q = -((a - torch.tensor(A_STAR, dtype=dtype)) ** 2).sum(1)
    return (ALPHA * lp - q).mean()


def train_sac_actor(dev, steps=TRAIN_STEPS, lr=TRAIN_LR):
    """-> the losses of the device run, of the float64 CPU run and of the Float32 CPU torch run"""
    import rlhip

    ns, d, n = 3, 2, 256
    state = np.random.default_rng(2025).normal(size=(ns, n))
    torch.manual_seed(11)
    lin_mu, lin_sg = torch.nn.Linear(ns, d), torch.nn.Linear(ns, d)
    init = [p.detach().clone() for p in (lin_mu.weight, lin_mu.bias, lin_sg.weight, lin_sg.bias)]
    draws = [G.draws(dev.sample, d, n, 1, SEED, BASE, t)[:, 0, :].T.copy() for t in range(steps + 1)]       # (n, d) per step

    def cpu_run(dtype):
        ps = [p.to(dtype).requires_grad_(True) for p in init]
        s = torch.tensor(state.T, dtype=dtype)
        opt = torch.optim.Adam(ps, lr=lr)
        out = []
        for t in range(steps + 1):
            loss = _sac_loss_torch(ps, s, torch.tensor(draws[t], dtype=dtype), dtype)
            out.append(float(loss.detach()))
            opt.zero_grad()
            loss.backward()
            opt.step()
        return out

    ref64, ref32 = cpu_run(torch.float64), cpu_run(torch.float32)
    lin_mu, lin_sg = lin_mu.cuda(), lin_sg.cuda()
    net = rlhip.SoftGaussianNetwork(mu=lambda s: lin_mu(s.t()).t(), sigma=lambda s: torch.nn.functional.softplus(lin_sg(s.t())).t(),
                                    min_sigma=TRAIN_LO, max_sigma=TRAIN_HI, seed=SEED, env_id_base=BASE)
    s32 = torch.tensor(state, dtype=torch.float32, device="cuda")
    a_star = torch.tensor(A_STAR, device="cuda")[:, None]
    opt = torch.optim.Adam(list(lin_mu.parameters()) + list(lin_sg.parameters()), lr=lr)
    got = []
    for t in range(steps + 1):
        a, lp = net(s32, is_sampling=True, is_return_log_prob=True)
        loss = (ALPHA * lp[0] + ((a - a_star) ** 2).sum(0)).mean()
        got.append(float(loss.detach()))
        opt.zero_grad()
        loss.backward()
        opt.step()
    assert net.step == steps + 1
    return got, ref64, ref32


def test_an_sac_style_actor_trains(dev):
    got, ref64, ref32 = train_sac_actor(dev)
    gap, gap32 = abs(got[-1] - ref64[-1]), abs(ref32[-1] - ref64[-1])
    bar = 10 * gap32
    print(f"device loss {got[0]:.6f} -> {got[-1]:.6f}; float64 loss {ref64[0]:.6f} -> {ref64[-1]:.6f}; Float32 torch loss -> {ref32[-1]:.6f}; "
          f"gap device - float64 {gap:.3e}, gap Float32 torch - float64 {gap32:.3e} (bar {bar:.3e})")
    assert got[-1] < got[0], "the loss did not fall"
    assert ref64[-1] < ref64[0]
    assert gap <= bar, f"final loss {got[-1]!r} is {gap:.3e} from the float64 run's {ref64[-1]!r} (bar 10 x {gap32:.3e})"
