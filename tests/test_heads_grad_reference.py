"""The model of csrc/heads_grad.hip (tests/heads_grad_ref.py) against float64 autograd of the reference's formulas, against the
reference's own gradient tests and against planted faults; its edge patterns; the host wrappers with the C calls stubbed; the four entry
points in the built library; and the wiring of rlhip/grad.py and rlhip/heads.py with the oracle and the model standing in for the C
calls.  CPU only: the draws come from the oracle's forward head (mu = 0, sigma = 1, identity), t = tanhf(z) from its soft head."""
import math
import os

import numpy as np
import pytest
import torch

import heads_grad_ref as G
import heads_ref as H
import oracle
from heads_ref import F32, F64
from test_heads_reference import OracleHeads as O
from test_mvnorm_grad_reference import J, _patch, _Stub

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMS = ["rlhip_normlogpdf_bwd_f32", "rlhip_diagnormlogpdf_bwd_f32", "rlhip_gaussian_head_logp_bwd_f32",
        "rlhip_gaussian_head_sample_bwd_f32"]
LO, HI = H.LO, H.HI
SEED, BASE, STEP = H.SEED, H.BASE, H.STEP
EPS64, LOG2PI64 = float(H.EPS), float(H.LOG2PI)


# ------------------------------------------------------------------- the reference's formulas in float64 torch, written independently
# Julia shapes throughout: mu, sigma (d, n) or (d, 1, n); z (d, K, n); the reductions over dims = 1 are over axis 0
def t64(a, grad=True):
    return torch.tensor(np.asarray(a, F64), requires_grad=grad)


def normlogpdf64(mu, sigma, x):
    """distributions.jl:18-21"""
    z = (x - mu) / (sigma + EPS64)
    return -(z * z + LOG2PI64) / 2.0 - torch.log(sigma + EPS64)


def diagnormlogpdf64(mu, sigma, x):
    """distributions.jl:31-34"""
    v = (sigma + EPS64) ** 2
    return -(torch.log(v.prod(0)) + ((x - mu) ** 2 / v).sum(0) + mu.shape[0] * LOG2PI64) / 2.0


def softplus64(x):
    return torch.log1p(torch.exp(-x.abs())) + torch.relu(x)


def head64(family, mu, raw, z, lo, hi):
    """the log-probability both networks attach to a pre-squash z (d, K, n): networks.jl:74 / :98 / :115 and :156 / :178 / :198"""
    squash, soft = H.SQUASH_SOFT[family]
    sg = raw.clamp(lo, hi)[:, None, :]                      # clamp's rule: the cotangent passes on [lo, hi], bounds included
    m = mu[:, None, :]
    if soft:
        return (normlogpdf64(m, sg, z) - 2.0 * (math.log(2.0) - z - softplus64(-2.0 * z))).sum(0)
    lp = diagnormlogpdf64(m, sg, z)
    return lp - torch.log(1.0 - torch.tanh(z) ** 2).sum(0) if squash else lp


def eval64(family, mu, raw, a, g, lo, hi):
    """gradient of sum(g * model(state, action)) wrt the heads' outputs; the actions are data"""
    squash, soft = H.SQUASH_SOFT[family]
    tm, tr, a = t64(mu), t64(raw), t64(a, False)
    z = torch.atanh(a) if (squash or soft) else a
    return [t.numpy() for t in torch.autograd.grad((head64(family, tm, tr, z, lo, hi) * t64(g, False)).sum(), (tm, tr))]


def sample64(family, mu, raw, eps, lo, hi, g=None, dact=None):
    """gradient of sum(g * logp) + sum(dact * action) through the sampling calls.  GaussianNetwork: z is drawn under
    ignore_derivatives (the Float32 z the kernel regenerates, as data); SoftGaussianNetwork: z = mu .+ sigma .* noise carries a gradient"""
    squash, soft = H.SQUASH_SOFT[family]
    tm, tr = t64(mu), t64(raw)
    if soft:
        z = tm[:, None, :] + tr.clamp(lo, hi)[:, None, :] * t64(eps, False)
    else:
        z = t64(F32(mu)[:, None, :] + H.clamp(raw, lo, hi)[:, None, :] * F32(eps), False)
    loss = 0.0
    if g is not None:
        loss = loss + (head64(family, tm, tr, z, lo, hi) * t64(g, False)).sum()
    if dact is not None:
        loss = loss + (torch.tanh(z) * t64(dact, False)).sum()
    return [t.numpy() for t in torch.autograd.grad(loss, (tm, tr))]


def _draws(d, n, K, seed=SEED, base=BASE, step=STEP):
    return G.draws(O.sample, d, n, K, seed, base, step)


def _soft_t(mu, raw, K, lo=LO, hi=HI, seed=SEED, base=BASE, step=STEP):
    """t = tanhf(z): the forward's own SoftGaussianNetwork action"""
    return O.sample(mu, raw, K, lo, hi, "soft", seed, base, step)[0]


def _actions(family, mu, raw, K, lo=LO, hi=HI):
    """the evaluation points of the forward suite: the oracle's own sampled (squashed) actions"""
    return np.ascontiguousarray(O.sample(mu, raw, K, lo, hi, family, SEED, BASE, STEP)[0])


def _exact(pair):
    c, e = pair
    assert not e.any(), "expected an exact replay"
    return c.astype(F32)


# ------------------------------------------------------------------------------------------------ (a) the model against autograd
@pytest.mark.parametrize("d,n,K", H.SHAPES)
def test_densities_match_float64_autograd(d, n, K):
    mu, raw = H.inputs(d, n, seed=d)
    x = (mu + 2 * np.random.default_rng(d).normal(size=(d, n))).astype(F32)
    ge, gc = G.cotangent((d, n), 4), G.cotangent((n,), 3)
    ts = [t64(a) for a in (mu, raw, x)]
    want = torch.autograd.grad((normlogpdf64(*ts) * t64(ge, False)).sum(), ts)
    for name, a, b in zip(("dmu", "dsigma", "dx"), G.normlogpdf_bwd(mu, raw, x, ge), want):
        assert G.approx(a, b.numpy()), f"normlogpdf {name}"
    ts = [t64(a) for a in (mu, raw, x)]
    want = torch.autograd.grad((diagnormlogpdf64(*ts) * t64(gc, False)).sum(), ts)
    for name, a, b in zip(("dmu", "dsigma", "dx"), G.diagnormlogpdf_bwd(mu, raw, x, gc), want):
        assert G.approx(a, b.numpy()), f"diagnormlogpdf {name}"


@pytest.mark.parametrize("family", H.FAMILIES)
@pytest.mark.parametrize("d,n,K", H.SHAPES)
def test_head_pullbacks_match_float64_autograd(family, d, n, K):
    """the sampling calls (K = 1: is_sampling; K > 1: action_samples) and (state, action), sigma clamped to [0.2, 1.7]"""
    mu, raw = H.inputs(d, n, seed=d)
    ok = G.passes(raw, LO, HI)
    assert (n * d < 50) or (0.02 < 1 - ok.mean() < 0.5), "the bounds must clamp some components"
    eps, g = _draws(d, n, K), G.cotangent((K, n), 1)
    tag = f"{family} d={d} n={n} K={K}"
    # (state, action)
    a = _actions(family, mu, raw, K)
    (cm, em), (cs, es) = G.logp_bwd(family, mu, raw, a, g, LO, HI)
    want = eval64(family, mu, raw, a, g, LO, HI)
    assert G.approx(cm, want[0]) and G.approx(cs, want[1]), "eval " + tag
    assert (family == "identity") == (not em.any() and not es.any())
    assert not cs[~ok].any() and not np.signbit(cs[~ok]).any()
    # sampling
    if family == "soft":
        t, da = _soft_t(mu, raw, K), G.cotangent((d, K, n), 2)
        for gg, dd in ((g, da), (g, None), (None, da)):
            got = G.sample_bwd(family, mu, raw, eps, LO, HI, g=gg, dact=dd, t=t)
            want = sample64(family, mu, raw, eps, LO, HI, g=gg, dact=dd)
            assert G.approx(got[0], want[0]) and G.approx(got[1], want[1]), f"sample {tag} g={gg is not None} dact={dd is not None}"
    else:
        got = G.sample_bwd(family, mu, raw, eps, LO, HI, g=g)
        want = sample64(family, mu, raw, eps, LO, HI, g=g)
        assert G.approx(got[0], want[0]) and G.approx(got[1], want[1]), "sample " + tag
    assert not got[1][~ok].any() and not np.signbit(got[1][~ok]).any()


# ------------------------------------------------------------------------------------------------ (b) the reference's own gradient tests
@pytest.mark.parametrize("K", [1, 3])
def test_reference_sampling_gradient_equals_the_state_action_gradient(K):
    """RLCore/test/utils/networks.jl:73-110 (10 actions x 3 states, cotangent 1): `g == g2`, the gradient through the sampling call
    and the one through (state, saved action) are identical -- here bit for bit, on the heads' outputs"""
    d, n = 10, 3
    mu, raw = H.inputs(d, n, seed=73)
    eps, one = _draws(d, n, K), np.ones((K, n), F32)
    a = _actions("identity", mu, raw, K, 0.0, np.inf)
    assert G.same(a, mu[:, None, :] + H.clamp(raw, 0.0, np.inf)[:, None, :] * eps)
    g1 = G.sample_bwd("identity", mu, raw, eps, 0.0, np.inf, g=one)
    g2 = G.logp_bwd("identity", mu, raw, a, one, 0.0, np.inf)
    assert G.same(g1[0], _exact(g2[0])) and G.same(g1[1], _exact(g2[1]))
    assert np.abs(g1[0]).max() > 0 and np.abs(g1[1]).max() > 0


# ------------------------------------------------------------------------------------------------ (c) planted faults must not pass
def _soft_case(d, n, K, seed=0):
    mu, raw = H.inputs(d, n, seed=seed or d)
    return mu, raw, _draws(d, n, K), _soft_t(mu, raw, K), G.cotangent((K, n), 1), G.cotangent((d, K, n), 2)


def test_fault_descending_j_sum():
    d, n, K = 2, 1, 300
    mu, raw, eps, t, g, da = _soft_case(d, n, K)
    raw[:] = 0.9                                                    # inside the bounds: dsg is not masked
    t = _soft_t(mu, raw, K)
    good, bad = G.sample_bwd("soft", mu, raw, eps, LO, HI, g=g, dact=da, t=t), G.sample_bwd("soft", mu, raw, eps, LO, HI, g=g, dact=da, t=t,
                                                                                          descending=True)
    assert not G.same(bad[0], good[0]) and not G.same(bad[1], good[1])
    assert G.approx(bad[0], good[0]) and G.approx(bad[1], good[1])   # ... a fault that only the bit-for-bit judge sees
    a = _actions("identity", mu, raw, K)
    good, bad = G.logp_bwd("identity", mu, raw, a, g, LO, HI), G.logp_bwd("identity", mu, raw, a, g, LO, HI, descending=True)
    assert not G.same(_exact(bad[0]), _exact(good[0])) and not G.same(_exact(bad[1]), _exact(good[1]))
    with pytest.raises(AssertionError):
        G.judge_grad(_exact(bad[1]), *good[1], tag="descending")


def test_fault_strict_bounds_lose_the_gradient_at_the_limit():
    case = H.edge_cases()["clamp_limits"]
    mu, raw, lo, hi, K = (case[k] for k in ("mu", "raw", "lo", "hi", "K"))
    d, n = mu.shape
    eps, g = _draws(d, n, K), G.cotangent((K, n), 1)
    good, bad = G.sample_bwd("identity", mu, raw, eps, lo, hi, g=g), G.sample_bwd("identity", mu, raw, eps, lo, hi, g=g, strict_pass=True)
    at = (raw == F32(lo)) | (raw == F32(hi))
    assert at.sum() >= 8 and G.same(bad[0], good[0]) and not G.same(bad[1], good[1])
    assert (good[1][at] != 0).all() and not bad[1][at].any() and G.same(bad[1][~at], good[1][~at])


def test_fault_clamp_as_a_product_leaks_nan():
    """raw below the bound where dsg is not finite (mu = Inf): the select gives +0, Julia's `delta * false`; a product gives NaN"""
    d, n, K = 3, 8, 2
    mu, raw = H.inputs(d, n, seed=3)
    raw[:, :4], raw[:, 4:], mu[1, :] = 0.05, 0.9, np.inf
    eps, g = _draws(d, n, K), G.cotangent((K, n), 1)
    good = G.sample_bwd("identity", mu, raw, eps, LO, HI, g=g)
    bad = G.sample_bwd("identity", mu, raw, eps, LO, HI, g=g, clamp_product=True)
    assert not good[1][:, :4].any() and not np.signbit(good[1][:, :4]).any() and np.isnan(good[1][1, 4:]).all()
    assert np.isnan(bad[1][1, :4]).all() and not G.same(bad[1], good[1])
    a = np.ascontiguousarray(np.broadcast_to(F32(0.5), (d, K, n)))
    good, bad = G.logp_bwd("soft", mu, raw, a, g, LO, HI), G.logp_bwd("soft", mu, raw, a, g, LO, HI, clamp_product=True)
    assert not good[1][0][:, :4].any() and np.isnan(bad[1][0][1, :4]).all()
    with pytest.raises(AssertionError):
        G.judge_grad(bad[1][0].astype(F32), *good[1], tag="product")


@pytest.mark.parametrize("fault", ["drop_dz_eps", "unsquashed_correction", "dact_without_jacobian"])
def test_fault_in_the_reparameterised_form(fault):
    d, n, K = 5, 33, 3
    mu, raw, eps, t, g, da = _soft_case(d, n, K)
    good = G.sample_bwd("soft", mu, raw, eps, LO, HI, g=g, dact=da, t=t)
    bad = G.sample_bwd("soft", mu, raw, eps, LO, HI, g=g, dact=da, t=t, **{fault: True})
    want = sample64("soft", mu, raw, eps, LO, HI, g=g, dact=da)
    assert G.approx(good[0], want[0]) and G.approx(good[1], want[1])
    if fault == "drop_dz_eps":                                      # dmu does not contain the term
        assert G.same(bad[0], good[0])
    else:
        assert not G.same(bad[0], good[0]) and not G.approx(bad[0], want[0])
    assert not G.same(bad[1], good[1]) and not G.approx(bad[1], want[1])


def test_fault_draw_index_j_plus_K_k():
    """odd d with K > 1: a Philox pair straddles two samples; the regenerated draws must be k + d j"""
    d, n, K = 5, 33, 3
    mu, raw, eps, t, g, da = _soft_case(d, n, K)
    wrong = G.misindexed(eps)
    assert G.same(np.sort(wrong.reshape(-1, n), 0), np.sort(eps.reshape(-1, n), 0)) and not G.same(wrong, eps)
    assert G.same(wrong[0, 0], eps[0, 0]) and G.same(G.misindexed(_draws(d, n, 1)), _draws(d, n, 1))       # K = 1 cannot see it
    for family, kw in (("soft", dict(g=g, dact=da, t=t)), ("identity", dict(g=g)), ("tanh", dict(g=g))):
        good, bad = G.sample_bwd(family, mu, raw, eps, LO, HI, **kw), G.sample_bwd(family, mu, raw, wrong, LO, HI, **kw)
        want = sample64(family, mu, raw, eps, LO, HI, g=g, dact=kw.get("dact"))
        assert not G.same(bad[0], good[0]) and not G.same(bad[1], good[1]) and not G.approx(bad[1], want[1]), family


def test_judge_grad_holds_a_rounded_centre_and_fails_a_shifted_one():
    d, n, K = 3, 700, 4
    mu, raw = H.inputs(d, n, seed=d)
    g = G.cotangent((K, n), 1)
    for family in ("tanh", "soft"):
        a = _actions(family, mu, raw, K)
        for c, e in G.logp_bwd(family, mu, raw, a, g, LO, HI):
            r = G.judge_grad(c.astype(F32), c, e, tag=family)
            assert r["worst_over_bar"] <= 0.5 and r["non_finite"] == 0    # rounding the centre costs half an ulp, inside the bar
            with pytest.raises(AssertionError):
                G.judge_grad((c + np.where(e > 0, 3 * e, 1.0)).astype(F32), c, e, tag="shifted")


# ------------------------------------------------------------------------------------------------ (d) edge patterns of the model
def test_model_clamp_limits_nan_sigma_and_sigma_zero():
    E = H.edge_cases()
    case = E["clamp_limits"]
    mu, raw, lo, hi, K = (case[k] for k in ("mu", "raw", "lo", "hi", "K"))
    d, n = mu.shape
    eps, g = _draws(d, n, K), G.cotangent((K, n), 1)
    inside = (raw >= F32(lo)) & (raw <= F32(hi))
    for family in H.FAMILIES:
        kw = dict(g=g, t=_soft_t(mu, raw, K, lo, hi), dact=G.cotangent((d, K, n), 2)) if family == "soft" else dict(g=g)
        dmu, dsg = G.sample_bwd(family, mu, raw, eps, lo, hi, **kw)
        assert np.isfinite(dmu).all() and (dsg[inside] != 0).all(), family                    # raw == lo and raw == hi pass
        assert not dsg[~inside].any() and not np.signbit(dsg[~inside]).any(), family          # below / above (and +Inf, -1): +0
    case = E["nan_sigma"]
    mu, raw, lo, hi, K = (case[k] for k in ("mu", "raw", "lo", "hi", "K"))
    d, n = mu.shape
    eps, g = _draws(d, n, K), G.cotangent((K, n), 1)
    nan = np.isnan(raw)
    for family in H.FAMILIES:
        kw = dict(g=g, t=_soft_t(mu, raw, K, lo, hi)) if family == "soft" else dict(g=g)
        dmu, dsg = G.sample_bwd(family, mu, raw, eps, lo, hi, **kw)
        assert np.array_equal(np.isnan(dmu), nan) and np.array_equal(np.isnan(dsg), nan), family  # a NaN passes the clamp, per component
        (cm, _), (cs, _) = G.logp_bwd(family, mu, raw, np.zeros((d, K, n), F32), g, lo, hi)
        assert np.array_equal(np.isnan(cm), nan) and np.array_equal(np.isnan(cs), nan), family
    case = E["sigma0_d3"]                                           # s = 1e-8: finite, large
    mu, raw, lo, hi, K = (case[k] for k in ("mu", "raw", "lo", "hi", "K"))
    d, n = mu.shape
    eps, g = _draws(d, n, K), G.cotangent((K, n), 1)
    for family in H.FAMILIES:
        kw = dict(g=g, t=_soft_t(mu, raw, K, lo, hi)) if family == "soft" else dict(g=g)
        dmu, dsg = G.sample_bwd(family, mu, raw, eps, lo, hi, **kw)
        assert np.isfinite(dmu).all() and np.isfinite(dsg).all() and np.abs(dsg).max() > 1e6, family
    x = np.zeros((d, n), F32)
    for out in G.normlogpdf_bwd(mu, raw, x, G.cotangent((d, n), 4)) + G.diagnormlogpdf_bwd(mu, raw, x, G.cotangent((n,), 3)):
        assert np.isfinite(out).all() and np.abs(out).max() > 1e6


def test_model_actions_at_plus_minus_one():
    """a = +-1: atanh is +-Inf.  GaussianNetwork tanh: e / v = +-Inf, (e e) / v = +Inf; SoftGaussianNetwork likewise -- and a state
    whose K samples hold both signs gives Inf - Inf = NaN in dmu"""
    d, n, K = 2, 6, 2
    mu, raw = H.inputs(d, n, seed=2)
    raw[:] = 0.9
    a = np.full((d, K, n), 0.25, F32)
    a[0, 0, 0], a[0, 1, 1], a[1, 0, 2], a[1, 1, 2] = 1.0, -1.0, 1.0, -1.0
    g = np.ones((K, n), F32)
    for family in ("tanh", "soft"):
        (cm, em), (cs, es) = G.logp_bwd(family, mu, raw, a, g, LO, HI)
        assert cm[0, 0] == np.inf and cm[0, 1] == -np.inf and np.isnan(cm[1, 2]), family
        assert cs[0, 0] == np.inf and cs[0, 1] == np.inf and cs[1, 2] == np.inf, family
        assert np.isfinite(cm[:, 3:]).all() and np.isfinite(cs[:, 3:]).all()
        G.judge_grad(cm.astype(F32), cm, em, tag=family)
        bad = cm.astype(F32)
        bad[0, 1] = np.inf
        with pytest.raises(AssertionError, match="non-finite pattern"):
            G.judge_grad(bad, cm, em, tag=family)


@pytest.mark.parametrize("d,n,K", H.SCALED_SHAPES)
def test_tanh_sampling_pullback_stays_finite_where_the_saved_action_saturates(d, n, K):
    """mu x 3: tanhf(z) rounds to +-1 for some samples.  The pullback through the saved action is not finite there; the one that
    regenerates z is, and agrees with float64 autograd"""
    mu, raw = H.inputs(d, n, seed=d, scale=3.0)
    eps, g = _draws(d, n, K), G.cotangent((K, n), 1)
    a = _actions("tanh", mu, raw, K)
    assert (np.abs(a) == 1).sum() >= 5
    (cm, _), (cs, _) = G.logp_bwd("tanh", mu, raw, a, g, LO, HI)
    assert not np.isfinite(cm).all() and not np.isfinite(cs).all()
    for family in ("tanh", "soft"):
        kw = dict(g=g, t=_soft_t(mu, raw, K), dact=G.cotangent((d, K, n), 2)) if family == "soft" else dict(g=g)
        got = G.sample_bwd(family, mu, raw, eps, LO, HI, **kw)
        want = sample64(family, mu, raw, eps, LO, HI, g=g, dact=kw.get("dact"))
        assert np.isfinite(got[0]).all() and np.isfinite(got[1]).all()
        assert G.approx(got[0], want[0]) and G.approx(got[1], want[1]), family


# ------------------------------------------------------------------------------------------------ (e) the host wrappers, C calls stubbed
@pytest.fixture
def stub(monkeypatch):
    s = _Stub()
    _patch(monkeypatch, s.call)
    return s


def test_backward_wrappers_shapes_and_nullable_outputs(stub):
    from rlhip import _lib, ops

    n, d, K = 6, 4, 3
    mu, act, lp = torch.zeros((n, d)), torch.zeros((n, K, d)), torch.zeros((n, K))
    outs = ops.normlogpdf_backward(mu, mu, mu, mu)
    name, args = stub.calls[-1]
    assert name == "rlhip_normlogpdf_bwd_f32" and args[4] == n * d and all(a is o for a, o in zip(args[5:8], outs))
    outs = ops.normlogpdf_backward(mu, mu, mu, mu, need=(False, True, False))
    assert outs[0] is None and outs[2] is None and outs[1].shape == (n, d) and stub.calls[-1][1][5] is None and stub.calls[-1][1][7] is None
    outs = ops.diagnormlogpdf_backward(mu, mu, mu, torch.zeros(n), need=(True, False, True))
    name, args = stub.calls[-1]
    assert name == "rlhip_diagnormlogpdf_bwd_f32" and args[4:6] == (d, n) and args[6] is outs[0] and args[7] is None and args[8] is outs[2]
    dmu, draw = ops.gaussian_head_logp_backward(mu, mu, act, lp, 0.2, 1.7, 1, 0)
    name, args = stub.calls[-1]
    assert name == "rlhip_gaussian_head_logp_bwd_f32" and args[4:11] == (d, n, K, 0.2, 1.7, 1, 0) and args[11] is dmu and args[12] is draw
    dmu, draw = ops.gaussian_head_logp_backward(mu, mu, act, lp, 0.2, 1.7, 1, 1, need=(False, True))
    assert dmu is None and stub.calls[-1][1][11] is None and draw.shape == (n, d)
    dmu, draw = ops.gaussian_head_sample_backward(mu, mu, K, 0.2, 1.7, 1, 1, 11, 5, 4, dact=act, dlogp=None, need=(True, False))
    name, args = stub.calls[-1]
    assert name == "rlhip_gaussian_head_sample_bwd_f32" and args[2:12] == (d, n, K, 0.2, 1.7, 1, 1, 11, 5, 4)
    assert args[12] is act and args[13] is None and args[14] is dmu and args[15] is None and draw is None
    ops.gaussian_head_sample_backward(mu, mu, K, 0.0, float("inf"), 0, 0, 1, 2, 3, dlogp=lp)
    assert stub.calls[-1][1][12] is None and stub.calls[-1][1][13] is lp
    for bad in (lambda: ops.normlogpdf_backward(mu, mu, mu, lp),
                lambda: ops.diagnormlogpdf_backward(mu, mu, mu, mu),
                lambda: ops.gaussian_head_logp_backward(mu, mu, act, torch.zeros((n, K + 1)), 0, 1, 0, 0),
                lambda: ops.gaussian_head_logp_backward(mu, mu, mu, lp, 0, 1, 0, 0),
                lambda: ops.gaussian_head_sample_backward(mu, mu, K, 0, 1, 1, 1, 0, 0, 0, dact=torch.zeros((n, K, d + 1))),
                lambda: ops.gaussian_head_sample_backward(mu, mu, K + 1, 0, 1, 0, 0, 0, 0, 0, dlogp=lp)):
        with pytest.raises(_lib.RLHipArgumentError):
            bad()


def test_grad_module_is_bypassed_when_nothing_requires_grad(stub, monkeypatch):
    import rlhip
    from rlhip import grad, ops

    def boom(*a, **k):
        raise AssertionError("rlhip/grad.py was entered although nothing requires a gradient")

    for cls in (grad.NormLogPdf, grad.DiagNormLogPdf, grad.GaussianHeadLogp, grad.GaussianHeadSample):
        monkeypatch.setattr(cls, "apply", boom)
    n, d, K = 3, 2, 2
    mu, raw = torch.zeros((n, d)), torch.ones((n, d))
    nets = [rlhip.GaussianNetwork(mu=lambda s: mu.t(), sigma=lambda s: raw.t(), squash="tanh"),
            rlhip.SoftGaussianNetwork(mu=lambda s: mu.t(), sigma=lambda s: raw.t())]
    state = torch.zeros((4, n))

    def run():
        ops.normlogpdf(mu, raw, mu), ops.diagnormlogpdf(mu, raw, mu)
        for net in nets:
            net(state), net(state, torch.zeros((d, n))), net(state, is_sampling=True), net(state, is_sampling=True, is_return_log_prob=True)
            net.sample(torch.zeros((4, 1, n)), K)

    run()
    assert len(stub.calls) == 2 + 2 * 4 and [net.step for net in nets] == [3, 3]
    for t in (mu, raw):
        t.requires_grad_(True)
    with torch.no_grad():                                           # inputs that require grad, but grad mode is off
        run()
    assert len(stub.calls) == 2 * (2 + 2 * 4) and [net.step for net in nets] == [6, 6]
    nets[0](state, is_sampling=True)                                # a GaussianNetwork's actions alone: nothing to differentiate
    assert nets[0].step == 7
    for call in (lambda: ops.normlogpdf(mu, raw, mu), lambda: ops.diagnormlogpdf(mu, raw, mu), lambda: nets[0](state, torch.zeros((d, n))),
                 lambda: nets[1](state, is_sampling=True), lambda: nets[0].sample(torch.zeros((4, 1, n)), K)):
        with pytest.raises(AssertionError, match="grad.py was entered"):
            call()


# ------------------------------------------------------------------------------------------------ the built library
def test_the_four_entry_points_are_exported_with_prototypes():
    from rlhip import _lib

    syms = _lib.declared_symbols()
    for s in SYMS:
        assert s in syms and s in _lib._PROTOS and hasattr(_lib.lib, s), s
    assert _lib.lib.rlhip_abi_version() == 2
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    glue = open(os.path.join(ROOT, "reinforcementlearning.jl_amd", "julia", "RLHip.jl")).read()
    for s in SYMS:
        assert s in text, s
        assert f"ccall((:{s}, LIB)" in glue, s
    for fn in ("normlogpdf", "diagnormlogpdf"):
        assert f"function ChainRulesCore.rrule(::typeof(ReinforcementLearningCore.{fn})," in glue, fn
    for fn in ("gaussian_head_logp", "gaussian_head_sample"):
        assert f"function ChainRulesCore.rrule(::typeof({fn})," in glue, fn


@pytest.mark.parametrize("d", [0, 65, -1])
def test_bad_arguments_are_refused_before_any_device_work(d):
    """argument checks come before any HIP call: RLHIP_EINVAL with a message, no device needed"""
    from rlhip import _lib

    one = (np.zeros(4096, F32)).ctypes.data            # a non-NULL host address: never dereferenced
    L = _lib.lib
    assert L.rlhip_diagnormlogpdf_bwd_f32(one, one, one, one, d, 4, one, one, one, None) == -1 and b"d must be" in L.rlhip_last_error()
    assert L.rlhip_gaussian_head_logp_bwd_f32(one, one, one, one, d, 4, 1, 0.0, 1.0, 0, 0, one, one, None) == -1
    assert L.rlhip_gaussian_head_sample_bwd_f32(one, one, d, 4, 1, 0.0, 1.0, 0, 0, 1, 0, 0, None, one, one, one, None) == -1
    # K < 1, NULL inputs, a dact for soft = 0, both cotangents NULL, squash / soft out of range -- with a good d
    assert L.rlhip_gaussian_head_logp_bwd_f32(one, one, one, one, 3, 4, 0, 0.0, 1.0, 0, 0, one, one, None) == -1
    assert L.rlhip_gaussian_head_sample_bwd_f32(one, one, 3, 4, 0, 0.0, 1.0, 0, 1, 1, 0, 0, one, one, one, one, None) == -1
    assert L.rlhip_gaussian_head_sample_bwd_f32(one, one, 3, 4, 1, 0.0, 1.0, 0, 0, 1, 0, 0, one, one, one, one, None) == -1
    assert b"dact must be NULL" in L.rlhip_last_error()
    assert L.rlhip_gaussian_head_sample_bwd_f32(one, one, 3, 4, 1, 0.0, 1.0, 1, 0, 1, 0, 0, None, None, one, one, None) == -1
    assert L.rlhip_gaussian_head_sample_bwd_f32(one, one, 3, 4, 1, 0.0, 1.0, 1, 1, 1, 0, 0, None, None, one, one, None) == -1
    assert b"NULL" in L.rlhip_last_error()
    assert L.rlhip_gaussian_head_sample_bwd_f32(None, one, 3, 4, 1, 0.0, 1.0, 1, 1, 1, 0, 0, one, one, one, one, None) == -1
    assert L.rlhip_gaussian_head_sample_bwd_f32(one, one, 3, 4, 1, 0.0, 1.0, 2, 1, 1, 0, 0, one, one, one, one, None) == -1
    assert L.rlhip_gaussian_head_logp_bwd_f32(one, one, None, one, 3, 4, 1, 0.0, 1.0, 0, 0, one, one, None) == -1
    assert L.rlhip_gaussian_head_logp_bwd_f32(one, one, one, None, 3, 4, 1, 0.0, 1.0, 0, 0, one, one, None) == -1
    assert L.rlhip_gaussian_head_logp_bwd_f32(one, one, one, one, 3, 4, 1, 0.0, 1.0, 0, 3, one, one, None) == -1
    assert L.rlhip_normlogpdf_bwd_f32(one, None, one, one, 4, one, one, one, None) == -1 and b"NULL" in L.rlhip_last_error()
    assert L.rlhip_normlogpdf_bwd_f32(one, one, one, one, -1, one, one, one, None) == -1
    assert L.rlhip_diagnormlogpdf_bwd_f32(one, one, one, None, 2, 4, one, one, one, None) == -1
    assert L.rlhip_diagnormlogpdf_bwd_f32(one, one, one, one, 2, -1, one, one, one, None) == -1
    # n = 0 and "no output asked for" are no-ops that need no device either
    assert L.rlhip_normlogpdf_bwd_f32(one, one, one, one, 0, one, one, one, None) == 0
    assert L.rlhip_normlogpdf_bwd_f32(one, one, one, one, 4, None, None, None, None) == 0
    assert L.rlhip_diagnormlogpdf_bwd_f32(one, one, one, one, 2, 0, one, one, one, None) == 0
    assert L.rlhip_gaussian_head_logp_bwd_f32(one, one, one, one, 3, 0, 1, 0.0, 1.0, 0, 0, one, one, None) == 0
    assert L.rlhip_gaussian_head_logp_bwd_f32(one, one, one, one, 3, 4, 1, 0.0, 1.0, 0, 0, None, None, None) == 0
    assert L.rlhip_gaussian_head_sample_bwd_f32(one, one, 3, 0, 1, 0.0, 1.0, 0, 1, 1, 0, 0, one, one, one, one, None) == 0
    assert L.rlhip_gaussian_head_sample_bwd_f32(one, one, 3, 4, 1, 0.0, 1.0, 0, 1, 1, 0, 0, one, None, None, None, None) == 0


# ------------------------------------------------------------------------------------------------ (f) the wiring of rlhip/grad.py
class _ModelLibrary:
    """a CPU stand-in for the C calls: the forward entries computed by the oracle, the pullbacks by the model, on the storages handed
    over (pointers are the tensors themselves), outputs written in place, NULL outputs skipped"""

    def __init__(self):
        self.calls = []

    @staticmethod
    def _put(out, a):
        if out is not None:
            out.copy_(torch.tensor(J(np.asarray(a, F32))))

    @staticmethod
    def _family(squash, soft):
        return "soft" if soft else ("tanh" if squash else "identity")

    def call(self, name, *a):
        self.calls.append(name)
        j = lambda t: None if t is None else J(t.detach().numpy())                                  # noqa: E731
        if name == "rlhip_normlogpdf_f32":
            mu, s, x = (j(t) for t in a[:3])
            self._put(a[3], normlogpdf64(*(t64(v, False) for v in (mu, s, x))).numpy())
        elif name == "rlhip_diagnormlogpdf_f32":
            self._put(a[5], oracle.diagnormlogpdf(*(j(t) for t in a[:3])))
        elif name == "rlhip_normlogpdf_bwd_f32":
            for out, v in zip(a[5:8], G.normlogpdf_bwd(*(j(t) for t in a[:4]))):
                self._put(out, v)
        elif name == "rlhip_diagnormlogpdf_bwd_f32":
            for out, v in zip(a[6:9], G.diagnormlogpdf_bwd(*(j(t) for t in a[:4]))):
                self._put(out, v)
        elif name == "rlhip_gaussian_head_sample_f32":
            mu, raw, d, n, K, lo, hi, squash, soft, seed, base, step, act, lp = a[:14]
            av, lv = oracle.gaussian_head_sample(j(mu), j(raw), K, lo, hi, squash, soft, seed=seed, env_id_base=base, step=step,
                                                 want_logp=lp is not None)
            self._put(act, av)
            self._put(lp, lv)
        elif name == "rlhip_gaussian_head_logp_f32":
            mu, raw, act, d, n, K, lo, hi, squash, soft, lp = a[:11]
            self._put(lp, oracle.gaussian_head_logp(j(mu), j(raw), j(act), lo, hi, squash, soft))
        elif name == "rlhip_gaussian_head_logp_bwd_f32":
            mu, raw, act, g, d, n, K, lo, hi, squash, soft, dmu, draw = a[:13]
            (cm, _), (cs, _) = G.logp_bwd(self._family(squash, soft), j(mu), j(raw), j(act), j(g), lo, hi)
            self._put(dmu, cm)
            self._put(draw, cs)
        elif name == "rlhip_gaussian_head_sample_bwd_f32":
            mu, raw, d, n, K, lo, hi, squash, soft, seed, base, step, dact, g, dmu, draw = a[:16]
            fam = self._family(squash, soft)
            t = O.sample(j(mu), j(raw), K, lo, hi, "soft", seed, base, step)[0] if soft else None
            vm, vs = G.sample_bwd(fam, j(mu), j(raw), G.draws(O.sample, d, n, K, seed, base, step), lo, hi, g=j(g), dact=j(dact), t=t)
            self._put(dmu, vm)
            self._put(draw, vs)
        else:
            raise AssertionError(f"unexpected call {name}")
        return 0


@pytest.fixture
def model_lib(monkeypatch):
    lib = _ModelLibrary()
    _patch(monkeypatch, lib.call)
    return lib


def _leaf(a, grad=True):
    return torch.tensor(np.asarray(a, F32), requires_grad=grad)


def test_density_functions_route_through_grad(model_lib):
    from rlhip import ops

    d, n = 4, 9
    mu, raw = H.inputs(d, n, seed=4)
    x, ge, gc = (mu + 1).astype(F32), G.cotangent((d, n), 4), G.cotangent((n,), 3)
    ts = [_leaf(J(a), w) for a, w in zip((mu, raw, x), (True, True, False))]
    out = ops.normlogpdf(*ts)
    with torch.no_grad():
        assert torch.equal(out, ops.normlogpdf(*ts))
    (out * torch.tensor(J(ge))).sum().backward()
    want = G.normlogpdf_bwd(mu, raw, x, ge)
    assert G.same(J(ts[0].grad.numpy()), want[0]) and G.same(J(ts[1].grad.numpy()), want[1]) and ts[2].grad is None
    ts = [_leaf(J(a)) for a in (mu, raw, x)]
    (ops.diagnormlogpdf(*ts) * torch.tensor(gc)).sum().backward()
    for t, w in zip(ts, G.diagnormlogpdf_bwd(mu, raw, x, gc)):
        assert G.same(J(t.grad.numpy()), w)


@pytest.mark.parametrize("family", H.FAMILIES)
def test_networks_are_differentiable_and_values_do_not_change(model_lib, family):
    """GaussianNetwork / SoftGaussianNetwork over leaf tensors as head outputs: the gradients autograd delivers are the model's, the
    forward values are those of the plain path, `step` advances alike, and only mu and raw_sigma are saved by the sampling Function"""
    import rlhip

    squash, soft = H.SQUASH_SOFT[family]
    d, n, K = 5, 7, 3
    mu, raw = H.inputs(d, n, seed=5)
    g, da = G.cotangent((K, n), 1), G.cotangent((d, K, n), 2)

    def net(m, r):
        kw = {} if soft else {"squash": "tanh" if squash else "identity"}
        return (rlhip.SoftGaussianNetwork if soft else rlhip.GaussianNetwork)(mu=lambda s: m, sigma=lambda s: r, min_sigma=LO, max_sigma=HI,
                                                                               seed=SEED, env_id_base=BASE, **kw)

    state3, state2 = torch.zeros((1, 1, n)), torch.zeros((1, n))
    plain, live = net(_leaf(mu, False), _leaf(raw, False)), net(_leaf(mu), _leaf(raw))
    plain.step = live.step = STEP
    m, r = live.mu(None), live.sigma(None)
    # action_samples
    a0, lp0 = plain.sample(state3, K)
    a1, lp1 = live.sample(state3, K)
    assert torch.equal(a0, a1) and torch.equal(lp0, lp1) and plain.step == live.step == STEP + 1
    assert a1.requires_grad == bool(soft) and lp1.requires_grad and not a0.requires_grad
    fn = lp1.grad_fn
    while fn is not None and not hasattr(fn, "saved_tensors"):
        fn = fn.next_functions[0][0]
    assert fn is not None and len(fn.saved_tensors) == 2 and all(tuple(t.shape) == (n, d) for t in fn.saved_tensors)
    loss = (lp1[0] * torch.tensor(g)).sum() + ((a1 * torch.tensor(da)).sum() if soft else 0.0)
    loss.backward()
    eps = G.draws(O.sample, d, n, K, SEED, BASE, STEP)
    kw = dict(g=g, dact=da, t=a0.numpy()) if soft else dict(g=g)
    want = G.sample_bwd(family, mu, raw, eps, LO, HI, **kw)
    assert G.same(m.grad.numpy(), want[0]) and G.same(r.grad.numpy(), want[1])
    # is_sampling = True, with and without the log-probability (step STEP + 1, STEP + 2)
    m.grad = r.grad = None
    a0, lp0 = plain(state2, is_sampling=True, is_return_log_prob=True)
    a1, lp1 = live(state2, is_sampling=True, is_return_log_prob=True)
    assert torch.equal(a0, a1) and torch.equal(lp0, lp1) and a1.shape == (d, n) and lp1.shape == (1, n)
    lp1.sum().backward()
    eps = G.draws(O.sample, d, n, 1, SEED, BASE, STEP + 1)
    kw = dict(g=np.ones((1, n), F32), t=a0.numpy()[:, None, :]) if soft else dict(g=np.ones((1, n), F32))
    want = G.sample_bwd(family, mu, raw, eps, LO, HI, **kw)
    assert G.same(m.grad.numpy(), want[0]) and G.same(r.grad.numpy(), want[1])
    m.grad = r.grad = None
    a0, a1 = plain(state2, is_sampling=True), live(state2, is_sampling=True)
    assert torch.equal(a0, a1) and plain.step == live.step == STEP + 3 and a1.requires_grad == bool(soft)
    if soft:                                                        # differentiable through the actions alone
        (a1 * torch.tensor(da[:, 0, :])).sum().backward()
        eps = G.draws(O.sample, d, n, 1, SEED, BASE, STEP + 2)
        want = G.sample_bwd(family, mu, raw, eps, LO, HI, dact=da[:, :1, :], t=a0.numpy()[:, None, :])
        assert G.same(m.grad.numpy(), want[0]) and G.same(r.grad.numpy(), want[1])
        m.grad = r.grad = None
    # (state, action): 3-D and 2-D actions
    act = O.sample(mu, raw, K, LO, HI, family, SEED, BASE, STEP)[0]
    lp0, lp1 = plain(state3, torch.tensor(act)), live(state3, torch.tensor(act))
    assert torch.equal(lp0, lp1) and lp1.shape == (1, K, n)
    (lp1[0] * torch.tensor(g)).sum().backward()
    (cm, _), (cs, _) = G.logp_bwd(family, mu, raw, act, g, LO, HI)
    assert G.same(m.grad.numpy(), cm.astype(F32)) and G.same(r.grad.numpy(), cs.astype(F32))
    m.grad = r.grad = None
    live(state2, torch.tensor(act[:, 0, :])).sum().backward()
    (cm, _), (cs, _) = G.logp_bwd(family, mu, raw, act[:, :1, :], np.ones((1, n), F32), LO, HI)
    assert G.same(m.grad.numpy(), cm.astype(F32)) and G.same(r.grad.numpy(), cs.astype(F32))
    with pytest.raises(NotImplementedError, match="actions .* are data"):
        live(state3, torch.tensor(act, requires_grad=True))
    assert "rlhip_gaussian_head_sample_bwd_f32" in model_lib.calls and "rlhip_gaussian_head_logp_bwd_f32" in model_lib.calls


def test_a_cotangent_nobody_supplied_is_passed_as_null(monkeypatch):
    """SoftGaussianNetwork: a loss on the log-probabilities alone hands dact = NULL to the launch, one on the actions alone dlogp = NULL"""
    import rlhip

    seen = []
    lib = _ModelLibrary()

    def call(name, *a):
        if name == "rlhip_gaussian_head_sample_bwd_f32":
            seen.append((a[12] is not None, a[13] is not None))
        return lib.call(name, *a)

    _patch(monkeypatch, call)
    d, n, K = 3, 4, 2
    mu, raw = H.inputs(d, n, seed=3)
    net = rlhip.SoftGaussianNetwork(mu=lambda s: m, sigma=lambda s: r, min_sigma=LO, max_sigma=HI)
    m, r = _leaf(mu), _leaf(raw)
    a, lp = net.sample(torch.zeros((1, 1, n)), K)
    lp.sum().backward()
    a, lp = net.sample(torch.zeros((1, 1, n)), K)
    a.sum().backward()
    a, lp = net.sample(torch.zeros((1, 1, n)), K)
    (a.sum() + lp.sum()).backward()
    assert seen == [(False, True), (True, False), (True, True)]
