"""The parts of the oracle whose arithmetic the reference delegates to un-vendored packages (Flux Dense /
Zygote backward / Optimisers.Adam / Flux.Losses.huber_loss, removed Zoo PPO & DQN losses) are "parity
unpinned" by the reference; they are cross-checked here against PyTorch fp32 on the CPU."""
import numpy as np
import pytest
import torch

import oracle


def split(p, n_in, h, n_out):
    o = 0
    W1 = p[o:o + h * n_in].reshape(n_in, h).T; o += h * n_in  # noqa: E702  (col-major h x n_in)
    b1 = p[o:o + h]; o += h  # noqa: E702
    W2 = p[o:o + n_out * h].reshape(h, n_out).T; o += n_out * h  # noqa: E702
    b2 = p[o:o + n_out]
    return W1, b1, W2, b2


def torch_mlp(p, n_in, h, n_out, act, x):
    W1, b1, W2, b2 = split(p, n_in, h, n_out)
    hid = W1 @ x + b1[:, None]
    hid = torch.relu(hid) if act == 0 else torch.tanh(hid)
    return W2 @ hid + b2[:, None]


@pytest.mark.parametrize("act", [0, 1])
def test_mlp_forward_backward(act):
    rng = np.random.default_rng(0)
    n_in, h, n_out, B = 4, 32, 3, 50
    p = (rng.standard_normal(oracle.mlp2_nparams(n_in, h, n_out)) * 0.3).astype(np.float32)
    x = rng.standard_normal((n_in, B)).astype(np.float32)
    dout = rng.standard_normal((n_out, B)).astype(np.float32)
    out = oracle.mlp2_forward(p, n_in, h, n_out, act, x)
    pt = torch.tensor(p, requires_grad=True)
    ref = torch_mlp(pt, n_in, h, n_out, act, torch.tensor(x))
    np.testing.assert_allclose(out, ref.detach().numpy(), rtol=1e-5, atol=1e-6)
    (ref * torch.tensor(dout)).sum().backward()
    g = oracle.mlp2_backward(p, n_in, h, n_out, act, x, dout)
    np.testing.assert_allclose(g, pt.grad.numpy(), rtol=1e-4, atol=1e-5)


@pytest.mark.parametrize("continuous", [False, True])
@pytest.mark.parametrize("act", [0, 1])
def test_ppo_loss_and_gradient(continuous, act):
    rng = np.random.default_rng(1)
    ns, na, h, B = (3, 1, 16, 200) if continuous else (4, 3, 16, 200)
    cfg = oracle.ppo_default(hidden=h, act=act, continuous=int(continuous))
    nout = 2 * na if continuous else na
    np_a = oracle.mlp2_nparams(ns, h, nout)
    np_c = oracle.mlp2_nparams(ns, h, 1)
    p = (rng.standard_normal(np_a + np_c) * 0.3).astype(np.float32)
    obs = rng.standard_normal((ns, B)).astype(np.float32)
    adv = rng.standard_normal(B).astype(np.float32)
    ret = rng.standard_normal(B).astype(np.float32)
    logp_old = (rng.standard_normal(B) * 0.3 - 1.0).astype(np.float32)
    if continuous:
        a = rng.standard_normal((1, B)).astype(np.float32)
    else:
        a = rng.integers(0, na, B).astype(np.int32)
    g, losses = oracle.ppo_loss_grad(cfg, ns, na, p, obs, a, logp_old, adv, ret)

    pt = torch.tensor(p, requires_grad=True)
    X = torch.tensor(obs)
    out = torch_mlp(pt[:np_a], ns, h, nout, act, X)
    v = torch_mlp(pt[np_a:], ns, h, 1, act, X)[0]
    lo = torch.clamp(torch.tensor(logp_old), min=float(np.log(1e-8)))
    A, R = torch.tensor(adv), torch.tensor(ret)
    if continuous:
        mu, ls = out[0], out[1]
        sg = torch.exp(ls)
        z = torch.tensor(a[0])
        log2pi = torch.log(torch.tensor(2.0 * np.float32(np.pi)))
        zz = (z - mu) / (sg + 1e-8)
        lp = -(zz ** 2 + log2pi) / 2 - torch.log(sg + 1e-8)
        ent = ((log2pi + 1) + ls).mean() / 2
    else:
        logp = torch.log_softmax(out, dim=0)
        lp = logp[torch.tensor(a, dtype=torch.long), torch.arange(B)]
        ent = -(torch.softmax(out, 0) * logp).sum() / B
    ratio = torch.exp(lp - lo)
    surr1, surr2 = ratio * A, torch.clamp(ratio, 1 - cfg.clip_range, 1 + cfg.clip_range) * A
    actor_loss = -torch.minimum(surr1, surr2).mean()
    critic_loss = ((R - v) ** 2).mean()
    loss = cfg.actor_loss_weight * actor_loss + cfg.critic_loss_weight * critic_loss - cfg.entropy_loss_weight * ent
    loss.backward()
    np.testing.assert_allclose(losses, [loss.item(), actor_loss.item(), critic_loss.item(), ent.item()], rtol=1e-4,
                               atol=1e-6)
    np.testing.assert_allclose(g, pt.grad.numpy(), rtol=2e-3, atol=2e-5 * np.abs(g).max())


def test_dqn_loss_and_gradient():
    rng = np.random.default_rng(2)
    ns, h, na, B = 4, 24, 2, 128
    p = (rng.standard_normal(oracle.mlp2_nparams(ns, h, na)) * 0.4).astype(np.float32)
    pt_ = (p + rng.standard_normal(p.size).astype(np.float32) * 0.1).astype(np.float32)
    s, sn = rng.standard_normal((ns, B)).astype(np.float32), rng.standard_normal((ns, B)).astype(np.float32)
    a = rng.integers(0, na, B).astype(np.int32)
    r = (rng.standard_normal(B) * 2).astype(np.float32)
    t = rng.random(B) < 0.2
    loss, g = oracle.dqn_loss_grad(ns, h, na, 0, p, pt_, s, a, r, t, sn, 0.99, 1.0)
    P = torch.tensor(p, requires_grad=True)
    q = torch_mlp(P, ns, h, na, 0, torch.tensor(s))[torch.tensor(a, dtype=torch.long), torch.arange(B)]
    with torch.no_grad():
        qn = torch_mlp(torch.tensor(pt_), ns, h, na, 0, torch.tensor(sn)).max(0).values
        G = torch.tensor(r) + 0.99 * (1 - torch.tensor(t, dtype=torch.float32)) * qn
    ref = torch.nn.HuberLoss(delta=1.0)(q, G)
    ref.backward()
    assert loss == pytest.approx(ref.item(), rel=1e-5)
    np.testing.assert_allclose(g, P.grad.numpy(), rtol=1e-3, atol=1e-6)


def test_adam_matches_torch():
    rng = np.random.default_rng(3)
    n = 1000
    p0 = rng.standard_normal(n).astype(np.float32)
    po, m, v = p0.copy(), np.zeros(n, np.float32), np.zeros(n, np.float32)
    pt = torch.tensor(p0.copy(), requires_grad=True)
    opt = torch.optim.Adam([pt], lr=1e-3, betas=(0.9, 0.999), eps=1e-8)
    for t in range(1, 11):
        g = rng.standard_normal(n).astype(np.float32)
        oracle.adam(po, g, m, v, 1e-3, 0.9, 0.999, 1e-8, t)
        pt.grad = torch.tensor(g)
        opt.step()
    np.testing.assert_allclose(po, pt.detach().numpy(), rtol=1e-5, atol=1e-6)


def test_huber_and_clip_and_gaussian():
    rng = np.random.default_rng(4)
    q, tg = (rng.standard_normal(333) * 2).astype(np.float32), rng.standard_normal(333).astype(np.float32)
    loss, dq = oracle.huber(q, tg, 1.0)
    Q = torch.tensor(q, requires_grad=True)
    ref = torch.nn.HuberLoss(delta=1.0)(Q, torch.tensor(tg))
    ref.backward()
    assert loss == pytest.approx(ref.item(), rel=1e-6)
    np.testing.assert_allclose(dq, Q.grad.numpy(), rtol=1e-6, atol=1e-9)
    g = rng.standard_normal(777).astype(np.float32)
    g2 = g.copy()
    gn = oracle.clip_by_global_norm(g2, 0.5)
    assert gn == pytest.approx(np.linalg.norm(g.astype(np.float64)), rel=1e-6)
    np.testing.assert_allclose(np.linalg.norm(g2.astype(np.float64)), 0.5, rtol=1e-5)
    G = [torch.tensor(g.copy(), requires_grad=True)]
    G[0].grad = torch.tensor(g.copy())
    torch.nn.utils.clip_grad_norm_(G, 0.5)
    np.testing.assert_allclose(g2, G[0].grad.numpy(), rtol=1e-4)
    assert oracle.normlogpdf(0.3, 1.7, -0.4) == pytest.approx(
        torch.distributions.Normal(0.3, 1.7).log_prob(torch.tensor(-0.4)).item(), rel=1e-5)


def test_gaussian_sampler_statistics_and_permutation():
    z = []
    for i in range(2000):
        w = oracle.philox(11, i, 0, 5, oracle.TAG["NORMAL"])
        import ctypes as C

        a, b = C.c_float(), C.c_float()
        oracle.lib().rlo_normal_pair_f32(C.c_uint32(w[0]), C.c_uint32(w[1]), C.byref(a), C.byref(b))
        z += [a.value, b.value]
    z = np.array(z)
    assert abs(z.mean()) < 0.06 and abs(z.std() - 1) < 0.05
    for n in (1, 2, 7, 64, 1000, 4097):
        p = oracle.permutation(5, 3, n)
        assert np.array_equal(np.sort(p), np.arange(n))
    assert not np.array_equal(oracle.permutation(5, 3, 1000), oracle.permutation(5, 4, 1000))


def test_weighted_dqn_loss_and_is_weights_match_torch():
    """round 4: importance-sampling weights of prioritized replay -- w = 1 / (p + 1e-10)^beta, normalised by the maximum;
    loss = mean(w .* huber(td)) (removed Zoo PrioritizedDQN, parity unpinned): oracle vs PyTorch autograd"""
    rng = np.random.default_rng(7)
    ns, h, na, B = 4, 24, 2, 128
    p = (rng.standard_normal(oracle.mlp2_nparams(ns, h, na)) * 0.4).astype(np.float32)
    pt_ = (p + rng.standard_normal(p.size).astype(np.float32) * 0.1).astype(np.float32)
    s, sn = rng.standard_normal((ns, B)).astype(np.float32), rng.standard_normal((ns, B)).astype(np.float32)
    a = rng.integers(0, na, B).astype(np.int32)
    r = (rng.standard_normal(B) * 2).astype(np.float32)
    t = rng.random(B) < 0.2
    prio = (rng.random(B).astype(np.float32) + 1e-3) ** 0.6
    for beta in (0.4, 1.0):
        w = oracle.per_is_weights(prio, beta)
        wt = 1.0 / (torch.tensor(prio, dtype=torch.float64) + 1e-10) ** beta
        wt = (wt / wt.max()).float()
        np.testing.assert_allclose(w, wt.numpy(), rtol=2e-7, atol=0)
        assert w.max() == 1.0 and (w > 0).all()
        loss, g = oracle.dqn_loss_grad(ns, h, na, 0, p, pt_, s, a, r, t, sn, 0.99, 1.0, weights=w)
        P = torch.tensor(p, requires_grad=True)
        q = torch_mlp(P, ns, h, na, 0, torch.tensor(s))[torch.tensor(a, dtype=torch.long), torch.arange(B)]
        with torch.no_grad():
            qn = torch_mlp(torch.tensor(pt_), ns, h, na, 0, torch.tensor(sn)).max(0).values
            G = torch.tensor(r) + 0.99 * (1 - torch.tensor(t, dtype=torch.float32)) * qn
        ref = (torch.tensor(w) * torch.nn.HuberLoss(delta=1.0, reduction="none")(q, G)).mean()
        ref.backward()
        assert loss == pytest.approx(ref.item(), rel=1e-5)
        np.testing.assert_allclose(g, P.grad.numpy(), rtol=1e-3, atol=1e-6)
    # beta = 0: all weights 1 -> the unweighted loss, bit for bit
    w0 = oracle.per_is_weights(prio, 0.0)
    assert np.array_equal(w0, np.ones(B, np.float32))
    l0, g0 = oracle.dqn_loss_grad(ns, h, na, 0, p, pt_, s, a, r, t, sn, 0.99, 1.0, weights=w0)
    l1, g1 = oracle.dqn_loss_grad(ns, h, na, 0, p, pt_, s, a, r, t, sn, 0.99, 1.0)
    assert l0 == l1 and np.array_equal(g0, g1)


# ------------------------------------------------------------------------------- Float64 autograd, bars from roundings
# The oracle evaluates every sample in Float32 (fmaf chains over the layer inputs, libm tanhf / expf / logf) and accumulates the
# gradient over samples in Float64.  First-order rounding analysis: each Float32 operation of a sample's chain has a relative
# error <= u = 2^-24 of its operands' magnitude (libm: <= 2 u), so a sample's gradient contribution g_b is off by at most
# K u |g_b| c_b, with K the number of roundings along its longest chain (ns + 1 in layer 1, h + 1 in layer 2, and a fixed
# count for the loss head and the backward products) and c_b the amplification of the one cancelling difference in the chain
# (TD error q - G, log-ratio lp - lo, a - mu), i.e. its operands' magnitude over its value.  The Float64 sum over samples and
# the final rounding to Float32 add u |g|.  Hence |g_oracle - g_64| <= K u sum_b c_b |g_b| + u |g| elementwise.
U = 2.0 ** -24


def _split64(p, n_in, h, n_out):
    W1 = p[:h * n_in].reshape(n_in, h).T
    b1 = p[h * n_in:h * n_in + h]
    W2 = p[h * n_in + h:h * n_in + h + n_out * h].reshape(h, n_out).T
    b2 = p[h * n_in + h + n_out * h:]
    return W1, b1, W2, b2


def _mlp64(p, n_in, h, n_out, act, x):
    """one sample: x (n_in,) -> (n_out,)"""
    W1, b1, W2, b2 = _split64(p, n_in, h, n_out)
    z = W1 @ x + b1
    return W2 @ (torch.relu(z) if act == 0 else torch.tanh(z)) + b2


def _assert_within_rounding_bar(g, g64, per_sample_abs, amp, K, tag):
    bar = K * U * (amp[:, None] * per_sample_abs).sum(0) + U * np.abs(g64)
    err = np.abs(g.astype(np.float64) - g64)
    worst = float(np.max(np.where(err > 0, err / np.maximum(bar, 1e-300), 0.0)))
    assert worst <= 1.0, f"{tag}: |g - g64| reaches {worst:.2f} x the rounding bar (K = {K})"
    return worst


@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("ns", [2, 3, 4])
@pytest.mark.parametrize("na", [2, 3])
def test_dqn_loss_and_gradient_float64(ns, na, act):
    from torch.func import grad, vmap

    rng = np.random.default_rng(100 + 10 * ns + na + 7 * act)
    h, B, gamma, delta = 24, 160, 0.99, 1.0
    p = (rng.standard_normal(oracle.mlp2_nparams(ns, h, na)) * 0.4).astype(np.float32)
    pt_ = (p + rng.standard_normal(p.size).astype(np.float32) * 0.1).astype(np.float32)
    s, sn = rng.standard_normal((ns, B)).astype(np.float32), rng.standard_normal((ns, B)).astype(np.float32)
    a = rng.integers(0, na, B).astype(np.int32)
    r = (rng.standard_normal(B) * 1.5).astype(np.float32)
    t = rng.random(B) < 0.2
    loss, g = oracle.dqn_loss_grad(ns, h, na, act, p, pt_, s, a, r, t, sn, gamma, delta)
    P, PT = torch.tensor(p, dtype=torch.float64), torch.tensor(pt_, dtype=torch.float64)
    S, SN = torch.tensor(s.T, dtype=torch.float64), torch.tensor(sn.T, dtype=torch.float64)
    A = torch.tensor(np.eye(na)[a])  # one-hot rows (vmap takes no data-dependent indexing)
    with torch.no_grad():
        qn = vmap(lambda x: _mlp64(PT, ns, h, na, act, x))(SN).max(1).values
        G = torch.tensor(r, dtype=torch.float64) + gamma * (1 - torch.tensor(t, dtype=torch.float64)) * qn
        q = (vmap(lambda x: _mlp64(P, ns, h, na, act, x))(S) * A).sum(1)
    d = (q - G).numpy()
    quad = np.abs(d) < delta
    assert 0.1 <= quad.mean() <= 0.9, f"both Huber branches: {quad.mean():.2f} quadratic"

    def loss_b(pp, x, ab, gb):
        e = (_mlp64(pp, ns, h, na, act, x) * ab).sum() - gb
        return torch.where(e.abs() < delta, 0.5 * e * e, delta * (e.abs() - 0.5 * delta)) / B

    gb = vmap(grad(loss_b), in_dims=(None, 0, 0, 0))(P, S, A, G).numpy()  # (B, np) per-sample gradients
    g64 = gb.sum(0)
    ref = float(vmap(loss_b, in_dims=(None, 0, 0, 0))(P, S, A, G).sum())
    # the TD error cancels in the quadratic branch: its operands' magnitude over its value (the linear branch uses only its sign)
    amp = np.where(quad, 1.0 + (np.abs(q.numpy()) + np.abs(G.numpy())) / np.maximum(np.abs(d), 1e-30), 1.0)
    K = (ns + 1) + (h + 1) + 2 * (ns + 1) + 12  # both forwards' layer 1 feed the same difference; head + backward products
    _assert_within_rounding_bar(g, g64, np.abs(gb), amp, K, f"dqn ns={ns} na={na} act={act}")
    lb = vmap(loss_b, in_dims=(None, 0, 0, 0))(P, S, A, G).numpy()
    assert abs(loss - ref) <= K * U * float((amp * 2 * np.abs(lb)).sum()) + U * abs(ref)


@pytest.mark.parametrize("continuous", [False, True])
@pytest.mark.parametrize("act", [0, 1])
def test_ppo_loss_and_gradient_two_observations_float64(continuous, act):
    """a 2-observation net (MountainCar's shape): discrete with 3 actions, and continuous (mu, log sigma)"""
    from torch.func import grad, vmap

    rng = np.random.default_rng(40 + 2 * act + int(continuous))
    ns, h, B = 2, 16, 200
    na = 1 if continuous else 3
    nout = 2 * na if continuous else na
    cfg = oracle.ppo_default(hidden=h, act=act, continuous=int(continuous))
    np_a, np_c = oracle.mlp2_nparams(ns, h, nout), oracle.mlp2_nparams(ns, h, 1)
    p = (rng.standard_normal(np_a + np_c) * 0.3).astype(np.float32)
    obs = rng.standard_normal((ns, B)).astype(np.float32)
    adv = rng.standard_normal(B).astype(np.float32)
    ret = rng.standard_normal(B).astype(np.float32)
    out = oracle.mlp2_forward(p[:np_a], ns, h, nout, act, obs).astype(np.float64)
    if continuous:
        a = (out[0] + np.exp(out[1]) * (0.25 + np.abs(rng.standard_normal(B))) * rng.choice([-1, 1], B)).astype(np.float32)[None]
    else:
        a = rng.integers(0, na, B).astype(np.int32)
    logp_old = (rng.standard_normal(B) * 0.3 - 1.0).astype(np.float32)
    g, losses = oracle.ppo_loss_grad(cfg, ns, na, p, obs, a, logp_old, adv, ret)
    eps, log2pi = cfg.clip_range, float(np.log(2.0 * np.float32(np.pi)))
    lo_min = float(np.log(1e-8))

    def terms(pp, x, ab, lo, A, R):
        o = _mlp64(pp[:np_a], ns, h, nout, act, x)
        v = _mlp64(pp[np_a:], ns, h, 1, act, x)[0]
        if continuous:
            mu, ls = o[0], o[1]
            sg = torch.exp(ls)
            zz = (ab - mu) / (sg + 1e-8)
            lp = -(zz ** 2 + log2pi) / 2 - torch.log(sg + 1e-8)
            ent = ((log2pi + 1) + ls) / 2
        else:
            logp = torch.log_softmax(o, 0)
            lp = (logp * ab).sum()
            ent = -(torch.softmax(o, 0) * logp).sum()
        ratio = torch.exp(lp - torch.clamp(lo, min=lo_min))
        actor = -torch.minimum(ratio * A, torch.clamp(ratio, 1 - eps, 1 + eps) * A)
        critic = (R - v) ** 2
        total = cfg.actor_loss_weight * actor + cfg.critic_loss_weight * critic - cfg.entropy_loss_weight * ent
        return torch.stack([total, actor, critic, ent]) / B, lp

    P = torch.tensor(p, dtype=torch.float64)
    X = torch.tensor(obs.T, dtype=torch.float64)
    AB = torch.tensor(a[0], dtype=torch.float64) if continuous else torch.tensor(np.eye(na)[a])
    ins = (X, AB, torch.tensor(logp_old, dtype=torch.float64), torch.tensor(adv, dtype=torch.float64),
           torch.tensor(ret, dtype=torch.float64))
    lt, lp = vmap(lambda pp, *z: terms(pp, *z), in_dims=(None, 0, 0, 0, 0, 0))(P, *ins)
    gb = vmap(grad(lambda pp, *z: terms(pp, *z)[0][0]), in_dims=(None, 0, 0, 0, 0, 0))(P, *ins).numpy()
    g64, ref = gb.sum(0), lt.sum(0).numpy()
    lp = lp.numpy()
    ratio = np.exp(lp - logp_old)
    assert ((ratio < 1 - eps) | (ratio > 1 + eps)).mean() >= 0.05 and (adv > 0).any() and (adv < 0).any()
    # cancelling differences: the log-ratio lp - lo (its error is the ratio's relative error), log-softmax's logit - lse,
    # and for the Gaussian head a - mu
    amp = 1.0 + np.abs(lp) + np.abs(logp_old) + np.abs(out).max(0)
    if continuous:
        amp = amp + (np.abs(a[0]) + np.abs(out[0])) / np.abs(a[0] - out[0])
    K = (ns + 1) + (h + 1) + 24  # layer 1, layer 2, head (softmax / Gaussian log-density, exp of the log-ratio, clip, min)
    _assert_within_rounding_bar(g, g64, np.abs(gb), amp, K, f"ppo ns=2 continuous={continuous} act={act}")
    lb = np.abs(lt.numpy())
    assert np.all(np.abs(losses - ref) <= K * U * (amp[:, None] * lb).sum(0) + U * np.abs(ref)), (losses, ref)
