"""Gaussian policy heads on the device (csrc/heads.hip) against the oracle (rlo_heads.c), through the C ABI."""
import json
import os

import numpy as np
import pytest
import torch

import heads_ref as H
import oracle
from conftest import GRAD_ERR_LOG

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rl():
    import rlhip
    return rlhip


def _inputs(d, n, seed=0):
    return H.inputs(d, n, seed)


def _head(rl, mu, raw, soft, squash, lo, hi, seed, base):
    m, s = torch.tensor(mu, device="cuda"), torch.tensor(raw, device="cuda")
    cls = rl.SoftGaussianNetwork if soft else rl.GaussianNetwork
    kw = {} if soft else {"squash": "tanh" if squash else "identity"}
    return cls(pre=None, mu=lambda x: m, sigma=lambda x: s, min_sigma=lo, max_sigma=hi, seed=seed, env_id_base=base, **kw)


class OracleHeads:
    @staticmethod
    def sample(mu, raw, K, lo, hi, family, seed, base, step):
        sq, soft = H.SQUASH_SOFT[family]
        return oracle.gaussian_head_sample(mu, raw, K, lo, hi, sq, soft, seed=seed, env_id_base=base, step=step)

    @staticmethod
    def logp(mu, raw, a, lo, hi, family):
        sq, soft = H.SQUASH_SOFT[family]
        return oracle.gaussian_head_logp(mu, raw, a, lo, hi, sq, soft)


class DeviceHeads:
    """csrc/heads.hip through GaussianNetwork / SoftGaussianNetwork, in the shapes of tests/heads_ref.py"""

    def __init__(self, rl):
        self.rl = rl

    def sample(self, mu, raw, K, lo, hi, family, seed, base, step):
        sq, soft = H.SQUASH_SOFT[family]
        gn = _head(self.rl, mu, raw, soft, sq, lo, hi, seed, base)
        gn.step = step
        a, lp = gn.sample(torch.zeros((1, 1, mu.shape[1]), device="cuda"), K)
        assert gn.step == step + 1
        return a.cpu().numpy(), lp.cpu().numpy()[0]

    def logp(self, mu, raw, a, lo, hi, family):
        sq, soft = H.SQUASH_SOFT[family]
        gn = _head(self.rl, mu, raw, soft, sq, lo, hi, 0, 0)
        return gn.logp(torch.zeros((1, 1, mu.shape[1]), device="cuda"), torch.tensor(a, device="cuda")).cpu().numpy()[0]


O = OracleHeads
BUDGET_LOG = os.path.join(os.path.dirname(GRAD_ERR_LOG), "heads_budget.jsonl")     # beside the gradient margins log of conftest.py


def _log(results):
    """what each check measured (worst error / bar, median budget, left-out share): kept out of git, read into profiles/heads_budget.md"""
    try:
        os.makedirs(os.path.dirname(BUDGET_LOG), exist_ok=True)
        with open(BUDGET_LOG, "a") as f:
            for r in results:
                f.write(json.dumps(r) + "\n")
    except OSError:
        pass
    return results


@pytest.mark.parametrize("d,n,K", H.SHAPES)
@pytest.mark.parametrize("soft,squash", [(0, 0), (0, 1), (1, 1)])
def test_head_matches_oracle(rl, d, n, K, soft, squash):
    """sampling and (model)(state, action) within 2 x the float64 model's budget (tests/heads_ref.py); the comparisons with the
    Float32 oracle that are tight stay: identity actions bit for bit, tanh actions, the non-tanh log-probabilities"""
    family = "soft" if soft else ("tanh" if squash else "identity")
    _log(H.run_shape(DeviceHeads(rl), O, family, d, n, K))
    mu, raw = _inputs(d, n, seed=d)
    lo, hi = H.LO, H.HI
    gn = _head(rl, mu, raw, soft, squash, lo, hi, seed=11, base=5)
    gn.step = 4
    state = torch.zeros((1, 1, n), device="cuda")
    a, lp = gn.sample(state, K)
    assert a.shape == (d, K, n) and lp.shape == (1, K, n) and gn.step == 5
    ao, lpo = oracle.gaussian_head_sample(mu, raw, K, lo, hi, squash, soft, seed=11, env_id_base=5, step=4)
    a, lp = a.cpu().numpy(), lp.cpu().numpy()[0]
    if not squash:
        assert np.array_equal(a, ao)                       # mu + sigma * noise: Float32 arithmetic on the same draws
    else:
        np.testing.assert_allclose(a, ao, rtol=0, atol=2.5e-7)   # tanhf: ocml vs glibc, <= 2 ulp near 1
    err = np.abs(lp - lpo)
    tol = 2e-5 + 2e-6 * np.abs(lpo) * d
    if not (squash and not soft):
        assert (err < tol * 4).all(), err.max()
    # (model)(state, action) on the oracle's actions
    lp2 = gn.logp(state, torch.tensor(ao, device="cuda")).cpu().numpy()[0]
    lp2o = oracle.gaussian_head_logp(mu, raw, ao, lo, hi, squash, soft)
    if not squash:
        assert (np.abs(lp2 - lp2o) < tol * 4).all()


@pytest.mark.parametrize("family", H.FAMILIES)
def test_head_saturating_means_and_pooled_left_out_share(rl, family):
    """mu x 3: tanhf saturates, GaussianNetwork's log(1 - t^2) is the log of an exact 0 and the +Inf pattern must match; and the
    0.5 % cap on the samples an evaluation leaves out, over all shapes together (heads_ref.run_shape on why)"""
    G = DeviceHeads(rl)
    res = []
    for d, n, K in H.SCALED_SHAPES:
        res += H.run_shape(G, O, family, d, n, K, scale=3.0)
    if family == "tanh":
        assert sum(r["non_finite"] for r in res) >= 20
    _log(res)
    ev = []
    for d, n, K in H.SHAPES:
        mu, raw = _inputs(d, n, seed=d)
        ao, _ = O.sample(mu, raw, K, H.LO, H.HI, family, H.SEED, H.BASE, H.STEP)
        ev.append(H.judge_eval(family, mu, raw, H.LO, H.HI, ao, G.logp(mu, raw, ao, H.LO, H.HI, family), 1.0, tag=f"eval {family} {d},{n},{K}"))
    share = H.pooled_left_out(ev)
    _log([{"tag": f"eval {family} pooled over the shapes", "left_out": share, "n": sum(r["n"] for r in ev)}])
    assert share <= (H.EVAL_CAP if family == "tanh" else 0.0)


@pytest.mark.parametrize("family", ["tanh", "soft"])
def test_head_evaluates_the_action_grid(rl, family):
    """|a| = 1 - 2^-e (e <= 12 GaussianNetwork tanh, e <= 23 SoftGaussianNetwork): nothing left out, everything within the bar"""
    assert _log([H.run_grid(DeviceHeads(rl), family)])[0]["left_out"] == 0


@pytest.mark.parametrize("name", sorted(H.edge_cases()))
@pytest.mark.parametrize("family", H.FAMILIES)
def test_head_saturation_and_sigma_edges(rl, family, name):
    """mu = +-12 at sigma = 0.05 (actions exactly +-1; +Inf for GaussianNetwork tanh, finite for SoftGaussianNetwork, the model's
    NaN at a = +-1); raw sigma around both clamp limits, min == max, NaN (passes the clamp), sigma = 0 (s = 1e-8: finite at
    d = 1, prod underflows at d = 3), prod in the Float32 subnormal range (a kernel that flushed it would answer +Inf)"""
    _log(H.run_edge(DeviceHeads(rl), O, family, name, H.edge_cases()[name]))


def test_tanhf_in_the_open(rl):
    """min_sigma = max_sigma = 0: the action is tanhf(mu).  +-0, subnormals, 2^-126 ... 2^4, the neighbours of the saturation
    point, +-Inf, NaN: within E_tanh ulps of float64, odd, |t| <= 1, NaN -> NaN"""
    x = H.tanh_sweep()[None, :]
    a, _ = DeviceHeads(rl).sample(x, np.ones_like(x), 1, 0.0, 0.0, "tanh", 1, 0, 0)
    worst = H.check_tanh_sweep(x[0], a[0, 0])
    _log([{"tag": "tanhf sweep", "tanh_ulps": worst, "n": int(x.size)}])
    a2, _ = DeviceHeads(rl).sample(x, np.ones_like(x), 1, 0.0, 0.0, "soft", 1, 0, 0)
    assert np.array_equal(a2, a, equal_nan=True)


@pytest.mark.parametrize("base,step,n", [(0xFFFFFFF0, 4, 64), (5, 2 ** 32 - 1, 64), (0xFFFFFFF0, 2 ** 32 - 1, 33)])
def test_head_counters_wrap_like_the_oracle(rl, base, step, n):
    """env_id_base + i wraps in uint32; step = 2^32 - 1: identity mode bit for bit"""
    d, K = 3, 3
    mu, raw = _inputs(d, n, seed=9)
    a, lp = DeviceHeads(rl).sample(mu, raw, K, H.LO, H.HI, "identity", 11, base, step)
    ao, _ = O.sample(mu, raw, K, H.LO, H.HI, "identity", 11, base, step)
    assert np.array_equal(a, ao)
    H.judge_sampling("identity", mu, raw, H.LO, H.HI, ao, a, lp, tag="counters")
    if base > 5:      # the states past the wrap are envs 0 ... of the same stream
        a0, _ = O.sample(mu[:, 16:], raw[:, 16:], K, H.LO, H.HI, "identity", 11, 0, step)
        assert np.array_equal(a[:, :, 16:], a0)


@pytest.mark.parametrize("family", H.FAMILIES)
def test_head_actions_do_not_depend_on_logp_out_and_n0_launches_nothing(rl, family):
    from rlhip._lib import call
    from rlhip.ops import ptr, stream_ptr

    d, n, K = 5, 33, 3
    sq, soft = H.SQUASH_SOFT[family]
    mu, raw = _inputs(d, n, seed=4)
    gn = _head(rl, mu, raw, soft, sq, H.LO, H.HI, seed=11, base=5)
    m, s = torch.tensor(mu, device="cuda"), torch.tensor(raw, device="cuda")
    gn.step = 4
    a_only, none = gn._sample(m, s, K, False)
    gn.step = 4
    a_both, lp = gn._sample(m, s, K, True)
    assert none is None and lp is not None and torch.equal(a_only, a_both)
    state = torch.zeros((1, n), device="cuda")
    gn.step = 4
    only = gn(state, is_sampling=True)
    gn.step = 4
    both, _ = gn(state, is_sampling=True, is_return_log_prob=True)
    assert torch.equal(only, both)
    # n = 0: status OK and no launch -- the output buffers keep their contents
    act = torch.full((K * d,), 7.0, device="cuda")
    out = torch.full((K,), 7.0, device="cuda")
    ms, ss = m.t().contiguous(), s.t().contiguous()
    call("rlhip_gaussian_head_sample_f32", ptr(ms), ptr(ss), d, 0, K, H.LO, H.HI, sq, soft, 11, 5, 4, ptr(act), ptr(out), stream_ptr())
    call("rlhip_gaussian_head_logp_f32", ptr(ms), ptr(ss), ptr(act), d, 0, K, H.LO, H.HI, sq, soft, ptr(out), stream_ptr())
    torch.cuda.synchronize()
    assert (act == 7).all() and (out == 7).all()


def test_reference_test_properties_and_call_forms(rl):
    """RLCore/test/utils/networks.jl:57-72 on the device head: shapes, logp ≈ diagnormlogpdf(m, L, a), logp ≈ gn(state, a)"""
    from rlhip import ops

    d, n = 10, 3
    mu, raw = _inputs(d, n, seed=3)
    gn = _head(rl, mu, raw, 0, 0, 0.0, float("inf"), seed=1, base=0)
    state = torch.zeros((20, n), device="cuda")
    m, L = gn(state)
    assert m.shape == L.shape == (d, n)
    a, logp = gn(state, is_sampling=True, is_return_log_prob=True)
    assert a.shape == (d, n) and logp.shape == (1, n)
    ref = ops.diagnormlogpdf(m.t().contiguous(), L.t().contiguous(), a.t().contiguous())
    assert torch.equal(logp[0], ref)
    assert torch.equal(logp, gn(state, a))
    only_a = gn(state, is_sampling=True)
    assert only_a.shape == (d, n) and not torch.equal(only_a, a)          # the step counter advanced
    acts, logps = gn.sample(state.unsqueeze(1), 5)
    assert acts.shape == (d, 5, n) and logps.shape == (1, 5, n)
    assert torch.equal(gn.logp(state.unsqueeze(1), acts), logps)
    with pytest.raises(ValueError):
        rl.GaussianNetwork(squash="sigmoid")
    with pytest.raises(rl.RLHipError):
        _head(rl, *_inputs(65, 2), 0, 0, 0.0, 1.0, 0, 0).sample(torch.zeros((1, 1, 2), device="cuda"), 1)


def test_head_throughput_is_streaming(rl):
    """2^20 states x d = 8: one launch, timed with HIP events (sanity bound only: > 0.5 TB/s of algorithmic traffic)"""
    d, n = 8, 1 << 20
    m = torch.randn((n, d), device="cuda")
    s = torch.rand((n, d), device="cuda") + 0.1
    gn = rl.GaussianNetwork(mu=lambda x: m.t(), sigma=lambda x: s.t(), squash="tanh")
    st = torch.zeros((1, 1, n), device="cuda")
    for _ in range(3):
        gn.sample(st, 1)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(10):
        gn.sample(st, 1)
    e1.record()
    torch.cuda.synchronize()
    us = e0.elapsed_time(e1) * 100
    byts = n * (3 * d + 1) * 4
    print(f"gaussian head d={d} n={n}: {us:.1f} us per call (incl. two transposes), {byts / us / 1e3:.1f} GB/s")
    assert byts / us / 1e3 > 100


def test_categorical_network_call_forms(rl):
    """CategoricalNetwork (networks.jl:405-432, masked :459-472): logits, one-hot Gumbel-max sample, (z, logits), mask"""
    na, n = 5, 2000
    lg = torch.randn((na, n), device="cuda")
    net = rl.CategoricalNetwork(lambda s: lg, seed=3, env_id_base=7)
    state = torch.zeros((4, n), device="cuda")
    assert torch.equal(net(state), lg)
    z, logits = net(state, is_sampling=True, is_return_log_prob=True)
    assert z.shape == (na, n) and torch.equal(logits, lg) and torch.equal(z.sum(0), torch.ones(n, device="cuda"))
    a_ref, _ = oracle.categorical_sample(lg.cpu().numpy(), seed=3, step=0, env_id_base=7)
    assert np.array_equal(net.actions.cpu().numpy(), a_ref) and np.array_equal(z.argmax(0).cpu().numpy(), a_ref)
    # empirical frequencies follow softmax(logits) on a constant-logit batch
    lg2 = torch.tensor([0.0, 1.0, 2.0, -1.0, 0.5], device="cuda").unsqueeze(1).expand(na, 20000).contiguous()
    net2 = rl.CategoricalNetwork(lambda s: lg2, seed=4)
    freq = net2(torch.zeros((1, 20000), device="cuda"), is_sampling=True).mean(1)
    np.testing.assert_allclose(freq.cpu().numpy(), torch.softmax(lg2[:, 0], 0).cpu().numpy(), atol=0.015)
    # masked: -Inf logits, never sampled
    mask = torch.ones((na, n), dtype=torch.bool, device="cuda")
    mask[1] = False
    mask[3, ::2] = False
    zm, lm = net(state, mask, is_sampling=True, is_return_log_prob=True)
    assert torch.isinf(lm[1]).all() and (zm[1] == 0).all() and (zm[3, ::2] == 0).all()
    assert torch.equal(net(state, mask)[0], lg[0])


def test_kernels_match_the_frozen_oracle_pins(rl):
    """tests/golden/oracle_pins/pins.json (frozen oracle outputs for the parts without a reference KAT): the Acrobot env
    kernel and the Gaussian head kernel reproduce them from the same seeds"""
    import json
    import os

    pins = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "oracle_pins", "pins.json")))

    def unhx(xs, dtype):
        return np.array([float.fromhex(x) for x in xs], np.float64).astype(dtype)

    for case in pins["acrobot"]:
        dt, T = (np.float64, torch.float64) if case["dtype"] == "f64" else (np.float32, torch.float32)
        kw = dict(case["kw"])
        if "nips" in kw:
            kw = {"book_or_nips": "nips"}
        env = rl.AcrobotRK4Env(6, T=T, seed=21, env_id_base=3, **kw)
        for a, want in zip(case["actions"], case["steps"]):
            env.act0_(torch.tensor(a, dtype=torch.int32, device="cuda"))
            for k in range(4):
                np.testing.assert_allclose(env.raw_state()[k].cpu().numpy(), unhx(want["s"][k], dt),
                                           rtol=1e-12 if dt == np.float64 else 1e-6, atol=0)
            assert env.is_terminated().cpu().numpy().astype(int).tolist() == want["done"]
            assert np.array_equal(env.reward().cpu().numpy(), unhx(want["reward"], dt))
    h = pins["heads"]
    d, n = h["shape"]
    mu, raw = unhx(h["mu"], np.float32).reshape(d, n), unhx(h["raw_sigma"], np.float32).reshape(d, n)
    for c in h["cases"]:
        gn = _head(rl, mu, raw, c["soft"], c["squash"], 0.2, 1.5, seed=9, base=1)
        gn.step = 4
        a, lp = gn.sample(torch.zeros((1, 1, n), device="cuda"), 2)
        np.testing.assert_allclose(a.cpu().numpy().ravel(), unhx(c["action"], np.float32), rtol=3e-7, atol=0)
        np.testing.assert_allclose(lp.cpu().numpy().ravel(), unhx(c["logp"], np.float32), rtol=2e-5, atol=2e-5)
