"""Every reachable instantiation of the two-layer Float32 learner kernels (tests/f32_learner_matrix.py) against the oracle.

One case per row of the table, the row's id in the test id.  The comparisons are against oracle/ (double accumulation,
the reference's expression order), never GPU against GPU -- except the rollout rows, which compare the fused rollout with the
per-step protocol bit for bit: that protocol's plan! kernel is the plan_wide / plan_scalar kernel of the same (NS, H, ACT),
pinned to the oracle by the ppo_plan rows, and its env step and pushes are pinned by tests/test_gpu_parity.py.  That chain
shares policy_noise, policy_select, env_step1 and env_reset1 between its two ends; every step of every rollout row against
the oracle itself is tests/test_gpu_rollout_audit.py.

The inputs are chosen so that an error is visible, and each case asserts it (the measured fractions are in the message):
tanh nets have at least half the hidden pre-activations in |z| < 2 (tanh' not ~ 0), relu nets 10 % .. 90 % active units;
PPO micro-batches have >= 5 % of the ratios below 1 - eps and >= 5 % above 1 + eps and advantages of both signs; DQN
batches have >= 10 % of the samples in each Huber branch and 5 % .. 40 % terminal transitions.
"""
import ctypes as C
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import f32_learner_matrix as M  # noqa: E402
import oracle  # noqa: E402
from conftest import F32_GRAD_TOL, assert_grad_close  # noqa: E402

KIND = {"cartpole": 0, "pendulum": 1, "mountaincar": 2}
GAMMA, DELTA = 0.99, 1.0


@pytest.fixture(scope="module")
def rl():
    import rlhip

    oracle.use_all_cores(True)  # the NT = 2 rows: micro-batches of > 16 384 samples
    yield rlhip
    oracle.use_all_cores(False)


def dev(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).cuda()


def host(t):
    return t.detach().cpu().numpy()


def ids(rows):
    return [r["id"] for r in rows]


# ------------------------------------------------------------------------------------------------------------ helpers
def perturbed_net(ns, h, nout, seed, net_id, rng, scale=0.05):
    return (oracle.mlp2_init(ns, h, nout, seed, net_id) + rng.standard_normal(oracle.mlp2_nparams(ns, h, nout)) * scale
            ).astype(np.float32)


def split(g, ns, h, nout):
    """flat 2-layer parameter vector -> (W1, b1, W2, b2) in the packing order of mlp2_nparams"""
    sizes = {"W1": h * ns, "b1": h, "W2": nout * h, "b2": nout}
    out, o = {}, 0
    for k, s in sizes.items():
        out[k] = g[o:o + s]
        o += s
    assert o == g.size
    return out


def assert_per_tensor(g, o, nets, tag):
    """nets: [(name, ns, h, nout)] in the order they sit in the flat vector.  One bar per tensor: a wrong third actor output
    moves only its own W2 row and b2 entry, which one max over all parameters would hide."""
    off = 0
    for name, ns, h, nout in nets:
        np_ = oracle.mlp2_nparams(ns, h, nout)
        gs, os_ = split(g[off:off + np_], ns, h, nout), split(o[off:off + np_], ns, h, nout)
        for k in gs:
            assert_grad_close(gs[k], os_[k], F32_GRAD_TOL, f"{tag} {name}.{k}")
        off += np_
    assert off == g.size


def assert_visible_net(p, ns, h, act, x, tag):
    """hidden pre-activations of a net on its inputs x (ns, B): tanh' not ~ 0 / relu neither dead nor linear"""
    W1 = p[:h * ns].reshape(ns, h).T.astype(np.float64)
    b1 = p[h * ns:h * ns + h].astype(np.float64)
    z = W1 @ np.asarray(x, np.float64) + b1[:, None]
    if act == 1:
        f = float((np.abs(z) < 2).mean())
        assert f >= 0.5, f"{tag}: only {f:.3f} of the tanh pre-activations have |z| < 2"
    else:
        f = float((z > 0).mean())
        assert 0.1 <= f <= 0.9, f"{tag}: {f:.3f} of the relu units are active (want 0.1 .. 0.9)"


def assert_visible_dqn(p, tp, ns, h, na, act, s, a, r, t, sn, tag):
    assert_visible_net(p, ns, h, act, s, tag)
    q = oracle.mlp2_forward(p, ns, h, na, act, s)[a, np.arange(a.size)].astype(np.float64)
    qn = oracle.mlp2_forward(tp, ns, h, na, act, sn).max(0).astype(np.float64)
    td = np.abs(q - (r + GAMMA * (1.0 - t) * qn))
    quad, term = float((td <= DELTA).mean()), float(np.asarray(t, bool).mean())
    assert 0.1 <= quad <= 0.9, f"{tag}: {quad:.3f} of the samples in the quadratic Huber branch (want 0.1 .. 0.9)"
    assert 0.05 <= term <= 0.4, f"{tag}: {term:.3f} of the samples terminal (want 0.05 .. 0.4)"


def obs_scale(env):
    # observations of the order the env produces (MountainCar: position ~ -0.5 +- 0.7, velocity ~ 0.07)
    return {"cartpole": np.array([1.0, 1.0, 0.2, 1.0]), "pendulum": np.array([1.0, 1.0, 3.0]),
            "mountaincar": np.array([0.7, 0.07])}[env]


# ------------------------------------------------------------------------------------------- PPO gradient and losses
def _oracle_microbatch(pol, tr, epoch_ctr, mb):
    n, T = tr.n, tr.T
    total = n * T
    bm = total // pol.cfg.n_microbatches
    perm = np.array([oracle.permute(pol.seed, epoch_ctr, total, mb * bm + b) for b in range(bm)])
    t, i = perm // n, perm % n
    obs = host(tr.obs)[t, :, i].T.copy()  # (ns, bm)
    flat = lambda x: host(x).reshape(-1)[perm]  # noqa: E731
    act = host(tr.action_f)[t, 0, i] if tr.continuous else host(tr.action_i).reshape(-1)[perm]
    return obs, act, flat(tr.logp), flat(tr.adv), flat(tr.ret), perm


def _logp(out, a, continuous):
    out = out.astype(np.float64)
    if continuous:
        mu, sg = out[0], np.exp(out[1])
        z = (a - mu) / (sg + 1e-8)
        return -(z * z + np.log(2 * np.pi)) / 2 - np.log(sg + 1e-8)
    m = out.max(0)
    lse = m + np.log(np.exp(out - m).sum(0))
    return out[a, np.arange(a.size)] - lse


@pytest.mark.parametrize("row", M.PPO_GRAD, ids=ids(M.PPO_GRAD))
def test_ppo_gradient_and_losses_vs_oracle(rl, row):
    """rlhip_ppo_grad_f32 on one micro-batch of a trajectory written from a seeded generator, against oracle.ppo_loss_grad
    on the GPU's own permuted micro-batch: every tensor of actor and critic under F32_GRAD_TOL, the four loss terms."""
    env_name, cont, h, act = row["env"], row["continuous"], row["hidden"], row["act"]
    n, T, nmb = row["n"], row["T"], row["n_microbatches"]
    rng = np.random.default_rng(zlib.crc32(row["id"].encode()))
    env = rl.HipVecEnv(env_name, n, seed=7, continuous=cont)
    pol = rl.PPOPolicy(env, update_freq=T, hidden=h, act=act, n_microbatches=nmb)
    ocfg = oracle.ppo_default(continuous=int(cont), hidden=h, act=act, n_microbatches=nmb)
    ns, na, nout = env.odim, pol.na, M.ppo_nout(env_name, cont)
    assert na == M.ppo_na(env_name, cont) and pol.np == oracle.ppo_nparams(env.kind, ocfg)
    pa, pc = perturbed_net(ns, h, nout, 7, 0, rng), perturbed_net(ns, h, 1, 7, 1, rng)
    p = np.concatenate([pa, pc])
    pol.params.copy_(dev(p))
    # the trajectory: observations, actions, logp_old = logp + N(0, 0.4) (ratios on both sides of the clip range), advantages
    # of both signs, returns off zero.  Actions and advantages lean one way (80 % on action 0 / above the mean, ~7 % of the
    # advantages negative) so that the per-tensor sums over the micro-batch do not cancel down to their rounding noise.
    obs = (rng.standard_normal((T + 1, ns, n)) * obs_scale(env_name)[None, :, None]).astype(np.float32)
    x = obs[:T].transpose(1, 0, 2).reshape(ns, T * n)
    out = oracle.mlp2_forward(pa, ns, h, nout, act, x)
    if cont:
        # |z| >= 0.25: an action within a few ulps of mu would turn the last-bit difference of mu (summation order) into an
        # O(1) relative difference of a - mu, a property of the input and not of the kernel
        z = (0.25 + np.abs(rng.standard_normal(T * n))) * np.where(rng.random(T * n) < 0.8, 1.0, -1.0)
        a = (out[0] + np.exp(out[1]) * z).astype(np.float32)
    else:
        a = np.where(rng.random(T * n) < 0.8, 0, rng.integers(1, na, T * n)).astype(np.int32)
    lp = _logp(out, a, cont)
    lo = (lp + rng.standard_normal(T * n) * 0.4).astype(np.float32)
    tr = pol.trajectory
    tr.obs.copy_(dev(obs))
    tr.logp.copy_(dev(lo.reshape(T, n)))
    tr.adv.copy_(dev((rng.standard_normal((T, n)) + 1.5).astype(np.float32)))
    tr.ret.copy_(dev((rng.standard_normal((T, n)) * 2 + 1).astype(np.float32)))
    if cont:
        tr.action_f.copy_(dev(a.reshape(T, 1, n)))
    else:
        tr.action_i.copy_(dev(a.reshape(T, n)))
    epoch_ctr, mb = 2, nmb - 1
    pol.grad_(epoch_ctr, mb)
    mobs, ma, mlp, madv, mret, perm = _oracle_microbatch(pol, tr, epoch_ctr, mb)
    bm = perm.size
    assert (bm > 256 * 64) == row["inst"].endswith(", 2>"), f"micro-batch of {bm} samples does not select {row['inst']}"
    tag = f"{row['id']} (h={h}, bm={bm})"
    assert_visible_net(pa, ns, h, act, mobs, tag + " actor")
    assert_visible_net(pc, ns, h, act, mobs, tag + " critic")
    ratio = np.exp(lp[perm] - mlp)
    eps = ocfg.clip_range
    below, above = float((ratio < 1 - eps).mean()), float((ratio > 1 + eps).mean())
    assert below >= 0.05 and above >= 0.05, f"{tag}: ratios below / above the clip range: {below:.3f} / {above:.3f}"
    assert (madv > 0).any() and (madv < 0).any()
    g, losses = oracle.ppo_loss_grad(ocfg, ns, na, p, mobs, ma, mlp, madv, mret)
    assert_per_tensor(host(pol.grad), g, [("actor", ns, h, nout), ("critic", ns, h, 1)], tag)
    np.testing.assert_allclose(host(pol.losses), losses, rtol=1e-4, atol=1e-6)


# ------------------------------------------------------------------------------------------------------- DQN gradient
def _ring(rl, ns, na, n_env=64, capacity=9, seed=0):
    """the same transitions pushed into a GPU record ring and an oracle.Ring"""
    from rlhip.trajectory import CircularArraySARTSTraces

    rng = np.random.default_rng(seed)
    tr = CircularArraySARTSTraces(capacity=capacity, n_env=n_env, obs_dim=ns)
    ref = oracle.Ring(capacity, n_env, ns)
    o = rng.standard_normal((ns, n_env)).astype(np.float32)
    tr.push_state_(dev(o))
    ref.push_state(o)
    for _ in range(capacity + 3):
        o = rng.standard_normal((ns, n_env)).astype(np.float32)
        a = rng.integers(0, na, n_env).astype(np.int32)
        r = (rng.standard_normal(n_env) * 1.5).astype(np.float32)
        t = (rng.random(n_env) < 0.2).astype(np.uint8)
        tr.push_transition_(dev(o), dev(a), dev(r), dev(t))
        ref.push_transition(o, a, r, t)
    return tr, ref


def _dqn_nets(ns, h, na, rng):
    p = (oracle.mlp2_init(ns, h, na, 5, 0) + rng.standard_normal(oracle.mlp2_nparams(ns, h, na)) * 0.1).astype(np.float32)
    pt = (p + rng.standard_normal(p.size) * 0.05).astype(np.float32)
    return p, pt


@pytest.mark.parametrize("row", M.DQN_GRAD, ids=ids(M.DQN_GRAD))
def test_dqn_gradient_vs_oracle(rl, row):
    """FUSE = false: rlhip_dqn_grad_f32.  FUSE = true: rlhip_dqn_update_f32 with <= 32 tiles and clipping off.  The fused tail
    (dqn_fused_tail) computes scale = 1 when clip_norm = 0 and writes grad[i] = (sum of the partial rows) * grad_scale before
    Adam reads it -- with grad_scale = 1 the plain batch-mean gradient, the quantity rlhip_dqn_grad_f32 returns -- and the loss
    line of dqn_reduce_kernel.  Both are compared with oracle.dqn_loss_grad on the parameters before the step, per tensor."""
    from rlhip import dqn

    ns, h, na, act, batch = M.ENVS[row["env"]], row["hidden"], row["n_actions"], row["act"], row["batch"]
    assert (h <= 128) == (row["upl"] == 2)
    rng = np.random.default_rng(zlib.crc32(row["id"].encode()))
    tr, ref = _ring(rl, ns, na, seed=int(rng.integers(1 << 30)))
    p, pt = _dqn_nets(ns, h, na, rng)
    seed, draw = 11, 4
    if row["fuse"]:
        np_ = p.size
        assert (batch + 63) // 64 <= 32 and np_ <= 4096, "the fused launch is not reached"
        P = dev(p)
        m, v = torch.zeros_like(P), torch.zeros_like(P)
        bp = torch.tensor([0.9, 0.999], device="cuda")
        g, loss = torch.empty_like(P), torch.empty(1, device="cuda")
        ws = dqn.dqn_workspace(ns, h, na, batch)
        dqn.dqn_update(tr, h, na, act, P, dev(pt), batch, GAMMA, DELTA, seed, draw, ws, g, loss, m, v, bp, 1.0, 0.0, 1e-3,
                       0.9, 0.999, 1e-8)
        assert not torch.equal(P, dev(p)), "the fused update did not step"
    else:
        g, loss = dqn.dqn_grad(tr, h, na, act, dev(p), dev(pt), batch, GAMMA, DELTA, seed=seed, draw_ctr=draw)
    idx = ref.sample_indices(batch, seed, draw)
    s, a, r, t, sn = ref.gather(idx)
    tag = f"{row['id']} (h={h}, na={na}, batch={batch})"
    assert_visible_dqn(p, pt, ns, h, na, act, s, a, r, t, sn, tag)
    ol, og = oracle.dqn_loss_grad(ns, h, na, act, p, pt, s, a, r, t, sn, GAMMA, DELTA)
    assert float(loss) == pytest.approx(ol, rel=1e-4)
    assert_per_tensor(host(g), og, [("q", ns, h, na)], tag)


@pytest.mark.parametrize("row", [r for r in M.EXTRA if r["kernel"] == "dqn_grad_kernel"],
                         ids=ids([r for r in M.EXTRA if r["kernel"] == "dqn_grad_kernel"]))
def test_dqn_gradient_on_explicit_indices_vs_oracle(rl, row):
    """the run-time branches off the default path at an NS != 4 tanh net: explicit (prioritized) indices, the TD errors they
    return (td_out) and, with per_beta, importance-sampling weights (isw)"""
    from rlhip import dqn
    from rlhip._lib import call
    from rlhip.ops import ptr, stream_ptr

    ns, h, na, act, batch = M.ENVS[row["env"]], row["hidden"], row["n_actions"], row["act"], row["batch"]
    rng = np.random.default_rng(zlib.crc32(row["id"].encode()))
    tr, ref = _ring(rl, ns, na, seed=3)
    p, pt = _dqn_nets(ns, h, na, rng)
    idx = rng.integers(0, len(ref) * 64, batch).astype(np.int64)  # with repeats, in no order
    w = None
    if "per_beta" in row:
        prio = ((rng.random(batch) + 1e-3) ** 0.6).astype(np.float32)
        w = oracle.per_is_weights(prio, row["per_beta"])
        assert w.min() < 0.5 * w.max()
    ws = dqn.dqn_workspace(ns, h, na, batch)
    P, PT, I = dev(p), dev(pt), dev(idx)
    g, loss, td = torch.empty_like(P), torch.empty(1, device="cuda"), torch.zeros(batch, device="cuda")
    if w is None:
        call("rlhip_dqn_grad_idx_f32", C.byref(tr.rb), h, na, act, ptr(P), ptr(PT), batch, ptr(I), GAMMA, DELTA, ptr(ws),
             ptr(g), ptr(loss), ptr(td), stream_ptr())
    else:
        W = dev(w)
        call("rlhip_dqn_grad_idx_w_f32", C.byref(tr.rb), h, na, act, ptr(P), ptr(PT), batch, ptr(I), ptr(W), GAMMA, DELTA,
             ptr(ws), ptr(g), ptr(loss), ptr(td), stream_ptr())
    s, a, r, t, sn = ref.gather(idx)
    tag = f"{row['id']} (h={h}, na={na}, batch={batch})"
    assert_visible_dqn(p, pt, ns, h, na, act, s, a, r, t, sn, tag)
    ol, og = oracle.dqn_loss_grad(ns, h, na, act, p, pt, s, a, r, t, sn, GAMMA, DELTA, weights=w)
    assert float(loss) == pytest.approx(ol, rel=1e-4)
    assert_per_tensor(host(g), og, [("q", ns, h, na)], tag)
    q = oracle.mlp2_forward(p, ns, h, na, act, s)[a, np.arange(batch)]
    y = oracle.td_target(oracle.mlp2_forward(pt, ns, h, na, act, sn), r, t, GAMMA)
    np.testing.assert_allclose(host(td), np.abs(q - y), rtol=1e-5, atol=1e-6)


# -------------------------------------------------------------------------------------------------------------- plans
@pytest.mark.parametrize("row", M.PPO_PLAN, ids=ids(M.PPO_PLAN))
def test_ppo_plan_vs_oracle(rl, row):
    """rlhip_ppo_plan_f32: value within the plan bar of oracle.mlp2_forward; a discrete head samples the oracle's actions
    (Gumbel-max on the same Philox draws; > 99.9 % agree, the rest are near ties) with the same log-probabilities, a Gaussian
    head returns the log-density of its own action under the oracle's (mu, sigma)."""
    from rlhip._lib import call
    from rlhip.ops import ptr, stream_ptr
    from rlhip.ppo import make_ppo_cfg

    env, cont, h, act, n = row["env"], row["continuous"], row["hidden"], row["act"], row["n"]
    ns, na, nout = M.ENVS[env], M.ppo_na(env, cont), M.ppo_nout(env, cont)
    rng = np.random.default_rng(zlib.crc32(row["id"].encode()))
    cfg = make_ppo_cfg(continuous=int(cont), hidden=h, act=act)
    pa, pc = perturbed_net(ns, h, nout, 3, 0, rng), perturbed_net(ns, h, 1, 3, 1, rng)
    assert pa.size + pc.size == int(rl._lib.lib.rlhip_ppo_nparams(KIND[env], C.byref(cfg)))
    obs = (rng.standard_normal((ns, n)) * obs_scale(env)[:, None]).astype(np.float32)
    assert_visible_net(pa, ns, h, act, obs, row["id"] + " actor")
    P, O = dev(np.concatenate([pa, pc])), dev(obs)
    ai, af = torch.zeros(n, dtype=torch.int32, device="cuda"), torch.zeros(n, device="cuda")
    logp, value = torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    seed, base, step = 21, 5, 9
    call("rlhip_ppo_plan_f32", KIND[env], C.byref(cfg), ptr(P), ptr(O), n, seed, base, step, ptr(ai), ptr(af), ptr(logp),
         ptr(value), stream_ptr())
    out = oracle.mlp2_forward(pa, ns, h, nout, act, obs)
    val = oracle.mlp2_forward(pc, ns, h, 1, act, obs)[0]
    np.testing.assert_allclose(host(value), val, rtol=2e-5, atol=2e-6)
    if cont:
        a = host(af)
        np.testing.assert_allclose(host(logp), _logp(out, a, True), rtol=1e-4, atol=1e-5)
        noise = (a - out[0]) / np.exp(out[1])
        assert abs(noise.mean()) < 0.1 and abs(noise.std() - 1) < 0.1
    else:
        oa, olp = oracle.categorical_sample(out, seed=seed, step=step, env_id_base=base)
        same = host(ai) == oa
        assert same.mean() > 0.999, f"only {same.mean():.5f} of the sampled actions agree"
        np.testing.assert_allclose(host(logp)[same], olp[same], rtol=2e-5, atol=2e-6)


def _dqn_plan_case(rl, row):
    from rlhip.dqn import dqn_plan

    env, h, na, act, n = row["env"], row["hidden"], row["n_actions"], row["act"], row["n"]
    ns = M.ENVS[env]
    rng = np.random.default_rng(zlib.crc32(row["id"].encode()))
    p = perturbed_net(ns, h, na, 5, 0, rng, 0.1)
    obs = (rng.standard_normal((ns, n)) * obs_scale(env)[:, None]).astype(np.float32)
    assert_visible_net(p, ns, h, act, obs, row["id"])
    oq = oracle.mlp2_forward(p, ns, h, na, act, obs)
    for eps in (0.0, 0.3):
        a, q = dqn_plan(dev(p), ns, h, na, act, dev(obs), eps, seed=8, env_id_base=100, step=42)
        np.testing.assert_allclose(host(q), oq, rtol=2e-5, atol=2e-6)
        # the selection is bit-exact given the GPU's Q-values and the same Philox draws
        assert np.array_equal(host(a), oracle.eps_greedy_select(host(q), eps, seed=8, step=42, env_id_base=100))


@pytest.mark.parametrize("row", M.DQN_PLAN, ids=ids(M.DQN_PLAN))
def test_dqn_plan_vs_oracle(rl, row):
    _dqn_plan_case(rl, row)


@pytest.mark.parametrize("row", [r for r in M.EXTRA if r["kernel"] == "dqn_plan_scalar_kernel"],
                         ids=ids([r for r in M.EXTRA if r["kernel"] == "dqn_plan_scalar_kernel"]))
def test_dqn_plan_beyond_the_wide_limit_vs_oracle(rl, row):
    """h = 128 but n * 16 > 2^22: the scalar kernel by size"""
    assert row["n"] * 16 > 1 << 22 and row["hidden"] in M.WIDE_L
    _dqn_plan_case(rl, row)


# ------------------------------------------------------------------------------------------------------------ rollout
@pytest.mark.parametrize("row", M.ROLLOUT, ids=ids(M.ROLLOUT))
def test_rollout_equals_stepwise_bit_exact(rl, row):
    """rlhip_ppo_rollout_f32 (the rollout_split / rollout_scalar instantiation of the row) against the per-step protocol
    (plan! -> push! -> act! -> push!, then GAE) on the same perturbed parameters: every trace, the env state and the counters bit
    for bit over two update periods."""
    env_name, cont, h, act, n, T = row["env"], row["continuous"], row["hidden"], row["act"], row["n"], row["T"]
    ns, nout = M.ENVS[env_name], M.ppo_nout(env_name, cont)
    rng = np.random.default_rng(zlib.crc32(row["id"].encode()))
    p = np.concatenate([perturbed_net(ns, h, nout, 3, 0, rng), perturbed_net(ns, h, 1, 3, 1, rng)])
    sides = []
    for _ in range(2):
        env = rl.HipVecEnv(env_name, n, seed=3, continuous=cont)
        pol = rl.PPOPolicy(env, update_freq=T, hidden=h, act=act)
        assert pol.na == M.ppo_na(env_name, cont)
        pol.params.copy_(dev(p))
        sides.append((env, pol))
    (envA, polA), (envB, polB) = sides
    for it in range(2):
        polA.rollout_()
        for t in range(T):
            a = polB.plan_()
            polB.push_preact_()
            envB.act_(a)
            polB.push_postact_()
        polB.finish_rollout_()
        polB.gae_()
        ta, tb = polA.trajectory, polB.trajectory
        for name in ("obs", "logp", "value", "reward", "terminal", "adv", "ret"):
            assert torch.equal(getattr(ta, name), getattr(tb, name)), f"{name} differs (period {it})"
        assert torch.equal(ta.action, tb.action)
        assert torch.equal(envA.raw_state(), envB.raw_state())
        assert torch.equal(envA._t, envB._t) and torch.equal(envA._episode, envB._episode)
        assert torch.equal(envA.reward(), envB.reward()) and torch.equal(envA._done, envB._done)
    x = host(polA.trajectory.obs)[:T].transpose(1, 0, 2).reshape(ns, T * n)
    assert_visible_net(p, ns, h, act, x, row["id"] + " actor")


def test_ppo_refuses_a_discrete_pendulum_of_other_than_three_actions(rl):
    """make_desc gives a discrete Pendulum policy 3 actions whatever the env's n_actions: the policy would never pick the last
    torques of a finer grid, and PPOPolicy sized its actor by n_actions (the critic's init wrote past the parameters).  Both
    the Python policy and the C rollout now refuse the combination."""
    from rlhip import _lib
    from rlhip._lib import call
    from rlhip.ops import ptr, stream_ptr

    env = rl.HipVecEnv("pendulum", 64, seed=1, continuous=False, n_actions=4)
    with pytest.raises(_lib.RLHipArgumentError, match="n_actions"):
        rl.PPOPolicy(env, update_freq=4, hidden=64)
    ok = rl.HipVecEnv("pendulum", 64, seed=1, continuous=False)
    pol = rl.PPOPolicy(ok, update_freq=4, hidden=64)
    with pytest.raises(_lib.RLHipArgumentError, match="n_actions"):
        call("rlhip_ppo_rollout_f32", pol.kind, C.byref(env.cfg), C.byref(env._st), env.n, pol.T, C.byref(pol.cfg),
             ptr(pol.params), pol.seed, 0, 0, C.byref(pol.trajectory.c), stream_ptr())
    pol.rollout_()  # three actions: fine
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------- fused DQN act
@pytest.mark.parametrize("row", M.DQN_ACT, ids=ids(M.DQN_ACT))
def test_fused_dqn_act_vs_oracle(rl, row):
    """rlhip_dqn_act_f32 (plan! + act! + push! in one launch), called directly: Q on the observations the kernel read within
    the plan bar of oracle.mlp2_forward; actions bit-exact with oracle.eps_greedy_select on the GPU's Q; the oracle env started
    from the GPU's state and stepped with those actions gives the same terminal flags, step and reset counters bit for bit
    (rewards too, except Pendulum's, which is a Float32 function of the state: within 2e-6); the ring records equal an
    oracle.Ring fed the same states and transitions.  A quarter of the envs start at t = max_steps, so resets happen."""
    from rlhip._lib import call
    from rlhip.ops import ptr, stream_ptr
    from rlhip.trajectory import CircularArraySARTSTraces

    env_name, h, act, n = row["env"], row["hidden"], row["act"], row["n"]
    kind = KIND[env_name]
    env = rl.HipVecEnv(env_name, n, seed=13, env_id_base=7, continuous=False, max_steps=40)
    ns, na = env.odim, len(env.action_space())
    assert int(rl._lib.lib.rlhip_dqn_act_supported(kind, n, h)) == 1
    rng = np.random.default_rng(zlib.crc32(row["id"].encode()))
    p = perturbed_net(ns, h, na, 9, 0, rng, 0.1)
    t0 = np.where(rng.random(n) < 0.25, 40, rng.integers(0, 30, n)).astype(np.int32)  # CartPole ends at t > max_steps
    env.set_raw_state(env.raw_state().clone(), t0)
    tr = CircularArraySARTSTraces(capacity=4, n_env=n, obs_dim=ns)
    ref = oracle.Ring(4, n, ns)
    obs0 = host(env.state()).copy()
    tr.push_state_(env.state())
    ref.push_state(obs0)
    oenv = oracle.VecEnv(kind, n, seed=13, env_id_base=7, continuous=False, max_steps=40)
    oenv.set_state([host(env.raw_state()[k]) for k in range(env.sdim)], host(env._t))
    oenv.episode[:] = host(env._episode).view(np.uint32)
    assert_visible_net(p, ns, h, act, obs0, row["id"])
    eps, xseed, step = 0.3, 17, 5
    P = dev(p)
    actions = torch.zeros(n, dtype=torch.int32, device="cuda")
    q = torch.zeros((na, n), device="cuda")
    obs_out, last_obs = torch.zeros((ns, n), device="cuda"), torch.zeros((ns, n), device="cuda")
    call("rlhip_dqn_act_f32", kind, C.byref(env.cfg), C.byref(env._st), n, ptr(P), h, na, act, eps, xseed, step, env.seed,
         env.env_id_base, C.byref(tr.rb), ptr(actions), ptr(q), ptr(obs_out), ptr(last_obs), stream_ptr())
    env._obs_valid = False
    gq, ga = host(q), host(actions)
    np.testing.assert_allclose(gq, oracle.mlp2_forward(p, ns, h, na, act, obs0), rtol=2e-5, atol=2e-6)
    assert np.array_equal(ga, oracle.eps_greedy_select(gq, eps, seed=xseed, step=step, env_id_base=env.env_id_base))
    oenv.step(ga)
    done = host(env._done)
    assert np.array_equal(done, oenv.done) and np.array_equal(host(env._t), oenv.t)
    assert np.array_equal(host(env._episode).view(np.uint32), oenv.episode)
    assert 0.2 <= done.mean() <= 0.5, f"{done.mean():.3f} of the envs terminated"
    if env_name == "pendulum":
        np.testing.assert_allclose(host(env.reward()), oenv.reward, rtol=2e-6, atol=1e-7)
    else:
        assert np.array_equal(host(env.reward()), oenv.reward)
    oatol = 2e-5 if env_name == "pendulum" else 1e-7
    np.testing.assert_allclose(host(obs_out), oenv.obs(), rtol=2e-6, atol=oatol)
    np.testing.assert_allclose(host(last_obs), oenv.last_obs, rtol=2e-6, atol=oatol)
    assert np.array_equal(host(obs_out), host(env.state())), "obs_out is not state(env) after the step"
    ref.push_transition(host(obs_out), ga, host(env.reward()), done)
    assert len(tr) == len(ref) == 1
    idx = np.arange(n, dtype=np.int64)
    for g_, o_ in zip((host(x) for x in tr.gather(dev(idx))), ref.gather(idx)):
        assert np.array_equal(g_, o_)
