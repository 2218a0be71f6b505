"""NoisyDense networks on the device (csrc/noisy.hip) against the Float64 model of tests/noisy_ref.py.

  fold / unfold    online and target pair in one launch; the derived budget |eff - ref| <= 4u |sigma xi| + u |ref|, |dsigma - ref| <= 4u |g xi|
                   (u = 2^-24: the cast of the draw, sqrtf, the one product, the one fmaf); dmu = g byte for byte
  forward / plan   logits, probs and q within 4 x the FLOOR, the error of the model evaluated in numpy Float32 against its Float64 self on
                   the same case (never below u, the format's own resolution: a floor from two logits can be 0), relative to the
                   largest magnitude of the output; actions byte for byte the selection kernel on the kernel's own q.  Measured
                   (profiles/noisy.md): logits floor 6.0e-8 .. 1.9e-7, kernel 2.3e-8 .. 2.6e-7 of max|l| over the five cases
  sigma = 0        byte for byte rlhip_c51_forward_f32 on the mu half
  learner          three updates, the target's sync rule, a checkpoint after update 1, the refusals, and CartPole with eps = 0"""
import types

import numpy as np
import pytest
import torch

import noisy_ref as R
from test_gpu_bench_shapes import host

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
SEED = 0x5EED0123456789


def _dev(x, dtype=np.float32, offset=0):
    """a device copy of x that starts `offset` floats behind a 16-byte boundary"""
    x = np.ascontiguousarray(x, dtype)
    buf = torch.zeros(x.size + 4, dtype=torch.from_numpy(x).dtype, device="cuda")
    buf[offset:offset + x.size] = torch.from_numpy(x.ravel()).cuda()
    return buf[offset:offset + x.size].view(x.shape)


@pytest.mark.parametrize("ns,h,M,offset", [(2, 4, 2, 0), (4, 128, 102, 0), (16, 256, 256, 0), (4, 12, 51, 1)])
def test_fold_and_unfold_against_the_model(ns, h, M, offset):
    import rlhip as rl
    from rlhip import ops

    rng = np.random.default_rng(ns * 1000 + M)
    np_ = rl.noisy_nparams(ns, h, M) // 2
    noisy, noisy2, g = (rng.normal(0, 0.5, k).astype(np.float32) for k in (2 * np_, 2 * np_, np_))
    d_noisy, d_noisy2, d_g = _dev(noisy, offset=offset), _dev(noisy2, offset=offset), _dev(g, offset=offset)
    eff, eff2 = (_dev(np.zeros(np_), offset=offset) for _ in range(2))
    ops.noisy_fold(d_noisy, eff, ns, h, M, SEED, 7, d_noisy2, eff2)
    for got, src, tag in ((eff, noisy, R.TAG_ONLINE), (eff2, noisy2, R.TAG_TARGET)):
        x = R.xi(SEED, 7, tag, ns, h, M)
        ref = R.fold(src, x)
        err = np.abs(host(got).astype(np.float64) - ref)
        bar = 4 * U * np.abs(src[np_:].astype(np.float64) * x) + U * np.abs(ref)
        print(f"fold ({ns}, {h}, {M}) tag {tag}: worst error / budget {np.max(err / np.maximum(bar, 1e-300)):.3f}")
        assert (err <= bar).all()
    assert not np.allclose(R.xi(SEED, 7, R.TAG_ONLINE, ns, h, M), R.xi(SEED, 7, R.TAG_TARGET, ns, h, M))
    same, other, single = (_dev(np.zeros(np_), offset=offset) for _ in range(3))
    ops.noisy_fold(d_noisy2, same, ns, h, M, SEED, 7)  # noisy2 under the ONLINE tag: other noise than eff2's
    ops.noisy_fold(d_noisy, single, ns, h, M, SEED, 7)
    ops.noisy_fold(d_noisy, other, ns, h, M, SEED, 8)
    assert torch.equal(single, eff) and not torch.equal(other, eff) and not torch.equal(same, eff2)
    gn = _dev(np.zeros(2 * np_), offset=offset)
    ops.noisy_unfold_grad(d_g, gn, ns, h, M, SEED, 7)
    x = R.xi(SEED, 7, R.TAG_ONLINE, ns, h, M)
    ref = R.unfold(g, x)
    assert torch.equal(gn[:np_], d_g), "dmu is not g byte for byte"
    assert (np.abs(host(gn[np_:]).astype(np.float64) - ref[np_:]) <= 4 * U * np.abs(ref[np_:])).all()


def _tile():
    import rlhip as rl

    return rl.noisy_plan_tile()


CASES = {"minimum": (2, 4, 1, 2, lambda t: 1, "relu", 0), "partial-tile": (4, 12, 2, 51, lambda t: t + 1, "tanh", 3),
         "shipped": (4, 128, 2, 51, lambda t: 2 * t + 1, "relu", 0), "largest": (16, 256, 4, 64, lambda t: t + 1, "relu", 0),
         "wrapping-ids": (4, 12, 2, 51, lambda t: t + 1, "relu", 2 ** 32 - 3)}


@pytest.mark.parametrize("case", list(CASES))
def test_forward_and_plan_against_the_model(case):
    import rlhip as rl
    from rlhip import ops

    ns, h, na, K, n_of, act, base = CASES[case]
    n, M, step, v = n_of(_tile()), na * K, 11, (-3.0, 5.0)
    rng = np.random.default_rng(len(case))
    noisy = host(rl.noisy_init(ns, h, M, seed=3, sigma0=0.5)) + rng.normal(0, 0.05, 2 * (h * ns + h + M * h + M)).astype(np.float32)
    obs = rng.normal(0, 1, (ns, n)).astype(np.float32)
    obs[:, -1] = obs[:, 0]  # two envs with the same observation
    args = (_dev(noisy), ns, h, na, K, {"relu": 0, "tanh": 1}[act], *v, _dev(obs))
    logits, probs = (torch.empty((M, n), dtype=torch.float32, device="cuda") for _ in range(2))
    q = rl.noisy_c51_forward(*args, SEED, base, step, probs=probs, logits=logits)
    ref = R.forward(noisy, ns, h, na, K, args[5], *v, obs, SEED, base, step)
    low = R.forward(noisy, ns, h, na, K, args[5], *v, obs, SEED, base, step, dtype=np.float32)
    for name, got, r64, r32 in zip(("logits", "probs", "q"), (logits, probs, q), ref, low):
        scale = np.abs(r64).max()
        floor = max(np.abs(r32.astype(np.float64) - r64).max() / scale, U)
        err = np.abs(host(got).astype(np.float64) - r64).max() / scale
        print(f"noisy forward {case} {name}: floor {floor:.3e}, kernel {err:.3e} of max |{name}| = {scale:.3g}")
        assert err <= 4 * floor, name
    if n > 1:
        assert not torch.equal(logits[:, 0], logits[:, -1]), "two envs with one observation drew the same noise"
    logits2 = torch.empty_like(logits)
    q2 = rl.noisy_c51_forward(*args, SEED, base, step, logits=logits2)
    assert torch.equal(q2, q) and torch.equal(logits2, logits)
    for eps in (0.0, 0.3):
        actions, qp = rl.noisy_c51_plan(*args, eps, SEED, base, step)
        assert torch.equal(qp, q)
        assert torch.equal(actions, ops.eps_greedy_select(qp, eps, SEED, step, base))


def test_sigma_zero_is_c51():
    import rlhip as rl

    ns, h, na, K, n = 4, 128, 2, 51, 2 * _tile() + 1
    mu = rl.ops.mlp2_init(ns, h, na * K, 9, 0)
    obs = torch.randn((ns, n), generator=torch.Generator().manual_seed(2)).cuda()
    outs = []
    for fwd, params, key in ((rl.noisy_c51_forward, torch.cat([mu, torch.zeros_like(mu)]), (SEED, 5, 2)), (rl.c51_forward, mu, ())):
        logits, probs = (torch.empty((na * K, n), dtype=torch.float32, device="cuda") for _ in range(2))
        outs.append((fwd(params, ns, h, na, K, 0, 0.0, 200.0, obs, *key, probs=probs, logits=logits), probs, logits))
    assert all(torch.equal(a, b) for a, b in zip(*outs))


def _agent(rl, n=64, seed=5, cap=64, **kw):
    env = rl.CartPoleEnv(n, seed=seed)
    net = rl.NoisyApproximator(4, 128, 2 * 51, seed=seed)
    learner = rl.RainbowLearner(rl.TargetNetwork(net, sync_freq=kw.pop("sync_freq", 2)), 2, n_atoms=51, v_min=0.0, v_max=200.0,
                                batchsize=kw.pop("batchsize", 64), min_replay_history=kw.pop("min_replay_history", 5 * n), seed=seed, **kw)
    policy = rl.QBasedPolicy(learner, rl.EpsilonGreedyExplorer(0.0, seed=seed))
    return env, rl.Agent(policy, rl.Trajectory(rl.CircularArraySARTSTraces(cap, n, 4)))


def test_three_updates_the_sync_rule_and_a_checkpoint_after_the_first():
    import rlhip as rl

    env, agent = _agent(rl)
    learner = agent.policy.learner
    tn, net = learner.approximator, learner.approximator.network
    sigma0 = net.noisy_params[net.noisy_params.numel() // 2:].clone()
    rl.run(agent, env, rl.StopAfterNSteps(5))
    assert learner.n_updates == 1
    sd = rl.state_dict({"env": env, "agent": agent})
    for k in ("network/noisy_params", "approximator/target_noisy", "network/m", "network/counter", "learner/n_updates"):
        assert any(p.endswith(k) for p in sd), k
    rl.run(agent, env, rl.StopAfterNSteps(1))
    assert learner.n_updates == 2 and torch.equal(tn.target_noisy, net.noisy_params)  # sync_freq = 2
    synced = tn.target_noisy.clone()
    rl.run(agent, env, rl.StopAfterNSteps(1))
    assert learner.n_updates == 3 and torch.equal(tn.target_noisy, synced) and not torch.equal(net.noisy_params, synced)
    assert net.m.numel() == net.noisy_params.numel() and not torch.equal(net.noisy_params[sigma0.numel():], sigma0), "sigma did not move"
    env2, agent2 = _agent(rl)
    rl.load_state_dict({"env": env2, "agent": agent2}, sd)
    rl.run(agent2, env2, rl.StopAfterNSteps(2))
    l2 = agent2.policy.learner
    assert l2.n_updates == 3 and torch.equal(l2.approximator.network.noisy_params, net.noisy_params)
    assert torch.equal(l2.approximator.target_noisy, tn.target_noisy) and torch.equal(env2.state(), env.state())


LEARN_STEPS = 1500  # from the measured curve (profiles/noisy.md): 83 after 1000 vec-steps, 137 after 1250, 162 after 1500 (0.3 s)


def test_it_learns_cartpole_without_epsilon():
    import rlhip as rl

    n, chunk = 4096, 250
    env, agent = _agent(rl, n=n, cap=256, sync_freq=100, batchsize=512, min_replay_history=n)
    tr = agent.trajectory.container
    curve = []
    for _ in range(LEARN_STEPS // chunk):
        rl.run(agent, env, rl.StopAfterNSteps(chunk))
        term = tr.gather(torch.arange(len(tr) * n, device="cuda"))[3]
        curve.append(round(len(tr) * n / max(1.0, float(term.sum())), 1))
    print(f"RainbowLearner(NoisyApproximator) on CartPole, eps = 0: mean episode length per {chunk} vec-steps {curve}")
    assert max(curve) >= 3.0 * 21.6, f"mean episode length never reached 3 x the random policy's 21.6: {curve}"


def _refusals(rl):
    tn = rl.TargetNetwork(rl.NoisyApproximator(4, 8, 2 * 4))
    fused = types.SimpleNamespace(policy=types.SimpleNamespace(learner=types.SimpleNamespace(approximator=tn)), trajectory=None)
    plain = rl.QBasedPolicy(types.SimpleNamespace(approximator=tn), rl.GreedyExplorer())
    return {"QRDQNLearner": lambda: rl.QRDQNLearner(tn, 2, n_quantiles=4), "IQNLearner": lambda: rl.IQNLearner(tn, 2),
            "DQNLearner": lambda: rl.DQNLearner(tn), "QBasedPolicy": lambda: plain.plan_(None),
            "run_fused_dqn": lambda: rl.run_fused_dqn(fused, None), "run_fused_dqn_folded": lambda: rl.run_fused_dqn_folded(fused, None),
            "run_fused_dqn_prioritized": lambda: rl.run_fused_dqn_prioritized(fused, None),
            "dueling": lambda: rl.NoisyApproximator(4, 8, 8, dueling=True), "three-layer": lambda: rl.NoisyApproximator(4, 8, 8, layers=3),
            "sharded": lambda: rl.RainbowLearner(tn, 2, n_atoms=4, process_group=object())}


@pytest.mark.parametrize("what", ["QRDQNLearner", "IQNLearner", "DQNLearner", "QBasedPolicy", "run_fused_dqn", "run_fused_dqn_folded",
                                  "run_fused_dqn_prioritized", "dueling", "three-layer", "sharded"])
def test_every_refused_combination_names_the_noisy_approximator(what):
    import rlhip as rl

    with pytest.raises(NotImplementedError, match="NoisyApproximator"):
        _refusals(rl)[what]()
