"""QRDQNLearner on the device: the update pipeline against the replay-driven learner model (tests/qrdqn_ref.py), the priority
write-back, the unchanged run loop with a checkpoint in the middle, and learning on CartPole.

  teacher-forced   6 updates per form; before each one the model takes the device's state (parameters, target, Adam moments) and the
                   batch the device gathered, then runs its own pipeline: replay gradient -> Adam (the oracle's) -> target sync.  Counters
                   equal; gradients GRAD_BAR of max|g|; parameters per step q99 <= 0.02 lr, max <= 2.5 lr (the Adam bars of
                   tests/test_gpu_c51_learner.py: Adam turns a gradient element near zero into a step of +-lr)
                   forms: uniform 1-step, n_step = 3, prioritized with per_beta > 0, Double DQN, on a record ring (ns = 4) and a frame ring
                   (ns = 6); the prioritized forms also check the written-back (ql + eps)^alpha under the drawn keys
  rlhip.run        64 CartPole envs x 40 vec-steps under Agent(QBasedPolicy(QRDQNLearner)); a checkpoint taken after 20 steps
                   continues bit-identically in a fresh agent
  it learns        the config of tests/test_gpu_c51_learner.py without a support: 51 quantiles, kappa = 1, on the per-stage loop"""
import numpy as np
import pytest
import torch

import oracle
import qrdqn_ref as R
from conftest import assert_grad_close
from heads_ref import F32
from test_gpu_bench_shapes import host, note
from test_qrdqn_reference import GRAD_BAR, loss_bar

pytestmark = pytest.mark.gpu

N_ENV, CAP, PUSHES = 8, 24, 30
KAPPA, N, NA = 1.0, 51, 3


def _fill(tr, ns, rng):
    up = lambda x: torch.tensor(np.ascontiguousarray(x), device="cuda")  # noqa: E731
    tr.push_state_(up(rng.normal(0, 1, (ns, N_ENV)).astype(F32)))
    for _ in range(PUSHES):
        tr.push_transition_(up(rng.normal(0, 1, (ns, N_ENV)).astype(F32)), up(rng.integers(0, NA, N_ENV).astype(np.int32)),
                            up(rng.normal(0.2, 1.0, N_ENV).astype(F32)), up((rng.uniform(size=N_ENV) < 0.15).astype(np.uint8)))
    return tr


FORMS = {"uniform-records": dict(ns=4), "nstep3-records": dict(ns=4, n_step=3), "per-records": dict(ns=4, per=True, per_beta=0.4),
         "per-nstep3-records": dict(ns=3, per=True, per_beta=0.4, n_step=3), "double-records": dict(ns=4, double_dqn=True),
         "uniform-frames": dict(ns=6), "nstep3-frames": dict(ns=6, n_step=3), "per-double-frames": dict(ns=6, per=True, per_beta=0.5, double_dqn=True)}


@pytest.mark.parametrize("form", list(FORMS))
def test_six_teacher_forced_updates_against_the_model_pipeline(form):
    import rlhip as rl

    kw = dict(FORMS[form])
    ns, per, n_step = kw.pop("ns"), kw.pop("per", False), kw.get("n_step", 1)
    h, b, lr, gamma, seed, sync = 20, 33, 1e-3, 0.9, 11, 4
    rng = np.random.default_rng(4242)
    net = rl.HipApproximator(ns, h, NA * N, act="tanh" if "nstep" in form else "relu", lr=lr, seed=seed)
    tn = rl.TargetNetwork(net, sync_freq=sync)
    tn.target.copy_(net.params + 0.1 * torch.randn(net.params.shape, generator=torch.Generator().manual_seed(1)).cuda())
    learner = rl.QRDQNLearner(tn, NA, n_quantiles=N, kappa=KAPPA, batchsize=b, gamma=gamma, min_replay_history=N_ENV, seed=seed, per_eps=1e-3,
                              per_alpha=0.6, **kw)
    if per and ns > 4:
        tr = rl.CircularPrioritizedFrameTraces(CAP, N_ENV, ns, n_step=n_step, default_priority=2.0)  # (near the written-back ones: later draws mix both)
    elif per:
        tr = rl.CircularPrioritizedTraces(CAP, N_ENV, ns, n_step=n_step, default_priority=2.0)
    else:
        tr = rl.CircularArraySARTSTraces(CAP, N_ENV, ns)
    assert tr.records_layout == (ns <= 4)
    traj = rl.Trajectory(_fill(tr, ns, rng), controller=rl.InsertSampleRatioController(ratio=1e9, threshold=1, n_inserted=PUSHES))
    written = []
    if per:
        inner = tr.set_priority_
        tr.set_priority_ = lambda keys, prio: (written.append((keys.clone(), prio.clone())), inner(keys, prio))[1]
    worst = dict(q99=0.0, dmax=0.0, grad=0.0)
    for u in range(6):
        p0, t0, m, v = (host(x).copy() for x in (net.params, tn.target, net.m, net.v))
        assert learner.optimise_(traj) is True and learner.n_updates == u + 1 and learner.vec_steps == u + 1 and learner.draw_ctr == u + 1
        s, a, r, t, sn, n_used = (None if x is None else host(x) for x in learner._batch.t)
        assert s.shape == (ns, b) and sn.shape == (ns, b)
        folded = n_step > 1 and ns <= 4  # the record rings fold the window: one discount gamma^n, no n_used
        assert (n_used is None) == (ns <= 4 or (n_step == 1 and not per))
        weights = host(learner.is_weights).copy() if per else None
        c = dict(ns=ns, h=h, na=NA, N=N, act=net.act, batch=b, kappa=KAPPA, params=p0, target=t0, s=s, sn=sn, a=a, r=r, term=t, n_used=n_used,
                 weights=weights, double=learner.double_dqn, gamma=float(R.gamma_pow(gamma, n_step)) if folded else gamma)
        rp = R.replay(c)
        bd = R.budgets(c, rp)
        rel = R.rel(host(learner.grad), rp["grad"])
        worst["grad"] = max(worst["grad"], rel)
        assert_grad_close(host(learner.grad), rp["grad"], GRAD_BAR, f"qrdqn pipeline {form} u{u} gradient")
        assert abs(float(learner.loss) - rp["loss"]) <= loss_bar(c, rp, bd)
        if per:  # the written-back priorities: (ql + eps)^alpha of the UNWEIGHTED loss, under the drawn keys, once per update
            assert len(written) == u + 1 and torch.equal(written[u][0], learner._key)
            want = (rp["ql"].astype(np.float64) + 1e-3) ** 0.6
            bar = 2.0 * 0.6 * bd["ql"] / (rp["ql"].astype(np.float64) + 1e-3) + 8.0 * 2.0 ** -23
            got = host(written[u][1]).astype(np.float64)
            assert (np.abs(got - want) <= bar * want).all(), f"update {u}: priorities off by {np.abs(got / want - 1).max():.2e}"
            if (weights < 0.99).any():  # (the first draw meets equal default priorities: every weight is 1)
                worst["weighted"] = worst.get("weighted", 0) + 1
                assert not np.allclose(got, ((rp["ql"] * weights).astype(np.float64) + 1e-3) ** 0.6, rtol=1e-3), "the weighted loss was written back"
        pm = p0.copy()
        oracle.adam(pm, rp["grad"].astype(F32), m, v, lr, 0.9, 0.999, 1e-8, u + 1)
        d = np.abs(host(net.params) - pm)
        q99, dmax = float(np.quantile(d, 0.99)), float(d.max())
        worst.update(q99=max(worst["q99"], q99), dmax=max(worst["dmax"], dmax))
        assert q99 <= 0.02 * lr + 1e-7 and dmax <= 2.5 * lr + 1e-7, f"update {u}: |dp| q99 {q99:.2e} max {dmax:.2e}"
        if (u + 1) % sync == 0:
            assert torch.equal(tn.target, net.params), "the target was not synchronised"
        else:
            assert np.array_equal(host(tn.target), t0)
    assert not per or worst["weighted"] >= 3, "the importance-sampling weights never left 1"
    note(f"QRDQNLearner pipeline vs model, {form}", updates=6, grad_worst=worst["grad"], dp_q99_worst=worst["q99"], dp_max_worst=worst["dmax"])


def _build_agent(n=64, cap=64, seed=5, **kw):
    import rlhip as rl

    env = rl.CartPoleEnv(n, seed=seed)
    net = rl.HipApproximator(4, 64, 2 * 51, seed=seed)
    learner = rl.QRDQNLearner(rl.TargetNetwork(net, sync_freq=10), 2, n_quantiles=51, batchsize=64, min_replay_history=5 * n, seed=seed, **kw)
    policy = rl.QBasedPolicy(learner, rl.EpsilonGreedyExplorer(0.05, kind="exp", decay_steps=20, seed=seed))
    return env, rl.Agent(policy, rl.Trajectory(rl.CircularArraySARTSTraces(cap, n, 4)))


def test_run_plans_on_the_mean_and_a_checkpoint_continues_bit_identically():
    import rlhip as rl

    env, agent = _build_agent()
    learner = agent.policy.learner
    rl.run(agent, env, rl.StopAfterNSteps(20))
    sd = rl.state_dict({"env": env, "agent": agent})
    for k in ("learner/approximator/network/params", "learner/approximator/target", "learner/approximator/network/m", "learner/n_updates",
              "learner/n_quantiles", "learner/kappa"):
        assert any(p.endswith(k) for p in sd), k
    assert not any("_batch" in p for p in sd)  # scratch
    rl.run(agent, env, rl.StopAfterNSteps(20))
    assert learner.vec_steps == 40 and learner.n_updates == 36  # 5 vec-steps of warm-up
    q = learner.forward(env.state())
    th = learner.quantiles(env.state())
    assert q.shape == (2, 64) and th.shape == (51, 2, 64)
    assert float((th.mean(0) - q).abs().max()) <= 1e-5 * max(1.0, float(q.abs().max()))  # Q is the mean of the quantiles
    greedy = rl.QBasedPolicy(learner, rl.GreedyExplorer()).plan_(env)
    assert torch.equal(greedy, q.argmax(0).to(torch.int32) + 1)
    tie = rl.QBasedPolicy(learner, rl.EpsilonGreedyExplorer(0.0, is_break_tie=True)).plan_(env)  # forward, then the selection kernel
    assert torch.equal(tie, greedy)
    env2, agent2 = _build_agent()
    rl.load_state_dict({"env": env2, "agent": agent2}, sd)
    rl.run(agent2, env2, rl.StopAfterNSteps(20))
    l2 = agent2.policy.learner
    n1, n2 = learner.approximator.network, l2.approximator.network
    for a, b in ((n1.params, n2.params), (n1.m, n2.m), (n1.v, n2.v), (n1.beta_pow, n2.beta_pow), (learner.approximator.target, l2.approximator.target),
                 (learner.grad, l2.grad), (env.state(), env2.state())):
        assert torch.equal(a, b), "the run does not continue bit-identically from the checkpoint"
    assert torch.equal(agent.trajectory.container.records, agent2.trajectory.container.records)
    assert (l2.n_updates, l2.vec_steps, agent2.policy.explorer.step) == (36, 40, agent.policy.explorer.step)


LEARN_STEPS = 3500  # from the measured curve (profiles/qrdqn.md): three windows clear the bar after 3000 vec-steps; the cap is 6500, as C51's


def test_it_learns_cartpole():
    import rlhip as rl
    from test_gpu_learn import _random_policy_episode_length

    n, cap, chunk = 4096, 256, 500
    base = _random_policy_episode_length(rl)
    assert 15.0 < base < 30.0, base
    env = rl.CartPoleEnv(n, seed=5)
    net = rl.HipApproximator(4, 128, 2 * 51, seed=5)
    learner = rl.QRDQNLearner(rl.TargetNetwork(net, sync_freq=100), 2, n_quantiles=51, batchsize=512, min_replay_history=n, seed=5)
    policy = rl.QBasedPolicy(learner, rl.EpsilonGreedyExplorer(0.01, kind="exp", decay_steps=500, seed=5))
    tr = rl.CircularArraySARTSTraces(capacity=cap, n_env=n, obs_dim=4)
    agent = rl.Agent(policy, rl.Trajectory(tr))
    curve = []
    for _ in range(LEARN_STEPS // chunk):
        rl.run(agent, env, rl.StopAfterNSteps(chunk))
        term = tr.gather(torch.arange(len(tr) * n, device="cuda"))[3]
        curve.append(round(len(tr) * n / max(1.0, float(term.sum())), 1))
    print(f"QRDQNLearner on CartPole: random {base:.1f}, mean episode length per {chunk} vec-steps {curve}, updates {learner.n_updates}")
    note("QRDQNLearner learns CartPole", random_policy_ep_len=round(base, 1), ep_len_per_500_vec_steps=curve, updates=learner.n_updates)
    assert torch.isfinite(net.params).all()
    assert max(curve) >= 2.0 * base, f"mean episode length never reached 2 x the random policy's {base:.1f}: {curve}"
    assert sum(c >= 2.0 * base for c in curve) >= 3, f"fewer than three 500-step windows above 2 x random ({base:.1f}): {curve}"
