"""TD3Policy(layers = 3) / DDPGPolicy(layers = 3) on the device, in the form of tests/test_gpu_td3_learner.py: four teacher-forced
updates against the model pipeline (tests/td3_mlp3_ref.py, torch Adam in Float64) under that test's bars, the unchanged run loop with
a checkpoint in the middle, and `layers = 2` constructing what it always did."""
import numpy as np
import pytest
import torch

import sac_cases as SC
import td3_mlp3_ref as R
from conftest import F32_GRAD_TOL, assert_grad_close
from test_gpu_bench_shapes import host
from test_gpu_sac_learner import LEARN_STEPS, _LastRewards

pytestmark = pytest.mark.gpu


def test_four_teacher_forced_updates_against_the_model_pipeline():
    import rlhip as rl
    from test_gpu_sac_kernels import SacDevice

    c, lr, tau, names = R.build("base"), 3e-3, 0.05, ("actor", "critics", "actor_target", "critic_targets")
    pol = rl.TD3Policy(rl.PendulumEnv(SC.N_ENV, seed=1), hidden=c["h"], layers=3, gamma=c["gamma"], tau=tau, batchsize=65, update_after=SC.N_ENV,
                       lr=lr, policy_freq=2, target_noise=c["tn"], noise_clip=c["clip"], seed=11)
    c = dict(c, lo=pol.action_lo, hi=pol.action_hi, scale=pol.action_scale)
    for k, src in zip(names, ("actor", "critics", "actor_t", "targets")):
        getattr(pol, k).copy_(torch.tensor(c[src]))
    traj = rl.Trajectory(SacDevice().traces(c), controller=rl.InsertSampleRatioController(ratio=1e9, threshold=1, n_inserted=SC.PUSHES))
    model = {k: torch.nn.Parameter(torch.zeros(getattr(pol, k).numel(), dtype=torch.float64)) for k in names[:2]}
    adam = {k: torch.optim.Adam([p], lr=lr, betas=(0.9, 0.999), eps=1e-8) for k, p in model.items()}

    def step(k, before, grad):
        model[k].data, model[k].grad = torch.tensor(before, dtype=torch.float64), torch.tensor(grad)
        adam[k].step()
        return model[k].detach().numpy()

    def near(k, want, bar):
        d = np.abs(host(getattr(pol, k)) - want)
        assert np.quantile(d, 0.99) <= 0.02 * lr * bar + 1e-7 and d.max() <= 2.5 * lr * bar + 1e-7, f"update {u} {k}: max |dp| {d.max():.2e}"

    for u in range(1, 5):
        before = {k: host(getattr(pol, k)).copy() for k in names}
        assert pol.optimise_(traj) is True and pol.n_updates == u
        cu = dict(c, actor=before["actor"], critics=before["critics"], actor_t=before["actor_target"], targets=before["critic_targets"])
        rec = R.records(c, host(pol.last_idx.t))
        rc = R.critic(cu, rec, host(pol.last_noise.t))
        assert_grad_close(host(pol.critic_grad), rc["grad"], F32_GRAD_TOL, f"td3 mlp3 pipeline u{u} critic gradient")
        assert_grad_close(host(pol.critic_loss), rc["loss"], F32_GRAD_TOL, f"td3 mlp3 pipeline u{u} critic loss")
        pc = step("critics", before["critics"], rc["grad"])
        near("critics", pc, 1.0)
        if u % 2:
            assert all(np.array_equal(host(getattr(pol, k)), before[k]) for k in ("actor", "actor_target", "critic_targets")), f"update {u}"
            continue
        ra = R.actor(cu, rec, critics=host(pol.critics))  # teacher-forced on the device's stepped critics
        assert_grad_close(host(pol.actor_grad), ra["grad"], F32_GRAD_TOL, f"td3 mlp3 pipeline u{u} actor gradient")
        assert_grad_close(host(pol.actor_stats), ra["stats"], F32_GRAD_TOL, f"td3 mlp3 pipeline u{u} actor statistics")
        pa = step("actor", before["actor"], ra["grad"])
        near("actor", pa, 1.0)
        near("actor_target", (1 - tau) * before["actor_target"] + tau * pa, tau)
        near("critic_targets", (1 - tau) * before["critic_targets"] + tau * pc, tau)


def _agent(cls, n=64, cap=64, seed=5, **kw):
    import rlhip as rl

    env = rl.PendulumEnv(n, seed=seed)
    pol = getattr(rl, cls)(env, **dict(dict(hidden=64, batchsize=64, update_after=5 * n, seed=seed, start_steps=3), **kw))
    traces = rl.CircularArraySARTSTraces(cap, n, 3, action_dtype=torch.float32)
    return env, rl.Agent(pol, rl.Trajectory(traces, controller=rl.InsertSampleRatioController(ratio=1e9, threshold=1)))


@pytest.mark.parametrize("cls,hidden", [("TD3Policy", 256), ("DDPGPolicy", 64)])
def test_a_checkpoint_mid_run_continues_bit_identically(cls, hidden):
    import rlhip as rl

    env, agent = _agent(cls, hidden=hidden, layers=3)
    rl.run(agent, env, rl.StopAfterNSteps(20))
    sd = rl.state_dict({"env": env, "agent": agent})
    assert sd["agent/policy/layers"] == 3 and sd["agent/policy/actor"].size == R.nparams(3, hidden)
    rl.run(agent, env, rl.StopAfterNSteps(20))
    env2, agent2 = _agent(cls, hidden=hidden, layers=3)
    rl.load_state_dict({"env": env2, "agent": agent2}, sd)
    rl.run(agent2, env2, rl.StopAfterNSteps(20))
    p, p2 = agent.policy, agent2.policy
    assert (p2.n_updates, p2.vec_steps, p2.plan_steps) == (36, 40, 40) == (p.n_updates, p.vec_steps, p.plan_steps)
    for k in ("actor", "critics", "actor_target", "critic_targets", "actor_grad", "critic_grad"):
        assert torch.equal(getattr(p, k), getattr(p2, k)), f"{k} differs after the checkpoint round trip"
        assert torch.isfinite(getattr(p, k)).all()
    for o, o2 in ((p.actor_opt, p2.actor_opt), (p.critic_opt, p2.critic_opt)):
        assert torch.equal(o.m, o2.m) and torch.equal(o.v, o2.v) and torch.equal(o.beta_pow, o2.beta_pow)


def test_layers_2_constructs_the_tensors_it_always_did():
    import rlhip as rl
    from rlhip.ops import mlp2_init

    env = rl.PendulumEnv(8, seed=2)
    p, q = rl.TD3Policy(env, hidden=48, seed=4), rl.TD3Policy(env, hidden=48, seed=4, layers=2)
    assert p.layers == 2 and torch.equal(p.actor, mlp2_init(3, 48, 1, 4, 0, env.device))
    assert all(torch.equal(getattr(p, k), getattr(q, k)) for k in ("actor", "critics", "actor_target", "critic_targets"))
    with pytest.raises(NotImplementedError, match="multiple of 32"):
        rl.TD3Policy(env, hidden=48, layers=3)


@pytest.mark.parametrize("cls", ["TD3Policy", "DDPGPolicy"])
def test_it_learns_pendulum(cls):
    """tests/test_gpu_td3_learner.py's check, unchanged but for layers = 3: more than 3 standard errors of RandomPolicy's per-env means
    above its mean"""
    import rlhip as rl

    n = 64
    env, agent = _agent(cls, n=n, cap=1024, seed=3, batchsize=256, update_after=10 * n, start_steps=10, gamma=0.9, tau=0.02, layers=3)
    hook, rhook = _LastRewards(n, LEARN_STEPS - 200), _LastRewards(n, LEARN_STEPS - 200)
    rl.run(agent, env, rl.StopAfterNSteps(LEARN_STEPS), hook)
    rl.run(rl.RandomPolicy(seed=3), rl.PendulumEnv(n, seed=3), rl.StopAfterNSteps(LEARN_STEPS), rhook)
    got, rnd = hook.per_env(), rhook.per_env()
    se = float(rnd.std(ddof=1) / np.sqrt(n))
    print(f"{cls}(layers = 3) mean reward per step over the last 200 of {LEARN_STEPS} vec-steps: {got.mean():.4f}; RandomPolicy: {rnd.mean():.4f} (se {se:.4f})")
    assert hook.k == 200 and agent.policy.n_updates > LEARN_STEPS - 20
    assert got.mean() > rnd.mean() + 3.0 * se, f"{cls} {got.mean():.4f} does not exceed random {rnd.mean():.4f} by 3 x {se:.4f}"
