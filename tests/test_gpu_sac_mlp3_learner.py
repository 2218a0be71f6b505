"""SACPolicy(layers = 3) on the device, in the form of tests/test_gpu_td3_mlp3_learner.py: four teacher-forced updates against the
model pipeline (tests/sac_mlp3_ref.py, torch Adam in Float64) under the bars of tests/test_gpu_sac_learner.py, the unchanged run loop
with a checkpoint in the middle, the envelope's refusals, and the Pendulum learning check of tests/test_gpu_sac_learner.py."""
import numpy as np
import pytest
import torch

import sac_cases as SC
import sac_mlp3_ref as R
import sac_ref
import td3_mlp3_ref as T
from conftest import F32_GRAD_TOL, assert_grad_close
from test_gpu_bench_shapes import host
from test_gpu_sac_learner import LEARN_STEPS, _build_agent, _LastRewards

pytestmark = pytest.mark.gpu


def test_four_teacher_forced_updates_against_the_model_pipeline():
    import rlhip as rl
    from test_gpu_sac_kernels import SacDevice

    dev, c, lr, tau, seed = SacDevice(), R.build("clamp"), 3e-3, 0.05, 11
    pol = rl.SACPolicy(rl.PendulumEnv(SC.N_ENV, seed=1), hidden=c["h"], layers=3, gamma=c["gamma"], tau=tau, alpha=c["alpha"], batchsize=65,
                       update_after=SC.N_ENV, lr=lr, lr_alpha=c["alpha_lr"], target_entropy=c["target_entropy"], min_sigma=c["lo"],
                       max_sigma=c["hi"], seed=seed)
    assert pol.action_scale == c["scale"] and pol.actor.numel() == c["actor"].size
    for k in ("actor", "critics", "targets"):
        getattr(pol, k).copy_(torch.tensor(c[k]))
    traj = rl.Trajectory(dev.traces(c), controller=rl.InsertSampleRatioController(ratio=1e9, threshold=1, n_inserted=SC.PUSHES))
    model = {k: torch.nn.Parameter(torch.zeros(getattr(pol, k).numel(), dtype=torch.float64)) for k in ("actor", "critics")}
    adam = {k: torch.optim.Adam([p], lr=lr, betas=(0.9, 0.999), eps=1e-8) for k, p in model.items()}

    def step(k, before, grad):
        model[k].data, model[k].grad = torch.tensor(before, dtype=torch.float64), torch.tensor(grad)
        adam[k].step()
        return model[k].detach().numpy()

    for u in range(4):
        before = {k: host(getattr(pol, k)).copy() for k in ("actor", "critics", "targets", "alpha")}
        assert pol.optimise_(traj) is True and pol.n_updates == u + 1
        cu = dict(c, actor=before["actor"], critics=before["critics"], targets=before["targets"], alpha=float(before["alpha"][0]))
        rec, (eps0, eps1) = T.records(c, host(pol.last_idx.t)), sac_ref.draw_pair(dev.sample, 65, seed + 1, u)
        rc = R.critic(cu, rec, eps0)
        assert_grad_close(host(pol.critic_grad), rc["grad"], F32_GRAD_TOL, f"sac mlp3 pipeline u{u} critic gradient")
        assert_grad_close(host(pol.critic_loss), rc["loss"], F32_GRAD_TOL, f"sac mlp3 pipeline u{u} critic loss")
        pc = step("critics", before["critics"], rc["grad"])
        ra = R.actor(cu, rec, eps1, critics=host(pol.critics))  # teacher-forced on the device's stepped critics
        assert_grad_close(host(pol.actor_grad), ra["grad"], F32_GRAD_TOL, f"sac mlp3 pipeline u{u} actor gradient")
        assert_grad_close(host(pol.actor_stats), ra["stats"], F32_GRAD_TOL, f"sac mlp3 pipeline u{u} actor statistics")
        pa = step("actor", before["actor"], ra["grad"])
        for k, want, bar in (("critics", pc, 1.0), ("actor", pa, 1.0), ("targets", (1 - tau) * before["targets"] + tau * pc, tau)):
            d = np.abs(host(getattr(pol, k)) - want)
            assert np.quantile(d, 0.99) <= 0.02 * lr * bar + 1e-7 and d.max() <= 2.5 * lr * bar + 1e-7, f"update {u} {k}: max |dp| {d.max():.2e}"
        assert abs(float(pol.alpha) - float(ra["alpha_new"][0])) <= 1e-6, f"update {u}: alpha {float(pol.alpha)!r}"


def test_a_checkpoint_mid_run_continues_bit_identically_and_restores_layers():
    import rlhip as rl

    env, agent = _build_agent(start_steps=3, hidden=256, layers=3)
    rl.run(agent, env, rl.StopAfterNSteps(20))
    sd = rl.state_dict({"env": env, "agent": agent})
    assert sd["agent/policy/layers"] == 3 and sd["agent/policy/actor"].size == R.nparams(3, 256, 2)
    rl.run(agent, env, rl.StopAfterNSteps(20))
    env2, agent2 = _build_agent(start_steps=3, hidden=256, layers=3)
    rl.load_state_dict({"env": env2, "agent": agent2}, sd)
    rl.run(agent2, env2, rl.StopAfterNSteps(20))
    p, p2 = agent.policy, agent2.policy
    assert (p2.n_updates, p2.vec_steps, p2.plan_steps, p2.layers) == (36, 40, 40, 3) == (p.n_updates, p.vec_steps, p.plan_steps, p.layers)
    for k in ("actor", "critics", "targets", "alpha", "actor_grad", "critic_grad"):
        assert torch.equal(getattr(p, k), getattr(p2, k)) and torch.isfinite(getattr(p, k)).all(), f"{k} after the checkpoint round trip"


@pytest.mark.parametrize("kw,exc,match", [(dict(hidden=48), NotImplementedError, "multiple of 32"), (dict(layers=4), ValueError, "layers must be"),
                                          (dict(ns=5), NotImplementedError, "obs_dim = 5")])
def test_the_envelope_is_refused_by_name(kw, exc, match):
    import rlhip as rl
    from rlhip import sac
    from rlhip.ops import mlp2_init

    env = rl.PendulumEnv(8, seed=2)
    if "ns" in kw:  # a continuous env of five components: the policy reads the width off env.state()
        env.state = lambda: torch.zeros(5, 8, device="cuda")
        with pytest.raises(ValueError, match="obs_dim 2..4"):
            sac.sac_workspace(5, 64, 64, layers=3)
    with pytest.raises(exc, match=match):
        rl.SACPolicy(env, **dict(dict(hidden=64, layers=3), **{k: v for k, v in kw.items() if k != "ns"}))
    p = rl.SACPolicy(rl.PendulumEnv(8, seed=2), hidden=48, seed=4)  # layers = 2, the default, constructs what it always did
    assert p.layers == 2 and torch.equal(p.actor, mlp2_init(3, 48, 2, 4, 0, "cuda"))


def test_it_learns_pendulum():
    """tests/test_gpu_sac_learner.py's check, unchanged but for layers = 3: more than 3 standard errors of RandomPolicy's per-env means
    above its mean"""
    import rlhip as rl

    n = 64
    env, agent = _build_agent(n=n, cap=1024, seed=3, batchsize=256, hidden=64, update_after=10 * n, start_steps=10, layers=3)
    hook, rhook = _LastRewards(n, LEARN_STEPS - 200), _LastRewards(n, LEARN_STEPS - 200)
    rl.run(agent, env, rl.StopAfterNSteps(LEARN_STEPS), hook)
    rl.run(rl.RandomPolicy(seed=3), rl.PendulumEnv(n, seed=3), rl.StopAfterNSteps(LEARN_STEPS), rhook)
    got, rnd = hook.per_env(), rhook.per_env()
    se = float(rnd.std(ddof=1) / np.sqrt(n))
    print(f"SACPolicy(layers = 3) mean reward per step over the last 200 of {LEARN_STEPS} vec-steps: {got.mean():.4f}; RandomPolicy: {rnd.mean():.4f} (se {se:.4f})")
    assert hook.k == 200 and agent.policy.n_updates > LEARN_STEPS - 20
    assert got.mean() > rnd.mean() + 3.0 * se, f"SAC {got.mean():.4f} does not exceed random {rnd.mean():.4f} by 3 x {se:.4f}"
