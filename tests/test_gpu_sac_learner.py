"""SACPolicy on the device: the update pipeline against the model (tests/sac_ref.py), the unchanged run loop with a checkpoint in the
middle, and learning on Pendulum.

  teacher-forced   6 updates; before each one the model takes the device's state, then runs its own pipeline: draw (the oracle's ring
                   sampler) -> critic gradient -> Adam (the oracle's) -> actor gradient against the stepped critics (the device's, so
                   that an Adam step of +-lr on a gradient element near zero does not leak into the next stage) -> Adam -> alpha ->
                   Polyak.  Drawn indices and counters equal; gradients F32_GRAD_TOL; parameters per step q99 <= 0.02 lr, max <= 2.5 lr
                   (the bars of tests/test_gpu_dqn_obsn_learner.py: Adam turns a gradient element near zero into a step of +-lr)
  rlhip.run        64 Pendulum envs x 40 vec-steps under Agent: the stored Float32 actions are the planned ones; a checkpoint taken
                   after 20 steps continues bit-identically in a fresh agent
  it learns        SAC against RandomPolicy on the same env and seed: mean reward per step over the last 200 vec-steps"""
import numpy as np
import pytest
import torch

import oracle
import sac_cases as SC
import sac_ref as R
from conftest import F32_GRAD_TOL, assert_grad_close
from heads_ref import F32
from test_gpu_bench_shapes import host, note
from test_gpu_sac_kernels import SacDevice

pytestmark = pytest.mark.gpu


def test_six_teacher_forced_updates_against_the_model_pipeline():
    import rlhip as rl

    dev = SacDevice()
    ns, h, b, lr, tau, seed = 3, 20, 65, 3e-3, 0.05, 11
    c = SC._build("learner", ns=ns, h=h, act=1, batch=b, seed=4242, scale=2.0, lo=0.05, hi=4.0)
    env = rl.PendulumEnv(SC.N_ENV, seed=1)
    pol = rl.SACPolicy(env, hidden=h, act="tanh", gamma=c["gamma"], tau=tau, alpha=c["alpha"], batchsize=b, update_after=SC.N_ENV, lr=lr,
                       lr_alpha=c["alpha_lr"], target_entropy=c["target_entropy"], min_sigma=c["lo"], max_sigma=c["hi"], seed=seed)
    assert pol.action_scale == 2.0 and pol.actor.numel() == c["actor"].size
    for t, src in ((pol.actor, c["actor"]), (pol.critics, c["critics"]), (pol.targets, c["targets"])):
        t.copy_(torch.tensor(src))
    # (the traces are filled directly: the controller is told of the pushes it did not see)
    traj = rl.Trajectory(dev.traces(c), controller=rl.InsertSampleRatioController(ratio=1e9, threshold=1, n_inserted=SC.PUSHES))
    oring = oracle.Ring(SC.CAP, SC.N_ENV, ns)
    oring.push_state(c["S"][0])
    for p in range(SC.PUSHES):
        oring.push_transition(c["S"][p + 1], np.zeros(SC.N_ENV, np.int32), c["Rw"][p], c["T"][p])
    worst = dict(q99=0.0, dmax=0.0)
    for u in range(6):
        before = {k: host(getattr(pol, k)).copy() for k in ("actor", "critics", "targets", "alpha")}
        mom = {k: (host(o.m).copy(), host(o.v).copy()) for k, o in (("actor", pol.actor_opt), ("critics", pol.critic_opt))}
        assert pol.optimise_(traj) is True and pol.n_updates == u + 1 and pol.vec_steps == u + 1
        idx = oring.sample_indices(b, seed + 1, u)
        assert np.array_equal(host(pol.last_idx.t), idx), f"update {u}: drawn indices differ"
        cu = dict(c, actor=before["actor"], critics=before["critics"], targets=before["targets"], alpha=float(before["alpha"][0]), idx=idx)
        li, e = idx // SC.N_ENV, idx % SC.N_ENV
        p = li + (SC.PUSHES - SC.CAP)
        cu["records"] = lambda p=p, e=e: (np.ascontiguousarray(c["S"][p, :, e].T), c["A"][p, e], c["Rw"][p, e], c["T"][p, e],
                                          np.ascontiguousarray(c["S"][p + 1, :, e].T))
        eps0, eps1 = R.draw_pair(dev.sample, b, seed + 1, u)
        rc = R.critic_replay(cu, eps0)
        assert_grad_close(host(pol.critic_grad), rc["grad"], F32_GRAD_TOL, f"sac pipeline u{u} critic gradient")
        assert_grad_close(host(pol.critic_loss), rc["loss"], F32_GRAD_TOL, f"sac pipeline u{u} critic loss")
        pc, (m, v) = before["critics"].copy(), mom["critics"]
        oracle.adam(pc, rc["grad"].astype(F32), m, v, lr, 0.9, 0.999, 1e-8, u + 1)
        stepped = host(pol.critics).copy()  # teacher-forced: the actor step reads the DEVICE's stepped critics (Polyak leaves them alone)
        ra = R.actor_replay(cu, eps1, critics=stepped)
        assert_grad_close(host(pol.actor_grad), ra["grad"], F32_GRAD_TOL, f"sac pipeline u{u} actor gradient")
        assert_grad_close(host(pol.actor_stats), ra["stats"], F32_GRAD_TOL, f"sac pipeline u{u} actor statistics")
        pa, (m, v) = before["actor"].copy(), mom["actor"]
        oracle.adam(pa, ra["grad"].astype(F32), m, v, lr, 0.9, 0.999, 1e-8, u + 1)
        pt = (F32(1.0 - tau) * before["targets"] + (F32(1) - F32(1.0 - tau)) * pc).astype(F32)
        for name, got, want, bar in (("critics", pol.critics, pc, 1.0), ("actor", pol.actor, pa, 1.0), ("targets", pol.targets, pt, tau)):
            d = np.abs(host(got) - want)
            q99, dmax = float(np.quantile(d, 0.99)), float(d.max())
            worst = dict(q99=max(worst["q99"], q99 / bar), dmax=max(worst["dmax"], dmax / bar))
            assert q99 <= 0.02 * lr * bar + 1e-7 and dmax <= 2.5 * lr * bar + 1e-7, f"update {u} {name}: |dp| q99 {q99:.2e} max {dmax:.2e}"
        assert abs(float(pol.alpha) - float(ra["alpha_new"])) <= 1e-6, f"update {u}: alpha {float(pol.alpha)!r} vs {float(ra['alpha_new'])!r}"
    note("SACPolicy pipeline vs model", updates=6, dp_q99_worst=worst["q99"], dp_max_worst=worst["dmax"])


def _build_agent(n=64, cap=64, seed=5, **kw):
    import rlhip as rl

    env = rl.PendulumEnv(n, seed=seed)
    args = dict(hidden=64, batchsize=64, update_after=5 * n, seed=seed)
    args.update(kw)
    pol = rl.SACPolicy(env, **args)
    traces = rl.CircularArraySARTSTraces(cap, n, 3, action_dtype=torch.float32)
    return env, rl.Agent(pol, rl.Trajectory(traces, controller=rl.InsertSampleRatioController(ratio=1e9, threshold=1)))


def _record_plans(pol):
    log, plan = [], pol.plan_

    def recording(env, **kw):
        a = plan(env, **kw)
        log.append(a.clone())
        return a

    pol.plan_ = recording
    return log


def test_run_stores_the_planned_actions_and_a_checkpoint_continues_bit_identically():
    import rlhip as rl

    env, agent = _build_agent(start_steps=3)
    pol, traces = agent.policy, agent.trajectory.container
    log = _record_plans(pol)
    rl.run(agent, env, rl.StopAfterNSteps(20))
    sd = rl.state_dict({"env": env, "agent": agent})
    assert any(k.endswith("policy/alpha") for k in sd) and any(k.endswith("actor_opt/m") for k in sd) and any(k.endswith("policy/targets") for k in sd)
    assert any(k.endswith("critic_opt/beta_pow") for k in sd) and any(k.endswith("policy/n_updates") for k in sd)
    rl.run(agent, env, rl.StopAfterNSteps(20))
    assert len(log) == 40 and pol.plan_steps == 40 and pol.vec_steps == 40 and pol.n_updates == 36  # 5 vec-steps of warm-up
    stored = traces.action[:40]
    assert stored.dtype == torch.float32
    assert torch.equal(stored, torch.stack(log)), "the ring's action words are not the planned Float32 actions"
    assert float(stored[:3].abs().max()) <= 2.0 and float(stored.abs().max()) <= 2.0
    s, a, r, t, sn = traces.gather(torch.arange(40 * 64, device="cuda"))
    assert a.dtype == torch.float32 and torch.equal(a.reshape(40, 64), stored)
    det = pol.plan_(env, deterministic=True)
    assert det.shape == (64,) and pol.plan_steps == 40 and float(det.abs().max()) <= 2.0
    env2, agent2 = _build_agent(start_steps=3)
    rl.load_state_dict({"env": env2, "agent": agent2}, sd)
    rl.run(agent2, env2, rl.StopAfterNSteps(20))
    p2 = agent2.policy
    for k in ("actor", "critics", "targets", "alpha", "actor_grad", "critic_grad"):
        assert torch.equal(getattr(pol, k), getattr(p2, k)), f"{k} differs after the checkpoint round trip"
    for o, o2 in ((pol.actor_opt, p2.actor_opt), (pol.critic_opt, p2.critic_opt)):
        assert torch.equal(o.m, o2.m) and torch.equal(o.v, o2.v) and torch.equal(o.beta_pow, o2.beta_pow)
    assert torch.equal(traces.records, agent2.trajectory.container.records) and torch.equal(env.state(), env2.state())
    assert (p2.n_updates, p2.vec_steps, p2.plan_steps) == (36, 40, 40)


class _LastRewards:
    """mean reward per step of every env over the vec-steps after `start` (accumulated on the device)"""

    def __init__(self, n, start):
        self.sum, self.start, self.t, self.k = torch.zeros(n, dtype=torch.float64, device="cuda"), start, 0, 0

    def push_(self, stage, policy, env):
        if stage == "PostActStage":
            self.t += 1
            if self.t > self.start:
                self.sum += env.reward().to(torch.float64)
                self.k += 1

    def per_env(self):
        return (self.sum / self.k).cpu().numpy()


LEARN_STEPS = 3000


def test_it_learns_pendulum():
    """SAC on 64 Pendulum envs against RandomPolicy on the same env and seed: the mean reward per step over the last 200 vec-steps must
    exceed the random policy's by more than 3 standard errors of the random policy's per-env means."""
    import rlhip as rl

    n = 64
    env, agent = _build_agent(n=n, cap=1024, seed=3, batchsize=256, hidden=64, update_after=10 * n, start_steps=10)
    hook = _LastRewards(n, LEARN_STEPS - 200)
    rl.run(agent, env, rl.StopAfterNSteps(LEARN_STEPS), hook)
    renv = rl.PendulumEnv(n, seed=3)
    rhook = _LastRewards(n, LEARN_STEPS - 200)
    rl.run(rl.RandomPolicy(seed=3), renv, rl.StopAfterNSteps(LEARN_STEPS), rhook)
    sac, rnd = hook.per_env(), rhook.per_env()
    se = float(rnd.std(ddof=1) / np.sqrt(n))
    print(f"SAC mean reward per step over the last 200 of {LEARN_STEPS} vec-steps: {sac.mean():.4f}; RandomPolicy: {rnd.mean():.4f} "
          f"(standard error {se:.4f}); updates {agent.policy.n_updates}, alpha {float(agent.policy.alpha):.4f}")
    note("SAC learns Pendulum", sac=float(sac.mean()), random=float(rnd.mean()), se=se, vec_steps=LEARN_STEPS)
    assert hook.k == 200 and agent.policy.n_updates > LEARN_STEPS - 20
    assert sac.mean() > rnd.mean() + 3.0 * se, f"SAC {sac.mean():.4f} does not exceed random {rnd.mean():.4f} by 3 x {se:.4f}"
