"""DQNLearner / QBasedPolicy on observations of six components (frame-layout rings; csrc/dqn_batch.hip), against the oracle.

  pipeline   a frame ring (capacity 24 < the 30 + 8 pushes: wrapped, 64 envs, obs_dim 6) filled through the push ABI together with
             oracle.Ring and the list model of tests/per_frames_nstep_ref.py from the same arrays; 8 updates, each teacher-forced
             (the reference starts every update from the GPU's parameters / moments / target) against the oracle sequence
             draw -> gather -> model gradient (tests/dqn_batch_ref.py) -> clip -> Adam -> target sync:
               drawn indices / keys / priorities equal; the gathered batch equal; gradients F32_GRAD_TOL; written-back priorities
               rtol 1e-3, atol 1e-6 (tests/test_gpu_per_nstep.py); parameters after each step q99 <= 0.02 lr, max <= 2.5 lr
               (test_fused_dqn_vec_step_teacher_forced_vs_oracle, layers = 2)
             for uniform 1-step, uniform n_step = 3, prioritized with beta > 0, prioritized n_step = 3, Double DQN, a dueling net
  agent      rlhip.run on AcrobotRK4Env, 256 envs x 40 vec-steps, teacher-forced against oracle.DQNRun(kind="acrobot", ns=6, na=3):
             counters equal, decisive plan! decisions equal, env states within the bar tests/test_gpu_parity.py uses for Acrobot
             (rtol 2e-6, atol 1e-7), parameters under the same per-step bars; one checkpoint round trip in the middle continues
             bit-identically
  it learns  DQN on AcrobotRK4Env against the random policy on the oracle's env (test_dqn_learns_acrobot)"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import oracle  # noqa: E402
import dqn_batch_ref as ref  # noqa: E402
import dueling_ref  # noqa: E402
from conftest import F32_GRAD_TOL, assert_grad_close  # noqa: E402
from per_frames_nstep_ref import PrioritizedFramesRef  # noqa: E402
from test_gpu_bench_shapes import dev, host, note  # noqa: E402

MODES = {
    "uniform": {},
    "nstep3": dict(n_step=3),
    "per-beta": dict(per=True, per_beta=0.4),
    "per-nstep3": dict(per=True, per_beta=0.4, n_step=3),
    "double": dict(double_dqn=True),
    "dueling": dict(dueling=True),
    "per-nstep3-double-dueling": dict(per=True, per_beta=0.4, n_step=3, double_dqn=True, dueling=True),
}


@pytest.mark.parametrize("mode", list(MODES))
def test_learner_pipeline_on_a_frame_ring_vs_oracle(mode):
    import rlhip as rl

    kw = MODES[mode]
    per, n_step, double, dueling, beta = kw.get("per", False), kw.get("n_step", 1), kw.get("double_dqn", False), kw.get("dueling", False), \
        kw.get("per_beta", 0.0)
    n, cap, od, h, na, b = 64, 24, 6, 64, 3, 96
    gamma, lr, clip, seed, sync, prio0 = 0.97, 1e-3, 0.5, 7, 3, 2.5
    rng = np.random.default_rng(len(mode) + 100 * n_step)
    net = (rl.DuelingApproximator if dueling else rl.HipApproximator)(od, h, na, seed=3, lr=lr)
    tn = rl.TargetNetwork(net, sync_freq=sync)
    learner = rl.DQNLearner(tn, batchsize=b, gamma=gamma, min_replay_history=n, seed=seed, n_step=n_step, double_dqn=double, per_beta=beta,
                            max_grad_norm=clip)
    traces = rl.CircularPrioritizedFrameTraces(cap, n, od, default_priority=prio0, n_step=n_step) if per else \
        rl.CircularArraySARTSTraces(cap, n, od)
    assert not traces.records_layout
    traj = rl.Trajectory(traces)
    model = PrioritizedFramesRef(cap, n, od, np.float32, n_step, prio0)
    oring = oracle.Ring(cap, n, od)

    def push():
        f = rng.standard_normal((od, n)).astype(np.float32)
        a, r, t = rng.integers(0, na, n).astype(np.int32), rng.standard_normal(n).astype(np.float32), (rng.random(n) < 0.2).astype(np.uint8)
        traj.push_transition_(dev(f), dev(a), dev(r), dev(t))
        model.push_transition(f, a, r, t)
        oring.push_transition(f, a, r, t)

    f0 = rng.standard_normal((od, n)).astype(np.float32)
    traj.push_state_(dev(f0)), model.push_state(f0), oring.push_state(f0)
    for _ in range(30):
        push()
    n_opt, worst = 0, dict(q99=0.0, dmax=0.0)
    for u in range(8):
        push()
        trained = "dueling_params" if dueling else "params"
        p_eff, pt_eff = host(net.params).copy(), host(tn.target).copy()
        p, m, v = host(getattr(net, trained)).copy(), host(net.m).copy(), host(net.v).copy()
        ctr = learner.draw_ctr
        assert learner.optimise_(traj) is True and learner.n_updates == u + 1 and learner.draw_ctr == ctr + 1
        # draw
        if per:
            idx, key, prio = model.draw(b, seed, ctr)
            assert np.array_equal(host(learner._key), key) and np.array_equal(host(learner._prio), prio)
        elif n_step > 1:
            idx = oracle.ring_sample_indices_nstep(oring, b, n_step, seed, ctr)
        else:
            idx = oring.sample_indices(b, seed, ctr)
        assert np.array_equal(host(learner._idx), idx), f"update {u}: drawn indices differ"
        # gather
        rows = [model.nstep_transition(*divmod(int(j), n), n_step, gamma) for j in idx]
        s, sn = np.stack([x[0] for x in rows], 1), np.stack([x[4] for x in rows], 1)
        a, ret, t, nu = (np.array([x[k] for x in rows], dt) for k, dt in ((1, np.int32), (2, np.float32), (3, np.uint8), (5, np.int32)))
        if not per:  # the oracle's gather says the same as the list model
            og = oracle.ring_gather_nstep(oring, idx, n_step, gamma) if n_step > 1 else oring.gather(idx)
            for x, y in zip((s, a, ret, t, sn), og):
                assert np.array_equal(x, y)
        gs, ga, gr, gt, gsn, gnu = learner._batch.t
        assert np.array_equal(host(gs), s) and np.array_equal(host(gsn), sn) and np.array_equal(host(ga), a) and np.array_equal(host(gt), t)
        np.testing.assert_allclose(host(gr), ret, rtol=1e-6, atol=1e-7)
        one_step_uniform = not per and n_step == 1
        assert (gnu is None) if one_step_uniform else np.array_equal(host(gnu), nu)
        # gradient
        w = oracle.per_is_weights(prio, beta) if per and beta > 0 else None
        loss, g_eff, td = ref.loss_grad(od, h, na, 0, p_eff, pt_eff, s, a, ret, t, sn, gamma, 1.0, None if one_step_uniform else nu, w, double)
        g = dueling_ref.unfold(g_eff, od, h, na, 2) if dueling else g_eff.copy()
        oracle.clip_by_global_norm(g, clip)
        if dueling:
            assert_grad_close(host(learner.grad), g_eff, F32_GRAD_TOL, f"obsn pipeline {mode} u{u} effective gradient")
            assert_grad_close(host(net._grad.t), g, F32_GRAD_TOL, f"obsn pipeline {mode} u{u} dueling gradient")
        else:
            for name, part in ref.split(host(learner.grad), od, h, na).items():
                assert_grad_close(part, ref.split(g, od, h, na)[name], F32_GRAD_TOL, f"obsn pipeline {mode} u{u} {name}")
        assert abs(float(learner.loss) - loss) <= 1e-4 * max(abs(loss), 1e-6)
        # priority write-back
        if per:
            np.testing.assert_allclose(host(learner.td), oracle.per_priority(td, learner.per_eps, learner.per_alpha), rtol=1e-3, atol=1e-6)
            model.st.update(key, host(learner.td))  # the reference tree takes the GPU's values: the write-back itself is compared bit for bit
            assert np.array_equal(host(traces.priorities), model.st.tree)
        # Adam, target sync
        oracle.adam(p, g, m, v, lr, 0.9, 0.999, 1e-8, u + 1)
        d = np.abs(host(getattr(net, trained)) - p)
        q99, dmax = float(np.quantile(d, 0.99)), float(d.max())
        worst = dict(q99=max(worst["q99"], q99), dmax=max(worst["dmax"], dmax))
        assert q99 <= 0.02 * lr and dmax <= 2.5 * lr, f"update {u}: |dp| q99 {q99:.2e} max {dmax:.2e}"
        due, n_opt = oracle.target_sync_due(n_opt, sync)
        assert tn.n_optimise == n_opt
        if due:
            gt_ = host(tn.target_dueling if dueling else tn.target)
            assert np.abs(gt_ - p).max() <= dmax + 1e-12
    note(f"DQNLearner on a frame ring vs oracle, {mode}", updates=8, dp_q99_worst=worst["q99"], dp_max_worst=worst["dmax"])


def test_agent_loop_on_acrobot_teacher_forced_vs_oracle(tmp_path):
    import rlhip as rl

    n, cap, K, batch, h, sync, lr = 256, 16, 40, 128, 128, 10, 1e-3

    def build():
        env = rl.AcrobotRK4Env(n, seed=9)
        net = rl.HipApproximator(6, h, 3, seed=9)
        tn = rl.TargetNetwork(net, sync_freq=sync)
        learner = rl.DQNLearner(tn, batchsize=batch, min_replay_history=n, seed=9)
        explorer = rl.EpsilonGreedyExplorer(0.01, kind="exp", decay_steps=20, seed=9)
        policy = rl.QBasedPolicy(learner, explorer)
        traces = rl.CircularArraySARTSTraces(capacity=cap, n_env=n, obs_dim=6)
        return env, rl.Agent(policy, rl.Trajectory(traces))

    env, agent = build()
    policy, traces = agent.policy, agent.trajectory.container
    learner, explorer = policy.learner, policy.explorer
    tn = learner.approximator
    net = tn.network
    o = oracle.DQNRun(kind="acrobot", n=n, ns=6, na=3, hidden=h, env_seed=9, net_seed=9, explorer_seed=9, sampler_seed=9, capacity=cap,
                      batch=batch, sync_freq=sync, decay_steps=20)
    assert np.array_equal(host(net.params), o.params)
    near_ties, worst_q99, worst_max, worst_state = 0, 0.0, 0.0, 0.0
    twin = None
    for k in range(K):
        if k == K // 2:  # a checkpoint round trip: a fresh agent loaded from the file continues bit-identically to the end
            path = str(tmp_path / "acrobot_dqn.npz")
            rl.save_checkpoint(path, dict(agent=agent, env=env))
            env2, agent2 = build()
            rl.load_checkpoint(path, dict(agent=agent2, env=env2), strict=False)
            twin = (env2, agent2)
        o.env.set_state([host(env.raw_state()[j]) for j in range(4)], host(env._t))
        o.env.episode[:] = host(env._episode).view(np.uint32)
        o.env.done[:] = host(env._done)
        for dst, src in ((o.params, net.params), (o.target, tn.target), (o.m, net.m), (o.v, net.v)):
            dst[:] = host(src)
        rl.run(agent, env, rl.StopAfterNSteps(1))
        if twin is not None:
            rl.run(twin[1], twin[0], rl.StopAfterNSteps(1))
        ga = host(policy._actions).astype(np.int32)
        o.vec_step(force_actions=ga)
        # plan!
        gq = host(policy._q)
        assert np.all(np.abs(gq - o.last_q) <= 5e-6 * (1 + np.abs(o.last_q)))
        srt = np.sort(o.last_q, axis=0)
        decisive = (srt[-1] - srt[-2]) > 1e-6 * (1 + np.abs(o.last_q).max(0))
        near_ties += int((~decisive).sum())
        assert np.array_equal(ga[decisive], o.last_plan[decisive]), f"vec-step {k}: a decisive plan! differs"
        # act!
        assert np.array_equal(host(env._t), o.env.t) and np.array_equal(host(env._done), o.env.done)
        assert np.array_equal(host(env.reward()), o.env.reward.astype(np.float32))
        for j in range(4):
            np.testing.assert_allclose(host(env.raw_state()[j]), o.env.s[j], rtol=2e-6, atol=1e-7)
            worst_state = max(worst_state, float(np.abs(host(env.raw_state()[j]) - o.env.s[j]).max()))
        # optimise!
        assert (learner.n_updates, learner.draw_ctr, explorer.step, tn.n_optimise) == (o.n_updates, o.draw_ctr, o.explorer_step, o.n_optimise)
        assert learner.n_updates == k + 1
        d = np.abs(host(net.params) - o.params)
        q99, dmax = float(np.quantile(d, 0.99)), float(d.max())
        worst_q99, worst_max = max(worst_q99, q99), max(worst_max, dmax)
        assert q99 <= 0.02 * lr and dmax <= 2.5 * lr, f"vec-step {k}: |dp| q99 {q99:.2e} max {dmax:.2e}"
        assert np.abs(host(tn.target) - o.target).max() <= dmax + 1e-12
    for name in ("head_sa", "len_sa", "head_rt", "len_rt"):
        assert getattr(traces.rb, name) == getattr(o.ring.rb, name), name
    idx = np.arange(cap * n, dtype=np.int64)
    gs, g_a, gr, gt, gsn = (host(x) for x in traces.gather(torch.as_tensor(idx).cuda()))
    os_, oa, or_, ot, osn = o.ring.gather(idx)
    assert np.array_equal(g_a, oa) and np.array_equal(gr, or_) and np.array_equal(gt, ot)
    np.testing.assert_allclose(gs, os_, rtol=2e-6, atol=1e-6)
    # the twin that was loaded from the checkpoint ended where the original did, bit for bit
    env2, agent2 = twin
    l2 = agent2.policy.learner
    for x, y in ((net.params, l2.approximator.network.params), (tn.target, l2.approximator.target), (net.m, l2.approximator.network.m),
                 (net.v, l2.approximator.network.v), (env._s, env2._s), (traces.state, agent2.trajectory.container.state),
                 (traces.reward, agent2.trajectory.container.reward), (policy._actions, agent2.policy._actions)):
        assert torch.equal(x, y)
    assert (l2.n_updates, l2.draw_ctr, agent2.policy.explorer.step) == (learner.n_updates, learner.draw_ctr, explorer.step)
    note("DQN agent loop on AcrobotRK4Env teacher-forced vs oracle", vec_steps=K, envs=n, near_tie_decisions=near_ties, decisions=K * n,
         dp_q99_worst_step=worst_q99, dp_max_worst_step=worst_max, env_state_err_max=worst_state)


def _random_policy_episode_length(seed, n=256, steps=3000):
    """mean length of the episodes a uniformly random policy finishes on the oracle's Acrobot (CPU)"""
    env = oracle.VecEnv("acrobot", n, seed=seed)
    rng = np.random.default_rng(seed)
    t, lens = np.zeros(n, np.int64), []
    for _ in range(steps):
        env.step(rng.integers(0, 3, n).astype(np.int32))
        t += 1
        d = env.done.astype(bool)
        lens += t[d].tolist()
        t[d] = 0
    return float(np.mean(lens))


def test_dqn_learns_acrobot():
    """DQN (6 -> 128 -> 3, n_step = 3, Double DQN, batch 512, one update per vec-step) through rlhip.run on AcrobotRK4Env, budget fixed at
    256 envs x 2400 vec-steps (0.6 s on the device).

    Yardstick: the random policy's mean episode length on oracle.VecEnv("acrobot"), five seeds on the CPU -- 201.0, 201.0, 200.9975,
    201.0, 201.0 (an episode the policy does not solve ends at max_steps = 200, which reads 201 steps): mean 200.9995, seed-to-seed
    spread (sample standard deviation) 0.0011.  The trained agent's mean episode length over its last window (the episodes that end in
    the last quarter of the run) has to lie below mean - 3 x spread = 200.996.
    Measured curve of the trained agent, eight windows of 300 vec-steps: 201.0, 192.97, 168.79, 177.27, 182.75, 183.15, 182.91, 183.11
    (profiles/dqn_obsn.md)."""
    import rlhip as rl

    control = [_random_policy_episode_length(seed) for seed in range(5)]
    mean, spread = float(np.mean(control)), float(np.std(control, ddof=1))
    n, K = 256, 2400
    env = rl.AcrobotRK4Env(n, seed=1)
    net = rl.HipApproximator(6, 128, 3, seed=1, lr=1e-3)
    learner = rl.DQNLearner(rl.TargetNetwork(net, sync_freq=100), batchsize=512, gamma=0.99, min_replay_history=n * 8, seed=1, n_step=3,
                            double_dqn=True)
    explorer = rl.EpsilonGreedyExplorer(0.02, kind="exp", decay_steps=400, seed=1)
    agent = rl.Agent(rl.QBasedPolicy(learner, explorer), rl.Trajectory(rl.CircularArraySARTSTraces(capacity=512, n_env=n, obs_dim=6)))
    hook = rl.DeviceEpisodeStats(n)
    rl.run(agent, env, rl.StopAfterNSteps(K), hook)
    rec = hook.records()
    last = rec["steps"][rec["vec_step"] >= K - K // 4]
    trained = float(last.mean())
    note("DQN learns AcrobotRK4Env", control_mean=mean, control_spread=spread, threshold=mean - 3 * spread, trained_last_window=trained,
         episodes_last_window=int(last.size), updates=learner.n_updates)
    print(f"control {control} -> mean {mean:.4f}, spread {spread:.4f}; trained, last window: {trained:.2f} over {last.size} episodes")
    assert last.size >= 100 and trained < mean - 3 * spread, (trained, mean, spread)
