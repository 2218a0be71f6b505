"""Prioritized n-step replay on the device: rlhip_ring_push_priority_nstep (the validity mask kept in the sum-tree),
rlhip_per_sample_fold_nstep_f32 (prioritized draw + window fold in one launch, csrc/per_nstep.hip) and DQNLearner(n_step = 3) on
CircularPrioritizedTraces(n_step = 3) -- against the two shipped launches on the GPU and against the composition of the oracle's
existing functions (tests/per_nstep_ref.py).

Bars (none of them new):
  trees, indices, keys, priorities, iota, folded records    bit for bit
  gradients    F32_GRAD_TOL on the whole vector / BF16_GRAD_TOL per tensor (tests/conftest.py), as tests/test_gpu_nstep.py:113,123 --
               taken at the GPU's own parameters before the update
  written-back priorities    rtol 1e-3 (two-layer) / 2e-2 (three-layer), atol 1e-6: tests/test_gpu_double_dqn.py:311
  learner parameters, free-running    |dp| q99 < 0.2 lr (two-layer) / 2 lr (three-layer), max < K 2 lr: tests/test_gpu_double_dqn.py:324"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import dueling_ref as dr  # noqa: E402
import oracle  # noqa: E402
from conftest import BF16_GRAD_TOL, F32_GRAD_TOL, assert_grad_close  # noqa: E402
from per_nstep_ref import Mirror, learner_update, record_words, sample_fold  # noqa: E402
from test_gpu_bench_shapes import dev, host, note  # noqa: E402

GAMMA = 0.97
DEFAULT = 2.5
TILE = 64  # FOLD_TILE of csrc/fold_device.h: batches 1, TILE, TILE + 1


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def _small_ring(rl, ns, n_step, pushes, cap=8, n_env=3, seed=0):
    """capacity 8 x 3 envs through the push ABI, mirrored into the oracle after every push (tree compared bit for bit each time).
    Terminal flags: env 0 ends on the NEWEST frame, env 1 two frames before it (windows that end early), env 2 at random."""
    rng = np.random.default_rng(seed + 10 * ns + n_step)
    tr = rl.CircularPrioritizedTraces(capacity=cap, n_env=n_env, obs_dim=ns, default_priority=DEFAULT, n_step=n_step)
    m = Mirror(cap, n_env, ns, n_step, DEFAULT)
    obs = rng.standard_normal((ns, n_env)).astype(np.float32)
    tr.push_state_(dev(obs))
    m.push_state(obs)
    for k in range(pushes):
        nobs = rng.standard_normal((ns, n_env)).astype(np.float32)
        a = rng.integers(0, 2, n_env).astype(np.int32)
        r = (rng.standard_normal(n_env) * 2).astype(np.float32)
        t = np.array([k == pushes - 1, k == pushes - 3, rng.random() < 0.3], np.uint8)
        tr.push_transition_(dev(nobs), dev(a), dev(r), dev(t))
        m.push_transition(nobs, a, r, t)
        assert np.array_equal(_bits(host(tr.priorities)), _bits(m.st.tree)), f"tree after push {k + 1}"
    return tr, m


@pytest.mark.parametrize("pushes", [5, 8, 13], ids=["not_full", "exactly_full", "wrapped"])
@pytest.mark.parametrize("n_step", [1, 3, 8])
@pytest.mark.parametrize("ns", [2, 4])
def test_masked_push_and_fused_draw_fold_bit_exact(ns, n_step, pushes):
    import rlhip as rl
    from rlhip._lib import RLHipArgumentError

    tr, m = _small_ring(rl, ns, n_step, pushes)
    cap, n_env = tr.capacity, tr.n_env
    if n_step == 1:  # the shipped push leaves the same tree
        plain = oracle.SumTree(cap * n_env)
        plain.fill_range(0, min(pushes, cap) * n_env, DEFAULT)
        assert np.array_equal(_bits(host(tr.priorities)), _bits(plain.tree))
    smp = rl.NStepBatchSampler(n_step, GAMMA, 4, seed=9)
    if len(tr) < n_step:  # 5 pushes, n_step = 8: the masked tree has no mass
        assert tr.total_priority() == 0.0
        with pytest.raises(RLHipArgumentError, match="fewer than n_step"):
            smp.sample_fold_prioritized(tr, 0)
        torch.cuda.synchronize()
        return
    # non-uniform priorities, one of them zero, under keys drawn from the masked tree (a masked leaf is never drawn)
    _, key, _ = oracle.ring_sample_prioritized(m.ring, m.st, 5, 3, 0)
    newp = np.array([0.0, 0.3, 7.0, 1.25, 4.0], np.float32)
    tr.set_priority_(dev(key), dev(newp))
    m.st.update(key, newp)
    assert np.array_equal(_bits(host(tr.priorities)), _bits(m.st.tree))
    for batch in (1, TILE, TILE + 1):
        smp = rl.NStepBatchSampler(n_step, GAMMA, batch, seed=9)
        two = rl.NStepBatchSampler(n_step, GAMMA, batch, seed=9)
        for ctr in (0, 3):
            folded, iota, idx, k1, p1 = smp.sample_fold_prioritized(tr, ctr)
            idx2 = two.sample_indices(tr, ctr)            # rlhip_ring_sample_prioritized ...
            folded2, iota2 = two.fold(tr, idx2)           # ... then rlhip_ring_fold_nstep
            torch.cuda.synchronize()
            oidx, okey, oprio, sarts = sample_fold(m.ring, m.st, batch, n_step, GAMMA, 9, ctr)
            assert (oidx // n_env).max() <= len(m.ring) - n_step and np.all(oprio > 0)
            for name, got, gpu2, ref in (("idx", idx, idx2, oidx), ("key", k1, two.key, okey), ("prio", p1, two.priority, oprio),
                                         ("iota", iota, iota2, np.arange(batch))):
                assert np.array_equal(host(got), host(gpu2)), f"{name}: fused != two launches (batch {batch}, draw {ctr})"
                assert np.array_equal(_bits(host(got)), _bits(np.asarray(ref, host(got).dtype))), f"{name}: fused != oracle"
            rec = host(folded.records.view(torch.int32)[0]).view(np.uint32)
            assert np.array_equal(rec, host(folded2.records.view(torch.int32)[0]).view(np.uint32)), "records: fused != two launches"
            assert np.array_equal(rec, record_words(ns, *sarts)), "records: fused != oracle"
            assert len(folded) == 1 and folded.n_env == batch
    # nullable outputs
    from rlhip._lib import call
    from rlhip.ops import ptr, stream_ptr

    idx3 = torch.empty(batch, dtype=torch.int64, device="cuda")
    call("rlhip_per_sample_fold_nstep_f32", C.byref(tr.rb), ptr(tr.priorities), batch, n_step, GAMMA, 9, 3, ptr(idx3), None, None,
         C.byref(folded2.rb), None, stream_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(host(idx3), oidx) and np.array_equal(host(folded2.records.view(torch.int32)[0]).view(np.uint32), rec)
    # the sampler's dictionary form
    b = rl.NStepBatchSampler(n_step, GAMMA, batch, seed=9)
    b.draw_ctr = 3
    d = b.sample(tr)
    assert np.array_equal(host(d["key"]), okey) and np.array_equal(host(d["priority"]), oprio) and b.draw_ctr == 4
    assert np.array_equal(host(d["reward"]), sarts[2]) and np.array_equal(host(d["action"]), sarts[1] + 1)


def test_fused_draw_fold_at_the_longest_window():
    """n_step = 32, the bound of the ABI: capacity 34 x 4 envs, 40 pushes (head_sa = 6: a 32-step window crosses the state trace's
    wrap slot), terminal flags written here -- env 0 never ends, env e ends every 3 + 2 e pushes.  The one launch against the two
    shipped launches byte for byte; the conditions on the drawn windows are asserted on the two launches' index list first
    (rlhip_ring_fold_nstep is pinned to the oracle at n_step = 32 by tests/test_gpu_nstep.py)."""
    import rlhip as rl

    ns, n_step, batch, cap, n_env, pushes = 4, 32, 37, 34, 4, 40
    rng = np.random.default_rng(32)
    tr = rl.CircularPrioritizedTraces(capacity=cap, n_env=n_env, obs_dim=ns, default_priority=DEFAULT, n_step=n_step)
    tr.push_state_(dev(rng.standard_normal((ns, n_env)).astype(np.float32)))
    flags = np.array([[e > 0 and k % (3 + 2 * e) == 0 for e in range(n_env)] for k in range(pushes)], np.uint8)
    for k in range(pushes):
        tr.push_transition_(dev(rng.standard_normal((ns, n_env)).astype(np.float32)), dev(rng.integers(0, 2, n_env).astype(np.int32)),
                            dev((rng.standard_normal(n_env) * 2).astype(np.float32)), dev(flags[k]))
    assert len(tr) == cap and tr.rb.head_sa == 6
    two = rl.NStepBatchSampler(n_step, GAMMA, batch, seed=9)
    idx2 = two.sample_indices(tr, 3)            # rlhip_ring_sample_prioritized ...
    folded2, iota2 = two.fold(tr, idx2)         # ... then rlhip_ring_fold_nstep
    torch.cuda.synchronize()
    li, e = host(idx2) // n_env, host(idx2) % n_env
    assert li.min() >= 0 and li.max() <= cap - n_step
    # logical step li is push li + pushes - cap; a window is cut short by a terminal flag before its last step
    cut = np.array([flags[l + pushes - cap:l + pushes - cap + n_step - 1, v].any() for l, v in zip(li, e)])
    assert (e == 0).any() and not cut[e == 0].any(), "no window of the full 32 steps (env 0) was drawn"
    assert tr.rb.head_sa + li[e == 0].min() <= cap < tr.rb.head_sa + li[e == 0].min() + n_step, "no wrap inside it"
    assert cut.any(), "no drawn window is cut short by a terminal"
    folded, iota, idx, key, prio = rl.NStepBatchSampler(n_step, GAMMA, batch, seed=9).sample_fold_prioritized(tr, 3)
    torch.cuda.synchronize()
    for name, got, ref in (("idx", idx, idx2), ("key", key, two.key), ("prio", prio, two.priority), ("iota", iota, iota2)):
        assert torch.equal(got, ref), f"{name}: fused != two launches"
    rec, rec2 = folded.records.view(torch.int32)[0], folded2.records.view(torch.int32)[0]
    differing = (rec != rec2).any(1).nonzero().flatten().tolist()
    assert not differing, f"records {differing[:8]} differ: fused {rec[differing[0]].tolist()} two launches {rec2[differing[0]].tolist()}"
    assert host(rec[:, 6])[e == 0].max() == 0 and host(rec[:, 6])[cut].min() == 1  # the folded terminal flag says the same


# ------------------------------------------------------------------------------------------------------------------ the learner
def _cartpole_ring(rl, n_step, n_env=16, cap=16, pushes=21, seed=0):
    """a wrapped 16-env CartPole ring of real transitions under random actions, mirrored into the oracle with its masked tree"""
    env = rl.HipVecEnv("cartpole", n_env, continuous=False, seed=seed + 1)
    tr = rl.CircularPrioritizedTraces(capacity=cap, n_env=n_env, obs_dim=4, default_priority=DEFAULT, n_step=n_step)
    m = Mirror(cap, n_env, 4, n_step, DEFAULT)
    g = torch.Generator(device="cpu").manual_seed(seed)
    obs = env.state().to(torch.float32)
    tr.push_state_(obs)
    m.push_state(host(obs))
    for _ in range(pushes):
        a0 = torch.randint(0, 2, (n_env,), generator=g, dtype=torch.int32).cuda()
        env.act0_(a0)
        nobs, r, t = env.state().to(torch.float32), env.reward().to(torch.float32), env._done
        tr.push_transition_(nobs, a0, r, t)
        m.push_transition(host(nobs), host(a0), host(r), host(t))
    torch.cuda.synchronize()
    return tr, m


CONFIGS = {"two_layer_beta0": dict(layers=2, h=64, beta=0.0), "two_layer_beta04": dict(layers=2, h=64, beta=0.4),
           "double_dqn": dict(layers=2, h=64, beta=0.4, double=True), "dueling": dict(layers=2, h=64, beta=0.4, dueling=True),
           "three_layer_h128": dict(layers=3, h=128, beta=0.4)}


@pytest.mark.parametrize("name", list(CONFIGS))
def test_learner_three_updates_vs_oracle_loop(name):
    import rlhip as rl

    cfg = CONFIGS[name]
    layers, h, beta, double, dueling = cfg["layers"], cfg["h"], cfg["beta"], cfg.get("double", False), cfg.get("dueling", False)
    ns, na, act, K, lr, batch, n_step, seed = 4, 2, 0, 3, 1e-3, 32, 3, 5
    tr, m = _cartpole_ring(rl, n_step)
    traj = rl.Trajectory(tr)
    traj.controller.on_insert_(10 ** 6)
    cls = rl.DuelingApproximator if dueling else rl.HipApproximator
    net = cls(ns, h, na, seed=seed, layers=layers, lr=lr)
    tn = rl.TargetNetwork(net, sync_freq=2)
    learner = rl.DQNLearner(tn, batchsize=batch, gamma=GAMMA, min_replay_history=1, seed=seed, max_grad_norm=0.5, n_step=n_step,
                            per_beta=beta, double_dqn=double)
    gamma_n = oracle.gamma_pow(GAMMA, n_step)
    assert learner._nstep.gamma_n == gamma_n
    trained = (lambda: host(net.dueling_params)) if dueling else (lambda: host(net.params))
    p, pt = trained().copy(), (host(tn.target_dueling) if dueling else host(tn.target)).copy()
    p0 = p.copy()
    mom, vel, n_opt = np.zeros_like(p), np.zeros_like(p), 0
    eff = (lambda x: dr.fold(x, ns, h, na, layers)) if dueling else (lambda x: x)
    tol = F32_GRAD_TOL if layers == 2 else BF16_GRAD_TOL
    # two-layer: the whole vector (tests/test_gpu_nstep.py:113); three-layer: per tensor (:121-124)
    sizes = [("W1", h * ns), ("b1", h), ("W2", h * h), ("b2", h), ("W3", na * h), ("b3", na)] if layers == 3 else [("all", p.size)]
    for k in range(K):
        assert np.array_equal(_bits(host(tr.priorities)), _bits(m.st.tree)), f"update {k}: trees differ before the draw"
        idx, key, prio, sarts = sample_fold(m.ring, m.st, batch, n_step, GAMMA, seed, k)
        assert (idx // tr.n_env).max() <= len(m.ring) - n_step
        pe_gpu, pte_gpu = host(net.params).copy(), host(tn.target).copy()   # the vectors the kernels read in this update
        assert learner.optimise_(traj)
        torch.cuda.synchronize()
        assert np.array_equal(host(learner._idx), idx), f"update {k}: other window starts drawn"
        assert np.array_equal(host(learner._key), key) and np.array_equal(_bits(host(learner._prio)), _bits(prio))
        # the gradient entry and the written-back priorities at the GPU's own parameters
        g_tf, prio_tf = learner_update(layers, ns, h, na, act, pe_gpu, pte_gpu, sarts, gamma_n, prio, beta, double)
        if not dueling:  # rlhip_clip_adam_f32 clips learner.grad in place (a dueling net clips the unfolded copy instead)
            oracle.clip_by_global_norm(g_tf, 0.5)
        o = 0
        for tname, n in sizes:
            assert_grad_close(host(learner.grad)[o:o + n], g_tf[o:o + n], tol, f"per n-step {name} update {k} {tname}")
            o += n
        np.testing.assert_allclose(host(learner.td), prio_tf, rtol=1e-3 if layers == 2 else 2e-2, atol=1e-6)
        m.st.update(key, host(learner.td))   # the reference tree takes the GPU's values: the write-back itself is compared bit for bit
        assert np.array_equal(_bits(host(tr.priorities)), _bits(m.st.tree)), f"update {k}: written-back tree differs"
        # the free-running oracle loop
        g, _ = learner_update(layers, ns, h, na, act, eff(p), eff(pt), sarts, gamma_n, prio, beta, double)
        if dueling:
            g = dr.unfold(g, ns, h, na, layers)
        oracle.clip_by_global_norm(g, 0.5)
        oracle.adam(p, g, mom, vel, lr, 0.9, 0.999, 1e-8, k + 1)
        due, n_opt = oracle.target_sync_due(n_opt, 2)
        if due:
            oracle.polyak(pt, p, 0.0)
    d = np.abs(trained() - p)
    q99, dmax = float(np.quantile(d, 0.99)), float(d.max())
    note("DQNLearner(n_step=3) on prioritized traces x 3 vs oracle loop", config=name, dp_q99=q99, dp_max=dmax,
         moved_q50=float(np.median(np.abs(p - p0))))
    print(f"{name}: |dp| q99 {q99:.3e} max {dmax:.3e}")
    assert learner.n_updates == K and np.median(np.abs(p - p0)) > lr  # (tests/test_gpu_double_dqn.py:323)
    assert q99 < (0.2 if layers == 2 else 2.0) * lr and dmax < K * 2 * lr
    assert np.abs((host(tn.target_dueling) if dueling else host(tn.target)) - pt).max() <= dmax + 1e-12


def test_checkpoint_resume_is_bit_identical(tmp_path):
    """save mid-run, restore into fresh objects (traces constructed WITHOUT the mask: the field travels), continue"""
    import rlhip

    def build(seed, traces_n_step):
        n = 16
        env = rlhip.CartPoleEnv(n, seed=seed)
        net = rlhip.HipApproximator(4, 64, 2, seed=seed)
        learner = rlhip.DQNLearner(rlhip.TargetNetwork(net, sync_freq=5), batchsize=32, min_replay_history=2 * n, seed=seed,
                                   max_grad_norm=1.0, n_step=3, double_dqn=True, per_beta=0.4)
        policy = rlhip.QBasedPolicy(learner, rlhip.EpsilonGreedyExplorer(0.05, kind="exp", decay_steps=30, seed=seed))
        traces = rlhip.CircularPrioritizedTraces(capacity=16, n_env=n, obs_dim=4, n_step=traces_n_step)
        return env, rlhip.Agent(policy, rlhip.Trajectory(traces))

    path = str(tmp_path / "ck.npz")
    env, agent = build(6, 3)
    saved = []

    def hook_fn(t, policy, e):
        if t == 20:
            saved.append(rlhip.save_checkpoint(path, {"agent": agent, "env": env}))

    rlhip.run(agent, env, rlhip.StopAfterNSteps(45), rlhip.DoEveryNSteps(hook_fn, n=20))
    assert saved and agent.policy.learner.n_updates > 30
    with np.load(path) as z:
        assert int(z["agent/trajectory/container/n_step"]) == 3
    small = rlhip.CircularPrioritizedTraces(capacity=2, n_env=16, obs_dim=4)
    with np.load(path) as z:
        with pytest.raises(ValueError, match="n_step exceeds the capacity"):   # checked when loaded, not at the next push
            rlhip.load_state_dict({"c": small}, {"c/n_step": z["agent/trajectory/container/n_step"]}, strict=False)
    assert small.n_step == 1
    env2, agent2 = build(99, 1)
    rlhip.load_checkpoint(path, {"agent": agent2, "env": env2})
    assert agent2.trajectory.container.n_step == 3
    rlhip.run(agent2, env2, rlhip.StopAfterNSteps(25))
    torch.cuda.synchronize()
    a, b = rlhip.state_dict({"agent": agent, "env": env}), rlhip.state_dict({"agent": agent2, "env": env2})
    assert set(a) == set(b)
    for k in a:
        if "workspace" in k or k.endswith("/grad") or "/_q" in k or "_nstep/_" in k or k.endswith("/_idx"):
            continue    # scratch
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k
    assert agent2.policy.learner.n_updates == agent.policy.learner.n_updates
