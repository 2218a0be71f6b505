"""Every step of every fused PPO rollout instantiation against the oracle, restarted from the GPU's own records.

One launch of PPOPolicy.rollout_() per update period, two periods per case (vec_step0 = 0 and T, the env's episode and step
counters carried over), then tests/rollout_audit.py: every sample (t, env) of value, log-prob, action, reward, terminal and next
observation, the env state the launch leaves behind, and adv / ret.  The cases are the rollout rows of
tests/f32_learner_matrix.py and tests/bf16_learner_matrix.py with shape and env arguments overridden (rollout_audit.CASES) so
that episodes end inside the launch (CartPole T >= 40, the others max_steps 5 .. 20 and at least two resets per env), the
16-step noise chunks of rollout_split_kernel are crossed twice (one case has T = 16 exactly), n is ragged against the envs per
workgroup, and env_id_base is not 0.  tests/test_rollout_audit_reference.py holds the CPU half.

Bars, and where each comes from:
  two-layer value, log-prob      rtol 2e-5, atol 2e-6: test_policy_init_and_plan_vs_oracle (tests/test_gpu_learners.py)
  two-layer Gaussian action      4 x the Float32 scale s: the largest |Float32 oracle - Float64 numpy| / (1 + |ref|) of
  two-layer logit delta          mu + exp(log sigma) * noise / of the logits on the recorded observations; delta is twice the
                                 logit bar, 8 s (1 + max |logit|).  Never wider than the free-running 2e-3 they replace
  three-layer value, action      close() of test_ppo3_rollout_vs_oracle: 2e-5 (relu CartPole value) or 1e-4 of 1 + |ref|, strict
                                 for relu, for tanh at most 1e-3 of the samples beyond and none beyond 5e-3
  three-layer log-prob           1e-3 absolute; tanh rows in the share form, the cap 1e-3 plus the first-order reach of a 5e-3
                                 output flip on the log-density
  three-layer logit delta        twice the value tolerance of the row, of 1 + max |logit|
  reward, observation, state     rtol 2e-6, atol 1e-7, Pendulum observations 2e-5 absolute: test_env_step_teacher_forced;
                                 observations after an auto-reset atol 1e-7, raw state bit for bit:
                                 test_env_reset_matches_oracle_bit_exact
  terminal, counters, adv, ret   bit for bit
  near-tie exceptions            at most 1e-3 of a case's samples (Float32 nets), 5e-3 (bf16 nets)

The test prints, per case and period, the largest error of each quantity in units of its bar and the near-tie exception
share.  No MI355X figures are recorded yet (profiles/rollout_audit.md).
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import oracle  # noqa: E402
import rollout_audit as A  # noqa: E402


@pytest.fixture(scope="module")
def rl():
    import rlhip

    oracle.use_all_cores(True)
    yield rlhip
    oracle.use_all_cores(False)


def host(t):
    return t.detach().cpu().numpy().copy()


def _snapshot(env):
    return dict(raw_state=host(env.raw_state()), t=host(env._t), episode=host(env._episode), reward=host(env.reward()),
                done=host(env._done))


@pytest.mark.parametrize("case", A.CASES, ids=[c["id"] for c in A.CASES])
def test_rollout_audit_vs_oracle(rl, case):
    c = case
    env = rl.HipVecEnv(c["env"], c["n"], seed=c["seed"], env_id_base=c["env_id_base"], **A.env_kwargs(c))
    pol = rl.PPOPolicy(env, update_freq=c["T"], hidden=c["hidden"], act=c["act"], **({"layers": 3} if c["layers"] == 3 else {}))
    params = A.make_params(c)
    assert pol.np == params[0].size and pol.np_actor == params[1] and pol.seed == c["seed"]
    pol.params.copy_(torch.as_tensor(params[0]).cuda())
    bars = A.make_bars(c)
    resets = np.zeros(c["n"], int)
    for period in range(2):
        env0 = _snapshot(env)
        assert pol.vec_step == period * c["T"]
        pol.rollout_()
        torch.cuda.synchronize()
        tr = pol.trajectory
        traj = {k: host(getattr(tr, k)) for k in ("obs", "value", "logp", "reward", "terminal", "adv", "ret", "action_i")}
        traj["action_f"] = host(tr.action_f)[:, 0]
        res = A.audit(traj, env0, _snapshot(env), params, c, period * c["T"])
        fails, summ = A.check(res, bars)
        print(f"\n{c['id']} period {period}: " + " ".join(f"{k}={v:.3g}" for k, v in summ.items()), res["scale"])
        assert not fails, fails
        resets += res["n_resets"]
    if c["env"] == "cartpole":
        assert (resets > 0).mean() > 0.5, "hardly an episode ends inside the launches"
    else:
        assert resets.min() >= 4, "an env reset fewer than twice per launch"


@pytest.mark.parametrize("case", A.INJECT_CASES, ids=[c["id"] for c in A.INJECT_CASES])
def test_rollout_audit_from_injected_states(rl, case):
    """One MountainCar and one CartPole case per rollout kernel (the three-layer kernels take CartPole only), T = 8, started
    from the goal / x-threshold rows of tests/env_edge_cases.py with max_steps far away: the same audit and bars, and on the
    first step at least 20 % of the envs record a terminal that the oracle attributes to the goal / the x-threshold, with
    reward 0 and the reset draw as the next observation (rollout_audit.check_injected); adv / ret over those terminals are
    among the audit's bit-for-bit quantities."""
    c = case
    env = rl.HipVecEnv(c["env"], c["n"], seed=c["seed"], env_id_base=c["env_id_base"], **A.env_kwargs(c))
    pol = rl.PPOPolicy(env, update_freq=c["T"], hidden=c["hidden"], act=c["act"], **({"layers": 3} if c["layers"] == 3 else {}))
    params = A.make_params(c)
    assert pol.np == params[0].size and pol.np_actor == params[1] and pol.seed == c["seed"]
    pol.params.copy_(torch.as_tensor(params[0]).cuda())
    env.set_raw_state(c["inject"]["s"], c["inject"]["t"])
    bars = A.make_bars(c)
    for period in range(2):
        env0 = _snapshot(env)
        pol.rollout_()
        torch.cuda.synchronize()
        tr = pol.trajectory
        traj = {k: host(getattr(tr, k)) for k in ("obs", "value", "logp", "reward", "terminal", "adv", "ret", "action_i")}
        traj["action_f"] = host(tr.action_f)[:, 0]
        res = A.audit(traj, env0, _snapshot(env), params, c, period * c["T"])
        fails, summ = A.check(res, bars)
        print(f"\n{c['id']} period {period}: " + " ".join(f"{k}={v:.3g}" for k, v in summ.items()), res["scale"])
        assert not fails, fails
        if period == 0:
            assert np.array_equal(env0["raw_state"], c["inject"]["s"]) and np.array_equal(env0["t"], c["inject"]["t"])
            fails = A.check_injected(traj, env0, c)
            assert not fails, fails
