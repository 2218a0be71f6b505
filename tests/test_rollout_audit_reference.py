"""The rollout audit (tests/rollout_audit.py) on the oracle alone -- the CPU half of tests/test_gpu_rollout_audit.py:

  * every rollout row of tests/f32_learner_matrix.py and tests/bf16_learner_matrix.py has an audit case, and the GPU test
    runs exactly these cases;
  * the stepwise oracle rollout the audit is built from equals oracle.ppo_rollout bit for bit;
  * the audit of the oracle's own free-running rollout of every case: no action disagreement, zero policy error, the
    transition part within its bars -- this is the error of the state reconstruction by itself.  Pendulum is reconstructed by
    the atan2 route (module docstring of rollout_audit) and has to sit at least 4 x inside its bars;
  * the samples at which a logit raised by delta would change the oracle's choice (fragile samples) are at most half the
    near-tie exception cap of each case;
  * every corruption on the list makes the audit fail.

The cases of more than 2^15 envs run here at 4097 envs (same T, max_steps, seeds and nets): the reconstruction error and the
fragile share are per-sample properties, and the oracle's three-layer forward of 400 000 samples takes tens of seconds."""
import numpy as np
import pytest

import oracle
import rollout_audit as A

IDS = [c["id"] for c in A.CASES]


def _cpu_case(c):
    return dict(c, n=4097) if c["n"] > 1 << 15 else c


@pytest.fixture(scope="module", autouse=True)
def all_cores():
    oracle.use_all_cores(True)
    yield
    oracle.use_all_cores(False)


def _by_id(cid):
    return _cpu_case(next(c for c in A.CASES if c["id"] == cid))


def _audit(c, params, rollout, **kw):
    tr, env0, env1, vs0 = rollout
    res = A.audit(tr, env0, env1, params, c, vs0, **kw)
    fails, summ = A.check(res, A.make_bars(c))
    return res, fails, summ


def test_every_rollout_row_of_the_matrices_is_audited():
    ids = set(IDS)
    assert len(ids) == len(IDS)
    assert A.MATRIX_IDS <= ids, A.MATRIX_IDS - ids
    import test_gpu_rollout_audit as G

    marks = [m for m in G.test_rollout_audit_vs_oracle.pytestmark if m.name == "parametrize"]
    assert len(marks) == 1 and set(marks[0].kwargs["ids"]) == ids and len(marks[0].args[1]) == len(IDS)
    # the shapes the issue of the audit asks for
    split = [c for c in A.CASES if c["kernel"] == "rollout_split_kernel"]
    assert sum(c["T"] == 16 for c in split) == 1 and all(c["T"] > 32 or c["T"] == 16 for c in split)
    assert any(c["kernel"] == "rollout_scalar_kernel" and c["n"] * 16 > 1 << 22 and c["hidden"] in (64, 128, 256) for c in A.CASES)
    assert all(c["env_id_base"] != 0 for c in A.CASES)


@pytest.mark.parametrize("cid", ["rollout-cartpole-h64-relu-head2", "rollout-pendulum-h128-tanh-head1",
                                 "rollout-mountaincar-scalar-relu", "ppo3_rollout32-pendulum-relu", "ppo3w_rollout-cartpole-tanh"])
def test_stepwise_oracle_rollout_equals_ppo_rollout(cid):
    c = _by_id(cid)
    params = A.make_params(c)
    env = A._new_env(c)
    ocfg = oracle.ppo_default(hidden=c["hidden"], continuous=int(c["continuous"]), layers=c["layers"], act=c["act"])
    for tr, env0, env1, vs0 in A.oracle_rollout(c, params):
        otr = oracle.PPOTraj(oracle.KIND[c["env"]], c["n"], c["T"], continuous=c["continuous"])
        oracle.ppo_rollout(env, c["T"], ocfg, params[0], otr, vs0)
        for name in ("obs", "value", "logp", "reward", "terminal"):
            assert np.array_equal(tr[name], getattr(otr, name)), name
        assert np.array_equal(tr["action_f"], otr.action_f[:, 0]) if c["continuous"] else np.array_equal(tr["action_i"], otr.action_i)
        assert np.array_equal(env1["raw_state"], np.stack(env.s)) and np.array_equal(env1["t"], env.t)


@pytest.mark.parametrize("cid", IDS)
def test_audit_of_the_oracles_own_rollout(cid):
    c = _by_id(cid)
    params = A.make_params(c)
    bars = A.make_bars(c)
    resets = np.zeros(c["n"], int)
    for period, rollout in enumerate(A.oracle_rollout(c, params)):
        res, fails, summ = _audit(c, params, rollout, count_fragile=True)
        print(f"{cid} period {period}: " + " ".join(f"{k}={v:.3g}" for k, v in summ.items()), res["scale"])
        assert not fails, fails
        assert res["n_disagree"] == 0 and not res["exception"].any()
        for q in ("value", "logp", "action"):
            assert q not in res or res[q][0].max() == 0, f"{q}: the audit does not reproduce the oracle's own policy step"
        # what the state reconstruction costs by itself: exact where the observation is the state, 4 x inside for Pendulum
        lim = 0.25 if c["env"] == "pendulum" else 0.0
        for q in ("reward", "env_reward", "obs", "obs_reset", "state"):
            assert summ[q] <= lim, f"{q}: {summ[q]:.3g} x its bar from the reconstruction alone"
        if not c["continuous"]:
            share = res["fragile"].mean()
            print(f"    fragile share {share:.3g} (delta <= {res['delta_max']:.3g})")
            assert share <= bars["exc_cap"] / 2
        if c["layers"] == 2:  # the Float32 scales stay inside the bars they are capped by
            assert 4 * res["scale"]["logit"] <= 2e-5 and 4 * res["scale"].get("action", 0) <= 2e-3
        resets += res["n_resets"]
        assert rollout[3] == period * c["T"]
    if c["env"] == "cartpole":
        assert (resets > 0).mean() > 0.5, "hardly an episode ends inside the launches"
    else:
        assert resets.min() >= 4, "an env reset fewer than twice per launch"


# ------------------------------------------------------------------------------------------------- injected states
def _cpu_inject_case(cid):
    c = next(c for c in A.INJECT_CASES if c["id"] == cid)
    if c["n"] > 1 << 15:
        c = dict(c, n=4097, inject=dict(s=c["inject"]["s"][:, :4097].copy(), t=c["inject"]["t"][:4097].copy()))
    return c


@pytest.mark.parametrize("cid", [c["id"] for c in A.INJECT_CASES])
def test_audit_of_the_oracles_own_rollout_from_injected_states(cid):
    """one MountainCar and one CartPole case per rollout kernel (the three-layer kernels: CartPole), started on the goal /
    x-threshold rows of tests/env_edge_cases.py: at least 20 % of the envs end at the first step, none through max_steps"""
    c = _cpu_inject_case(cid)
    params = A.make_params(c)
    for period, rollout in enumerate(A.oracle_rollout(c, params)):
        res, fails, summ = _audit(c, params, rollout)
        print(f"{cid} period {period}: " + " ".join(f"{k}={v:.3g}" for k, v in summ.items()))
        assert not fails, fails
        assert res["n_disagree"] == 0 and not res["exception"].any()
        for q in ("reward", "env_reward", "obs", "obs_reset", "state"):
            assert summ[q] == 0.0
        if period == 0:
            tr, env0 = rollout[0], rollout[1]
            assert np.array_equal(env0["raw_state"], c["inject"]["s"]) and np.array_equal(env0["t"], c["inject"]["t"])
            assert not A.check_injected(tr, env0, c)
            assert 0.2 <= tr["terminal"][0].mean() <= 0.5
            assert tr["terminal"][0].sum() >= (4 if c["n"] == 16 else 8)


def test_injected_cases_cover_every_rollout_kernel():
    kernels = {c["kernel"] for c in A.CASES}
    assert {c["kernel"] for c in A.INJECT_CASES} == kernels and len(kernels) == 5
    for k in ("rollout_split_kernel", "rollout_scalar_kernel"):
        assert {c["env"] for c in A.INJECT_CASES if c["kernel"] == k} == {"mountaincar", "cartpole"}
    assert all(c["T"] == 8 and c["env_id_base"] != 0 for c in A.INJECT_CASES)
    assert not {c["id"] for c in A.INJECT_CASES} & set(IDS)
    import test_gpu_rollout_audit as G

    marks = [m for m in G.test_rollout_audit_from_injected_states.pytestmark if m.name == "parametrize"]
    assert len(marks) == 1 and set(marks[0].kwargs["ids"]) == {c["id"] for c in A.INJECT_CASES}


def test_check_injected_catches_a_shifted_terminal_and_a_stale_next_observation():
    c = _cpu_inject_case("rollout-mountaincar-scalar-relu-injected")
    params = A.make_params(c)
    tr, env0, _, _ = A.oracle_rollout(c, params, periods=1)[0]
    assert not A.check_injected(tr, env0, c)
    bad = dict(tr, terminal=np.roll(tr["terminal"], -1, axis=0))  # terminal[0] is the next step's
    assert A.check_injected(bad, env0, c)
    env = A._new_env(c)
    env.auto_reset = False
    A.apply_inject(c, env)
    env.episode[:] = env0["episode"].view(np.uint32)
    env.step(tr["action_i"][0])
    stale = dict(tr, obs=tr["obs"].copy())
    stale["obs"][1] = env.last_obs  # the pre-reset observation recorded as the next one
    assert A.check_injected(stale, env0, c)


# ------------------------------------------------------------------------------------------------------- corruptions
DISC, GAUSS, DISC3 = "rollout-cartpole-h64-tanh-head2", "rollout-pendulum-h128-relu-head1", "rollout-mountaincar-h128-relu-head3"


def _shift(x):
    y = x.copy()
    y[1:] = x[:-1]
    return y


def _post(name, c, params, tr):
    tr = {k: v.copy() for k, v in tr.items()}
    T = c["T"]
    if name == "logp_other_action":
        X = tr["obs"][:T].transpose(1, 0, 2).reshape(A.NS[c["env"]], -1)
        lsm = A.log_softmax(A.forward(c, params[0][:params[1]], A.nout_of(c), X))
        other = (tr["action_i"].reshape(-1) + 1) % A.nout_of(c)
        tr["logp"] = lsm[other, np.arange(other.size)].reshape(T, -1)
    elif name == "reward_shifted":
        tr["reward"] = _shift(tr["reward"])
    elif name == "terminal_shifted":
        tr["terminal"] = _shift(tr["terminal"])
    elif name == "last_value_from_previous_obs":
        X = tr["obs"][T - 1]
        tr["value"][T] = A.forward(c, params[0][params[1]:], 1, X)[0]
    elif name == "action_clamped":
        assert (np.abs(tr["action_f"]) > 2).any()
        tr["action_f"] = np.clip(tr["action_f"], -2, 2)
    else:
        raise KeyError(name)
    if name in ("reward_shifted", "terminal_shifted", "last_value_from_previous_obs"):  # a consistent fault: the scan saw it too
        adv = oracle.generalized_advantage_estimation(tr["reward"].T, tr["value"].T, A.GAMMA, A.LAM, terminal=tr["terminal"].T,
                                                      dims=2, dtype=np.float32).T
        tr["adv"], tr["ret"] = np.ascontiguousarray(adv), (adv + tr["value"][:T]).astype(np.float32)
    return tr


@pytest.mark.parametrize("fault,cid", [
    ("noise_step", DISC), ("noise_step", GAUSS), ("noise_env", DISC3), ("noise_env", GAUSS),
    ("logp_other_action", DISC), ("logp_other_action", DISC3),
    ("reward_shifted", GAUSS), ("reward_shifted", DISC), ("terminal_shifted", DISC), ("terminal_shifted", GAUSS),
    ("stale_episode", DISC), ("stale_episode", GAUSS), ("stale_episode", DISC3),
    ("step_counter", DISC), ("step_counter", GAUSS), ("step_counter", DISC3),
    ("last_value_from_previous_obs", DISC), ("last_value_from_previous_obs", GAUSS),
    ("action_clamped", GAUSS),
])
def test_the_audit_catches(fault, cid):
    c = _by_id(cid)
    params = A.make_params(c)
    in_loop = fault in ("noise_step", "noise_env", "stale_episode", "step_counter")
    rollouts = A.oracle_rollout(c, params, fault=fault if in_loop else None)
    caught = []
    for tr, env0, env1, vs0 in rollouts:
        if not in_loop:
            tr = _post(fault, c, params, tr)
        _, fails, _ = _audit(c, params, (tr, env0, env1, vs0))
        caught.append(fails)
    print(fault, cid, caught)
    assert caught[0], f"{fault} passes the audit of the first period"
    assert caught[1], f"{fault} passes the audit of the second period"
