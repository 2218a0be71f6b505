"""The fused consumers of env_step1 + env_reset1 on goal and x-threshold terminations (tests/env_edge_cases.py, the grids
without truncation: max_steps = 100000, so no env ends through its step counter).

The fused act tests of the learner matrices give MountainCar and Pendulum max_steps = 40: the only termination those kernels
ever saw outside CartPole was truncation.  Here rlhip_dqn_act_f32 (every hidden size), rlhip_env_act_push_f32 and
rlhip_dqn3_act_f32 start from injected states of which about half reach the goal / leave the track at the first step, with the
harness of test_fused_dqn_act_vs_oracle:

  * flags, counters and rewards against the oracle env started from the kernel's state and stepped with the kernel's actions;
  * the cause of every termination, from the oracle's last_obs: goal (x >= goal_pos and v >= goal_velocity) or |x| beyond the
    x-threshold with the pole inside its own, never the step counter;
  * last_obs holds the pre-reset observation of such a step (x >= goal_pos), obs_out and the next pushed state the reset
    draw, bit for bit with the oracle's reset;
  * the ring record of a terminating step is {s, a, r = 0, terminal = 1} followed by the reset draw as the next state (the
    MultiThreadEnv protocol: the pre-reset observation is an output of the launch, not a ring entry), all of it bit for bit
    against oracle.Ring.

Pendulum (discrete, 3 actions; it ends through t alone, so nothing terminates) runs the same rows for the state arithmetic next
to the range-reduction edges.  The PPO rollout kernels start from the same grids in tests/rollout_audit.py.
"""
import ctypes as C
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import env_edge_cases as E  # noqa: E402
import oracle  # noqa: E402

KIND = {"cartpole": 0, "pendulum": 1, "mountaincar": 2}
GRID = {"cartpole": "cartpole-f32-disc-default", "pendulum": "pendulum-f32-disc-na3", "mountaincar": "mountaincar-f32-disc-default"}
N = 1024


@pytest.fixture(scope="module")
def rl():
    import rlhip

    return rlhip


def dev(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).cuda()


def host(t):
    return t.detach().cpu().numpy()


def assert_cause(g, oenv, done):
    """every termination is a goal / x-threshold one, and they are 20 .. 50 % of the envs"""
    lo, p = oenv.last_obs, g.p
    assert (oenv.t < 2000).all() and p["max_steps"] == E.NO_TRUNC_MAX_STEPS
    if g.kind == "mountaincar":
        cause = (lo[0] >= p["goal_pos"]) & (lo[1] >= p["goal_velocity"])
    elif g.kind == "cartpole":
        cause = (np.abs(lo[0]) > p["xthreshold"]) & (np.abs(lo[2]) <= p["thetathreshold"])
    else:
        assert not done.any()
        return
    assert np.array_equal(done.astype(bool), cause)
    assert 0.2 <= done.mean() <= 0.5, f"{done.mean():.3f} of the envs terminated"
    assert (oenv.reward[done.astype(bool)] == 0).all()


def fused_case(rl, env_name, launch, tag):
    """launch(env, tr, obs0, rng) -> (actions i32[n], obs_out, last_obs) as host arrays, after ONE fused plan/act/push launch"""
    from rlhip.trajectory import CircularArraySARTSTraces

    g = E.grid(GRID[env_name], N, truncation=False)
    env = rl.HipVecEnv(env_name, N, seed=g.seed, env_id_base=g.env_id_base, continuous=False, **g.cfg)
    # the policy picks the actions here, and a row solved to land one ulp short of the goal under ITS action may cross it
    # under another: an eighth of the terminating rows become plain rows, so that the share stays inside 20 .. 50 %
    s0 = g.s.copy()
    late = np.nonzero(g.term & (np.arange(N) >= N - 128))[0]
    if late.size:
        s0[:, late] = s0[:, np.nonzero(~g.term)[0][-late.size:]]
    env.set_raw_state(s0, g.t)
    ns = env.odim
    tr = CircularArraySARTSTraces(capacity=4, n_env=N, obs_dim=ns)
    ref = oracle.Ring(4, N, ns)
    obs0 = host(env.state()).copy()
    tr.push_state_(env.state())
    ref.push_state(obs0)
    oenv = oracle.VecEnv(KIND[env_name], N, seed=g.seed, env_id_base=g.env_id_base, continuous=False, **g.cfg)
    oenv.set_state([host(env.raw_state()[k]) for k in range(env.sdim)], host(env._t))
    oenv.episode[:] = host(env._episode).view(np.uint32)
    ep0 = oenv.episode.copy()
    ga, obs_out, last_obs = launch(env, tr, obs0, np.random.default_rng(zlib.crc32(tag.encode())))
    env._obs_valid = False
    oenv.step(ga)
    done = host(env._done)
    assert np.array_equal(done, oenv.done) and np.array_equal(host(env._t), oenv.t)
    assert np.array_equal(host(env._episode).view(np.uint32), oenv.episode)
    assert np.array_equal(oenv.episode - ep0, oenv.done)
    assert_cause(g, oenv, done)
    d = done.astype(bool)
    if env_name == "pendulum":
        np.testing.assert_allclose(host(env.reward()), oenv.reward, rtol=2e-6, atol=1e-7)
    else:
        assert np.array_equal(host(env.reward()), oenv.reward)
    # the pre-reset observation is last_obs; obs_out, state(env) and the raw state of a terminated env are the reset draw
    if env_name != "pendulum":
        assert np.array_equal(last_obs, oenv.last_obs)
        assert np.array_equal(obs_out, oenv.obs())
    else:  # (sin, cos) of the kernel's own theta; against the oracle's theta as an angle within 2 ulp of theta
        probe = oracle.VecEnv(1, N, continuous=False, auto_reset=False, **g.cfg)
        probe.set_state(host(env.raw_state()))
        np.testing.assert_allclose(obs_out, probe.obs(), rtol=2e-6, atol=1e-7)
        assert np.array_equal(obs_out, last_obs)  # nothing terminated
        dist = np.hypot(last_obs[0] - oenv.last_obs[0], last_obs[1] - oenv.last_obs[1])
        assert (dist <= 2 * np.spacing(np.abs(oenv.s[0])) + 1e-6).all()
        np.testing.assert_allclose(last_obs[2], oenv.last_obs[2], rtol=2e-6, atol=1e-7)
    assert np.array_equal(host(env.raw_state())[:, d], np.stack(oenv.s)[:, d])
    assert np.array_equal(obs_out, host(env.state())), "obs_out is not state(env) after the step"
    if env_name == "mountaincar":
        assert (last_obs[0, d] >= g.p["goal_pos"]).all() and (obs_out[0, d] < -0.39).all() and (obs_out[1, d] == 0).all()
    # the ring: {s, a, r, terminal} of the step, then the next pushed state
    ref.push_transition(obs_out, ga, host(env.reward()), done)
    assert len(tr) == len(ref) == 1
    idx = np.arange(N, dtype=np.int64)
    got = [host(x) for x in tr.gather(dev(idx))]
    for g_, o_ in zip(got, ref.gather(idx)):
        assert np.array_equal(g_, o_)
    s, a, r, t, sn = got
    assert np.array_equal(s, obs0) and np.array_equal(a, ga) and np.array_equal(t, done)
    assert (r[d] == 0).all() and np.array_equal(sn, obs_out)


@pytest.mark.parametrize("h", [64, 128, 256])
@pytest.mark.parametrize("env_name", ["mountaincar", "cartpole", "pendulum"])
def test_fused_dqn_act_on_goal_and_threshold_steps(rl, env_name, h):
    from rlhip._lib import call
    from rlhip.ops import ptr, stream_ptr

    act = (h // 64) % 2
    kind = KIND[env_name]

    def launch(env, tr, obs0, rng):
        ns, na = env.odim, len(env.action_space())
        assert int(rl._lib.lib.rlhip_dqn_act_supported(kind, N, h)) == 1
        p = (oracle.mlp2_init(ns, h, na, 9, 0) + rng.standard_normal(oracle.mlp2_nparams(ns, h, na)) * 0.1).astype(np.float32)
        P = dev(p)
        actions = torch.zeros(N, dtype=torch.int32, device="cuda")
        q = torch.zeros((na, N), device="cuda")
        obs_out, last_obs = torch.zeros((ns, N), device="cuda"), torch.zeros((ns, N), device="cuda")
        eps, xseed, step = 0.3, 17, 5
        call("rlhip_dqn_act_f32", kind, C.byref(env.cfg), C.byref(env._st), N, ptr(P), h, na, act, eps, xseed, step, env.seed,
             env.env_id_base, C.byref(tr.rb), ptr(actions), ptr(q), ptr(obs_out), ptr(last_obs), stream_ptr())
        gq, ga = host(q), host(actions)
        np.testing.assert_allclose(gq, oracle.mlp2_forward(p, ns, h, na, act, obs0), rtol=2e-5, atol=2e-6)
        assert np.array_equal(ga, oracle.eps_greedy_select(gq, eps, seed=xseed, step=step, env_id_base=env.env_id_base))
        return ga, host(obs_out), host(last_obs)

    fused_case(rl, env_name, launch, f"dqn_act-{env_name}-{h}")


@pytest.mark.parametrize("env_name", ["mountaincar", "cartpole", "pendulum"])
def test_env_act_push_on_goal_and_threshold_steps(rl, env_name):
    from rlhip._lib import call
    from rlhip.ops import ptr, stream_ptr

    kind = KIND[env_name]

    def launch(env, tr, obs0, rng):
        ns, na = env.odim, len(env.action_space())
        ga = rng.integers(0, na, N).astype(np.int32)
        obs_out, last_obs = torch.zeros((ns, N), device="cuda"), torch.zeros((ns, N), device="cuda")
        call("rlhip_env_act_push_f32", kind, C.byref(env.cfg), C.byref(env._st), N, ptr(dev(ga)), env.seed, env.env_id_base,
             C.byref(tr.rb), ptr(obs_out), ptr(last_obs), stream_ptr())
        return ga, host(obs_out), host(last_obs)

    fused_case(rl, env_name, launch, f"env_act_push-{env_name}")


@pytest.mark.parametrize("env_name", ["mountaincar", "cartpole", "pendulum"])
def test_fused_dqn3_act_on_goal_and_threshold_steps(rl, env_name):
    from rlhip import dqn
    from rlhip._lib import call
    from rlhip.ops import ptr, stream_ptr

    kind, h = KIND[env_name], 128
    act = 0 if env_name == "cartpole" else 1

    def launch(env, tr, obs0, rng):
        ns, na = env.odim, len(env.action_space())
        assert int(rl._lib.lib.rlhip_dqn3_act_supported(kind, N, h, na)) == 1
        p = oracle.mlp3_init(ns, h, na, 9 + act, 0)
        P = dev(p)
        packed = dqn.mlp3_pack(P, ns, h, na)
        actions = torch.zeros(N, dtype=torch.int32, device="cuda")
        q = torch.zeros((na, N), device="cuda")
        obs, last_obs = dev(obs0), torch.zeros((ns, N), device="cuda")  # obs: read (this step's), rewritten (the next one's)
        eps, xseed, step = 0.3, 17, 5
        call("rlhip_dqn3_act_f32", kind, C.byref(env.cfg), C.byref(env._st), N, ptr(P), ptr(packed), h, na, act, eps, xseed, step,
             env.seed, env.env_id_base, C.byref(tr.rb), ptr(actions), ptr(q), ptr(obs), ptr(last_obs), stream_ptr())
        gq, ga = host(q), host(actions)
        # the fused kernel is rlhip_dqn3_plan_f32 (pinned to the oracle by the dqn3_plan32 rows) followed by act! + push!
        pa, pq = dqn.dqn3_plan(P, packed, ns, h, na, act, dev(obs0), eps, xseed, env.env_id_base, step)
        assert np.array_equal(host(pq), gq) and np.array_equal(host(pa), ga)
        assert np.array_equal(ga, oracle.eps_greedy_select(gq, eps, seed=xseed, step=step, env_id_base=env.env_id_base))
        return ga, host(obs), host(last_obs)

    fused_case(rl, env_name, launch, f"dqn3_act-{env_name}")
