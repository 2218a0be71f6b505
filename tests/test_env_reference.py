"""oracle.VecEnv against an independent numpy model (tests/env_ref.py) on every injected-state grid of
tests/env_edge_cases.py -- the CPU half of tests/test_gpu_env_edges.py.

The oracle is what the GPU kernels are judged by, and before this module its wall, clamp, goal, x-threshold, success and
velocity-bound branches were pinned by one hand-made wall step and one goal step.  Here both restatements start from the
same rows (auto-reset off) and one act! is compared:

  * done, t and reward bit for bit;
  * Float32 states and observations bit for bit; Float64 ones within the project's Float64 bar (rtol 1e-12, atol 1e-14: the
    two sides may differ in the last bit of a double-precision libm call);
  * the reference terminates exactly the prescribed envs (the lane pattern of the grids);
  * every census count the grid names is >= 8, so no grid misses the branch it was built for;
  * two planted faults (a wall rule one ulp wide, `>=` at the x-threshold) each make the comparison fail.
"""
import numpy as np
import pytest

import env_edge_cases as E
import env_ref
import oracle

IDS = [f"{sid}-n{n}" for sid, n in E.all_grid_ids()]


def oracle_env(g, auto_reset):
    kw = dict(g.cfg)
    if g.kind != "acrobot":
        kw["continuous"] = g.continuous
    env = oracle.VecEnv(g.kind, g.n, seed=g.seed, env_id_base=g.env_id_base, dtype=g.dtype, auto_reset=auto_reset, **kw)
    env.set_state(g.s, g.t)
    return env


def noise_uniforms(g, episode):
    """rand(env.rng, T) of the coming act! as the project numbers it: Philox(seed, env, t + 1, episode, ENVNOISE)"""
    if g.kind != "acrobot" or not g.cfg.get("max_torque_noise"):
        return None
    u = np.empty(g.n, g.dtype)
    for i in range(g.n):
        w = oracle.philox(g.seed, g.env_id_base + i, int(g.t[i]) + 1, int(episode[i]), oracle.TAG["ENVNOISE"])
        u[i] = oracle.u01_f32(w[0]) if g.dtype is np.float32 else oracle.u01_f64(w[0], w[1])
    return u


def compare(g, fault=None):
    ref = oracle_env(g, auto_reset=False)
    u = noise_uniforms(g, ref.episode)
    ref.step(g.a)
    s1, t1, reward, done = env_ref.step(g.kind, g.p, g.s, g.t, g.a, noise_u=u, fault=fault)
    assert np.array_equal(ref.done.astype(bool), done), f"done differs at {np.nonzero(ref.done.astype(bool) != done)[0][:8]}"
    assert np.array_equal(ref.t, t1)
    assert reward.dtype == ref.reward.dtype and np.array_equal(ref.reward, reward), "reward"
    obs = env_ref.observation(g.kind, s1)
    if g.dtype is np.float32:
        for k in range(s1.shape[0]):
            assert np.array_equal(ref.s[k], s1[k]), f"state {k} differs at {np.nonzero(ref.s[k] != s1[k])[0][:8]}"
        assert np.array_equal(ref.last_obs, obs)
        assert np.array_equal(ref.obs(), obs)
    else:
        np.testing.assert_allclose(np.stack(ref.s), s1, rtol=1e-12, atol=1e-14)
        np.testing.assert_allclose(ref.last_obs, obs, rtol=1e-12, atol=1e-14)
    return ref


@pytest.mark.parametrize("gid", E.all_grid_ids(), ids=IDS)
def test_oracle_matches_the_independent_model(gid):
    g = E.grid(*gid)
    ref = compare(g)
    assert np.array_equal(ref.done.astype(bool), g.term), "the reference does not terminate exactly the prescribed envs"
    census = g.census(np.stack(ref.s), ref.t, ref.done)
    print(g.id, census)
    for name in g.required:
        assert census[name] >= E.MIN_HITS, f"{g.id}: {name} is hit {census[name]} times"


@pytest.mark.parametrize("gid", E.all_grid_ids(), ids=IDS)
def test_grids_without_truncation_end_by_goal_or_threshold_only(gid):
    """the grids of the fused consumers: the same rows, no termination through max_steps"""
    g = E.grid(*gid, truncation=False)
    ref = compare(g)
    assert (ref.t < 2000).all() and g.cfg["max_steps"] == E.NO_TRUNC_MAX_STEPS
    assert np.array_equal(ref.done.astype(bool), g.term)
    if g.kind != "pendulum":
        assert 0.2 <= ref.done.mean() <= 0.5
    census = g.census(np.stack(ref.s), ref.t, ref.done)
    for name in g.required:
        assert census[name] >= E.MIN_HITS, f"{g.id}: {name} is hit {census[name]} times"


@pytest.mark.parametrize("fault,sid", [
    ("wall_ulp", "mountaincar-f32-disc-default"), ("wall_ulp", "mountaincar-f64-cont-gv002"),
    ("x_ge", "cartpole-f32-disc-default"), ("x_ge", "cartpole-f64-cont-heavy"),
])
@pytest.mark.parametrize("n", E.SIZES)
def test_the_comparison_catches(fault, sid, n):
    g = E.grid(sid, n)
    compare(g)
    with pytest.raises(AssertionError):
        compare(g, fault=fault)


def test_lane_pattern_has_every_mix_in_every_wavefront():
    m = E.term_mask(1024).reshape(-1, 64, 4)  # wavefront, lane, env of the lane
    code = (m * (1 << np.arange(4))).sum(-1)
    for wave in code:
        assert set(wave) == set(range(16))
    assert E.term_mask(1001).mean() > 0.49
