"""Every branch of the env step on the GPU: the stand-alone step kernel started from the injected-state grids of
tests/env_edge_cases.py, teacher-forced against the oracle (which tests/test_env_reference.py pins to an independent model
on the same grids).

One act0_ per grid -- every kind, Float32 and Float64, discrete and continuous, packed and separate episode counters,
n = 1024 (vector path) and n = 1001 (scalar path); one more case per kind at n = 2^20 (the non-temporal instantiation and the
staggered layout).  The oracle starts from the kernel's raw state, t and episode counters.  Checked:

  * done, t, episode bit for bit; rewards bit for bit (Pendulum: the bar of test_env_step_teacher_forced);
  * the post-reset state of every terminated env bit for bit; the others within the existing bars (rtol 2e-6 / atol 1e-7
    Float32, 1e-12 / 1e-14 Float64);
  * exact results where the rule is an equality: x == min_pos and v == 0 at the wall, v == +-max_speed and x == max_pos at
    the clamps, thdot == +-max_speed for Pendulum;
  * obs_out, and last_obs of the envs that go on, against the oracle's observation OF THE KERNEL'S OWN raw state (at
    |theta| ~ 6e4 one ulp of theta is 0.0078 rad: two independently stepped angles would say nothing); last_obs of a terminated
    env against the oracle's, as an angle within 2 ulp of theta for Pendulum;
  * the lane pattern: the envs that restarted are exactly the prescribed ones, their episode counters rose by one, nobody
    else's did;
  * the census of the grid on the reference side (every named branch hit >= 8 times).

Share of state values whose last bit differs from the oracle, over these grids (envs that did not restart; the restarted
ones are compared bit for bit anyway), measured on an MI355X (profiles/env_edges.md).  The kernel's sin / cos of a Float32
equal (float) sin((double) x) for every |x| <= 2^16 by enumeration (tools/micro/trig_f32arg.hip) and the oracle evaluates
that same expression, so the Float32 CartPole, MountainCar and Pendulum-inside-2^16 rows are ASSERTED to be exactly 0; the
others keep the existing bars and are recorded (each case appends its counts to
env_edges_lastbit.jsonl in the suite's scratch directory, next to conftest's grad_err.jsonl).

    kind          dtype     rows           differing / compared
    mountaincar   Float32   all                    0 / 2 113 440
    cartpole      Float32   all                    0 / 4 243 168
    pendulum      Float32   inside 2^16            0 / 2 014 112
    pendulum      Float32   beyond 2^16            0 /   103 400
    acrobot       Float32   all                    0 / 4 226 880
    mountaincar   Float64   all                   12 /    16 288   (ocml's against glibc's double sin / cos: both < 1 ulp,
    cartpole      Float64   all                   32 /    48 864    neither correctly rounded; all inside rtol 1e-12)
    pendulum      Float64   inside 2^16          196 /    19 264
    pendulum      Float64   beyond 2^16            4 /     1 096
    acrobot       Float64   all                  508 /    32 576
"""
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import env_edge_cases as E  # noqa: E402
import oracle  # noqa: E402
from conftest import GRAD_ERR_LOG  # noqa: E402

SHARE_LOG = os.path.join(os.path.dirname(GRAD_ERR_LOG), "env_edges_lastbit.jsonl")  # scratch, like the gradient margins
CASES = [(sid, n, packed) for sid, n in E.all_grid_ids() for packed in (False, True)]
CASE_IDS = [f"{sid}-n{n}-{'packed' if packed else 'unpacked'}" for sid, n, packed in CASES]
BIG = ["mountaincar-f32-disc-default", "cartpole-f32-disc-default", "pendulum-f32-cont-default", "acrobot-f32-disc-book-noise"]


@pytest.fixture(scope="module")
def rl():
    import rlhip

    return rlhip


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def make_env(rl, g, packed, auto_reset=True, **over):
    T = torch.float32 if g.dtype is np.float32 else torch.float64
    kw = dict(g.cfg, **over)
    return rl.HipVecEnv(g.kind, g.n, T=T, continuous=None if g.kind == "acrobot" else g.continuous, seed=g.seed,
                        env_id_base=g.env_id_base, packed_episode=packed, auto_reset=auto_reset, **kw)


def make_ref(g, auto_reset=True, **over):
    kw = dict(g.cfg, **over)
    if g.kind != "acrobot":
        kw["continuous"] = g.continuous
    return oracle.VecEnv(g.kind, g.n, seed=g.seed, env_id_base=g.env_id_base, dtype=g.dtype, auto_reset=auto_reset, **kw)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _log_share(g, n_diff, n_cmp, inside):
    rec = {"grid": g.id, "kind": g.kind, "dtype": np.dtype(g.dtype).name, "differing": int(n_diff), "compared": int(n_cmp),
           "inside_2p16": bool(inside)}
    print("last-bit", json.dumps(rec))
    try:
        os.makedirs(os.path.dirname(SHARE_LOG), exist_ok=True)
        with open(SHARE_LOG, "a") as f:
            f.write(json.dumps(rec) + "\n")
    except OSError:
        pass


def one_step_checks(rl, g, packed):
    f32 = g.dtype is np.float32
    rtol, atol = (2e-6, 1e-7) if f32 else (1e-12, 1e-14)
    env = make_env(rl, g, packed)
    env.set_raw_state(g.s, t=g.t)
    s0, t0, ep0 = host(env.raw_state()), host(env.step_counter()), host(env.episode_counter()).view(np.uint32).copy()
    assert same_bits(s0, g.s) and np.array_equal(t0, g.t)
    ref, ref0 = make_ref(g), make_ref(g, auto_reset=False)  # ref0: the post-step state BEFORE the reset
    for r in (ref, ref0):
        r.set_state(s0, t0)
        r.episode[:] = ep0
    env.act0_(dev(g.a))
    ref.step(g.a)
    ref0.step(g.a)
    done = ref.done.astype(bool)
    s1, t1, ep1 = host(env.raw_state()), host(env.step_counter()), host(env.episode_counter()).view(np.uint32)
    last_obs, obs_out, reward = host(env.last_state()), host(env.state()), host(env.reward())

    # flags, counters, rewards
    assert np.array_equal(host(env._done), ref.done), f"done differs at {np.nonzero(host(env._done) != ref.done)[0][:8]}"
    assert np.array_equal(t1, ref.t) and np.array_equal(ep1, ref.episode)
    if g.kind == "pendulum":
        np.testing.assert_allclose(reward, ref.reward, rtol=rtol, atol=1e-7)
    else:
        assert np.array_equal(reward, ref.reward)

    # the lane pattern
    assert np.array_equal(done, g.term), "the reference does not terminate exactly the prescribed envs"
    assert np.array_equal(ep1 - ep0, g.term.astype(np.uint32)), "an episode counter moved that should not, or did not move by one"
    code = np.zeros(((g.n + 3) // 4) * 4, int)
    code[:g.n] = (ep1 != ep0)
    want = np.zeros_like(code)
    want[:g.n] = g.term
    for pat in range(16):
        lanes = np.nonzero((np.arange(code.size // 4) % 16) == pat)[0]
        assert np.array_equal(code.reshape(-1, 4)[lanes], want.reshape(-1, 4)[lanes]), f"lane pattern {pat:04b}"

    # states: restarted envs bit for bit, the others within the bars
    rs = np.stack(ref.s)
    assert same_bits(s1[:, done], rs[:, done]), "post-reset state"
    np.testing.assert_allclose(s1[:, ~done], rs[:, ~done], rtol=rtol, atol=atol)
    inside = np.ones(g.n, bool)
    if g.kind == "pendulum":
        inside = np.abs((g.s[0] + g.dtype(np.pi)).astype(g.dtype)) <= E.TRIG_MEDIUM_MAX
    keep = ~done & inside
    n_diff = int((s1[:, keep] != rs[:, keep]).sum())
    _log_share(g, n_diff, s1[:, keep].size, True)
    if g.kind == "pendulum" and (~done & ~inside).any():
        out = ~done & ~inside
        _log_share(g, int((s1[:, out] != rs[:, out]).sum()), s1[:, out].size, False)
    if f32 and g.kind != "acrobot":
        assert n_diff == 0, f"{n_diff} Float32 state values differ from the oracle in the last bit"

    # equalities hold exactly (pre-reset values: the state of the envs that go on, last_obs where it is the state)
    pre = np.stack(ref0.s)
    p = g.p
    if g.kind == "mountaincar":
        for name, m in (("x == min_pos", pre[0] == p["min_pos"]), ("v == 0 at the wall", (pre[0] == p["min_pos"]) & (pre[1] == 0)),
                        ("x == max_pos", pre[0] == p["max_pos"]), ("v == +-max_speed", np.abs(pre[1]) == p["max_speed"])):
            assert m.sum() >= E.MIN_HITS, name
            assert same_bits(last_obs[:, m], pre[:, m]), name
    if g.kind == "pendulum":
        m = np.abs(pre[1]) == p["max_speed"]
        assert m.sum() >= E.MIN_HITS and np.array_equal(last_obs[2, m], pre[1, m])
        assert np.array_equal(s1[1, m & ~done], pre[1, m & ~done])

    # observations: of the kernel's own raw state
    probe = make_ref(g, auto_reset=False)
    probe.set_state(s1)
    own = probe.obs()
    np.testing.assert_allclose(obs_out, own, rtol=rtol, atol=atol)
    np.testing.assert_allclose(last_obs[:, ~done], own[:, ~done], rtol=rtol, atol=atol)
    if g.kind == "pendulum":  # (sin, cos) of a terminated env: the same angle as the oracle's up to 2 ulp of theta
        d = np.hypot(last_obs[0, done] - ref.last_obs[0, done], last_obs[1, done] - ref.last_obs[1, done])
        assert (d <= 2 * np.spacing(np.abs(pre[0, done])) + 10 * atol).all()
        np.testing.assert_allclose(last_obs[2, done], ref.last_obs[2, done], rtol=rtol, atol=atol)
    else:
        np.testing.assert_allclose(last_obs[:, done], ref.last_obs[:, done], rtol=rtol, atol=atol)

    census = g.census(pre, ref0.t, ref0.done)
    for name in g.required:
        assert census[name] >= E.MIN_HITS, f"{g.id}: {name} is hit {census[name]} times"
    return census


@pytest.mark.parametrize("sid,n,packed", CASES, ids=CASE_IDS)
def test_env_step_on_every_branch(rl, sid, n, packed):
    one_step_checks(rl, E.grid(sid, n), packed)


@pytest.mark.parametrize("sid", BIG)
def test_env_step_on_every_branch_at_2p20(rl, sid):
    """n = 2^20: the non-temporal instantiation over the staggered layout; the n = 1024 grid 1024 times over"""
    g = E.tiled(E.grid(sid, 1024), 1024)
    g.required = ()  # the census of the tile is asserted at n = 1024
    for packed in (False, True):
        one_step_checks(rl, g, packed)
        torch.cuda.empty_cache()


@pytest.mark.parametrize("continuous", [False, True])
def test_mountaincar_energy_pumping_reaches_goal_and_wall(rl, continuous):
    """Free-running MountainCar under a = 2 if v >= 0 else 0 (continuous: +-1), 1024 envs, 260 steps, max_steps = 200: the
    cars reach the goal from step ~105 on and hit the wall on the way.  Flags and counters against the oracle at every step."""
    n = 1024
    env = rl.HipVecEnv("mountaincar", n, continuous=continuous, seed=31, env_id_base=17)
    ref = oracle.VecEnv("mountaincar", n, seed=31, env_id_base=17, continuous=continuous)
    goal, gv, lo = np.float32(ref.cfg.goal_pos), np.float32(ref.cfg.goal_velocity), np.float32(ref.cfg.min_pos)
    goals = walls = 0
    for step in range(260):
        v = host(env.raw_state()[1])
        a = np.where(v >= 0, 1.0, -1.0).astype(np.float32) if continuous else np.where(v >= 0, 2, 0).astype(np.int32)
        env.act0_(dev(a))
        ref.step(a)
        assert np.array_equal(host(env._done), ref.done), f"done differs at step {step}"
        assert np.array_equal(host(env._t), ref.t), f"t differs at step {step}"
        assert np.array_equal(host(env._episode).view(np.uint32), ref.episode), f"episode differs at step {step}"
        assert np.array_equal(host(env.reward()), ref.reward)
        goals += int(((ref.last_obs[0] >= goal) & (ref.last_obs[1] >= gv) & (ref.done == 1)).sum())
        walls += int((ref.last_obs[0] == lo).sum())
    assert goals >= 1024 and walls >= 256, (goals, walls)
    for k in range(2):
        np.testing.assert_allclose(host(env.raw_state()[k]), ref.s[k], rtol=1e-4, atol=1e-5)
