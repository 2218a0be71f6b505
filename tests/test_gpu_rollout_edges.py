"""The parts of the fused rollout (csrc/ppo.hip rollout_split_kernel) that lie outside its step loop: the net and state loads
and the first noise chunk in front of step 0; behind step T - 1 the bootstrap value, the GAE + returns scan -- whose operands
the critic wave keeps in LDS while T fits the scan buffer (32 steps), read back from global memory beyond -- and the state
write-back.  Every trace, the env state and adv / ret of two consecutive periods must be bit for bit what the per-step protocol
gives (plan / push / act / push launches and the stand-alone scan: none of the fused kernel's machinery), adv / ret bit for bit
the oracle's scan of the recorded traces, and every step must pass the per-step audit of tests/rollout_audit.py.

Shapes: T = 1 and 2 are shorter than a noise chunk and than a lane group, 15 / 16 / 17 straddle the chunk, 33 is one step past
the scan buffer; n = 5 / 16 / 37 leave the last workgroup ragged at every width (16 / 32 / 64 envs per workgroup); max_steps = 5
ends an episode every few steps, so the scan meets terminals at every T >= 5 and the write-back a fresh reset.  The last test
hands the kernel a parameter vector 4 bytes past a 16-byte boundary."""
import itertools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import oracle  # noqa: E402
import rollout_audit as A  # noqa: E402

HEADS = {"2-action": ("cartpole", False), "3-action": ("mountaincar", False), "gaussian": ("pendulum", True)}
HIDDEN = (64, 128, 256)  # L = 4 / 8 / 16 lanes per env
ACTS = (0, 1)            # relu, tanh
NS = (5, 16, 37)
TS = (1, 2, 15, 16, 17, 33)
MAX_STEPS = 5
PERIODS = 2
GRID = list(itertools.product(HEADS, HIDDEN, ACTS, NS, TS))
OFFSET_GRID = list(itertools.product(HEADS, HIDDEN, ACTS))


@pytest.fixture(scope="module")
def rl():
    import rlhip

    return rlhip


def host(t):
    return t.detach().cpu().numpy().copy()


def _case(head, hidden, act, n, T):
    env, cont = HEADS[head]
    return dict(id=f"edges-{head}-h{hidden}-act{act}-n{n}-T{T}", kernel="rollout_split_kernel", env=env, hidden=hidden, act=act,
                layers=2, continuous=cont, n=n, T=T, max_steps=MAX_STEPS, seed=3 + (n + T) % 5, env_id_base=1000 + 17 * T + n,
                bf16=False)


def _pair(rl, c, params, offset=False):
    env = rl.HipVecEnv(c["env"], c["n"], seed=c["seed"], env_id_base=c["env_id_base"], **A.env_kwargs(c))
    pol = rl.PPOPolicy(env, update_freq=c["T"], hidden=c["hidden"], act=c["act"])
    assert pol.np == params[0].size and pol.np_actor == params[1] and pol.seed == c["seed"]
    if offset:  # the same values, one Float32 past a 16-byte boundary
        buf = torch.empty(pol.np + 5, dtype=torch.float32, device=pol.params.device)
        pol.params = buf[(16 - buf.data_ptr() % 16) // 4 % 4 + 1:][:pol.np]
        assert pol.params.data_ptr() % 16 == 4
    pol.params.copy_(torch.as_tensor(params[0]).cuda())
    return env, pol


def _snapshot(env):
    return dict(raw_state=host(env.raw_state()), t=host(env._t), episode=host(env._episode), reward=host(env.reward()),
                done=host(env._done))


def _run(rl, c, offset=False):
    params = A.make_params(c)
    envA, polA = _pair(rl, c, params, offset)
    envB, polB = _pair(rl, c, params)
    bars, T = A.make_bars(c), c["T"]
    terminals = 0
    for period in range(PERIODS):
        env0 = _snapshot(envA)
        polA.rollout_()
        for _ in range(T):
            a = polB.plan_()
            polB.push_preact_()
            envB.act_(a)
            polB.push_postact_()
        polB.finish_rollout_()
        polB.gae_()
        ta, tb = polA.trajectory, polB.trajectory
        for name in ("obs", "logp", "value", "reward", "terminal", "adv", "ret"):
            assert torch.equal(getattr(ta, name), getattr(tb, name)), f"{name} differs from the per-step protocol (period {period})"
        assert torch.equal(ta.action, tb.action)
        assert torch.equal(envA.raw_state(), envB.raw_state())
        assert torch.equal(envA._t, envB._t) and torch.equal(envA._episode, envB._episode)
        assert torch.equal(envA.reward(), envB.reward()) and torch.equal(envA._done, envB._done)
        # the oracle: its scan of the recorded traces bit for bit (inside audit()), every step against a restarted env
        traj = {k: host(getattr(ta, k)) for k in ("obs", "value", "logp", "reward", "terminal", "adv", "ret", "action_i")}
        traj["action_f"] = host(ta.action_f)[:, 0]
        adv = oracle.generalized_advantage_estimation(traj["reward"].T, traj["value"].T, A.GAMMA, A.LAM, terminal=traj["terminal"].T,
                                                      dims=2, dtype=np.float32).T
        assert np.array_equal(traj["adv"], adv), f"adv differs from the oracle's scan (period {period})"
        assert np.array_equal(traj["ret"], (adv + traj["value"][:T]).astype(np.float32)), f"ret differs (period {period})"
        fails, _ = A.check(A.audit(traj, env0, _snapshot(envA), params, c, period * T), bars)
        assert not fails, fails
        terminals += int(traj["terminal"].sum())
    if PERIODS * T >= 2 * MAX_STEPS:
        assert terminals >= c["n"], "the scan met hardly a terminal"


@pytest.mark.parametrize("head,hidden,act,n,T", GRID)
def test_rollout_edges_equal_stepwise_and_oracle_bit_exact(rl, head, hidden, act, n, T):
    _run(rl, _case(head, hidden, act, n, T))


@pytest.mark.parametrize("head,hidden,act", OFFSET_GRID)
def test_rollout_edges_with_params_off_16_byte_alignment(rl, head, hidden, act):
    """n = 37 and T = 17: a ragged workgroup, a second noise chunk, the LDS scan"""
    _run(rl, _case(head, hidden, act, 37, 17), offset=True)
