"""The two-action head of the fused rollout (csrc/ppo.hip rollout_split_kernel, HEAD == 2) decides the action without the
log-sum-exp (csrc/select_decide.h) and leaves logp to the critic wave, one step per lane every L steps.  Every trace must stay
bit for bit what the per-step protocol gives -- which runs categorical_select1 as before and shares none of that machinery --
on every flush boundary (T around multiples of L = 4 / 8 / 16), with ragged workgroups, on the exact-selection branch
(RLHIP_ROLLOUT_SELECT_MARGIN=inf, read once per process: a fresh child) and on a forced near-tie."""
import hashlib
import itertools
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIDDEN = (64, 128, 256)   # L = 4 / 8 / 16 lanes per env
ACTS = (0, 1)             # relu, tanh
NS = (5, 37, 130)         # fewer envs than one workgroup holds; ragged; more than one workgroup at L = 4 / 8 / 16
TS = (1, 15, 16, 17, 33, 40)
GRID = list(itertools.product(HIDDEN, ACTS, NS, TS))
PERIODS = 3
TRACES = ("obs", "logp", "value", "reward", "terminal", "adv", "ret", "action_i")


def _pair(rl, hidden, act, n, T, seed=3, params=None):
    env = rl.HipVecEnv("cartpole", n, seed=seed)
    return env, rl.PPOPolicy(env, update_freq=T, hidden=hidden, act=act, params=params)


def _digests(rl):
    """sha256 over every trace and the env state of PERIODS consecutive fused rollouts, per case of GRID"""
    import torch

    out = {}
    for hidden, act, n, T in GRID:
        env, pol = _pair(rl, hidden, act, n, T)
        h = hashlib.sha256()
        for _ in range(PERIODS):
            pol.rollout_()
            tr = pol.trajectory
            for t in [getattr(tr, name) for name in TRACES] + [env.raw_state(), env._t, env._episode, env.reward(), env._done]:
                h.update(t.cpu().numpy().tobytes())
        torch.cuda.synchronize()
        out[f"{hidden}-{act}-{n}-{T}"] = h.hexdigest()
    return out


if __name__ == "__main__":  # the child of test_exact_selection_branch_gives_the_same_bits
    for p in (ROOT, os.path.join(ROOT, "reinforcementlearning.jl_amd")):
        sys.path.insert(0, p)
    import rlhip

    with open(sys.argv[1], "w") as fh:
        json.dump(_digests(rlhip), fh)
    sys.exit(0)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import oracle  # noqa: E402


@pytest.fixture(scope="module")
def rl():
    import rlhip

    return rlhip


@pytest.mark.parametrize("hidden,act,n,T", GRID)
def test_fast_select_rollout_equals_stepwise_bit_exact(rl, hidden, act, n, T):
    envA, polA = _pair(rl, hidden, act, n, T)
    envB, polB = _pair(rl, hidden, act, n, T)
    for it in range(PERIODS):
        polA.rollout_()
        for t in range(T):
            a = polB.plan_()
            polB.push_preact_()
            envB.act_(a)
            polB.push_postact_()
        polB.finish_rollout_()
        polB.gae_()
        ta, tb = polA.trajectory, polB.trajectory
        for name in ("obs", "logp", "value", "reward", "terminal", "adv", "ret"):
            assert torch.equal(getattr(ta, name), getattr(tb, name)), f"{name} differs (period {it})"
        assert torch.equal(ta.action, tb.action)
        assert torch.equal(envA.raw_state(), envB.raw_state())
        assert torch.equal(envA._t, envB._t) and torch.equal(envA._episode, envB._episode)
        assert torch.equal(envA.reward(), envB.reward()) and torch.equal(envA._done, envB._done)


def test_exact_selection_branch_gives_the_same_bits(rl, tmp_path):
    """RLHIP_ROLLOUT_SELECT_MARGIN=inf: no draw is decided by the fast rule, every wavefront runs categorical_select1 behind
    the wave-uniform branch -- same traces as the default margin, over the whole grid"""
    out = str(tmp_path / "digests.json")
    env = dict(os.environ, RLHIP_ROLLOUT_SELECT_MARGIN="inf")
    subprocess.run([sys.executable, os.path.abspath(__file__), out], check=True, env=env, timeout=300)
    with open(out) as fh:
        child = json.load(fh)
    assert os.environ.get("RLHIP_ROLLOUT_SELECT_MARGIN") in (None, "", "1")
    here = _digests(rl)
    assert len(child) == len(GRID)
    assert {k for k in here if here[k] != child.get(k)} == set()


def _gumbel(seed, idx, step):
    w = oracle.philox(seed, idx, 0, step, oracle.TAG["GUMBEL"])
    return [-math.log(-math.log(oracle.u01_f64(w[0], w[1]))), -math.log(-math.log(oracle.u01_f64(w[2], w[3])))]


@pytest.mark.parametrize("hidden", HIDDEN)
def test_forced_near_tie_takes_the_oracles_action(rl, hidden):
    """zero actor weights, so the logits are the output biases (0, b1) for every env and step; b1 = RN32(nz0 - nz1) of (env 0,
    step 0) puts that draw within 2^-24 |nz0 - nz1| of the tie, inside the threshold of the default margin"""
    n, T, ns = 5, 17, 4
    env, pol = _pair(rl, hidden, 0, n, T)
    nz0, nz1 = _gumbel(pol.seed, env.env_id_base, 0)
    b1 = np.float32(nz0 - nz1)
    p = pol.params.cpu().numpy().copy()
    p[: pol.np_actor] = 0.0
    p[hidden * (ns + 3) + 1] = b1  # W1 (h x ns), b1 (h), W2 (2 x h), b2 (2)
    assert pol.np_actor == hidden * (ns + 3) + 2
    d = abs(float(b1))
    delta = (nz1 - nz0) + float(b1)
    thr = 2.0 ** -22 * (d + 2) + 2.0 ** -48 * (abs(nz0) + abs(nz1) + d + 2)
    assert abs(delta) < thr / 4, (delta, thr)
    env, pol = _pair(rl, hidden, 0, n, T, params=p)
    pol.rollout_()
    oenv = oracle.VecEnv("cartpole", n, seed=3)
    otr = oracle.PPOTraj(0, n, T)
    oracle.ppo_rollout(oenv, T, oracle.ppo_default(hidden=hidden), p, otr, 0)
    tr = pol.trajectory
    # the logits are exact on both sides, so every action of every env is the oracle's -- the near-tie one included
    assert int(tr.action_i[0, 0]) == int(otr.action_i[0, 0])
    assert np.array_equal(tr.action_i.cpu().numpy(), otr.action_i)
    assert np.array_equal(tr.terminal.cpu().numpy(), otr.terminal)
    np.testing.assert_allclose(tr.logp.cpu().numpy(), otr.logp, rtol=1e-6, atol=0)
