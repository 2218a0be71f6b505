"""The oracle's advantage normalisation branch (oracle/rlo_learn.c, rlo_ppo_loss_grad_f32 with normalize_advantage = 1) pinned
against a sequential Float64 restatement: the removed Zoo PPO's `(A - mean) / clamp(std, 1e-8, 1000)` per micro-batch, the
corrected std (divisor bm - 1, or 1 when bm <= 1), each sample rounded once to Float32.  The loss and gradient with the flag on
must equal, bit for bit, those with the flag off fed the restated advantages.  CPU only."""
import math

import numpy as np
import pytest

import oracle


def restate(adv):
    """sequential Float64 sums in sample order, as the oracle's loops"""
    bm = adv.size
    mu = 0.0
    for x in adv:
        mu += float(x)
    mu /= bm
    s2 = 0.0
    for x in adv:
        s2 += (float(x) - mu) * (float(x) - mu)
    sd = math.sqrt(s2 / (bm - 1 if bm > 1 else 1))
    sd = min(max(sd, 1e-8), 1000.0)
    return np.array([np.float32((float(x) - mu) / sd) for x in adv], np.float32), mu, sd


def _batch(rng, bm, ns, cont, adv):
    obs = rng.standard_normal((ns, bm)).astype(np.float32)
    act = rng.standard_normal((1, bm)).astype(np.float32) if cont else rng.integers(0, 2, bm).astype(np.int32)
    logp = (-rng.random(bm) - 0.3).astype(np.float32)
    ret = rng.standard_normal(bm).astype(np.float32)
    return obs, act, logp, adv.astype(np.float32), ret


def _check(cfg_kw, ns, na, cont, adv, seed=0):
    rng = np.random.default_rng(seed)
    on = oracle.ppo_default(normalize_advantage=1, continuous=int(cont), **cfg_kw)
    off = oracle.ppo_default(normalize_advantage=0, continuous=int(cont), **cfg_kw)
    kind = 1 if cont else 0
    params = (rng.standard_normal(oracle.ppo_nparams(kind, on)) * 0.3).astype(np.float32)
    obs, act, logp, adv, ret = _batch(rng, adv.size, ns, cont, adv)
    normed, mu, sd = restate(adv)
    g1, l1 = oracle.ppo_loss_grad(on, ns, na, params, obs, act, logp, adv, ret)
    g0, l0 = oracle.ppo_loss_grad(off, ns, na, params, obs, act, logp, normed, ret)
    assert np.array_equal(g1, g0) and np.array_equal(l1, l0)
    # and the flag changes something whenever the advantages are not already standardised
    graw, _ = oracle.ppo_loss_grad(off, ns, na, params, obs, act, logp, adv, ret)
    return g1, graw, mu, sd


@pytest.mark.parametrize("cont", [False, True])
@pytest.mark.parametrize("hidden,act", [(64, 0), (32, 1)])
def test_oracle_branch_equals_sequential_restatement(cont, hidden, act):
    rng = np.random.default_rng(3)
    adv = (300.0 + 40.0 * rng.standard_normal(517)).astype(np.float32)  # mean far from 0, std far from 1
    ns, na = (3, 1) if cont else (4, 2)
    g1, graw, mu, sd = _check(dict(hidden=hidden, act=act), ns, na, cont, adv)
    assert 250 < mu < 350 and 30 < sd < 50
    assert not np.array_equal(g1, graw)


def test_layers3_branch():
    rng = np.random.default_rng(4)
    adv = (-800.0 + 150.0 * rng.standard_normal(96)).astype(np.float32)  # Pendulum-like returns
    _check(dict(hidden=128, layers=3), 3, 1, True, adv)


def test_edge_single_sample():
    """bm = 1: divisor 1, std 0 -> clamped to 1e-8, the sample becomes exactly 0"""
    adv = np.array([42.5], np.float32)
    normed, mu, sd = restate(adv)
    assert sd == 1e-8 and normed[0] == 0.0
    _check(dict(hidden=16), 4, 2, False, adv)


def test_edge_constant_advantages():
    adv = np.full(64, 3.25, np.float32)
    normed, mu, sd = restate(adv)
    assert sd == 1e-8 and not normed.any()
    _check(dict(hidden=16), 4, 2, False, adv)


def test_edge_std_above_1000():
    rng = np.random.default_rng(5)
    adv = (5e4 * rng.standard_normal(200)).astype(np.float32)
    normed, mu, sd = restate(adv)
    assert sd == 1000.0 and np.abs(normed).max() > 10
    _check(dict(hidden=16), 4, 2, False, adv)


def test_ragged_split_microbatch():
    """100 envs x 7 steps, 3 micro-batches of 233 (one sample in none): the stats of the permuted micro-batch only"""
    n, T, nmb, seed, epoch = 100, 7, 3, 11, 2
    total, bm = n * T, (n * T) // nmb
    rng = np.random.default_rng(6)
    adv_all = (20.0 + 7.0 * rng.standard_normal(total)).astype(np.float32)
    for mb in range(nmb):
        perm = np.array([oracle.permute(seed, epoch, total, mb * bm + b) for b in range(bm)])
        _check(dict(hidden=32, n_microbatches=nmb), 4, 2, False, adv_all[perm], seed=mb)
