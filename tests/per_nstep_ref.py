"""Prioritized n-step replay composed from the oracle's existing Python binding (no new oracle code): `Ring`, `SumTree.fill_range` for
the lagged push, `ring_sample_prioritized` on the masked tree, `ring_gather_nstep` for the window fold, `per_is_weights`,
`dqn_loss_grad` / `dqn3_loss_grad` with `weights`, `per_priority`, `SumTree.update`, and the oracle's clip + Adam.
Shared by tests/test_per_nstep_reference.py (CPU) and tests/test_gpu_per_nstep.py."""
import numpy as np

import oracle
from double_dqn_ref import compose, forward, loss_grad


def push_priority_nstep(ring, st, priority, n_step):
    """after ring.push_transition, in place of oracle.ring_push_priority: the newest frame := 0, then logical frame
    len - n_step := priority once it exists (n_step = 1: the newest frame := priority)"""
    cap, n_env, head, ln = ring.rb.capacity, ring.rb.n_env, ring.rb.head_rt, len(ring)
    newest = (head + ln - 1) % cap
    if n_step > 1:
        st.fill_range(newest * n_env, n_env, 0.0)
        if ln < n_step:
            return
    st.fill_range(((head + ln - n_step) % cap) * n_env, n_env, priority)


class Mirror:
    """an oracle ring with its masked sum-tree, pushed in step with the device traces"""

    def __init__(self, capacity, n_env, obs_dim, n_step, default_priority):
        self.ring = oracle.Ring(capacity, n_env, obs_dim)
        self.st = oracle.SumTree(capacity * n_env)
        self.n_step, self.default_priority = n_step, default_priority

    def push_state(self, obs):
        self.ring.push_state(obs)

    def push_transition(self, nobs, a, r, t):
        self.ring.push_transition(nobs, a, r, t)
        push_priority_nstep(self.ring, self.st, self.default_priority, self.n_step)


def sample_fold(ring, st, batch, n_step, gamma, seed, draw_ctr):
    """-> (idx, key, prio, (s, a, R, t, s_n)): the prioritized draw on the masked tree, then the n-step window of every start"""
    idx, key, prio = oracle.ring_sample_prioritized(ring, st, batch, seed, draw_ctr)
    return idx, key, prio, oracle.ring_gather_nstep(ring, idx, n_step, gamma)


def record_words(ns, s, a, R, t, sn):
    """the folded batch as the (batch, 16) uint32 words of its 64-byte records (csrc/ring_device.h)"""
    b = len(a)
    w = np.zeros((b, 16), np.uint32)
    w[:, :ns] = np.ascontiguousarray(s.T, np.float32).view(np.uint32)
    w[:, 4] = np.asarray(a, np.int32).view(np.uint32)
    w[:, 5] = np.asarray(R, np.float32).view(np.uint32)
    w[:, 6] = (np.asarray(t) != 0).astype(np.uint32)
    w[:, 8:8 + ns] = np.ascontiguousarray(sn.T, np.float32).view(np.uint32)
    return w


def learner_update(layers, ns, h, na, act, p, pt, batch_sarts, gamma_n, prio, beta, double_dqn, delta=1.0):
    """one update's target side from the oracle: -> (plain gradient of p, priorities to write back)"""
    s, a, R, t, sn = batch_sarts
    w = oracle.per_is_weights(prio, beta) if beta > 0.0 else None
    qa = forward(layers, p, ns, h, na, act, s)[a, np.arange(len(a))]
    if double_dqn:
        y, *_ = compose(layers, ns, h, na, act, p, pt, R, t, sn, gamma_n)
        _, g = loss_grad(layers, ns, h, na, act, p, pt, s, a, y, sn, gamma_n, delta, weights=w)
    else:
        cont = np.where(np.asarray(t) != 0, np.float32(0), np.float32(1)).astype(np.float32)
        y = (R + (np.float32(gamma_n) * cont) * forward(layers, pt, ns, h, na, act, sn).max(0)).astype(np.float32)
        if layers == 2:
            _, g = oracle.dqn_loss_grad(ns, h, na, act, p, pt, s, a, R, t, sn, gamma_n, delta, weights=w)
        else:
            _, g, _ = oracle.dqn3_loss_grad(ns, h, na, act, p, pt, s, a, R, t, sn, gamma_n, delta, weights=w)
    return g, oracle.per_priority(np.abs(qa - y), 1e-6, 0.6)
