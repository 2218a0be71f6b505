"""The Double DQN target composed from the oracle's existing C functions (no new oracle code): Q(s') and Qt(s') from
`oracle.mlp2_forward` / `oracle.mlp3_forward`, a* from `oracle.findmax` (first maximum wins, RLCore/src/utils/basic.jl:91-120),
y = r + gamma * (1 - t) * Qt(s')[a*] in Float32 without contraction -- the order of the target line of oracle/rlo_learn.c.
Shared by tests/test_double_dqn_reference.py (CPU) and tests/test_gpu_double_dqn.py."""
import numpy as np

import oracle


def forward(layers, p, ns, h, na, act, x):
    return (oracle.mlp2_forward if layers == 2 else oracle.mlp3_forward)(p, ns, h, na, act, x)


def compose(layers, ns, h, na, act, p, pt, r, t, sn, gamma):
    """-> (y, a*, Q(s'), Qt(s')): the oracle's Double DQN target of a batch"""
    q, qt = forward(layers, p, ns, h, na, act, sn), forward(layers, pt, ns, h, na, act, sn)
    b = q.shape[1]
    astar = np.array([oracle.findmax(np.ascontiguousarray(q[:, i]), dtype=np.float32) for i in range(b)], np.int64)
    cont = np.where(np.asarray(t) != 0, np.float32(0), np.float32(1)).astype(np.float32)
    y = (np.asarray(r, np.float32) + (np.float32(gamma) * cont) * qt[astar, np.arange(b)]).astype(np.float32)
    return y, astar, q, qt


def top_two_gap(q):
    s = np.sort(q, axis=0)
    return s[-1] - s[-2]


def loss_grad(layers, ns, h, na, act, p, pt, s, a, y, sn, gamma, delta=1.0, weights=None):
    """the oracle's DQN loss / gradient on the folded batch (reward = y, terminal = 1): its target line gives y + 0 = y"""
    one = np.ones(len(y), np.uint8)
    if layers == 2:
        return oracle.dqn_loss_grad(ns, h, na, act, p, pt, s, a, y, one, sn, gamma, delta, weights=weights)
    return oracle.dqn3_loss_grad(ns, h, na, act, p, pt, s, a, y, one, sn, gamma, delta, weights=weights)[:2]


def trained_nets(layers, ns, h, na, act, seed, steps=300, batch=256):
    """(online, target) parameters whose Q-values have separated: Glorot from mlp*_init, then `steps` Adam steps of the oracle's own
    DQN update on synthetic transitions (target synchronised every 50 steps, last 25 steps before the end: online != target)"""
    rng = np.random.default_rng(seed)
    init = oracle.mlp2_init if layers == 2 else oracle.mlp3_init
    p = init(ns, h, na, seed, 0)
    pt = p.copy()
    m, v = np.zeros_like(p), np.zeros_like(p)
    for k in range(steps):
        s = rng.standard_normal((ns, batch)).astype(np.float32)
        sn = (s + 0.1 * rng.standard_normal((ns, batch))).astype(np.float32)
        a = rng.integers(0, na, batch).astype(np.int32)
        r = (s[0] * (a - (na - 1) / 2) + 0.5 * np.sin(3 * s[1] + a)).astype(np.float32)  # rewards that tell the actions apart
        t = (rng.random(batch) < 0.05).astype(np.uint8)
        if layers == 2:
            _, g = oracle.dqn_loss_grad(ns, h, na, act, p, pt, s, a, r, t, sn, 0.9, 1.0)
        else:
            _, g, _ = oracle.dqn3_loss_grad(ns, h, na, act, p, pt, s, a, r, t, sn, 0.9, 1.0)
        oracle.adam(p, g, m, v, 3e-3, 0.9, 0.999, 1e-8, k + 1)
        if (k + 1) % 50 == 25:
            pt = p.copy()
    return p, pt
