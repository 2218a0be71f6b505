"""The loss / gradient of rlhip_dqn_grad_batch_f32 (include/rlhip.h) composed from the oracle's existing C functions -- no new oracle code:

    sel  = max_o Qt(s')[o], or Qt(s')[findmax(Q(s'))] for Double DQN     oracle.mlp2_forward, oracle.findmax (the first maximum wins)
    y    = r + (disc * cont) * sel                                       numpy Float32, one rounding per operation, no contraction;
                                                                         disc = gamma, or oracle.gamma_pow(gamma, clamp(n_used, 0, 32))
    loss, grad = oracle.dqn_loss_grad(..., r = y, term = 1, gamma)       its target line gives y + gamma * 0 * max = y + 0 = y: the
                                                                         trick of DoubleTargetFold (tests/double_dqn_ref.py)

and the seeded input sets of tests/test_gpu_dqn_batch.py with their census.  Shared by tests/test_dqn_batch_reference.py (CPU) and the GPU
tests."""
import numpy as np

import oracle

TILE = 64            # samples per tile of dqn_grad_batch_kernel
MAX_ROWS = 256       # partial rows: a batch above TILE * MAX_ROWS gives workgroup 0 a second tile
NS, HS, NAS, ACTS = (5, 6, 16), (4, 64, 128, 256), (1, 3, 4), (0, 1)
BATCHES = (1, TILE - 1, TILE, TILE + 1, 512)
BIG_BATCH = TILE * MAX_ROWS + 1
DELTA = 1.0
U = 2.0 ** -24


def discounts(gamma, n_used):
    if n_used is None:
        return np.float32(gamma)
    pw = np.array([oracle.gamma_pow(gamma, n) for n in range(33)], np.float32)
    return pw[np.clip(np.asarray(n_used, np.int64), 0, 32)]


def target(ns, h, na, act, p, pt, r, term, sn, gamma, n_used=None, double_dqn=False):
    """-> (y, index of the selected action)"""
    qt = oracle.mlp2_forward(pt, ns, h, na, act, sn)
    b = qt.shape[1]
    src = oracle.mlp2_forward(p, ns, h, na, act, sn) if double_dqn else qt
    astar = np.array([oracle.findmax(np.ascontiguousarray(src[:, i]), dtype=np.float32) for i in range(b)], np.int64)
    sel = qt[astar, np.arange(b)]
    cont = np.where(np.asarray(term) != 0, np.float32(0), np.float32(1)).astype(np.float32)
    dc = (discounts(gamma, n_used) * cont).astype(np.float32)
    y = (np.asarray(r, np.float32) + (dc * sel).astype(np.float32)).astype(np.float32)
    return y, astar


def loss_grad(ns, h, na, act, p, pt, s, a, r, term, sn, gamma, delta=DELTA, n_used=None, weights=None, double_dqn=False, dropped=()):
    """-> (loss, grad, td).  dropped: samples that contribute nothing (the kernel's rule for an action outside 0 .. na - 1): their
    weight is 0 and their action is replaced by a valid one"""
    y, _ = target(ns, h, na, act, p, pt, r, term, sn, gamma, n_used, double_dqn)
    a = np.asarray(a, np.int32).copy()
    w = None if weights is None else np.asarray(weights, np.float32).copy()
    if len(dropped):
        w = np.ones(len(y), np.float32) if w is None else w
        w[list(dropped)] = 0.0
        a[list(dropped)] = 0
    loss, grad = oracle.dqn_loss_grad(ns, h, na, act, p, pt, s, a, y, np.ones(len(y), np.uint8), sn, gamma, delta, weights=w)
    q = oracle.mlp2_forward(p, ns, h, na, act, s)
    td = np.abs(q[a, np.arange(len(y))] - y).astype(np.float32)
    if len(dropped):
        td[list(dropped)] = 0.0
    return loss, grad, td


def split(g, ns, h, na):
    """flat vector -> {W1, b1, W2, b2}"""
    o1, o2, o3 = h * ns, h * ns + h, h * ns + h + na * h
    return {"W1": g[:o1], "b1": g[o1:o2], "W2": g[o2:o3], "b2": g[o3:]}


def _hidden64(p, ns, h, act, x):
    W1 = p[:h * ns].reshape(ns, h).T.astype(np.float64)
    z = W1 @ x.astype(np.float64) + p[h * ns:h * ns + h].astype(np.float64)[:, None]
    return np.maximum(z, 0.0) if act == 0 else np.tanh(z)


def reorder_bound(p, ns, h, na, act, x):
    """per sample: the largest, over the outputs o, of (h + 2) 2^-24 (|b2[o]| + sum_j |W2[o, j] h_j|) -- what a re-ordered Float32
    sum of Q[o] can move by"""
    hid = np.abs(_hidden64(p, ns, h, act, x))
    W2 = np.abs(p[h * ns + h:h * ns + h + na * h].reshape(h, na).T.astype(np.float64))
    b2 = np.abs(p[h * ns + h + na * h:].astype(np.float64))
    return (h + 2) * U * (b2[:, None] + W2 @ hid).max(0)


def top_two_gap(q):
    if q.shape[0] == 1:
        return np.full(q.shape[1], np.inf)
    s = np.sort(q.astype(np.float64), axis=0)
    return s[-1] - s[-2]


def census(case):
    """number of samples whose Double DQN decision a re-ordered sum could flip: top-two gap of the model's online Q(s') <= 2 x bound"""
    ns, h, na, act = case["shape"]
    q = oracle.mlp2_forward(case["p"], ns, h, na, act, case["sn"])
    return int((top_two_gap(q) <= 2.0 * reorder_bound(case["p"], ns, h, na, act, case["sn"])).sum())


def flags(k):
    """the k-th combination of (n_used, weights, double_dqn, td_out)"""
    return dict(n_used=bool(k & 1), weights=bool(k & 2), double_dqn=bool(k & 4), td=not (k & 8))


def make_case(ns, h, na, act, batch, seed, n_used=False, weights=False, double_dqn=False, td=True, gamma=0.97):
    """a seeded input set.  Next states whose online top-two gap is within 4 x the re-ordering bound are drawn again (the census
    asks for 2 x); the first rows are made terminal with d = 0 in the model, and the rewards put |d| on both sides of delta."""
    rng = np.random.default_rng(seed)
    npar = oracle.mlp2_nparams(ns, h, na)
    p = oracle.mlp2_init(ns, h, na, seed, 0) + (0.05 * rng.standard_normal(npar)).astype(np.float32)
    pt = oracle.mlp2_init(ns, h, na, seed, 1) + (0.05 * rng.standard_normal(npar)).astype(np.float32)
    s = rng.standard_normal((ns, batch)).astype(np.float32)
    sn = (s + 0.5 * rng.standard_normal((ns, batch))).astype(np.float32)
    for _ in range(64):
        q = oracle.mlp2_forward(p, ns, h, na, act, sn)
        close = top_two_gap(q) <= 4.0 * reorder_bound(p, ns, h, na, act, sn)
        if not close.any():
            break
        sn[:, close] = rng.standard_normal((ns, int(close.sum()))).astype(np.float32)
    a = rng.integers(0, na, batch).astype(np.int32)
    # Conditioning.  A re-ordered Float32 sum moves Q(s)[a] and the target by a few 2^-24 of their magnitude, i.e. it moves a sample's
    # dL/dq = d / batch by an ABSOLUTE amount that does not shrink with d.  The bar of the GPU test is relative to the largest element of
    # a tensor, and db2 has only `na` elements, each the sum of dL/dq over the samples that took the action: were the TD errors centred
    # on zero that sum would cancel and the bar would measure the cancellation, not the kernel (a batch of one sample is the same
    # statement about its single d).  So the rewards are laid around the model's own values such that d = Q - y = -(1.5 + N(0, 1)):
    # negative for most samples, of either sign for some, |d| on both sides of delta, and `conditioning` (asserted on the CPU, from
    # the model alone) stays of order one.
    term = (rng.random(batch) < 0.2).astype(np.uint8)
    nu = rng.integers(1, 33, batch).astype(np.int32) if n_used else None  # (a terminal row with n_used < 32: a window cut by it)
    w = rng.uniform(0.1, 1.0, batch).astype(np.float32) if weights else None
    boot, _ = target(ns, h, na, act, p, pt, np.zeros(batch, np.float32), term, sn, gamma, nu, double_dqn)  # (disc * cont) * sel
    dwant = -(1.5 + rng.standard_normal(batch))
    if batch < 8:  # few samples: none of them may sit on a cancelling difference
        dwant[np.abs(dwant) < 0.5] -= 1.0
    r = (oracle.mlp2_forward(p, ns, h, na, act, s)[a, np.arange(batch)] - boot - dwant).astype(np.float32)
    # d = 0: terminal rows whose reward is the model's Q(s)[a] -- beside other rows only: a batch of nothing but such rows has the
    # gradient 0, against which no relative bar can be stated
    k0 = 3 if batch >= 8 else 0
    q = oracle.mlp2_forward(p, ns, h, na, act, s)
    term[:k0] = 1
    r[:k0] = q[a[:k0], np.arange(k0)]
    return dict(shape=(ns, h, na, act), batch=batch, p=p, pt=pt, s=s, a=a, r=r, term=term, sn=sn, gamma=gamma, delta=DELTA, n_used=nu,
                weights=w, double_dqn=double_dqn, td=td)


def conditioning(c):
    """the largest, over the actions o, of sum_{i: a_i = o} (|Q(s_i)[a_i]| + |y_i|) w_i / batch, over the largest |db2[o]| (the bar is
    relative to a tensor's largest element): how many times the absolute rounding error of the dL/dq (see make_case) is amplified in
    the gradient's smallest tensor"""
    ns, h, na, act = c["shape"]
    b = c["batch"]
    y, _ = target(ns, h, na, act, c["p"], c["pt"], c["r"], c["term"], c["sn"], c["gamma"], c["n_used"], c["double_dqn"])
    q = oracle.mlp2_forward(c["p"], ns, h, na, act, c["s"])[c["a"], np.arange(b)].astype(np.float64)
    d = q - y
    w = np.ones(b) if c["weights"] is None else c["weights"].astype(np.float64)
    gi = np.clip(d, -c["delta"], c["delta"]) * w / b
    mag = (np.abs(q) + np.abs(y)) * w / b
    db2 = np.array([gi[c["a"] == o].sum() for o in range(na)])
    return float(max(mag[c["a"] == o].sum() for o in range(na)) / np.abs(db2).max())


def case_loss_grad(c, dropped=()):
    ns, h, na, act = c["shape"]
    return loss_grad(ns, h, na, act, c["p"], c["pt"], c["s"], c["a"], c["r"], c["term"], c["sn"], c["gamma"], c["delta"], c["n_used"],
                     c["weights"], c["double_dqn"], dropped)


def grid():
    """(ns, h, na, act) x the batches, each with its combination of the optional arguments: all sixteen are hit many times"""
    out, k = [], 0
    for ns in NS:
        for h in HS:
            for na in NAS:
                for act in ACTS:
                    out.append(((ns, h, na, act), [(b, k + i) for i, b in enumerate(BATCHES)]))
                    k += len(BATCHES)
    return out
