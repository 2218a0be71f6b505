"""The seeded case grid of the QR-DQN kernels with its census (plain numpy and the CPU models of tests/qrdqn_ref.py; no GPU): the grid and
the census of tests/c51_cases.py with n_quantiles and kappa in place of the atoms and the support.

A case is a dictionary: the online and the target network (flat Float32 vectors, non-zero biases, the target far enough from the online
net that their greedy actions differ on many samples), a GATHERED batch (s, a, r, term, s' [, n_used] [, weights]) and the scalars.
Rewards are planted, four samples in turn (kind = i % 5; kind 4 keeps its drawn reward), from the sample's own quantiles th_k = th(s)[k, a_i]:
  0  the whole row above: every T_j > every th_k + kappa                    1  the whole row below: every T_j < every th_k - kappa
  2  terminal (c = 0, every T_j = r): r = th_k0 + 0.37 kappa, strictly inside for quantile k0
  3  terminal: r = th_k0 to the bit, u == 0 for quantile k0
(kinds 2 and 3 are not planted where the case has no terminal sample).

Axes (every value below occurs; `test_every_class_of_the_census_is_populated` counts them):
  batch    1, TILE - 1, TILE, TILE + 1, 2 TILE + 2 (TILE = 8, the gradient kernel's tile)       N  1, 2, 3, 51, 64      kappa  0.25, 1, 10
  na       1, 2, 4                      ns  2, 4, 5, 16                    h  4, 64, 256            act      relu, tanh
  term     all terminal, none terminal, mixed                             n_used  -1, 0, 1, 32, 40 (cycled) or NULL
  weights  given, NULL                  double_dqn  both flags             action  one outside 0 .. na - 1

Decisions.  With kappa > 0 the gradient is continuous in u, so the only decisions are a* and the sign of a ReLU pre-activation.  A sample
is COUNTED when (i) the float64 model's top-two gap of the selecting Q(s') exceeds 4 x the Float32 budget of those values (two
evaluations, each within 2 x budget of its centre) and (ii), ReLU cases only, every layer-1 pre-activation of every pass has
|z1| >= 1e-5.  The builder walks the case's seed upwards until NO sample is excluded (the cap is 2 % per case; zero is inside it), at
most 64 steps, so the grid is a fixed function of this file and every comparison runs on all samples."""
import functools

import numpy as np

import qrdqn_ref as R
from c51_cases import _net
from heads_ref import F32

TILE = 8
BATCHES = (1, TILE - 1, TILE, TILE + 1, 2 * TILE + 2)
N_USED = (-1, 0, 1, 32, 40)
QUANTILES = (1, 2, 3, 51, 64)
KAPPAS = (0.25, 1.0, 10.0)
GAMMA = 0.9
CLASSES = ("u_below", "u_neg_inside", "u_zero", "u_pos_inside", "u_above")


def _build(name, ns, h, na, N, act, batch, seed, kappa=1.0, term="mixed", n_used=False, weights=False, double=False, bad_action=False):
    rng = np.random.default_rng(seed)
    M = na * N
    c = dict(name=name, ns=ns, h=h, na=na, N=N, act=act, batch=batch, seed=seed, kappa=kappa, gamma=GAMMA, double=bool(double), term_mode=term)
    c["params"] = _net(rng, ns, h, M)
    c["target"] = (c["params"] + rng.normal(0, 0.25, c["params"].shape)).astype(F32)
    c["s"] = rng.normal(0, 1, (ns, batch)).astype(F32)
    c["sn"] = rng.normal(0, 1, (ns, batch)).astype(F32)
    a = rng.integers(0, na, batch).astype(np.int32)
    t = {"all": np.ones(batch), "none": np.zeros(batch), "mixed": rng.uniform(size=batch) < 0.3}[term].astype(np.uint8)
    r = rng.normal(0.3, 1.0, batch).astype(F32)
    th = R.forward(c["params"], ns, h, M, act, c["s"])[0].reshape(na, N, batch)[a, :, np.arange(batch)]  # (batch, N): th(s)[k, a_i]
    tht = np.abs(R.forward(c["target"], ns, h, M, act, c["sn"])[0]).max(0)                                 # (batch,): max |th_t(s')|
    kind = np.full(batch, -1)
    for i in range(batch):  # the planted rewards, four samples in turn; kinds 2 and 3 are terminal unless the case has no terminal
        k = i % 5
        far = F32(kappa) + F32(1) + tht[i]  # |c| <= 1: c th_t(s') cannot bring a T_j back
        if k == 0:
            r[i] = F32(th[i].max() + far)
        elif k == 1:
            r[i] = F32(th[i].min() - far)
        elif k == 2 and term != "none":
            r[i], t[i] = F32(th[i, (i // 5) % N] + F32(0.37) * F32(kappa)), 1
        elif k == 3 and term != "none":
            r[i], t[i] = th[i, (i // 5) % N], 1
        kind[i] = k
    c.update(a=a, r=r, term=t, kind=kind)
    c["n_used"] = np.array([N_USED[i % 5] for i in range(batch)], np.int32) if n_used else None
    c["weights"] = rng.uniform(0.2, 1.0, batch).astype(F32) if weights else None
    if bad_action:
        c["a"][batch // 2] = na if (batch // 2) % 2 == 0 else -1
    return c


def census(c):
    """-> (number of samples on a decision, dict of what the case holds, (replay, model, budgets))"""
    rp = R.replay(c)
    m = R.torch_model(c, rp)
    b = R.budgets(c, rp)
    bq = b["q_o"] if c["double"] else b["q_t"]
    bad = np.zeros(c["batch"], bool)
    if c["na"] > 1:
        bad |= m["gap"] <= 4.0 * bq.max(0)
    if c["act"] == 0:
        for zz in (rp["z1"], rp["z1_t"]) + ((rp["z1_o"],) if c["double"] else ()):
            bad |= (np.abs(zz) < 1e-5).any(0)
    u, kap = rp["u"][:, :, rp["known"]], F32(c["kappa"])
    rows = rp["u"]  # (Nj, Nk, B)
    sel_t = np.argmax(rp["qt"], 0)
    holds = dict(u_below=int((u < -kap).sum()), u_neg_inside=int(((u >= -kap) & (u < 0)).sum()), u_zero=int((u == 0).sum()),
                 u_pos_inside=int(((u > 0) & (u <= kap)).sum()), u_above=int((u > kap).sum()),
                 row_above=int((rows > kap).all((0, 1)).sum()), row_below=int((rows < -kap).all((0, 1)).sum()),
                 c0=int((rp["cc"] == 0).sum()), terminal=int((c["term"] != 0).sum()), not_terminal=int((c["term"] == 0).sum()),
                 argmax_differs=int((np.argmax(rp["qo"], 0) != sel_t).sum()) if c["double"] else 0,
                 bad_action=int((~rp["known"]).sum()), sel_not_first=int((rp["sel"] != 0).sum()))
    assert sum(holds[k] for k in CLASSES) == u.size
    return int(bad.sum()), holds, (rp, m, b)


def _spec():
    out = []
    k = 0
    # the shape axes, walked together so that every value of every axis occurs (24 cases)
    for ns in (2, 4, 5, 16):
        for h in (4, 64, 256):
            for act in (0, 1):
                na, N, kappa = (1, 2, 4)[k % 3], QUANTILES[(k // 2) % 5], KAPPAS[(k // 3) % 3]
                out.append((f"ns{ns}-h{h}-act{act}-na{na}-n{N}-kap{kappa:g}-b{BATCHES[k % 5]}",
                            dict(ns=ns, h=h, na=na, N=N, act=act, kappa=kappa, batch=BATCHES[k % 5], seed=3000 + 64 * k,
                                 term=("mixed", "all", "none")[k % 3], n_used=k % 2 == 1, weights=k % 4 < 2, double=(k // 3) % 2 == 1)))
                k += 1
    # planted rows
    out += [("plain", dict(ns=4, h=64, na=2, N=51, act=0, batch=33, seed=19700)),
            ("plain-kappa-quarter", dict(ns=4, h=64, na=2, N=51, act=0, batch=33, seed=19750, kappa=0.25)),
            ("double-4-actions", dict(ns=4, h=64, na=4, N=51, act=0, batch=66, seed=19000, double=True, kappa=10.0)),
            ("double-nused-weights", dict(ns=5, h=64, na=2, N=51, act=1, batch=33, seed=19100, double=True, n_used=True, weights=True)),
            ("bad-action", dict(ns=4, h=64, na=2, N=51, act=0, batch=33, seed=19200, bad_action=True, weights=True)),
            ("bad-action-frames", dict(ns=6, h=20, na=3, N=3, act=1, batch=66, seed=19300, bad_action=True, n_used=True, kappa=0.25)),
            ("largest", dict(ns=16, h=256, na=4, N=64, act=0, batch=66, seed=19400, double=True, n_used=True, weights=True)),
            # more tiles than partial rows: some workgroups take a second tile, the last one ragged (the byte cap gives 16 MiB /
            # (4 * 20800) = 201 rows at 16 -> 256 -> 1 x 64; the smallest shape meets the cap of 256 rows)
            ("second-tiles-byte-cap", dict(ns=16, h=256, na=1, N=64, act=1, batch=201 * TILE + TILE + 3, seed=19800, weights=True)),
            ("second-tiles-smallest", dict(ns=2, h=4, na=1, N=1, act=1, batch=256 * TILE + TILE + 3, seed=19900, n_used=True, kappa=0.25)),
            ("all-terminal", dict(ns=3, h=64, na=2, N=51, act=0, batch=32, seed=19500, term="all")),
            ("none-terminal", dict(ns=3, h=64, na=2, N=51, act=1, batch=31, seed=19600, term="none", n_used=True))]
    return out


SPEC = dict(_spec())
NAMES = list(SPEC)
MAX_EXCLUDED = 0.02


@functools.lru_cache(maxsize=None)
def case(name):
    """the case `name` with its replay, float64 model and budgets under `replays`"""
    kw = dict(SPEC[name])
    seed = kw.pop("seed")
    for tries in range(64):
        c = _build(name, seed=seed + tries, **kw)
        n_bad, holds, replays = census(c)
        if n_bad == 0:
            c.update(tries=tries, holds=holds, excluded=0, replays=replays)
            return c
    raise AssertionError(f"{name}: no seed in {seed} .. {seed + 63} passes the census")
