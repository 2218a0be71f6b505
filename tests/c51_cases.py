"""The seeded case grid of the C51 kernels with its census (plain numpy and the CPU models of tests/c51_ref.py; no GPU).

A case is a dictionary: the online and the target network (flat Float32 vectors, non-zero biases, the target far enough from the online
net that their greedy actions differ on many samples), a GATHERED batch (s, a, r, term, s' [, n_used] [, weights]) and the scalars.
Rewards are planted, four samples in turn: Tz below v_min, above v_max, exactly on an inner atom (the sample is terminal: c = 0, all mass
on one atom), strictly between two atoms (terminal: mass on two atoms).

Axes (every value below occurs; `test_every_class_of_the_census_is_populated` counts them):
  batch    1, TILE - 1, TILE, TILE + 1, 2 TILE + 2 (TILE = 8, the gradient kernel's tile)       n_atoms  2, 3, 51, 64
  na       1, 2, 4                      ns  2, 4, 5, 16                    h  4, 64, 256            act      relu, tanh
  term     all terminal, none terminal, mixed                             n_used  -1, 0, 1, 32, 40 (cycled) or NULL
  weights  given, NULL                  double_dqn  both flags             action  one outside 0 .. na - 1

Decisions.  A sample is COUNTED when (i) the float64 model's top-two gap of the selecting Q(s') exceeds 4 x the Float32 budget of those
values (two evaluations, each within 2 x budget of its centre) and (ii), ReLU cases only, every layer-1 pre-activation of every pass has
|z1| >= 1e-5.  The builder walks the case's seed upwards until NO sample is excluded (the cap is 2 % per case; zero is inside it), at
most 64 steps, so the grid is a fixed function of this file and every comparison runs on all samples."""
import functools

import numpy as np

import c51_ref as R
from heads_ref import F32

TILE = 8
BATCHES = (1, TILE - 1, TILE, TILE + 1, 2 * TILE + 2)
N_USED = (-1, 0, 1, 32, 40)
V_MIN, V_MAX, GAMMA = -2.0, 3.0, 0.9


def _net(rng, ni, h, no, l1_scale=4.0):
    s1, s2 = l1_scale * np.sqrt(6.0 / (ni + h)), np.sqrt(6.0 / (h + min(no, 16)))
    return R.join(rng.uniform(-s1, s1, (h, ni)), l1_scale * rng.uniform(-0.3, 0.3, h), rng.uniform(-s2, s2, (no, h)),
                  rng.uniform(-0.3, 0.3, no)).astype(F32)


def _build(name, ns, h, na, n_atoms, act, batch, seed, term="mixed", n_used=False, weights=False, double=False, bad_action=False):
    rng = np.random.default_rng(seed)
    M = na * n_atoms
    c = dict(name=name, ns=ns, h=h, na=na, n_atoms=n_atoms, act=act, batch=batch, seed=seed, v_min=V_MIN, v_max=V_MAX, gamma=GAMMA,
             double=bool(double), term_mode=term)
    c["params"] = _net(rng, ns, h, M)
    c["target"] = (c["params"] + rng.normal(0, 0.25, c["params"].shape)).astype(F32)
    c["s"] = rng.normal(0, 1, (ns, batch)).astype(F32)
    c["sn"] = rng.normal(0, 1, (ns, batch)).astype(F32)
    a = rng.integers(0, na, batch).astype(np.int32)
    t = {"all": np.ones(batch), "none": np.zeros(batch), "mixed": rng.uniform(size=batch) < 0.3}[term].astype(np.uint8)
    delta, z = R.support(c)
    r = rng.normal(0.3, 1.0, batch).astype(F32)
    kind = np.full(batch, -1)
    for i in range(batch):  # the planted rewards, four samples in turn; kinds 2 and 3 are terminal unless the case has no terminal
        k = i % 5
        if k == 0:
            r[i] = F32(V_MIN - 4.5)
        elif k == 1:
            r[i] = F32(V_MAX + 4.0)
        elif k == 2 and term != "none":
            r[i], t[i] = z[(i // 5) % max(n_atoms - 2, 1) + (1 if n_atoms > 2 else 0)], 1
        elif k == 3 and term != "none":
            r[i], t[i] = F32(z[(i // 5) % (n_atoms - 1)] + F32(0.37) * delta), 1
        kind[i] = k
    c.update(a=a, r=r, term=t, kind=kind)
    c["n_used"] = np.array([N_USED[i % 5] for i in range(batch)], np.int32) if n_used else None
    c["weights"] = rng.uniform(0.2, 1.0, batch).astype(F32) if weights else None
    if bad_action:
        c["a"][batch // 2] = na if (batch // 2) % 2 == 0 else -1
    return c


def census(c):
    """-> (number of samples on a decision, dict of what the case holds, (replay, model))"""
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
    tz, z = rp["tz"], rp["z"]
    lo, hi = tz == F32(c["v_min"]), tz == F32(c["v_max"])
    raw = (c["r"][None, :] + (rp["cc"][None, :] * z[:, None]).astype(F32)).astype(F32)
    inner = (tz[:, None, :] == z[None, 1:-1, None]).any(1) if c["n_atoms"] > 2 else np.zeros(tz.shape, bool)
    between = ~(tz[:, None, :] == z[None, :, None]).any(1)
    sel_t = np.argmax(rp["qt"], 0)
    holds = dict(below=int((lo & (raw < F32(c["v_min"]))).sum()), above=int((hi & (raw > F32(c["v_max"]))).sum()), on_atom=int(inner.sum()),
                 between=int(between.sum()), c0=int((rp["cc"] == 0).sum()), terminal=int((c["term"] != 0).sum()),
                 not_terminal=int((c["term"] == 0).sum()),
                 argmax_differs=int((np.argmax(rp["qo"], 0) != sel_t).sum()) if c["double"] else 0,
                 bad_action=int((~rp["known"]).sum()), sel_not_first=int((rp["sel"] != 0).sum()),
                 # (a Float32 atom one ulp off its exact place leaves a neighbour a weight of one rounding: not mass)
                 two_atoms=int(((rp["proj"] > 1e-6).sum(0) <= 2)[rp["cc"] == 0].sum()))
    return int(bad.sum()), holds, (rp, m, b)


def _spec():
    out = []
    k = 0
    # the shape axes, walked together so that every value of every axis occurs (24 cases)
    for ns in (2, 4, 5, 16):
        for h in (4, 64, 256):
            for act in (0, 1):
                na, n_atoms = (1, 2, 4)[k % 3], (2, 3, 51, 64)[(k // 2) % 4]
                out.append((f"ns{ns}-h{h}-act{act}-na{na}-k{n_atoms}-b{BATCHES[k % 5]}",
                            dict(ns=ns, h=h, na=na, n_atoms=n_atoms, act=act, batch=BATCHES[k % 5], seed=2000 + 64 * k,
                                 term=("mixed", "all", "none")[k % 3], n_used=k % 2 == 1, weights=k % 4 < 2, double=(k // 3) % 2 == 1)))
                k += 1
    # planted rows
    out += [("plain", dict(ns=4, h=64, na=2, n_atoms=51, act=0, batch=33, seed=9700)),
            ("double-4-actions", dict(ns=4, h=64, na=4, n_atoms=51, act=0, batch=66, seed=9000, double=True)),
            ("double-nused-weights", dict(ns=5, h=64, na=2, n_atoms=51, act=1, batch=33, seed=9100, double=True, n_used=True, weights=True)),
            ("bad-action", dict(ns=4, h=64, na=2, n_atoms=51, act=0, batch=33, seed=9200, bad_action=True, weights=True)),
            ("bad-action-frames", dict(ns=6, h=20, na=3, n_atoms=3, act=1, batch=66, seed=9300, bad_action=True, n_used=True)),
            ("largest", dict(ns=16, h=256, na=4, n_atoms=64, act=0, batch=66, seed=9400, double=True, n_used=True, weights=True)),
            # more tiles than partial rows: some workgroups take a second tile, the last one ragged (the byte cap gives 16 MiB /
            # (4 * 20800) = 201 rows at 16 -> 256 -> 64; the smallest shape meets the cap of 256 rows)
            ("second-tiles-byte-cap", dict(ns=16, h=256, na=1, n_atoms=64, act=1, batch=201 * TILE + TILE + 3, seed=9800, weights=True)),
            ("second-tiles-smallest", dict(ns=2, h=4, na=1, n_atoms=2, act=1, batch=256 * TILE + TILE + 3, seed=9900, n_used=True)),
            ("all-terminal", dict(ns=3, h=64, na=2, n_atoms=51, act=0, batch=32, seed=9500, term="all")),
            ("none-terminal", dict(ns=3, h=64, na=2, n_atoms=51, act=1, batch=31, seed=9600, term="none", n_used=True))]
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
