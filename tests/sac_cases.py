"""Seeded case grids for the SAC kernels, each with a census (plain numpy; no oracle, no GPU).

A case is a dictionary: the networks (flat Float32 vectors with non-zero biases), the pushes of a record ring -- 8 envs, capacity 24,
30 pushed transitions, so the ring has wrapped and logical transition 0 is push 6 -- the batch indices, and the scalars of the
update.  `records()` gives the sampled transitions (s (ns, B), a, r, t, s'); `fill(traces)` pushes the same data into device traces.

Census (`census`, on the replay (a) of tests/sac_ref.py).  A case is usable when nothing in it sits on a decision:
  * every |Q1 - Q2| >= 1e-4, at x' (the target critics of the critic step) and at x (the critics of the actor step);
  * ReLU cases: every critic layer-1 pre-activation on a SAMPLED action (the four passes just named) has |z1| >= 1e-5 -- a tanh case
    has no decision there;
  * every raw sigma = softplus(rho) is at least 1e-4 from both clamp bounds, on either side (rho itself meets no bound): a planted
    clamped component lies clearly beyond its bound.
The builder walks the case's seed upwards until the census holds with NO sample excluded (at most 64 steps; the step count is kept
in the case as `tries`), so the grid is a fixed function of this file.  tests/test_sac_reference.py asserts zero exclusions and that
every planted row is present."""
import functools

import numpy as np

import sac_ref as R
from heads_ref import F32

N_ENV, CAP, PUSHES = 8, 24, 30
STREAM_SEED, STEP = 77, 5   # the update stream's (seed, step) of every kernel case
BATCHES = (1, 63, 64, 65, 130)
BIG_BATCH = 256 * 64 + 3    # the grid cap (256 workgroups) x the tile (64) + 3: every workgroup a second tile, the last one ragged


def _net(rng, ni, h, no, w2_scale=1.0, l1_scale=1.0):
    s1, s2 = l1_scale * np.sqrt(6.0 / (ni + h)), np.sqrt(6.0 / (h + no))
    return R.join(rng.uniform(-s1, s1, (h, ni)), l1_scale * rng.uniform(-0.3, 0.3, h), w2_scale * rng.uniform(-s2, s2, (no, h)),
                  rng.uniform(-0.3, 0.3, no)).astype(F32)


def _build(name, ns, h, act, batch, seed, alpha=0.2, scale=1.0, lo=0.0, hi=np.inf, wide_mu=False, q_scale=1.0, plant_terminal=True):
    rng = np.random.default_rng(seed)
    c = dict(name=name, ns=ns, h=h, act=act, batch=batch, seed=seed, alpha=alpha, scale=scale, lo=lo, hi=hi, gamma=0.99,
             alpha_lr=3e-3, target_entropy=-1.0, n_env=N_ENV, cap=CAP, stream_seed=STREAM_SEED, step=STEP)
    c["actor"] = _net(rng, ns, h, 2)
    if wide_mu:  # mu spread over +-30: some |z| > 9, where tanhf gives +-1 exactly
        W1, b1, W2, b2 = R.split(c["actor"], ns, h, 2)
        W2 = W2.copy()
        W2[0] *= 40.0
        c["actor"] = R.join(W1, b1, W2, b2).astype(F32)
    # layer 1 of the critics four times Glorot's width: 133 000 pre-activations (h = 256, batch 130, four passes) of unit scale leave
    # |z1| < 1e-5 about once per case, of Glorot's scale four times
    c["critics"] = np.concatenate([_net(rng, ns + 1, h, 1, q_scale, 4.0), _net(rng, ns + 1, h, 1, q_scale, 4.0)])
    c["targets"] = (c["critics"] + rng.normal(0, 0.02, c["critics"].shape) * q_scale).astype(F32)
    c["S"] = rng.normal(0, 1, (PUSHES + 1, ns, N_ENV)).astype(F32)
    c["A"] = rng.uniform(-scale, scale, (PUSHES, N_ENV)).astype(F32)
    c["Rw"] = rng.normal(0, 1, (PUSHES, N_ENV)).astype(F32)
    c["T"] = (rng.uniform(size=(PUSHES, N_ENV)) < 0.15).astype(np.uint8)
    idx = rng.integers(0, CAP * N_ENV, batch).astype(np.int64)
    if plant_terminal and batch > 1:
        li, e = np.argwhere(c["T"][PUSHES - CAP:] != 0)[0]
        idx[1] = li * N_ENV + e
    c["idx"] = idx

    def records():
        li, e = idx // N_ENV, idx % N_ENV
        p = li + (PUSHES - CAP)  # logical transition li is push p: the ring has dropped the oldest PUSHES - CAP
        return (np.ascontiguousarray(c["S"][p, :, e].T), c["A"][p, e], c["Rw"][p, e], c["T"][p, e], np.ascontiguousarray(c["S"][p + 1, :, e].T))

    c["records"] = records
    return c


def fill(c, traces, torch):
    """push the case's transitions into device traces (CircularArraySARTSTraces(CAP, N_ENV, ns, action_dtype = torch.float32))"""
    up = lambda x: torch.tensor(np.ascontiguousarray(x), device="cuda")  # noqa: E731
    traces.push_state_(up(c["S"][0]))
    for p in range(PUSHES):
        traces.push_transition_(up(c["S"][p + 1]), up(c["A"][p]), up(c["Rw"][p]), up(c["T"][p]))
    return traces


def census(c, sample):
    """-> (number of samples on a decision, dict of what the case holds); `sample`: an implementation's unchanged forward entry"""
    eps0, eps1 = R.draw_pair(sample, c["batch"], c["stream_seed"] + 1, c["step"])
    rc, ra = R.critic_replay(c, eps0), R.actor_replay(c, eps1)
    bad = np.abs(rc["qt"][0] - rc["qt"][1]) < 1e-4
    bad_a = np.abs(ra["qs"][0] - ra["qs"][1]) < 1e-4
    if c["act"] == 0:
        for z in rc["z_t"]:
            bad |= (np.abs(z) < 1e-5).any(0)
        for z in ra["z"]:
            bad_a |= (np.abs(z) < 1e-5).any(0)
    for hd, b in ((rc["head"], bad), (ra["head"], bad_a)):
        for bound in (c["lo"], c["hi"]):
            if np.isfinite(bound):
                b |= np.abs(hd["raw"].astype(np.float64) - float(F32(bound))) < 1e-4
    hd = ra["head"]
    holds = dict(terminal=int((c["records"]()[3] != 0).sum()), clamped_lo=int((hd["raw"] < F32(c["lo"])).sum()),
                 clamped_hi=int((hd["raw"] > F32(c["hi"])).sum()), saturated=int((np.abs(hd["z"]) > 9).sum()),
                 saturated_exact=int(((np.abs(hd["z"]) > 9) & (np.abs(hd["a"]) == 1)).sum()), sel2=int((ra["sel"] == 2).sum()),
                 sel_t2=int((rc["sel_t"] == 2).sum()))
    return int(bad.sum() + bad_a.sum()), holds, (eps0, eps1, rc, ra)


def _spec():
    out = []
    k = 0
    for ns in (2, 3, 4):
        for h in (4, 20, 64, 256):
            for act in (0, 1):
                out.append((f"ns{ns}-h{h}-act{act}-b{BATCHES[k % 5]}", dict(ns=ns, h=h, act=act, batch=BATCHES[k % 5], seed=1000 + 64 * k)))
                k += 1
    # planted rows (terminal = 1 and the wrapped ring are in every case)
    out += [("sigma-clamped", dict(ns=3, h=20, act=1, batch=65, seed=9000, lo=0.55, hi=0.8)),
            ("saturated", dict(ns=3, h=20, act=0, batch=65, seed=9100, wide_mu=True)),
            ("alpha0", dict(ns=2, h=64, act=0, batch=64, seed=9200, alpha=0.0)),
            ("scale2", dict(ns=3, h=64, act=1, batch=63, seed=9300, scale=2.0)),
            ("scale2-clamped-relu", dict(ns=4, h=20, act=0, batch=130, seed=9400, scale=2.0, lo=0.5, hi=0.9)),
            ("two-tiles-ragged", dict(ns=3, h=4, act=1, batch=BIG_BATCH, seed=9500, q_scale=20.0))]
    return out


SPEC = dict(_spec())
NAMES = list(SPEC)
PLANTED = {"sigma-clamped": ("clamped_lo", "clamped_hi"), "saturated": ("saturated_exact",), "scale2-clamped-relu": ("clamped_lo", "clamped_hi")}


@functools.lru_cache(maxsize=None)
def _case(name, sample):
    kw = dict(SPEC[name])
    seed = kw.pop("seed")
    for tries in range(64):
        c = _build(name, seed=seed + tries, **kw)
        n_bad, holds, replays = census(c, sample)
        planted_ok = all(holds[k] > 0 for k in PLANTED.get(name, ())) and (c["batch"] == 1 or holds["terminal"] > 0)
        if n_bad == 0 and planted_ok:
            c.update(tries=tries, holds=holds, excluded=0, replays=replays)
            return c
    raise AssertionError(f"{name}: no seed in {seed} .. {seed + 63} passes the census")


def case(name, sample):
    """the case `name` with its replays (eps0, eps1, critic replay, actor replay) under `replays`"""
    return _case(name, sample)
