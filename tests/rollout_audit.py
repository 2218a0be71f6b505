"""Per-step audit of a complete PPO rollout against the oracle, restarted from the rollout's own records at every step.

Not a test module.  tests/test_rollout_audit_reference.py runs it on the oracle's own rollouts (what the state reconstruction
costs by itself, how many samples sit at a sampling near-tie, that every corruption on its list is caught);
tests/test_gpu_rollout_audit.py runs it on one launch of every rollout instantiation of tests/f32_learner_matrix.py (ROLLOUT)
and tests/bf16_learner_matrix.py (the rollout rows of PPO3 and PPO3W).

A free-running comparison loses an env at its first flipped action and a Gaussian head at its first differing bit.  Here every
sample (t, env) is checked on its own:

  policy part      the nets (oracle.mlp2_forward / mlp3_forward) on the *recorded* obs[t]: value[t] for t = 0 .. T, logp[t] of the
                   recorded action, the action itself (oracle.categorical_sample, or mu + exp(log_sigma) * noise with the oracle's
                   normal for (seed, env_id_base + i, vec_step0 + t)).  A discrete disagreement is accepted only as a shown
                   near-tie: raising the recorded action's oracle logit by delta makes the oracle pick it.
  transition part  an oracle.VecEnv restarted from obs[t] and the counters rebuilt from the terminal trace, stepped with the
                   recorded action: reward[t], terminal[t], obs[t + 1] (post-reset where terminal), and after the last step
                   the env's raw state, counters, reward and done; adv / ret bit for bit against the oracle's GAE.

Injected cases (INJECT_CASES): a case may carry an `inject` field, raw state and t written into the env before the first
launch (HipVecEnv.set_raw_state / oracle.VecEnv.set_state); the audit takes the pre-launch raw state at t = 0 anyway.  They
start one MountainCar and one CartPole env set per rollout kernel (the three-layer kernels take CartPole only) on the
goal / x-threshold rows of tests/env_edge_cases.py with max_steps far away: the only terminations the rollout kernels met
outside CartPole were truncations.  check_injected() adds what these cases are for.  They are a list of their own: the
shape rules of CASES (T > 32 or T = 16 for the split kernel, max_steps 5 .. 20) do not apply to them.

Pendulum reconstruction (the route taken: atan2): the observation holds (sin, cos, thetadot) of an unwrapped angle.
theta = atan2(sin, cos) in Float64, moved by the multiple of 2 pi that brings it next to the angle the oracle's previous step
(or, at t = 0, the raw state before the launch) arrived at, rounded to Float32; where several neighbouring Float32
angles fit the record to its last bit (0.5 <= |theta| < 1) the one nearest the oracle's previous step is taken.  One step changes theta by at most max_speed * dt = 0.4 < pi, so the
branch is never in doubt; the value of theta comes from the record alone.

Bars (tests/test_gpu_rollout_audit.py lists where each comes from):
  allclose  |x - ref| <= atol + rtol * |ref|
  close     e = |x - ref| / (1 + |ref|): max e <= tol -- or, share form, at most 1e-3 of the samples beyond tol and max e <= 5e-3
  scaled    |x - ref| <= 4 * s * (1 + |ref|), s the largest error of the Float32 oracle against a Float64 numpy evaluation of
            the same expression on the same inputs (the GPU differs from the oracle in summation order only), never wider than
            the free-running bar it replaces
"""
import ctypes as C
import ctypes.util
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import bf16_learner_matrix as MB
import env_edge_cases as EDGE
import f32_learner_matrix as MF
import oracle

GAMMA, LAM = 0.99, 0.95  # rlhip_ppo_default / rlo_ppo_default
NS = {"cartpole": 4, "pendulum": 3, "mountaincar": 2}
SHARE, FLIP_MAX = 1e-3, 5e-3  # the share form of close()
EXC_CAP = {False: 1e-3, True: 5e-3}  # near-tie exceptions: share of a row's samples, by bf16


# ----------------------------------------------------------------------------------------------------------------- cases
def _case(row, layers, **over):
    c = dict(id=row["id"], kernel=row["kernel"], env=row["env"], hidden=row["hidden"], act=row["act"], layers=layers,
             continuous=row["continuous"] if layers == 2 else MB.PPO_ENVS[row["env"]], n=row["n"], T=row["T"], max_steps=None)
    c.update(over)
    return c


def _f32_cases():
    out = []
    for i, row in enumerate(MF.ROLLOUT):
        env, cart = row["env"], row["env"] == "cartpole"
        if row["kernel"] == "rollout_split_kernel":
            epw = 256 // MF.WIDE_L[row["hidden"]]  # envs per workgroup
            n = row["n"] if row["n"] % epw else 37
            assert n % epw
            # T > 32: two boundaries of the 16-step noise chunks; CartPole T >= 40; the others reset at least twice
            T = (40, 45, 49)[i % 3] if cart else (33, 37, 49)[i % 3]
            ms = (None, 12)[i % 2] if cart else (5, 7, 11, 16)[i % 4]
        else:
            n, T, ms = 301, (40 if cart else 17), (None if cart else (5, 8)[i % 2])
        out.append(_case(row, 2, n=n, T=T, max_steps=ms))
    # one noise chunk exactly
    out.append(dict(id="rollout-pendulum-h128-relu-head1-T16", kernel="rollout_split_kernel", env="pendulum", hidden=128, act=0,
                    layers=2, continuous=True, n=77, T=16, max_steps=5))
    # the scalar kernel by size: n * 16 > 2^22 at a listed hidden size
    out.append(dict(id="rollout-mountaincar-large_n-h64-relu", kernel="rollout_scalar_kernel", env="mountaincar", hidden=64,
                    act=0, layers=2, continuous=False, n=(1 << 18) + 37, T=11, max_steps=5))
    return out


def _bf16_cases():
    out = []
    for i, row in enumerate(r for r in MB.PPO3 + MB.PPO3W if "rollout" in r["id"]):
        cart = row["env"] == "cartpole"
        if row["kernel"] == "ppo3_rollout_kernel":  # n = 2^15 + 1: one env past a tile of TR = 128
            assert row["n"] % 128
            over = dict(T=13 if cart else 11, max_steps=5)
        elif row["kernel"] == "ppo3_rollout32_kernel":
            assert row["n"] % 32
            over = dict(T=40, max_steps=(None, 15)[row["act"]]) if cart else dict(T=21, max_steps=(10, 7)[row["act"]])
        else:
            assert row["kernel"] == "ppo3w_rollout_kernel" and row["n"] % 32
            over = dict(T=41, max_steps=(14, None)[row["act"]]) if cart else dict(T=33, max_steps=(16, 6)[row["act"]])
        out.append(_case(row, 3, **over))
    return out


def _finish(cases):
    for i, c in enumerate(cases):
        c["seed"] = 3 + i % 5
        c["env_id_base"] = 1000 + 17 * i
        c["bf16"] = c["layers"] == 3
        if c["env"] != "cartpole":
            assert 5 <= c["max_steps"] <= 20 and c["T"] >= 2 * c["max_steps"]
        else:
            assert c["T"] >= 40 or c["n"] > 1 << 15
        assert c["T"] <= 49 and (c["n"] <= 1000 or c["T"] <= 13)
    return cases


CASES = _finish(_f32_cases() + _bf16_cases())
MATRIX_IDS = {r["id"] for r in MF.ROLLOUT} | {r["id"] for r in MB.PPO3 + MB.PPO3W if "rollout" in r["id"]}


def _inject_cases():
    """(kernel, env) -> the first audited case of that kernel and env, restarted with T = 8 on the no-truncation grid"""
    out = []
    for kernel, envs in (("rollout_split_kernel", ("mountaincar", "cartpole")), ("rollout_scalar_kernel", ("mountaincar", "cartpole")),
                         ("ppo3_rollout_kernel", ("cartpole",)), ("ppo3_rollout32_kernel", ("cartpole",)),
                         ("ppo3w_rollout_kernel", ("cartpole",))):
        for env in envs:
            base = min((c for c in CASES if c["kernel"] == kernel and c["env"] == env), key=lambda c: c["n"])
            n = base["n"]  # the smallest n the kernel's rows of this env use, with that row's hidden size and head
            g = EDGE.grid(f"{env}-f32-{'cont' if base['continuous'] else 'disc'}-default", 1024, truncation=False)
            # columns from the filler half of the grid (their class holds under any action), lane pattern from lane 0 on
            cols = (512 + np.arange(n)) % 1024
            c = dict(base, id=base["id"] + "-injected", n=n, T=8, max_steps=EDGE.NO_TRUNC_MAX_STEPS, seed=11 + len(out),
                     env_id_base=3000 + 19 * len(out), inject=dict(s=np.ascontiguousarray(g.s[:, cols]), t=g.t[cols].copy()),
                     edge_params=g.p)
            out.append(c)
    return out


INJECT_CASES = _inject_cases()


def apply_inject(c, env):
    """write the case's injected rows into an oracle.VecEnv (the GPU side: HipVecEnv.set_raw_state)"""
    if c.get("inject"):
        env.set_state(c["inject"]["s"], c["inject"]["t"])


def check_injected(traj, env0, c):
    """What the injected cases are for, on the first step of a launch that started from the injected rows: at least 20 % of
    the envs record terminal[0] = 1 and the oracle names goal / x-threshold (never the step counter) as the cause of each,
    reward[0] = 0 there and obs[1] is the reset draw, bit for bit.  (adv / ret over those terminals: audit(), exact.)"""
    env, p = _new_env(c), c["edge_params"]
    env.set_state(env0["raw_state"], env0["t"])
    env.episode[:] = env0["episode"].view(np.uint32)
    env.step(traj["action_f"][0] if c["continuous"] else traj["action_i"][0])
    lo, done = env.last_obs, env.done.astype(bool)
    if c["env"] == "mountaincar":
        cause = (lo[0] >= p["goal_pos"]) & (lo[1] >= p["goal_velocity"])
    else:
        cause = (np.abs(lo[0]) > p["xthreshold"]) & (np.abs(lo[2]) <= p["thetathreshold"])
    term0 = np.asarray(traj["terminal"][0]).astype(bool)
    fails = []
    if not np.array_equal(term0, done):
        fails.append(f"terminal[0] differs from the oracle at {int((term0 != done).sum())} envs")
    if not np.array_equal(done, cause) or (env.t[~done] > 2000).any():
        fails.append("a termination of the first step is not a goal / x-threshold one")
    if term0.mean() < 0.2:
        fails.append(f"only {term0.mean():.3f} of the envs terminate at the first step")
    if (traj["reward"][0][term0] != 0).any():
        fails.append("reward[0] != 0 at a terminal step")
    if not np.array_equal(np.asarray(traj["obs"][1])[:, term0], env.obs()[:, term0]):
        fails.append("obs[1] of a terminated env is not the oracle's reset draw")
    return fails


def na_of(c):
    return 1 if c["continuous"] else (2 if c["env"] == "cartpole" else 3)


def nout_of(c):
    return 2 if c["continuous"] else na_of(c)


def make_params(c):
    """Actor and critic parameters of a case (flat, actor first): the oracle's init, every entry (two-layer) or every bias
    (three-layer) moved off its initial value so that no bias path is silent"""
    ns, h, nout = NS[c["env"]], c["hidden"], nout_of(c)
    rng = np.random.default_rng(c["seed"] * 1000 + len(c["id"]))
    nets = []
    for net_id, no in ((0, nout), (1, 1)):
        if c["layers"] == 2:
            p = oracle.mlp2_init(ns, h, no, c["seed"], net_id)
            p = (p + rng.standard_normal(p.size) * 0.05).astype(np.float32)
        else:
            p = oracle.mlp3_init(ns, h, no, c["seed"], net_id)
            o = 0
            for name, sz in (("W1", h * ns), ("b1", h), ("W2", h * h), ("b2", h), ("W3", no * h), ("b3", no)):
                if name[0] == "b":
                    p[o:o + sz] = rng.standard_normal(sz).astype(np.float32) * 0.1
                o += sz
            assert o == p.size
        nets.append(p)
    return np.concatenate(nets), nets[0].size


def env_kwargs(c):
    kw = dict(continuous=c["continuous"])
    if c["max_steps"] is not None:
        kw["max_steps"] = c["max_steps"]
    return kw


def make_bars(c):
    """the bars of a case (module docstring; sources in tests/test_gpu_rollout_audit.py)"""
    if c["layers"] == 2:
        b = dict(value=("allclose", 2e-5, 2e-6), logp=("allclose", 2e-5, 2e-6), action=("scaled", 2e-3, 2e-3), logit="scaled")
    else:
        share = c["act"] == 1
        vtol = 1e-4 if (c["continuous"] or c["act"] == 1) else 2e-5
        b = dict(value=("close", vtol, share), logp=("abs", 1e-3, share), action=("close", 1e-4, share), logit=("close", vtol))
    pend = c["env"] == "pendulum"
    b.update(reward=("allclose", 2e-6, 1e-7), obs=("allclose", 2e-6, 2e-5 if pend else 1e-7), obs_reset=("allclose", 0.0, 1e-7),
             state=("allclose", 2e-6, 1e-7), exc_cap=EXC_CAP[c["bf16"]])
    return b


# ------------------------------------------------------------------------------------------------------------- the nets
def forward(c, p, nout, X):
    """oracle forward of one net on X (ns, B) -> (nout, B); the three-layer net in parallel over column blocks"""
    ns, h, act = NS[c["env"]], c["hidden"], c["act"]
    X = np.ascontiguousarray(X, np.float32)
    if c["layers"] == 2:
        return oracle.mlp2_forward(p, ns, h, nout, act, X)
    B = X.shape[1]
    nthr = oracle.usable_cpus()
    if B < 4096 or nthr == 1:
        return oracle.mlp3_forward(p, ns, h, nout, act, X)
    cuts = np.linspace(0, B, 4 * nthr + 1).astype(int)
    with ThreadPoolExecutor(nthr) as ex:  # ctypes releases the GIL for the duration of the call
        parts = list(ex.map(lambda ab: oracle.mlp3_forward(p, ns, h, nout, act, X[:, ab[0]:ab[1]]), zip(cuts[:-1], cuts[1:])))
    return np.concatenate(parts, axis=1)


def forward64(c, p, nout, X):
    """Float64 numpy evaluation of the two-layer net, the expression of rlo_mlp2_forward_f32"""
    ns, h = NS[c["env"]], c["hidden"]
    p = p.astype(np.float64)
    W1, b1 = p[:h * ns].reshape(ns, h).T, p[h * ns:h * ns + h]
    o = h * ns + h
    W2, b2 = p[o:o + nout * h].reshape(h, nout).T, p[o + nout * h:]
    out = np.empty((nout, X.shape[1]))
    for a in range(0, X.shape[1], 1 << 16):
        z = W1 @ X[:, a:a + (1 << 16)].astype(np.float64) + b1[:, None]
        out[:, a:a + (1 << 16)] = W2 @ (np.maximum(z, 0) if c["act"] == 0 else np.tanh(z)) + b2[:, None]
    return out


_libm = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.expf.restype, _libm.expf.argtypes = C.c_float, [C.c_float]


def expf(x):
    """the host libm's expf, element by element: what rlo_ppo_rollout_f32 calls for sigma = exp(log sigma)"""
    f = _libm.expf
    return np.array([f(v) for v in x.ravel().tolist()], np.float32).reshape(x.shape)


def normlogpdf(mu, sg, x):
    f = oracle.lib().rlo_normlogpdf_f32
    return np.array([f(a, b, d) for a, b, d in zip(mu.ravel().tolist(), sg.ravel().tolist(), x.ravel().tolist())],
                    np.float32).reshape(mu.shape)


def log_softmax(l):
    """log-softmax of Float32 logits (na, B) as rlo_categorical_sample_f32 evaluates it: exp / log in Float64, rounded once"""
    l = np.asarray(l, np.float32)
    d = l - l.max(0)
    se = np.zeros(l.shape[1], np.float32)
    for k in range(l.shape[0]):
        se = se + np.exp(d[k].astype(np.float64)).astype(np.float32)
    return d - np.log(se.astype(np.float64)).astype(np.float32)


def sample(c, logits, t, vec_step0):
    """oracle.categorical_sample of the n envs at step t"""
    return oracle.categorical_sample(logits, seed=c["seed"], step=vec_step0 + t, env_id_base=c["env_id_base"])


# ---------------------------------------------------------------------------------------------------------------- audit
def _new_env(c):
    return oracle.VecEnv(c["env"], c["n"], seed=c["seed"], env_id_base=c["env_id_base"], auto_reset=True, **env_kwargs(c))


def snapshot(env):
    return dict(raw_state=np.stack(env.s).copy(), t=env.t.copy(), episode=env.episode.view(np.int32).copy(),
                reward=env.reward.copy(), done=env.done.copy())


def _restart(c, env, obs_t, pred_theta):
    if c["env"] == "pendulum":
        th = np.arctan2(obs_t[0].astype(np.float64), obs_t[1].astype(np.float64))
        th = (th + 2 * np.pi * np.round((pred_theta.astype(np.float64) - th) / (2 * np.pi))).astype(np.float32)
        # The Float32 sin / cos pin theta to ~6e-8 while an ulp of |theta| ~ 8 is 5e-7, so above |theta| = 1 one Float32 angle
        # fits the record.  In 0.5 <= |theta| < 1 an ulp of theta is as fine as the record, and the reward's Float32
        # theta + pi turns one such ulp into 2.4e-7: of the angles that fit the record (sin and cos within 6e-8) the one
        # nearest the oracle's previous step is taken; the record alone decides which angles fit.
        ulp = np.spacing(np.abs(th)).astype(np.float64)
        cand = np.stack([(th.astype(np.float64) + k * ulp).astype(np.float32) for k in (-2, -1, 0, 1, 2)])
        ds = np.abs(np.sin(cand.astype(np.float64)) - obs_t[0])
        dc = np.abs(np.cos(cand.astype(np.float64)) - obs_t[1])
        fits = (ds <= 6e-8) & (dc <= 6e-8)
        score = np.where(fits, np.abs(cand.astype(np.float64) - pred_theta.astype(np.float64)), 1e3 + ds + dc)
        env.set_state([cand[score.argmin(0), np.arange(th.size)], obs_t[2]])
    else:
        env.set_state([obs_t[k] for k in range(env.sdim)])


def audit(traj, env0, env1, params, cfg, vec_step0, count_fragile=False):
    """traj: obs (T + 1, ns, n), value (T + 1, n), logp, action_i (0-based) or action_f, reward, terminal, adv, ret (T, n);
    env0 / env1: raw_state (sdim, n), t, episode before / after the launch, env1 also reward and done; params (flat, actor
    first); cfg: a case of CASES.  Returns per-quantity (error, reference) arrays, the exact-mismatch counts, the near-tie
    exception mask and the Float32 scales; check() turns them into a verdict."""
    c, n = cfg, cfg["n"]
    obs, T = np.asarray(traj["obs"], np.float32), traj["logp"].shape[0]
    ns, nout, cont = NS[c["env"]], nout_of(c), c["continuous"]
    assert obs.shape == (T + 1, ns, n)
    p, np_a = params
    pa, pc = p[:np_a], p[np_a:]
    res = dict(T=T, n=n, exact={}, scale={})

    # ---- policy part
    X = obs.transpose(1, 0, 2).reshape(ns, (T + 1) * n)
    vref = forward(c, pc, 1, X)[0].reshape(T + 1, n)
    res["value"] = (np.abs(traj["value"] - vref), vref)
    out = forward(c, pa, nout, X[:, :T * n])
    out64 = forward64(c, pa, nout, X[:, :T * n]) if c["layers"] == 2 else None
    if out64 is not None:
        res["scale"]["logit"] = float((np.abs(out - out64) / (1 + np.abs(out64))).max())
    exc = np.zeros((T, n), bool)
    if cont:
        mu, ls = out[0].reshape(T, n), out[1].reshape(T, n)
        sg = expf(ls)
        noise = oracle.ppo_rollout_noise(c["seed"], c["env_id_base"], n, [vec_step0 + t for t in range(T)])
        aref = mu + sg * noise
        a = np.asarray(traj["action_f"], np.float32).reshape(T, n)
        res["action"] = (np.abs(a - aref), aref)
        lref = normlogpdf(mu, sg, a)
        if out64 is not None:
            a64 = out64[0].reshape(T, n) + np.exp(out64[1].reshape(T, n)) * noise.astype(np.float64)
            res["scale"]["action"] = float((np.abs(aref - a64) / (1 + np.abs(a64))).max())
        # first-order reach of a (mu, log sigma) error e on the log-density: |z| / sigma * e_mu + (z^2 + 1) * e_ls
        z = (a - mu) / sg
        res["logp_gain"] = np.abs(z) / sg * (1 + np.abs(mu)) + (z * z + 1) * (1 + np.abs(ls))
        res["n_disagree"] = 0
    else:
        a = np.asarray(traj["action_i"]).reshape(T, n)
        assert a.min() >= 0 and a.max() < nout
        lsm = log_softmax(out)
        lref = lsm[a.reshape(-1), np.arange(T * n)].reshape(T, n)
        L = out.reshape(nout, T, n)
        amax = np.abs(L).max(0)
        bars = make_bars(c)
        tol = 4 * res["scale"]["logit"] if bars["logit"] == "scaled" else bars["logit"][1]
        delta = (2 * tol * (1 + amax)).astype(np.float32)
        res["delta_max"] = float(delta.max())
        oa = np.empty((T, n), np.int32)
        fragile = np.zeros((T, n), bool)
        for t in range(T):
            lt = np.ascontiguousarray(L[:, t, :])
            oa[t], olp = sample(c, lt, t, vec_step0)
            # the numpy log-softmax above is the oracle's own, bit for bit
            assert np.array_equal(olp, lsm.reshape(nout, T, n)[oa[t], t, np.arange(n)])
            bad = np.nonzero(a[t] != oa[t])[0]
            if bad.size:
                l2 = lt.copy()
                l2[a[t, bad], bad] += delta[t, bad]
                exc[t, bad] = sample(c, l2, t, vec_step0)[0][bad] == a[t, bad]
            if count_fragile:
                for k in range(nout):
                    l2 = lt + np.where(np.arange(nout)[:, None] == k, delta[t][None, :], np.float32(0)).astype(np.float32)
                    fragile[t] |= (sample(c, l2, t, vec_step0)[0] != oa[t]) & (oa[t] != k)
        res["n_disagree"] = int((a != oa).sum())
        res["exact"]["action (not a near-tie)"] = int(((a != oa) & ~exc).sum())
        res["fragile"] = fragile
    res["logp"] = (np.abs(traj["logp"] - lref), lref)
    res["exception"] = exc

    # ---- transition part
    env = _new_env(c)
    tc, ep = env0["t"].astype(np.int32).copy(), env0["episode"].astype(np.int32).copy()
    pred = env0["raw_state"][0].astype(np.float32)
    term = np.asarray(traj["terminal"]).astype(np.uint8)
    acts = np.asarray(traj["action_f"], np.float32).reshape(T, n) if cont else np.asarray(traj["action_i"], np.int32)
    r_err, r_ref = np.empty((T, n)), np.empty((T, n), np.float32)
    o_err, o_ref = np.empty((T, ns, n)), np.empty((T, ns, n), np.float32)
    was_reset = np.zeros((T, n), bool)
    bad_term = 0
    for t in range(T):
        _restart(c, env, obs[t], pred)
        env.t[:] = tc
        env.episode[:] = ep.view(np.uint32)
        env.step(acts[t])
        bad_term += int((env.done != term[t]).sum())
        r_ref[t], o_ref[t] = env.reward, env.obs()
        r_err[t], o_err[t] = np.abs(traj["reward"][t] - env.reward), np.abs(obs[t + 1] - o_ref[t])
        was_reset[t] = env.done.astype(bool)
        pred = env.s[0].copy()
        # the counters of the next step follow the rollout's own terminal trace
        tc = np.where(term[t] != 0, 0, tc + 1).astype(np.int32)
        ep = (ep + (term[t] != 0)).astype(np.int32)
    res["reward"] = (r_err, r_ref)
    m = np.broadcast_to(was_reset[:, None, :], o_err.shape)
    res["obs"] = (np.where(m, 0, o_err), o_ref)
    res["obs_reset"] = (np.where(m, o_err, 0), o_ref)
    res["n_resets"] = was_reset.sum(0)
    s_ref = np.stack(env.s)
    m = np.broadcast_to(was_reset[T - 1][None, :], s_ref.shape)
    res["state"] = (np.where(m, 0, np.abs(env1["raw_state"] - s_ref)), s_ref)
    res["exact"].update({
        "terminal": bad_term,
        "raw state after a reset": int((m & (env1["raw_state"] != s_ref)).sum()),
        "_t": int((env1["t"] != env.t).sum()), "_episode": int((env1["episode"] != env.episode.view(np.int32)).sum()),
        "_done": int((env1["done"] != env.done).sum()),
    })
    res["env_reward"] = (np.abs(env1["reward"] - env.reward), env.reward.copy())
    adv = oracle.generalized_advantage_estimation(traj["reward"].T, traj["value"].T, GAMMA, LAM, terminal=term.T, dims=2,
                                                  dtype=np.float32).T
    res["exact"]["adv"] = int((traj["adv"] != adv).sum())
    res["exact"]["ret"] = int((traj["ret"] != (adv + traj["value"][:T]).astype(np.float32)).sum())
    return res


def _normalised(q, res, bar):
    """error / bar per element, and the failures of the bar's own form"""
    err, ref = res[q]
    kind = bar[0]
    if kind == "allclose":
        e = err / (bar[2] + bar[1] * np.abs(ref))
        return e, ([] if e.max() <= 1 else [f"{q}: {e.max():.3g} x the bar (rtol {bar[1]}, atol {bar[2]})"])
    if kind == "scaled":
        s = res["scale"][q]
        lim = np.minimum(4 * s * (1 + np.abs(ref)), bar[2] + bar[1] * np.abs(ref))
        e = err / lim
        return e, ([] if e.max() <= 1 else [f"{q}: {e.max():.3g} x the bar (4 x the Float32 scale {s:.3g})"])
    if kind == "close":
        e = err / (1 + np.abs(ref)) / bar[1]
    else:
        assert kind == "abs"
        e = err / bar[1]
    if not bar[2]:
        return e, ([] if e.max() <= 1 else [f"{q}: {e.max():.3g} x the bar ({kind} {bar[1]}, strict)"])
    fails = []
    if (e > 1).mean() > SHARE:
        fails.append(f"{q}: {(e > 1).mean():.3g} of the samples beyond {bar[1]} (share form)")
    # the cap of the share form: 5e-3 on a net output; a log-density moves by logp_gain per unit of that
    cap = FLIP_MAX / bar[1] if kind == "close" else (bar[1] + FLIP_MAX * res.get("logp_gain", 1.0)) / bar[1]
    if (e > cap).any():
        fails.append(f"{q}: max {e.max():.3g} x the bar beyond the cap of the share form")
    return e, fails


def check(res, bars):
    """-> (failures, summary): every bar and every exact quantity of an audit; summary holds, per quantity, the largest
    error in units of its bar (share rows: also the share beyond) and the near-tie exception share"""
    fails, summ = [], {}
    for q in ("value", "logp", "action", "reward", "env_reward", "obs", "obs_reset", "state"):
        if q not in res:
            continue
        e, f = _normalised(q, res, bars["reward" if q == "env_reward" else q])
        fails += f
        summ[q] = float(e.max())
        summ[q + "_abs"] = float(res[q][0].max())
    for k, v in res["exact"].items():
        if v:
            fails.append(f"{k}: {v} mismatches")
    share = float(res["exception"].mean())
    summ["exceptions"] = share
    summ["disagree"] = res["n_disagree"]
    if share > bars["exc_cap"]:
        fails.append(f"near-tie exceptions: {share:.3g} of the samples (cap {bars['exc_cap']})")
    return fails, summ


# ------------------------------------------------------------------------------------- the oracle's own rollout, stepwise
def oracle_rollout(c, params, periods=2, fault=None):
    """The oracle's free-running rollout of a case, sequenced step by step from the functions the audit calls (equal to
    oracle.ppo_rollout bit for bit: tests/test_rollout_audit_reference.py), `periods` update periods on one env.
    -> [(traj, env0, env1, vec_step0)].  fault injects one of the in-loop faults of the reference test."""
    n, T, ns, nout, cont = c["n"], c["T"], NS[c["env"]], nout_of(c), c["continuous"]
    p, np_a = params
    env = _new_env(c)
    apply_inject(c, env)
    out = []
    for period in range(periods):
        vs0 = period * T
        tr = dict(obs=np.zeros((T + 1, ns, n), np.float32), value=np.zeros((T + 1, n), np.float32),
                  logp=np.zeros((T, n), np.float32), reward=np.zeros((T, n), np.float32), terminal=np.zeros((T, n), np.uint8),
                  action_i=np.zeros((T, n), np.int32), action_f=np.zeros((T, n), np.float32))
        env0 = snapshot(env)
        cs = dict(c)
        if fault == "noise_env":
            cs["env_id_base"] = c["env_id_base"] + 1
        for t in range(T + 1):
            tr["obs"][t] = env.obs()
            tr["value"][t] = forward(c, p[np_a:], 1, tr["obs"][t])[0]
            if t == T:
                break
            o = forward(c, p[:np_a], nout, tr["obs"][t])
            ts = t + 1 if fault == "noise_step" else t
            if cont:
                sg = expf(o[1])
                a = o[0] + sg * oracle.ppo_rollout_noise(cs["seed"], cs["env_id_base"], n, [vs0 + ts])[0]
                tr["action_f"][t], tr["logp"][t] = a, normlogpdf(o[0], sg, a)
            else:
                a, tr["logp"][t] = sample(cs, o, ts, vs0)
                tr["action_i"][t] = a
            t_before, ep_before = env.t.copy(), env.episode.copy()
            env.step(a)
            done = env.done.astype(bool)
            if fault == "stale_episode" and done.any():  # the reset drew from the previous episode's counter
                env.episode[done] = ep_before[done] - 1
                rew = env.reward.copy()
                env.reset(done)
                env.done[:], env.reward[:] = done, rew
                env.episode[done] = ep_before[done] + 1
            if fault == "step_counter":  # the reset left the step counter running
                env.t[done] = t_before[done] + 1
            tr["reward"][t], tr["terminal"][t] = env.reward, env.done
        adv = oracle.generalized_advantage_estimation(tr["reward"].T, tr["value"].T, GAMMA, LAM, terminal=tr["terminal"].T,
                                                      dims=2, dtype=np.float32).T
        tr["adv"], tr["ret"] = np.ascontiguousarray(adv), (adv + tr["value"][:T]).astype(np.float32)
        out.append((tr, env0, snapshot(env), vs0))
    return out
