"""Injected-state grids that reach every branch of the env step (TEST INFRASTRUCTURE ONLY; a helper, not a test module).

Random-action and policy-driven runs never execute most branches of the env physics (MountainCar's wall, clamps and goal,
CartPole's x-threshold, Acrobot's success and velocity bounds, the range-reduction fall-backs behind Pendulum's angle), so
the tests built on this module START every env on such a branch: `grid(spec, n)` returns one deterministic set of
(raw state, t, action) rows per env kind, element type, action form and configuration, for

    n = 1024   the vector path of the step kernel (4 Float32 / 2 Float64 envs per lane)
    n = 1001   its scalar path

Placement.  Rows are NOT shuffled: for lane L = i // 4 the env 4 L + j is a TERMINATING row iff bit j of L mod 16 is set
(`term_mask`), so each of the 16 termination patterns of a lane -- none and all four included -- occurs in every
wavefront, and a reset loop that works off several terminated envs of one lane meets a prescribed mix.  `Grid.term` is
that prescribed set: the tests assert that the reference terminates exactly there.

How the rows are made.  A row that has to land EXACTLY on a comparison (x + v == min_pos, x' one ulp either side of
goal_pos, v' == goal_velocity, |x'| one ulp either side of xthreshold, theta + pi == RN(k 2 pi)) is found by solving the one
addition backwards in the env's own element type (`solve_add`), trying the neighbouring values; where no value lands
there the row is left out and the census below shows it.  The class of a row (terminating or not) follows from the target
it was solved for.  Acrobot's rows move by radians per step, so their class is read off tests/env_ref.py with a margin of
0.05 around the success threshold (both extremes of the torque noise, where there is noise).

Census.  `Grid.census(post, t1, done)` takes the REFERENCE's post-step, pre-reset raw state, counters and flags and counts
the hits of every branch the grid is meant to reach; `Grid.required` names the counts that must be >= 8.  A grid can thus
never silently miss its target.

`truncation=False` gives the grids of the fused consumers: no row terminates through max_steps (cfg max_steps = 100000,
t far below it), every termination is a goal / x-threshold one.
"""
import functools
import math
from types import SimpleNamespace

import numpy as np

import env_ref

PI = math.pi
MIN_HITS = 8
NO_TRUNC_MAX_STEPS = 100000


def term_mask(n):
    """bit j of (lane mod 16) decides env 4 * lane + j"""
    i = np.arange(n)
    return (((i // 4) % 16) >> (i % 4)) & 1 == 1


def up(x):
    return np.nextafter(x, type(x)(np.inf))


def dn(x):
    return np.nextafter(x, type(x)(-np.inf))


def neighbours(x, k):
    """x, then the values 1 .. k ulps either side of it"""
    out = [x]
    lo = hi = x
    for _ in range(k):
        lo, hi = dn(lo), up(hi)
        out += [hi, lo]
    return out


def solve_add(target, b, T, k=8):
    """a of type T with fl(a + b) == target in T arithmetic, or None"""
    target, b = T(target), T(b)
    for a in neighbours(T(target - b), k):
        if T(a + b) == target:
            return a
    return None


def cosT(x, T):
    return T(math.cos(float(x)))


# ------------------------------------------------------------------------------------------------------------ specs
def _spec(kind, dtype, continuous, tag, **cfg):
    T = np.dtype(dtype).type
    name = f"{kind}-{'f32' if T is np.float32 else 'f64'}-{'cont' if continuous else 'disc'}-{tag}"
    return SimpleNamespace(id=name, kind=kind, dtype=T, continuous=continuous, cfg=cfg)


MC_CFG2 = dict(goal_velocity=0.02, power=0.0015, gravity=0.003)
CP_CFG2 = dict(masscart=2.6, masspole=0.37, halflength=0.8, forcemag=7.0, dt=0.013, gravity=3.7)
SPECS = []
for _T in (np.float32, np.float64):
    for _c in (False, True):
        SPECS.append(_spec("mountaincar", _T, _c, "default"))
        SPECS.append(_spec("mountaincar", _T, _c, "gv002", **MC_CFG2))
        SPECS.append(_spec("cartpole", _T, _c, "default"))
        SPECS.append(_spec("cartpole", _T, _c, "theta90", thetathreshold=90.0))
        SPECS.append(_spec("cartpole", _T, _c, "heavy", **CP_CFG2))
    SPECS.append(_spec("pendulum", _T, True, "default"))
    for _na in (2, 3, 5, 9):
        SPECS.append(_spec("pendulum", _T, False, f"na{_na}", n_actions=_na))
    for _nips in (0, 1):
        for _noise in (0.0, 0.4):
            SPECS.append(_spec("acrobot", _T, False, ("nips" if _nips else "book") + ("-noise" if _noise else ""), nips=_nips,
                               max_torque_noise=_noise))
SPEC_BY_ID = {s.id: s for s in SPECS}
assert len(SPEC_BY_ID) == len(SPECS)


# ----------------------------------------------------------------------------------------------------------- assembly
def _assemble(spec, n, p, term_rows, safe_rows, fill_term, fill_safe, rng, census, required, truncation):
    """rows are (state tuple, t, action); the specials come first in index order, the fillers take what is left"""
    T = spec.dtype
    mask = term_mask(n)
    sdim = env_ref.SDIM[spec.kind]
    s = np.zeros((sdim, n), T)
    t = np.zeros(n, np.int32)
    a = np.zeros(n, T if spec.continuous else np.int32)
    it_term, it_safe = iter(term_rows), iter(safe_rows)
    for i in range(n):
        row = next(it_term if mask[i] else it_safe, None)
        if row is None:
            row = (fill_term if mask[i] else fill_safe)(rng)
        s[:, i], t[i], a[i] = row[0], row[1], row[2]
    assert next(it_term, None) is None and next(it_safe, None) is None, f"{spec.id}: more special rows than slots at n = {n}"
    cfg = dict(spec.cfg)
    if not truncation:
        cfg["max_steps"] = NO_TRUNC_MAX_STEPS
    g = SimpleNamespace(id=f"{spec.id}-n{n}", spec=spec, kind=spec.kind, dtype=T, continuous=spec.continuous, n=n, cfg=cfg, p=p,
                        s=s, t=t, a=a, term=mask, required=tuple(required), seed=1234 + len(spec.id), env_id_base=7 + n)
    g.census = functools.partial(census, g)
    return g


def _rand_t(rng, p):
    return int(rng.integers(0, max(1, min(p["max_steps"], 1000) - 2)))


# -------------------------------------------------------------------------------------------------------- MountainCar
def _mc_force(p, a):
    return p["T"](a) if p["continuous"] else p["T"](int(a) - 1)


def _mc_acc(p, x, a):
    """the increment of v in _step! (MountainCarEnv.jl:122), in T"""
    T = p["T"]
    return T(_mc_force(p, a) * p["power"] + cosT(T(3) * x, T) * (-p["gravity"]))


def _mc_row(p, Xp, Vp, a):
    """(x, v) from which one unclamped step lands exactly on (Xp, Vp)"""
    T = p["T"]
    Xp, Vp = T(Xp), T(Vp)
    for x in neighbours(T(Xp - Vp), 8):
        if T(x + Vp) != Xp or not (p["min_pos"] <= x <= p["max_pos"]):
            continue
        v = solve_add(Vp, _mc_acc(p, x, a), T)
        if v is not None and abs(v) <= p["max_speed"]:
            return x, v
    return None


def _mc_actions(p, k):
    return [p["T"](v) for v in np.linspace(-1, 1, k)] if p["continuous"] else [i % 3 for i in range(k)]


def _mountaincar(spec, n, truncation):
    T = spec.dtype
    cfg = dict(spec.cfg) if truncation else dict(spec.cfg, max_steps=NO_TRUNC_MAX_STEPS)
    p = env_ref.params("mountaincar", T, continuous=spec.continuous, **cfg)
    rng = np.random.default_rng(sum(map(ord, spec.id)))
    lo, hi, ms, goal, gv, steps = p["min_pos"], p["max_pos"], p["max_speed"], p["goal_pos"], p["goal_velocity"], p["max_steps"]
    acts = _mc_actions(p, 8)
    a_push = T(1) if spec.continuous else 2  # force +1
    a_pull = T(-1) if spec.continuous else 0
    a_zero = T(0) if spec.continuous else 1
    term, safe = [], []

    def add(rows, xv, t, a):
        if xv is not None:
            rows.append(((xv[0], xv[1]), t, a))

    vps = [T(v) for v in np.linspace(float(gv) + 0.005, 0.065, 8)]
    for j, vp in enumerate(vps):
        add(term, _mc_row(p, goal, vp, acts[j]), j, acts[j])                         # x' == goal_pos
        add(term, _mc_row(p, up(goal), vp, acts[j]), 3 * j, acts[j])                 # one ulp beyond
        add(safe, _mc_row(p, dn(goal), vp, acts[j]), 5 * j, acts[j])                 # one ulp short: not done
    for j, xp in enumerate(np.linspace(float(goal) + 0.002, float(hi) - 0.002, 8)):
        add(term, _mc_row(p, T(xp), gv, acts[j]), 7 * j, acts[j])                    # v' == goal_velocity: done (>=)
        if gv > 0:
            add(safe, _mc_row(p, T(xp), dn(gv), acts[j]), 11 * j, acts[j])           # one ulp slower: not done
    for j in range(8):
        term.append(((T(float(hi) + 0.002 * (j + 1)), T(0.03)), j, acts[j]))         # x starts beyond max_pos
        term.append(((T(float(hi) - 0.01), T(0.04 + 0.003 * j)), 2 * j, acts[j]))    # x + v beyond max_pos
        term.append(((T(float(goal) - 0.06 + 0.001 * j), ms), 4 * j, a_push))        # speed clamp, then the goal
    # x + max_speed one ulp either side of goal_pos, with v clamped to exactly max_speed
    for tgt, rows in ((dn(goal), safe), (goal, term), (up(goal), term)):
        for x in neighbours(T(tgt - ms), 8):
            if T(x + ms) == tgt:
                for v0 in (ms, dn(ms), up(ms)):
                    rows.append(((x, v0), 9, a_push))
                break
    if truncation:
        for j in range(10):
            add(term, _mc_row(p, T(float(goal) + 0.01 + 0.002 * j), vps[j % 8], acts[j % 8]), steps - 1, acts[j % 8])  # goal AND t == max_steps
            term.append(((T(-0.5 - 0.05 * j), T(0.01 * (j - 4))), steps - 1, acts[j % 8]))   # max_steps alone
            safe.append(((T(-0.5 - 0.05 * j), T(0.01 * (j - 4))), steps - 2, acts[j % 8]))   # one step before it
    for a in (a_pull, a_zero, a_push):
        for v0 in (T(-0.03), T(-0.0), T(0.0), T(0.03)):                              # x == min_pos, the four signs of v
            for rep in range(3):
                safe.append(((lo, T(v0 * (1 + 0.5 * rep)) if v0 != 0 else v0), 13 * rep, a))
        add(safe, _mc_row(p, lo, T(0.0), a), 17, a)                                   # lands on the wall with v' == +0
    for j, vp in enumerate(np.linspace(-0.06, -0.005, 8)):
        add(safe, _mc_row(p, lo, T(vp), acts[j]), 19 * j, acts[j])                    # x + v == min_pos exactly, v < 0
        add(safe, _mc_row(p, up(lo), T(vp), acts[j]), 21 * j, acts[j])                # one ulp inside: v stays (the rule is ==)
        add(safe, _mc_row(p, up(lo), T(vp * 0.9), acts[7 - j]), 22 * j, acts[7 - j])
    # v one ulp beyond +-max_speed before the clamp: force 0 next to a zero of cos(3 x), where the increment is ~1 ulp of v
    x0 = T(-PI / 6)
    for sign in (1, -1):
        found = 0
        xs = x0
        for _ in range(6000):
            xs = dn(xs) if sign > 0 else up(xs)
            vpre = T(T(sign) * ms + _mc_acc(p, xs, a_zero))
            if vpre == (up(ms) if sign > 0 else dn(-ms)):
                safe.append(((xs, T(sign) * ms), 23, a_zero))
                found += 1
                if found == 6:
                    break

    def fill_term(r):
        # 4e-3 clear of both comparisons: another action moves v' and x' by at most 2 * power, the class of the row holds
        xp, vp, a = r.uniform(float(goal) + 4e-3, float(hi) - 1e-3), r.uniform(float(gv) + 4e-3, 0.065), acts[r.integers(8)]
        x = T(xp - vp)
        return (x, T(vp - float(_mc_acc(p, x, a)))), _rand_t(r, p), a

    def fill_safe(r):
        a = acts[r.integers(8)]
        c = r.integers(3)
        if c == 0:    # next to the wall: clamp and zeroing, or bouncing off
            xv = (T(r.uniform(-1.2, -1.19)), T(r.uniform(-0.07, 0.07)))
        elif c == 1:  # in the goal region, moving away from it
            xv = (T(r.uniform(0.44, 0.6)), T(r.uniform(-0.07, -0.01)))
        else:         # the whole box short of the goal
            xv = (T(r.uniform(-1.2, float(goal) - 0.08)), T(r.uniform(-0.07, 0.07)))
        return xv, _rand_t(r, p), a

    required = ["wall_v_zeroed", "min_pos_clamp", "landed_on_min_pos", "one_ulp_inside_wall_v_kept", "max_pos_clamp", "x_started_beyond_max_pos", "speed_clamp",
                "speed_clamp_within_2ulp", "goal", "goal_exact", "goal_plus_ulp", "goal_minus_ulp", "v_eq_goal_velocity",
                "x_min_v_neg", "x_min_v_negzero", "x_min_v_poszero", "x_min_v_pos"]
    if gv > 0:
        required.append("v_ulp_below_goal_velocity")
    if truncation:
        required += ["goal_and_max_steps", "max_steps_only"]
    return _assemble(spec, n, p, term, safe, fill_term, fill_safe, rng, _mc_census, required, truncation)


def _mc_census(g, post, t1, done):
    p, T = g.p, g.dtype
    f8 = lambda v: np.asarray(v, np.float64)  # noqa: E731
    x, v = f8(g.s[0]), f8(g.s[1])
    force = f8(g.a) if g.continuous else f8(g.a) - 1
    vpre = v + (force * f8(p["power"]) - f8(p["gravity"]) * np.cos(3 * x))
    ms, lo, hi, goal, gv = (f8(p[k]) for k in ("max_speed", "min_pos", "max_pos", "goal_pos", "goal_velocity"))
    vcl = np.clip(vpre, -ms, ms)
    xpre = x + vcl
    ulp_v, ulp_x = f8(np.spacing(p["max_speed"])), f8(np.spacing(p["min_pos"]))
    x1, v1, done = post[0], post[1], np.asarray(done, bool)
    at_goal = (x1 >= p["goal_pos"]) & (v1 >= p["goal_velocity"])
    trunc = np.asarray(t1) >= p["max_steps"]
    c = dict(
        wall_v_zeroed=(x1 == p["min_pos"]) & (vcl < -ulp_v) & (v1 == 0),
        min_pos_clamp=xpre < lo + ulp_x * -0.5,
        landed_on_min_pos=(x1 == p["min_pos"]) & (np.abs(xpre - lo) <= 0.5 * abs(ulp_x)) & (np.abs(vpre) < ms),
        one_ulp_inside_wall_v_kept=(x1 == up(p["min_pos"])) & (v1 < 0),
        max_pos_clamp=(xpre > hi + 1e-6) & (x1 == p["max_pos"]),
        x_started_beyond_max_pos=g.s[0] > p["max_pos"],
        speed_clamp=(np.abs(vpre) > ms + 0.25 * ulp_v) & (np.abs(v1) <= p["max_speed"]),
        speed_clamp_within_2ulp=(np.abs(vpre) > ms + 0.25 * ulp_v) & (np.abs(vpre) < ms + 2 * ulp_v),
        goal=done & at_goal & ~trunc,
        goal_exact=done & at_goal & (x1 == p["goal_pos"]),
        goal_plus_ulp=done & at_goal & (x1 == up(p["goal_pos"])),
        goal_minus_ulp=~done & (x1 == dn(p["goal_pos"])) & (v1 >= p["goal_velocity"]),
        v_eq_goal_velocity=done & (x1 >= p["goal_pos"]) & (v1 == p["goal_velocity"]),
        v_ulp_below_goal_velocity=~done & (x1 >= p["goal_pos"]) & (v1 == dn(p["goal_velocity"])),
        goal_and_max_steps=done & at_goal & trunc,
        max_steps_only=done & ~at_goal & trunc,
        x_min_v_neg=(g.s[0] == p["min_pos"]) & (g.s[1] < 0),
        x_min_v_negzero=(g.s[0] == p["min_pos"]) & (g.s[1] == 0) & np.signbit(g.s[1]),
        x_min_v_poszero=(g.s[0] == p["min_pos"]) & (g.s[1] == 0) & ~np.signbit(g.s[1]),
        x_min_v_pos=(g.s[0] == p["min_pos"]) & (g.s[1] > 0),
    )
    return {k: int(np.sum(m)) for k, m in c.items()}


# ----------------------------------------------------------------------------------------------------------- CartPole
def _cartpole(spec, n, truncation):
    T = spec.dtype
    cfg = dict(spec.cfg) if truncation else dict(spec.cfg, max_steps=NO_TRUNC_MAX_STEPS)
    p = env_ref.params("cartpole", T, continuous=spec.continuous, **cfg)
    rng = np.random.default_rng(sum(map(ord, spec.id)))
    thr, dt, thth, steps = p["xthreshold"], p["dt"], float(p["thetathreshold"]), p["max_steps"]
    thd_max = min(6.0, 0.2 * thth / float(dt))

    def act(r):
        return T(r.uniform(-1, 1)) if spec.continuous else int(r.integers(2))

    def pole(r):
        return T(r.uniform(-0.7, 0.7) * thth), T(r.uniform(-thd_max, thd_max))

    def row(r, x, xdot, t):
        th, thd = pole(r)
        return (x, xdot, th, thd), t, act(r)

    term, safe = [], []
    for sign in (1, -1):
        for j in range(6):
            xdot = T(sign * (0.3 + 0.45 * j) * (1 if j % 2 else -1))
            dx = T(dt * xdot)
            for tgt, rows in ((up(thr), term), (thr, safe), (dn(thr), safe)):  # strict >: |x'| == xthreshold goes on
                x = solve_add(T(sign) * tgt, dx, T)
                if x is not None:
                    rows.append(row(rng, x, xdot, 3 * j))
    if truncation:
        for j in range(8):  # an episode ends at t > max_steps: t' = max_steps goes on, max_steps + 1 and + 2 end
            safe.append(row(rng, T(rng.uniform(-2, 2)), T(rng.uniform(-1, 1)), steps - 1))
            term.append(row(rng, T(rng.uniform(-2, 2)), T(rng.uniform(-1, 1)), steps))
            term.append(row(rng, T(rng.uniform(-2, 2)), T(rng.uniform(-1, 1)), steps + 1))

    def fill(r, ends):
        # |x| uniform in [2.3, 2.5]; the cart's speed decides on which side of the threshold it lands (1e-3 clear of it)
        sign = 1 if r.integers(2) else -1
        ax = r.uniform(2.3, 2.5)
        need = (float(thr) - ax) / float(dt)
        m = 1e-3 / float(dt)
        xd = max(need + m, -3.0) + r.uniform(0, 3) if ends else min(need - m, 3.0) - r.uniform(0, 3)
        return row(r, T(sign * ax), T(sign * xd), _rand_t(r, p))

    required = ["x_only", "x_plus_ulp", "x_eq_threshold", "x_minus_ulp", "started_beyond_and_came_back"]
    if truncation:
        required += ["t_eq_max_steps_goes_on", "t_max_steps_plus_1", "t_max_steps_plus_2"]
    return _assemble(spec, n, p, term, safe, lambda r: fill(r, True), lambda r: fill(r, False), rng, _cp_census, required,
                     truncation)


def _cp_census(g, post, t1, done):
    p = g.p
    done, t1 = np.asarray(done, bool), np.asarray(t1)
    ax, ath = np.abs(post[0]), np.abs(post[2])
    inside = (ath <= p["thetathreshold"]) & (t1 <= p["max_steps"])
    c = dict(
        x_only=done & (ax > p["xthreshold"]) & inside,
        x_plus_ulp=done & (ax == up(p["xthreshold"])) & inside,
        x_eq_threshold=~done & (ax == p["xthreshold"]),
        x_minus_ulp=~done & (ax == dn(p["xthreshold"])),
        started_beyond_and_came_back=~done & (np.abs(g.s[0]) > p["xthreshold"]),
        t_eq_max_steps_goes_on=~done & (t1 == p["max_steps"]),
        t_max_steps_plus_1=done & (t1 == p["max_steps"] + 1) & (ax <= p["xthreshold"]) & (ath <= p["thetathreshold"]),
        t_max_steps_plus_2=done & (t1 == p["max_steps"] + 2) & (ax <= p["xthreshold"]) & (ath <= p["thetathreshold"]),
    )
    return {k: int(np.sum(m)) for k, m in c.items()}


# ----------------------------------------------------------------------------------------------------------- Pendulum
PENDULUM_K = (1, 2, 3, 7, 100, 1000, 10000)
TRIG_SMALL_MAX = np.float32(0.78539816)  # the kernel's pi / 4 split, a Float32 constant
TRIG_MEDIUM_MAX = 65536.0


def _pendulum(spec, n, truncation):
    T = spec.dtype
    cfg = dict(spec.cfg) if truncation else dict(spec.cfg, max_steps=NO_TRUNC_MAX_STEPS)
    p = env_ref.params("pendulum", T, continuous=spec.continuous, **cfg)
    rng = np.random.default_rng(sum(map(ord, spec.id)))
    na, steps, ms = p["n_actions"], p["max_steps"], p["max_speed"]
    piT = T(PI)

    def act(r):
        return T(r.uniform(-2.4, 2.4)) if spec.continuous else int(r.integers(na))

    rows = []  # (theta, thdot, action); t comes from the slot

    def add(th, thd=None, a=None):
        if th is not None:
            rows.append((T(th), T(rng.uniform(-7, 7)) if thd is None else T(thd), act(rng) if a is None else a))

    a0 = T(0) if spec.continuous else na // 2
    tq0 = float(np.clip(env_ref.pendulum_torque(p, np.array([a0]))[0], -p["max_torque"], p["max_torque"]))

    def before(th1, a):
        """theta from which a step at thdot = 0 under the torque of a0 ends near th1 (fixed point in Float64; the bands are wide)"""
        g_, l_, m_, dt_ = (float(p[k]) for k in ("g", "l", "m", "dt"))
        th = th1
        for _ in range(8):
            th = th1 - dt_ * dt_ * (-3 * g_ / (2 * l_) * math.sin(th + PI) + 3 * tq0 / (m_ * l_ * l_))
        return th

    for k in PENDULUM_K:  # theta + pi == RN(k 2 pi) and its two neighbours: both corrections of the quotient
        for sk in (k, -k):
            tgt = T(sk * 2 * PI)
            for v in (dn(tgt), tgt, up(tgt)):
                add(solve_add(v, piT, T))
    for j in range(10):
        add(-piT)  # theta + pi == 0: the r == 0 exit of the floored modulo
    for sign in (1, -1):
        for j in range(24):
            add(sign * rng.uniform(6e4, 65536 - 4))     # the last values of the fast range reduction
            add(sign * rng.uniform(65536 + 4, 7e4))     # the fall-back
        for v in (T(TRIG_MEDIUM_MAX), up(T(TRIG_MEDIUM_MAX)), dn(T(TRIG_MEDIUM_MAX))):
            add(solve_add(T(sign) * v, piT, T))
        for j in range(12):  # either side of pi / 4 = 0.78539...
            for lo_, hi_ in ((0.78, 0.7853), (0.7855, 0.79)):
                add(sign * rng.uniform(lo_, hi_), thd=rng.uniform(-0.05, 0.05))                 # theta
                add(before(sign * rng.uniform(lo_, hi_), a0), thd=0.0, a=a0)   # theta' (the observation's sin / cos)
                add(T(T(sign * rng.uniform(lo_, hi_)) - piT))                  # theta + pi (the step's sin)
        for v in (T(TRIG_SMALL_MAX), up(T(TRIG_SMALL_MAX)), dn(T(TRIG_SMALL_MAX))):
            add(solve_add(T(sign) * v, piT, T))
            add(T(sign) * v, thd=0.0, a=T(0) if spec.continuous else na // 2)
        a_out = (T(sign * 2) if spec.continuous else (na - 1 if sign > 0 else 0))
        for j in range(8):  # thdot at +-max_speed, torque outward: the speed clamp
            add(rng.uniform(-0.3, 0.3), thd=T(sign) * ms, a=a_out)
        if spec.continuous:
            for a in (up(T(2)), T(2.5), T(3), T(7)):  # torque beyond +-max_torque
                add(rng.uniform(-3, 3), a=T(sign) * a)
                add(rng.uniform(-3, 3), thd=T(sign) * ms, a=T(sign) * a)
    mask = term_mask(n)
    it = iter(rows)

    def nxt(r):
        row = next(it, None)
        if row is None:
            row = (T(r.uniform(-4 * PI, 4 * PI)), T(r.uniform(-8, 8)), act(r))
        return row

    # every row is as good in a terminating slot as in any other: Pendulum ends through t alone (t' >= max_steps)
    def fill_term(r):
        row = nxt(r)
        return (row[0], row[1]), (steps - 1 if truncation else _rand_t(r, p)), row[2]

    def fill_safe(r):
        row = nxt(r)
        return (row[0], row[1]), int(r.integers(0, min(steps, 1000) - 2)), row[2]

    required = ["near_multiple_of_2pi", "thpi_zero", "thpi_beyond_2p16", "thpi_just_inside_2p16", "step_arg_below_pio4",
                "step_arg_above_pio4", "obs_arg_below_pio4", "obs_arg_above_pio4", "speed_clamp"]
    if spec.continuous:
        required.append("torque_clamp")
    if truncation:
        required.append("ended_by_t")
    g = _assemble(spec, n, p, [], [], fill_term, fill_safe, rng, _pd_census, required, truncation)
    assert next(it, None) is None, f"{spec.id}: more special rows than envs"
    if not truncation:
        g.term = np.zeros(n, bool)
    return g


def _pd_census(g, post, t1, done):
    p, T = g.p, g.dtype
    th, thd = g.s[0], g.s[1]
    thpi = (th + T(PI)).astype(T)
    near = np.zeros(g.n, bool)
    for k in PENDULUM_K:
        for sk in (k, -k):
            tgt = T(sk * 2 * PI)
            near |= (thpi == tgt) | (thpi == up(tgt)) | (thpi == dn(tgt))
    a = env_ref.pendulum_torque(p, g.a)
    athpi, ath1 = np.abs(thpi), np.abs(post[0])
    band = (athpi >= 0.77) & (athpi <= 0.80)
    band1 = (ath1 >= 0.77) & (ath1 <= 0.80)
    c = dict(
        near_multiple_of_2pi=near,
        thpi_zero=thpi == 0,
        thpi_beyond_2p16=athpi > TRIG_MEDIUM_MAX,
        thpi_just_inside_2p16=(athpi <= TRIG_MEDIUM_MAX) & (athpi >= 6e4),
        step_arg_below_pio4=band & (athpi <= TRIG_SMALL_MAX),
        step_arg_above_pio4=band & (athpi > TRIG_SMALL_MAX),
        obs_arg_below_pio4=band1 & (ath1 <= TRIG_SMALL_MAX),
        obs_arg_above_pio4=band1 & (ath1 > TRIG_SMALL_MAX),
        speed_clamp=(np.abs(post[1]) == p["max_speed"]) & (np.abs(thd) == p["max_speed"]) & (np.sign(a) == np.sign(thd)),
        torque_clamp=np.abs(a) > p["max_torque"],
        ended_by_t=np.asarray(done, bool),
    )
    return {k: int(np.sum(m)) for k, m in c.items()}


# ------------------------------------------------------------------------------------------------------------ Acrobot
def _acrobot(spec, n, truncation):
    T = spec.dtype
    cfg = dict(spec.cfg) if truncation else dict(spec.cfg, max_steps=NO_TRUNC_MAX_STEPS)
    p = env_ref.params("acrobot", T, **cfg)
    rng = np.random.default_rng(sum(map(ord, spec.id)))
    steps = p["max_steps"]
    u = rng.uniform
    sg = lambda: 1.0 if rng.integers(2) else -1.0  # noqa: E731
    cats = [[], [], [], []]
    for _ in range(500):
        cats[0].append((sg() * (PI - u(0, 0.3)), u(-0.2, 0.2), u(-0.5, 0.5), u(-0.5, 0.5)))            # near upright: success
        cats[1].append((u(-PI, PI), u(-PI, PI), sg() * u(12, 14), sg() * u(27, 30)))                   # both velocity bounds
        s1, s2 = sg(), sg()
        folded = rng.integers(2)
        cats[2].append((s1 * (PI - u(0, 0.05)), s2 * (PI - u(0, 0.05)) if folded else u(-0.2, 0.2),   # within one step of +-pi
                        s1 * u(0.5, 2), s2 * u(0.5, 2) if folded else u(-0.5, 0.5)))
        cats[3].append((u(-PI, PI), u(-PI, PI), u(-2, 2), u(-3, 3)))                                   # anywhere
    cand = np.array([c for quad in zip(*cats) for c in quad], T).T  # interleaved: every category in every stretch of four
    acts = rng.integers(0, 3, cand.shape[1]).astype(np.int32)
    crit = []
    for noise_u in ((0.0, 1.0) if p["max_torque_noise"] > 0 else (0.5,)):
        s1, _, _, _ = env_ref.acrobot_step(p, cand, np.zeros(cand.shape[1], np.int32), acts, noise_u=np.full(cand.shape[1], noise_u, T))
        crit.append(-np.cos(s1[0].astype(np.float64)) - np.cos(s1[1].astype(np.float64) + s1[0].astype(np.float64)))
    crit = np.array(crit)
    succ, fail = (crit > 1.05).all(0), (crit < 0.95).all(0)
    term = [(tuple(cand[:, i]), None, int(acts[i])) for i in np.nonzero(succ)[0]]
    safe = [(tuple(cand[:, i]), None, int(acts[i])) for i in np.nonzero(fail)[0]]
    if truncation:  # t' == max_steps goes on; max_steps + 1 and + 2 end whatever the state (e.t > max_steps after the increment)
        ts = [steps - 1] * 10
        safe = [(r[0], ts.pop() if ts and j % 3 == 0 else None, r[2]) for j, r in enumerate(safe)]
        late = [(r[0], steps + (j % 2), r[2]) for j, r in enumerate(safe[40:60])]
        term = term[:8] + [x for pair in zip(late, term[8:28]) for x in pair] + term[28:]
    it_term, it_safe = iter(term), iter(safe)

    def fill(it):
        def f(r):
            row = next(it)
            return row[0], (_rand_t(r, p) if row[1] is None else row[1]), row[2]
        return f

    required = ["success", "vel_a_bound", "vel_b_bound", "wrap_theta1", "wrap_theta2"]
    if truncation:
        required += ["t_eq_max_steps_goes_on", "ended_by_t_alone"]
    return _assemble(spec, n, p, [], [], fill(it_term), fill(it_safe), rng, _ac_census, required, truncation)


def _ac_census(g, post, t1, done):
    p = g.p
    done, t1 = np.asarray(done, bool), np.asarray(t1)
    f8 = lambda v: np.asarray(v, np.float64)  # noqa: E731
    succ = (-np.cos(f8(post[0])) - np.cos(f8(post[1]) + f8(post[0]))) > 1.0
    c = dict(
        success=done & succ & (t1 <= p["max_steps"]),
        vel_a_bound=np.abs(post[2]) == p["max_vel_a"],
        vel_b_bound=np.abs(post[3]) == p["max_vel_b"],
        wrap_theta1=np.abs(f8(post[0]) - f8(g.s[0])) > PI,
        wrap_theta2=np.abs(f8(post[1]) - f8(g.s[1])) > PI,
        t_eq_max_steps_goes_on=~done & (t1 == p["max_steps"]),
        ended_by_t_alone=done & ~succ & (t1 > p["max_steps"]),
    )
    return {k: int(np.sum(m)) for k, m in c.items()}


# --------------------------------------------------------------------------------------------------------------- API
_BUILDERS = {"mountaincar": _mountaincar, "cartpole": _cartpole, "pendulum": _pendulum, "acrobot": _acrobot}
SIZES = (1024, 1001)


@functools.lru_cache(maxsize=None)
def _grid(spec_id, n, truncation):
    spec = SPEC_BY_ID[spec_id]
    return _BUILDERS[spec.kind](spec, n, truncation)


def grid(spec, n=1024, truncation=True):
    """The grid of one spec (or spec id).  Treat the arrays as read-only: grids are shared between tests."""
    return _grid(spec if isinstance(spec, str) else spec.id, int(n), bool(truncation))


def tiled(g, reps):
    """the same grid `reps` times over (n = 1024 keeps the lane pattern: 1024 is a multiple of 64)"""
    t = SimpleNamespace(**vars(g))
    t.n, t.s, t.t, t.a, t.term = g.n * reps, np.tile(g.s, (1, reps)), np.tile(g.t, reps), np.tile(g.a, reps), np.tile(g.term, reps)
    t.id = f"{g.id}x{reps}"
    t.census = functools.partial(g.census.func, t)
    return t


def all_grid_ids():
    return [(s.id, n) for s in SPECS for n in SIZES]


if __name__ == "__main__":  # the census tables of profiles/env_edges.md: python tests/env_edge_cases.py
    import os
    import sys

    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import oracle

    for spec in SPECS:
        counts = []
        for n in SIZES:
            g = grid(spec, n)
            kw = dict(g.cfg) if g.kind == "acrobot" else dict(g.cfg, continuous=g.continuous)
            ref = oracle.VecEnv(g.kind, n, seed=g.seed, env_id_base=g.env_id_base, dtype=g.dtype, auto_reset=False, **kw)
            ref.set_state(g.s, g.t)
            ref.step(g.a)
            counts.append(g.census(np.stack(ref.s), ref.t, ref.done))
        print(f"### {spec.id}\n\n| branch | hits | required |\n|---|---|---|")
        for k in counts[0]:
            print(f"| {k} | {counts[0][k]} / {counts[1][k]} | {'yes' if k in g.required else ''} |")
        print()
