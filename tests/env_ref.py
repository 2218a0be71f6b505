"""An independent numpy model of one act! of the four envs (TEST INFRASTRUCTURE ONLY; a helper, not a test module).

Written from the reference's Julia sources, formula by formula, WITHOUT looking at oracle/ or csrc/:

    RLEnvs = src/ReinforcementLearningEnvironments/src/environments
    CartPoleEnv      RLEnvs/examples/CartPoleEnv.jl      act! :106-116   _step! :118-140   reward :84
    PendulumEnv      RLEnvs/examples/PendulumEnv.jl      act! :94-98     _step! :100-118   torque :120-122   state :70
    MountainCarEnv   RLEnvs/examples/MountainCarEnv.jl   act! :107-117   _step! :119-135   reward :95
    AcrobotEnv       RLEnvs/3rd_party/AcrobotEnv.jl      act! :101-132   dsdt :134-187     wrap :192-212  bound :214-225

What it is for: tests/test_env_reference.py steps oracle.VecEnv (auto-reset off) and this model from the same injected
states (tests/env_edge_cases.py) and compares them.  Two restatements made by different routes agree only where both read
the source the same way.

Conventions
  * no auto-reset, no RNG: `step(kind, p, s, t, a, noise_u=None)` maps (state, t, action) to (state', t', reward, done).  The
    one random number of an act! (Acrobot's torque noise, `rand(env.rng, T, 1)` :109) is an ARGUMENT, so that the model
    does not depend on the project's counter-based generator.
  * actions are 0-based like the C ABI: Julia's `a` is `a0 + 1`.  Continuous actions have the env's element type T (the
    vector env stores them as T).
  * T = Float32 reproduces Julia's promotions: Float32 op Float64 -> Float64, Int op Float32 -> Float32,
    Float32 + pi -> Float32, 2 * pi -> Float64, `a * b * c` and `a + b + c` fold to the left, no FMA contraction, a store
    into Vector{T} or a ::T field rounds to T.  Every promotion is spelled out with `_f64(...)`; every array below has an
    explicit dtype, so numpy's own promotion rules never decide anything.
  * sin / cos of a Float32 are the Float64 libm value rounded once (`np.float32(math.sin(float(x)))`), elementwise, as Julia's
    sin(::Float32) is a double-precision kernel behind a Float32 interface.
  * Acrobot: the reference integrates with OrdinaryDiffEq's adaptive solve(ode, RK4()) (:115-116); the project pins ONE
    classic RK4 step of length dt over the reference's dsdt, in Float64, the state stored as T (AcrobotRK4Env).  The
    success test (:128) reads the state as stored, i.e. as T.

`fault=` plants a wrong rule on purpose (tests/test_env_reference.py shows that the comparison catches it):
    "wall_ulp"  MountainCar: zero v at x <= min_pos + 1 ulp instead of x == min_pos
    "x_ge"      CartPole: abs(x) >= xthreshold instead of >
"""
import math

import numpy as np

F64 = np.float64
KINDS = ("cartpole", "pendulum", "mountaincar", "acrobot")
SDIM = {"cartpole": 4, "pendulum": 2, "mountaincar": 2, "acrobot": 4}
PI = math.pi


def _f64(x):
    return np.asarray(x, dtype=F64)


def _map(fn, x):
    """libm, one element at a time: math.sin / math.cos of the Float64 value, rounded once to x's own type"""
    x = np.asarray(x)
    out = np.empty(x.shape, x.dtype)
    xf, of = x.reshape(-1), out.reshape(-1)
    for i in range(xf.size):
        of[i] = fn(float(xf[i]))
    return out


def sin(x):
    return _map(math.sin, x)


def cos(x):
    return _map(math.cos, x)


def _clamp(x, lo, hi):
    """Base.clamp(x, lo, hi) = ifelse(x > hi, hi, ifelse(x < lo, lo, x)), all of one type"""
    return np.where(x > hi, hi, np.where(x < lo, lo, x)).astype(x.dtype)


# ----------------------------------------------------------------------------------------------------- parameters
def params(kind, T, continuous=None, **kw):
    """The params struct of the env's constructor: keyword defaults of the source, derived fields computed in Float64 from the
    Float64 keywords, every field then converted to T by the struct constructor."""
    T = np.dtype(T).type
    if kind == "cartpole":  # CartPoleEnv.jl:22-46
        d = dict(gravity=9.8, masscart=1.0, masspole=0.1, halflength=0.5, forcemag=10.0, max_steps=200, dt=0.02,
                 thetathreshold=12.0, xthreshold=2.4)
        _update(d, kw)
        p = dict(gravity=T(d["gravity"]), masscart=T(d["masscart"]), masspole=T(d["masspole"]),
                 totalmass=T(d["masscart"] + d["masspole"]), halflength=T(d["halflength"]),
                 polemasslength=T(d["masspole"] * d["halflength"]), forcemag=T(d["forcemag"]), dt=T(d["dt"]),
                 thetathreshold=T(d["thetathreshold"] * PI / 180), xthreshold=T(d["xthreshold"]))
        continuous = bool(continuous)  # :74 continuous = false
    elif kind == "pendulum":  # PendulumEnv.jl:41-53
        d = dict(max_speed=8.0, max_torque=2.0, g=10.0, m=1.0, l=1.0, dt=0.05, max_steps=200, n_actions=3)
        _update(d, kw)
        p = {k: T(d[k]) for k in ("max_speed", "max_torque", "g", "m", "l", "dt")}
        p["n_actions"] = int(d["n_actions"])
        continuous = True if continuous is None else bool(continuous)  # :50 continuous = true
    elif kind == "mountaincar":  # MountainCarEnv.jl:19-40, :73-77
        continuous = bool(continuous)
        d = dict(min_pos=-1.2, max_pos=0.6, max_speed=0.07, goal_pos=0.5, goal_velocity=0.0, power=0.001, gravity=0.0025,
                 max_steps=200)
        if continuous:
            d.update(goal_pos=0.45, power=0.0015)  # :74
        _update(d, kw)
        p = {k: T(d[k]) for k in ("min_pos", "max_pos", "max_speed", "goal_pos", "goal_velocity", "power", "gravity")}
    elif kind == "acrobot":  # AcrobotEnv.jl:21-55
        d = dict(link_length_a=1.0, link_length_b=1.0, link_mass_a=1.0, link_mass_b=1.0, link_com_pos_a=0.5,
                 link_com_pos_b=0.5, link_moi=1.0, max_torque_noise=0.0, max_vel_a=4 * PI, max_vel_b=9 * PI, g=9.8,
                 dt=0.2, max_steps=200, nips=0)
        _update(d, kw)
        p = {k: T(v) for k, v in d.items() if k not in ("max_steps", "nips")}
        p["nips"] = int(d["nips"])  # book_or_nips = "book" :37
        continuous = False
    else:
        raise KeyError(kind)
    p["max_steps"] = int(d["max_steps"])
    p["continuous"] = continuous
    p["T"] = T
    return p


def _update(d, kw):
    for k, v in kw.items():
        if k not in d:
            raise TypeError(f"unknown keyword argument {k}")
        d[k] = v


# ------------------------------------------------------------------------------------------------------- CartPole
def cartpole_step(p, s, t, a, fault=None):
    T = p["T"]
    x, xdot, theta, thetadot = (np.asarray(s[k], T) for k in range(4))
    if p["continuous"]:
        a = np.asarray(a, T)  # :106-110
    else:
        a = np.where(np.asarray(a) + 1 == 2, 1, -1).astype(T)  # :115  a == 2 ? 1 : -1; Int * T -> T below
    t = np.asarray(t, np.int64) + 1  # :119
    force = a * p["forcemag"]  # :120
    costheta = cos(theta)  # :122
    sintheta = sin(theta)  # :123
    tmp = (force + p["polemasslength"] * (thetadot * thetadot) * sintheta) / p["totalmass"]  # :124
    # :125-129  `4 / 3` is Float64: the bracket, the denominator and thetaacc are Float64; the numerator is T
    num = p["gravity"] * sintheta - costheta * tmp
    bracket = F64(4) / F64(3) - _f64(p["masspole"] * (costheta * costheta) / p["totalmass"])
    thetaacc = _f64(num) / (_f64(p["halflength"]) * bracket)
    # :130  T * Float64 * T / T -> Float64, left to right
    xacc = _f64(tmp) - _f64(p["polemasslength"]) * thetaacc * _f64(costheta) / _f64(p["totalmass"])
    nx = x + p["dt"] * xdot  # :131
    nxdot = (_f64(xdot) + _f64(p["dt"]) * xacc).astype(T)  # :132  Float64 sum stored into Vector{T}
    ntheta = theta + p["dt"] * thetadot  # :133
    nthetadot = (_f64(thetadot) + _f64(p["dt"]) * thetaacc).astype(T)  # :134
    beyond = (np.abs(nx) >= p["xthreshold"]) if fault == "x_ge" else (np.abs(nx) > p["xthreshold"])
    done = beyond | (np.abs(ntheta) > p["thetathreshold"]) | (t > p["max_steps"])  # :135-138
    reward = np.where(done, T(0), T(1)).astype(T)  # :84
    return np.stack([nx, nxdot, ntheta, nthetadot]), t, reward, done


# ------------------------------------------------------------------------------------------------------- Pendulum
def jl_mod(x, y):
    """Base.mod(x::Float64, y::Float64): r = rem(x, y) (exact, = fmod); r == 0 -> copysign(r, y); signs differ -> r + y"""
    r = np.fmod(_f64(x), F64(y))
    return np.where(r == 0, np.copysign(r, y), np.where((r > 0) != (y > 0), r + y, r))


def pendulum_torque(p, a):
    """torque :120-122, then `env.action = ...` (a ::T field) rounds"""
    T = p["T"]
    if p["continuous"]:
        return np.asarray(a, T)
    n1 = p["n_actions"] - 1
    a1 = _f64(np.asarray(a) + 1)
    return ((F64(4) / F64(n1)) * (a1 - F64(n1) / F64(2) - F64(1))).astype(T)


def pendulum_step(p, s, t, a, fault=None):
    T = p["T"]
    th, thdot = np.asarray(s[0], T), np.asarray(s[1], T)
    a = pendulum_torque(p, a)
    t = np.asarray(t, np.int64) + 1  # :101
    a = _clamp(a, -p["max_torque"], p["max_torque"])  # :103
    # :104 with angle_normalize :71: x + pi stays T, 2 * pi is Float64, so mod and everything after it is Float64
    thpi = th + T(PI)
    an = jl_mod(_f64(thpi), F64(2) * F64(PI)) - F64(PI)
    costs = an * an + F64(0.1) * _f64(thdot * thdot) + F64(0.001) * _f64(a * a)
    # :105-110  all T; sin(th + pi) as written
    newthdot = thdot + (T(-3) * p["g"] / (T(2) * p["l"]) * sin(thpi) + T(3) * a / (p["m"] * (p["l"] * p["l"]))) * p["dt"]
    nth = th + newthdot * p["dt"]  # :111  before the clamp
    newthdot = _clamp(newthdot, -p["max_speed"], p["max_speed"])  # :112
    done = t >= p["max_steps"]  # :115
    reward = (-costs).astype(T)  # :116  env.reward::T
    return np.stack([nth, newthdot]), t, reward, done


# ---------------------------------------------------------------------------------------------------- MountainCar
def mountaincar_step(p, s, t, a, fault=None):
    T = p["T"]
    x, v = np.asarray(s[0], T), np.asarray(s[1], T)
    force = np.asarray(a, T) if p["continuous"] else (np.asarray(a) + 1 - 2).astype(T)  # :110 / :116  a - 2
    t = np.asarray(t, np.int64) + 1  # :120
    v = v + (force * p["power"] + cos(T(3) * x) * (-p["gravity"]))  # :122
    v = _clamp(v, -p["max_speed"], p["max_speed"])  # :123
    x = x + v  # :124
    x = _clamp(x, p["min_pos"], p["max_pos"])  # :125
    at_wall = (x <= np.nextafter(p["min_pos"], T(np.inf))) if fault == "wall_ulp" else (x == p["min_pos"])
    v = np.where(at_wall & (v < 0), T(0), v).astype(T)  # :126-128
    done = ((x >= p["goal_pos"]) & (v >= p["goal_velocity"])) | (t >= p["max_steps"])  # :129-131
    reward = np.where(done, T(0), T(-1)).astype(T)  # :95
    return np.stack([x, v]), t, reward, done


# -------------------------------------------------------------------------------------------------------- Acrobot
def acrobot_dsdt(p, s, a):
    """dsdt :134-187 on Float64 arrays; the params are read back from their T fields (:136-143)"""
    m1, m2, l1 = F64(p["link_mass_a"]), F64(p["link_mass_b"]), F64(p["link_length_a"])
    lc1, lc2 = F64(p["link_com_pos_a"]), F64(p["link_com_pos_b"])
    I1 = I2 = F64(p["link_moi"])
    g = F64(p["g"])
    theta1, theta2, dtheta1, dtheta2 = s
    c2, s2 = cos(theta2), sin(theta2)
    d1 = m1 * (lc1 * lc1) + m2 * ((l1 * l1) + (lc2 * lc2) + 2 * l1 * lc2 * c2) + I1 + I2  # :158
    d2 = m2 * ((lc2 * lc2) + l1 * lc2 * c2) + I2  # :159
    phi2 = m2 * lc2 * g * cos(theta1 + theta2 - F64(PI) / 2.0)  # :160
    phi1 = (-m2 * l1 * lc2 * (dtheta2 * dtheta2) * s2 - 2 * m2 * l1 * lc2 * dtheta2 * dtheta1 * s2
            + (m1 * lc1 + m2 * l1) * g * cos(theta1 - F64(PI) / 2) + phi2)  # :161-166
    if p["nips"]:
        ddtheta2 = (a + d2 / d1 * phi1 - phi2) / (m2 * (lc2 * lc2) + I2 - (d2 * d2) / d1)  # :170
        ddtheta1 = np.zeros_like(ddtheta2)  # :154
    else:
        ddtheta2 = (a + d2 / d1 * phi1 - m2 * l1 * lc2 * (dtheta1 * dtheta1) * s2 - phi2) / (m2 * (lc2 * lc2) + I2 - (d2 * d2) / d1)  # :174-177
        ddtheta1 = -(d2 * ddtheta2 + phi1) / d1  # :178
    return np.stack([dtheta1, dtheta2, ddtheta1, ddtheta2])  # :182-185 (du[5] = 0: the torque is constant)


def _wrap(x, m, M):  # :192-212
    x = x.copy()
    diff = M - m
    while (x > M).any():
        x = np.where(x > M, x - diff, x)
    while (x < m).any():
        x = np.where(x < m, x + diff, x)
    return x


def acrobot_step(p, s, t, a, noise_u=None, fault=None):
    T = p["T"]
    s = np.stack([np.asarray(s[k], T) for k in range(4)])
    t = np.asarray(t, np.int64) + 1  # :103
    torque = (np.asarray(a) + 1 - 2).astype(T)  # :104  avail_torque = [-1, 0, 1]
    if p["max_torque_noise"] > 0:  # :107-110   torque += T(2.0 * noise_range) * rand(T) .- T(noise_range)
        nr = p["max_torque_noise"]
        torque = torque + T(F64(2.0) * F64(nr)) * np.asarray(noise_u, T) - nr
    y = _f64(s)
    a64 = _f64(torque)
    h = F64(p["dt"])
    k1 = acrobot_dsdt(p, y, a64)
    k2 = acrobot_dsdt(p, y + h / 2 * k1, a64)
    k3 = acrobot_dsdt(p, y + h / 2 * k2, a64)
    k4 = acrobot_dsdt(p, y + h * k3, a64)
    ns = y + h / 6 * (k1 + 2 * k2 + 2 * k3 + k4)
    ns[0] = _wrap(ns[0], -F64(PI), F64(PI))  # :122-123
    ns[1] = _wrap(ns[1], -F64(PI), F64(PI))
    va, vb = F64(p["max_vel_a"]), F64(p["max_vel_b"])
    ns[2] = np.minimum(np.maximum(ns[2], -va), va)  # :124-125  bound = min(max(x, m), M)
    ns[3] = np.minimum(np.maximum(ns[3], -vb), vb)
    ns = ns.astype(T)  # :126  the state as stored
    succeeded = (-cos(_f64(ns[0])) - cos(_f64(ns[1]) + _f64(ns[0]))) > 1.0  # :128
    done = succeeded | (t > p["max_steps"])  # :129
    reward = np.where(succeeded, T(0), T(-1)).astype(T)  # :130
    return ns, t, reward, done


# --------------------------------------------------------------------------------------------------- common surface
def step(kind, p, s, t, a, noise_u=None, fault=None):
    if kind == "cartpole":
        return cartpole_step(p, s, t, a, fault=fault)
    if kind == "pendulum":
        return pendulum_step(p, s, t, a, fault=fault)
    if kind == "mountaincar":
        return mountaincar_step(p, s, t, a, fault=fault)
    return acrobot_step(p, s, t, a, noise_u=noise_u, fault=fault)


def observation(kind, s):
    """state(env): CartPoleEnv.jl:86, PendulumEnv.jl:70, MountainCarEnv.jl:97, AcrobotEnv.jl:72"""
    s = np.asarray(s)
    if kind in ("cartpole", "mountaincar"):
        return s.copy()
    if kind == "pendulum":
        return np.stack([sin(s[0]), cos(s[0]), s[1]])
    return np.stack([cos(s[0]), sin(s[0]), cos(s[1]), sin(s[1]), s[2], s[3]])
