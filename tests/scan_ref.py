"""An independent numpy model of the reverse-time scans (TEST INFRASTRUCTURE ONLY; a helper, not a test module).

Written from the reference's Julia text, line by line: no statement here is taken from oracle/rlo_scans.c or csrc/scans.hip.

    RLCore = src/ReinforcementLearningCore/src
    discount_rewards[!]                    RLCore/utils/basic.jl:138-235   the step :227-235
    discount_rewards_reduced[!]            RLCore/utils/basic.jl:237-319   the step :256-263
    generalized_advantage_estimation[!]    RLCore/utils/basic.jl:334-417   the step :408-417
  and, for the two small DQN helpers, the published definitions
    Flux.Losses.huber_loss    abs_error = abs.(yhat .- y); mean of 0.5 abs_error^2 where abs_error < delta,
                              delta (abs_error - 0.5 delta) elsewhere; its pullback d / mean's 1 / n
    the DQN target            target = r .+ gamma .* (1 .- t) .* q'   with q' = maximum over the actions

What the text says, operation by operation (Julia's `*` and `+` associate to the left, Bool is a number):
    :230 / :259 / :411   is_continue = isnothing(terminal) ? true : !terminal[i]
    :231 / :260          gain = rewards[i] + ((gamma * gain) * is_continue)
    :412                 delta = (rewards[i] + ((gamma * values[i + 1]) * is_continue)) - values[i]
    :413                 gae = delta + (((gamma * lambda) * is_continue) * gae)
    :225 / :254          init = nothing is zero(eltype);  :409 gae starts at 0
    :155 ...             the matrix drivers scan ALONG the user's `dims` (dims = 1 down each column, dims = 2 along each row;
                         values has one element more along that axis), init[i] is slice i's
  `x * false` is copysign(0, x) for every x, Inf and NaN included (Base: `*(x::AbstractFloat, y::Bool)`): a STRONG zero.  In
  :413 the Bool multiplies gamma * lambda, not gae: a terminal step in front of an infinite gae is 0 * Inf = NaN in the
  reference too.

`replay` evaluates exactly that in the array's own type (np.float32 / np.float64 arrays: one rounding per operation, no
contraction).  gamma, lambda and init are converted to that type FIRST: the C ABI takes them as T (`float gamma` /
`double gamma`), where Julia would promote a Float64 gamma over Float32 rewards to a Float64 result -- the project's scans are
the T-typed methods.  It is vectorised over the slices with a Python loop over time, and it is the bit-for-bit judge of the
oracle and of the kernels.

The bit pattern of a NaN that an invalid operation CREATES (0 * Inf, Inf - Inf) is the platform's: IEEE 754 leaves its sign
and payload open.  x86 SSE and gfx950 both create the negative quiet NaN with an empty payload (0xFFC00000,
0xFFF8000000000000) and both hand an input NaN on unchanged, so numpy on the host is the judge of the kernels down to the
NaN bits; the case grids carry only np.nan, the positive quiet NaN, as input.

`exact` judges the model: the same recurrences in Float64 for Float32 inputs, with a running first-order bound of what a
Float32 evaluation with one rounding per operation (unit roundoff u = 2^-24) may be off by, carried beside the value:
    RN(a op b) = (a op b)(1 + d), |d| <= u, plus 2^-149 absolute for a product that may underflow
    gg = RN(gamma g)          E_gg = |gamma| E_g + u (|gamma g| + |gamma| E_g)
    gain = RN(r + gg c)       E    = c E_gg + u (|gain| + c E_gg)                         (c = 0 cuts value AND error)
    gv = RN(gamma V')         E_1  = u |gv|
    s = RN(r + gv c)          E_2  = c E_1 + u (|s| + c E_1)
    delta = RN(s - V)         E_3  = E_2 + u (|delta| + E_2)
    gl = RN(gamma lambda)     E_gl = u |gl|
    p = RN((gl c) gae)        E_p  = c (|gl| E + E_gl (|gae| + E)) + u (|p| + that)
    gae = RN(delta + p)       E'   = E_3 + E_p + u (|gae| + E_3 + E_p)
    ret = RN(gae + V)         E_r  = E' + u (|ret| + E')
  every magnitude is the Float64 value's plus its own bound, and the total is scaled by SLACK = 1 + 2^-10 for what is still
  second order.  No tolerance is chosen: replay must lie inside the bound on every finite cell.

`fault=` plants ONE misreading of the text on purpose (tests/test_scan_reference.py shows that each is caught on every route it
applies to; FAULT_APPLIES says which outputs a fault can touch at all):
    "weak_zero"               x * false as x * 0.0 (NaN for Inf / NaN)
    "unsigned_zero"           x * false as +0.0 whatever the sign of x
    "boot_not_cut"            :412 without `* is_continue`
    "lambda_not_cut"          :413 without `* is_continue`
    "term_next"               terminal[i + 1] read for step i (no flag past the end)
    "term_prev"               terminal[i - 1]
    "last_value_zero"         values[T + 1] ignored
    "returns_next_value"      returns = gae + values[i + 1]
    "reassociated"            :412 as (rewards[i] - values[i]) + boot
    "contracted"              the product and the add of :231 / :412 / :413 as one fused multiply-add
    "init_ignored"            gain starts at zero although init is given
    "init_scalar_for_slices"  every slice starts from init[1]
    "reduced_last"            the reduced form returns the LAST element of the full scan instead of the first
    "chunk_carry_lost:CH"     gae is reset to zero every CH steps (a register-staged chunk that forgets its carry)
    "lane_flag_swapped"       slice e reads the terminal flag of slice e xor 1
"""
from types import SimpleNamespace

import numpy as np

F32, F64 = np.float32, np.float64
U = 2.0 ** -24  # unit roundoff of Float32
SLACK = 1.0 + 2.0 ** -10  # second-order terms of the first-order bounds
TINY = 2.0 ** -149  # a Float32 product that underflows is off by at most this
FAULTS = ("weak_zero", "unsigned_zero", "boot_not_cut", "lambda_not_cut", "term_next", "term_prev", "last_value_zero",
          "returns_next_value", "reassociated", "contracted", "init_ignored", "init_scalar_for_slices", "reduced_last",
          "chunk_carry_lost:8", "chunk_carry_lost:16", "chunk_carry_lost:32", "lane_flag_swapped")
# the outputs a fault can change: "scan" / "reduced" (discount_rewards[_reduced]), "gae", "returns"; and what the call must
# carry for the fault to mean anything ("terminal", "init", "init_per_slice")
FAULT_APPLIES = {
    "weak_zero": ({"scan", "reduced", "gae", "returns"}, {"terminal"}),
    "unsigned_zero": ({"scan", "reduced", "gae"}, {"terminal"}),  # returns = -0.0 + V: the sign of the zero is absorbed
    "boot_not_cut": ({"gae", "returns"}, {"terminal"}),
    "lambda_not_cut": ({"gae", "returns"}, {"terminal"}),
    "term_next": ({"scan", "reduced", "gae", "returns"}, {"terminal"}),
    "term_prev": ({"scan", "reduced", "gae", "returns"}, {"terminal"}),
    "last_value_zero": ({"gae", "returns"}, set()),
    "returns_next_value": ({"returns"}, set()),
    "reassociated": ({"gae", "returns"}, set()),
    "contracted": ({"scan", "reduced", "gae", "returns"}, set()),
    "init_ignored": ({"scan", "reduced"}, {"init"}),
    "init_scalar_for_slices": ({"scan", "reduced"}, {"init_per_slice"}),
    "reduced_last": ({"reduced"}, set()),
    "chunk_carry_lost:8": ({"gae", "returns"}, set()),
    "chunk_carry_lost:16": ({"gae", "returns"}, set()),
    "chunk_carry_lost:32": ({"gae", "returns"}, set()),
    "lane_flag_swapped": ({"scan", "reduced", "gae", "returns"}, {"terminal"}),
}
assert set(FAULT_APPLIES) == set(FAULTS)


def _quiet():
    return np.errstate(all="ignore")


def _time_major(a, dims, dtype=None):
    """the mathematical array of a call -> (len, n_slices) C-contiguous, time first"""
    a = np.asarray(a) if dtype is None else np.asarray(a, dtype=dtype)
    if a.ndim == 1:
        if dims != 0:
            raise TypeError("a vector takes dims = 0")
        return np.ascontiguousarray(a[:, None])
    if dims == 1:
        return np.ascontiguousarray(a)
    if dims == 2:
        return np.ascontiguousarray(a.T)
    raise TypeError("MethodError: a matrix requires dims = 1 or 2")


def _math(tm, dims):
    if dims == 0:
        return tm[:, 0]
    return tm if dims == 1 else tm.T


def _times_bool(x, keep, fault):
    """x * keep for a Bool `keep`: copysign(0, x) where it is false"""
    if fault == "weak_zero":
        return x * keep.astype(x.dtype)
    if fault == "unsigned_zero":
        return np.where(keep, x, x.dtype.type(0))
    return np.where(keep, x, np.copysign(x.dtype.type(0), x))


def _fma(a, b, c):
    """a * b + c with ONE rounding (the planted contraction): Float32 through the exact Float64 product, Float64 through
    the extended type -- wide enough to differ from the twice-rounded value wherever a contraction would"""
    wide = F64 if c.dtype == F32 else np.longdouble
    return (np.asarray(a, wide) * np.asarray(b, wide) + np.asarray(c, wide)).astype(c.dtype)


def _flags(term, T, n, fault):
    """is_continue for every step, (T, n) bool, under the planted misreadings of the flag's address"""
    if term is None:
        return np.ones((T, n), bool)
    t = np.asarray(term) != 0
    if fault == "lane_flag_swapped":
        e = np.arange(n) ^ 1
        e = np.where(e < n, e, np.arange(n))
        t = t[:, e]
    if fault == "term_next":
        t = np.concatenate([t[1:], np.zeros((1, n), bool)], 0)
    if fault == "term_prev":
        t = np.concatenate([np.zeros((1, n), bool), t[:-1]], 0)
    return ~t


def replay(rewards, gamma, lam=None, values=None, terminal=None, init=None, dims=0, dtype=None, fault=None):
    """The four scans on one call's arguments, which are MATHEMATICAL arrays like the reference's: rewards and terminal
    (n1,) or (n1, n2), values one longer along `dims`, init None, a scalar (a vector's) or one per slice.
    -> namespace: scan, reduced (discount_rewards, discount_rewards_reduced); gae, returns (None without `values`)."""
    assert fault is None or fault in FAULTS, fault
    r = _time_major(rewards, dims, dtype)
    T_ = r.dtype.type
    assert T_ in (F32, F64), T_
    T, n = r.shape
    g = T_(gamma)
    cont = _flags(None if terminal is None else _time_major(terminal, dims), T, n, fault)
    out = SimpleNamespace(scan=None, reduced=None, gae=None, returns=None)
    with _quiet():
        # ------------------------------------------------------------------ :227-235, :256-263
        if init is None or fault == "init_ignored":
            gain = np.zeros(n, T_)  # :225, :254
        else:
            ini = np.atleast_1d(np.asarray(init, dtype=T_))
            assert ini.shape in ((1,), (n,)), "init: a scalar or one per slice"
            gain = np.full(n, ini[0], T_) if (ini.size == 1 or fault == "init_scalar_for_slices") else ini.copy()
        scan = np.empty((T, n), T_)
        for i in range(T - 1, -1, -1):
            c = cont[i]
            if fault == "contracted":
                gain = np.where(c, _fma(g, gain, r[i]), r[i] + _times_bool(g * gain, c, None))
            else:
                gain = r[i] + _times_bool(g * gain, c, fault)  # :231
            scan[i] = gain  # :232
        reduced = scan[T - 1].copy() if (fault == "reduced_last" and T > 0) else gain.copy()  # :262
        out.scan, out.reduced = _math(scan, dims), reduced
        # ------------------------------------------------------------------ :408-417
        if values is not None:
            v = _time_major(values, dims, T_)
            assert v.shape == (T + 1, n), "values: one element more along the scanned axis"
            l_ = T_(lam)
            gl = np.full(n, g * l_, T_)  # gamma * lambda, one rounding
            ch = int(fault.split(":")[1]) if fault and fault.startswith("chunk_carry_lost") else 0
            gae = np.zeros(n, T_)  # :409
            adv, ret = np.empty((T, n), T_), np.empty((T, n), T_)
            for i in range(T - 1, -1, -1):
                c = cont[i]
                if ch and i != T - 1 and (T - 1 - i) % ch == 0:
                    gae = np.zeros(n, T_)
                vn = np.zeros(n, T_) if (fault == "last_value_zero" and i == T - 1) else v[i + 1]
                gv = g * vn
                boot = gv if fault == "boot_not_cut" else _times_bool(gv, c, fault)
                if fault == "reassociated":
                    delta = (r[i] - v[i]) + boot
                elif fault == "contracted":
                    delta = np.where(c, _fma(g, vn, r[i]), r[i] + boot) - v[i]
                else:
                    delta = (r[i] + boot) - v[i]  # :412
                glc = gl if fault == "lambda_not_cut" else _times_bool(gl, c, fault)
                gae = _fma(glc, gae, delta) if fault == "contracted" else delta + glc * gae  # :413
                adv[i] = gae  # :414
                ret[i] = gae + (v[i + 1] if fault == "returns_next_value" else v[i])
            out.gae, out.returns = _math(adv, dims), _math(ret, dims)
    return out


def exact(rewards, gamma, lam=None, values=None, terminal=None, init=None, dims=0):
    """The same recurrences in Float64 for Float32 arguments, with the bound of the module docstring beside each value.
    -> namespace: scan, reduced, gae, returns and scan_bound, reduced_bound, gae_bound, returns_bound (Float64, the shapes
    of replay's).  A non-finite value carries a non-finite or NaN bound: the caller judges the finite cells."""
    r32 = _time_major(rewards, dims, F32)
    r = r32.astype(F64)
    T, n = r.shape
    g = F64(F32(gamma))
    cont = _flags(None if terminal is None else _time_major(terminal, dims), T, n, None)
    out = SimpleNamespace(gae=None, returns=None, gae_bound=None, returns_bound=None)
    with _quiet():
        gain = np.zeros(n) if init is None else np.broadcast_to(np.atleast_1d(np.asarray(init, F32)).astype(F64), (n,)).copy()
        E = np.zeros(n)
        scan, scan_b = np.empty((T, n)), np.empty((T, n))
        for i in range(T - 1, -1, -1):
            c = cont[i]
            gg = g * gain
            Egg = abs(g) * E + U * (np.abs(gg) + abs(g) * E) + TINY
            Ec = np.where(c, Egg, 0.0)
            gain = r[i] + np.where(c, gg, 0.0)
            E = Ec + U * (np.abs(gain) + Ec)
            scan[i], scan_b[i] = gain, E
        out.scan, out.scan_bound = _math(scan, dims), _math(scan_b, dims) * SLACK
        out.reduced, out.reduced_bound = gain.copy(), E * SLACK
        if values is not None:
            v = _time_major(values, dims, F32).astype(F64)
            gl = g * F64(F32(lam))
            Egl = U * abs(gl) + TINY
            gae, E = np.zeros(n), np.zeros(n)
            adv, adv_b, ret, ret_b = (np.empty((T, n)) for _ in range(4))
            for i in range(T - 1, -1, -1):
                c = cont[i]
                gv = g * v[i + 1]
                E1 = np.where(c, U * np.abs(gv) + TINY, 0.0)
                s = r[i] + np.where(c, gv, 0.0)
                E2 = E1 + U * (np.abs(s) + E1)
                delta = s - v[i]
                E3 = E2 + U * (np.abs(delta) + E2)
                p = np.where(c, gl * gae, 0.0)
                Ein = np.where(c, abs(gl) * E + Egl * (np.abs(gae) + E), 0.0)
                Ep = Ein + np.where(c, U * (np.abs(p) + Ein) + TINY, 0.0)
                gae = delta + p
                E = E3 + Ep + U * (np.abs(gae) + E3 + Ep)
                adv[i], adv_b[i] = gae, E
                ret[i] = gae + v[i]
                ret_b[i] = E + U * (np.abs(ret[i]) + E)
            out.gae, out.gae_bound = _math(adv, dims), _math(adv_b, dims) * SLACK
            out.returns, out.returns_bound = _math(ret, dims), _math(ret_b, dims) * SLACK
    return out


# ------------------------------------------------------------------------------------------------- the two DQN helpers
def huber(q, target, delta):
    """Flux.Losses.huber_loss(q, target; delta) and its pullback, per sample in Float32 as written:
    -> (l (n,) Float32 per-sample losses, dq (n,) Float32 = dl / dq / n, loss = Float32(sum of l in Float64 / n))"""
    q, t = np.asarray(q, F32).reshape(-1), np.asarray(target, F32).reshape(-1)
    d_ = F32(delta)
    n = q.size
    with _quiet():
        d = q - t
        e = np.abs(d)
        small = e < d_
        l = np.where(small, (e * e) * F32(0.5), d_ * (e - F32(0.5) * d_))
        gi = np.where(small, d, np.where(d > 0, d_, np.where(d < 0, -d_, F32(0))))
        dq = (gi / F32(n)).astype(F32)
    return l.astype(F32), dq, F32(l.astype(F64).sum() / n)


def td_target(q, reward, terminal, gamma):
    """target = r .+ gamma .* (1 .- t) .* maximum(q, dims = 1) in Float32, q (na, n); the broadcast multiplies left to
    right: (gamma * (1 - t)) * q', so an infinite q' on a terminal sample is 0 * Inf = NaN here too.  NaN Q-values are out
    of the model's domain (Base.maximum propagates a NaN from any position; see profiles/scan_routes.md)."""
    q = np.asarray(q, F32)
    assert not np.isnan(q).any(), "NaN Q-values: outside the pinned domain"
    with _quiet():
        qmax = q.max(0)
        cont = F32(1) - (np.asarray(terminal) != 0).astype(F32)
        return (np.asarray(reward, F32) + (F32(gamma) * cont) * qmax).astype(F32)
