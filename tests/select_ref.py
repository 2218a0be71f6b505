"""An independent numpy model of action selection (TEST INFRASTRUCTURE ONLY; a helper, not a test module).

Written from the reference's Julia text, rule by rule: no statement here is taken from oracle/rlo_select.c or csrc/select*,
and where they and the text differed (a masked NaN logit, networks.jl:468) the text decided.

    RLCore = src/ReinforcementLearningCore/src
    EpsilonGreedyExplorer    RLCore/policies/explorers/epsilon_greedy_explorer.jl   plan! :102-131   prob :141-194
    WeightedExplorer         RLCore/policies/explorers/weighted_explorer.jl         plan! :25-34     prob :36-45
    WeightedSoftmaxExplorer  RLCore/policies/explorers/weighted_softmax_explorer.jl plan! :20-26     prob :28-34
    GumbelSoftmaxExplorer    RLCore/policies/explorers/gumbel_softmax_explorer.jl   plan! :12-24
    UCBExplorer              RLCore/policies/explorers/UCB_explorer.jl              plan! :24-30
    find_all_max             RLCore/utils/basic.jl:91-114       findmax_masked  :117-118
    sample_categorical       RLCore/utils/networks.jl:425-432   mask: `logits .+= ifelse.(mask, 0f0, typemin)` :468
  and the published algorithms of the un-vendored packages
    Base.findmax / argmax     first maximal index, "NaN is treated as greater than all other values"
    Base.maximum              propagates NaN
    StatsBase.sample(rng, wv) t = rand(rng) * sum(wv); i = 1; cw = wv[1]; while cw < t && i < n: i += 1; cw += wv[i]
    NNlib.softmax             exp.(x .- max) ./ sum(exp.(x .- max))
    NNlib.logsoftmax          x .- max .- log(sum(exp.(x .- max)))

What it is for: tests/test_select_reference.py (oracle) and tests/test_gpu_select_edges.py (kernels) run the case grids of
tests/select_cases.py through this model and through the code under test.  Two restatements made by different routes agree
only where both read the source the same way.

Conventions
  * one COLUMN per env instance: `values` is a (na, n) array, every rule is vectorised over the n columns.  Actions are
    0-based like the C ABI (Julia's index minus one).
  * all arithmetic is Float64, whatever the reference's element type: the Float32 evaluation of the project is judged against
    the exact value through a derived budget (below), not imitated.  Only `logits .+= ifelse(mask, 0f0, typemin)` is done in
    Float32 as written: it is exact for every finite logit and decides what a masked NaN or +Inf becomes (NaN).
  * NO RNG.  Random numbers are ARGUMENTS: Float64 uniforms `u`, Float32 uniforms `u32` and raw 32-bit words for the index
    draws (`rand_w`, `tie_w`): `rand(rng, inds)` needs length(inds), which only the rule knows, so the rule turns the word
    into an index by the documented `(w * n) >> 32`.  `draws(...)` maps Philox words to those arguments from the layout
    that include/rlhip.h documents, through oracle.philox (pinned by the Random123 vectors of
    tests/test_oracle_golden.py::test_philox_kat).
  * UNDEFINED (-1): the reference THROWS there -- rand(rng, Int[]) after find_all_max met a NaN maximum (`count(==(NaN), x)`
    is 0), maximum / findall over an all-false mask.  The project pins index 0 for those columns (include/rlhip.h); the
    tests check that pin where the model says UNDEFINED.

Every rule returns a namespace with
    decision   (n,) int64 actions
    q          the Float64 quantities behind it (log-probabilities, cumulative weights, UCB scores, ...)
    margin     (n,) the rule's distance from a different decision: the gap between the winner's and the runner-up's score of
               an argmax; the distance of t from the cumulative boundary that is nearest in units of its budget for the
               weighted walk; |u - eps| for eps-greedy.  +inf where no arithmetic decides (a NaN rule, na = 1).
    budget     (n,) what a correct Float32 evaluation may be off by at that margin; a column is JUDGED iff margin > budget, or
               the budget is 0 (exact arithmetic: every column, eps-greedy at u == eps included).

The Float32 budget (u = 2^-24, the unit roundoff; every bound first order, the total scaled by 1 + 2^-10 for the
second-order terms, which are below 2^-13 of it for na <= 2^10).  The documented evaluation order of the project is
    d_k  = RN(x_k - mx)                       |err| <= u |d_k|
    e_k  = RN(exp(d_k))    rounded once       relative error <= u (from the rounding) + u |d_k| (from d_k's error)
    se   = e_1 + ... + e_na, running sum      relative error <= (na - 1) u + sum_k (1 + |d_k|) u e_k / se     =: r_se
    lse  = RN(log(se))     rounded once       |err| <= r_se + u |lse|
    lp_k = RN(d_k - lse)                      |err| <= u |d_k| + r_se + u |lse| + u |lp_k|                     =: B_k
  categorical (Float64 Gumbel noise gn_k = -log(-log(u_k)), libm within 1 ulp twice): g_k = gn_k + lp_k is off by at most
    B_k + 2^-51 (1 + |gn_k|); the decision can differ only if the gap between the two largest g is at most
    B_winner + max_k B_k.  The returned logp is judged against B_winner.
  gumbel_softmax (all Float32): inner = RN(log(u)), gum = RN(log(-inner)), g = RN(lp - gum).  inner's relative error u becomes
    an absolute error u of gum, plus u |gum| for gum's own rounding and u |g| for the subtraction: B_k + u (1 + |gum_k| + |g_k|).
  weighted walk: cw_j = w_0 + ... + w_j as a running Float32 sum of non-negative terms is off by at most j u C_j; the total
    S (any summation order) by (na - 1) u S, which moves t = u01 * S at the boundary t = C_j by (na - 1) u C_j:
    B_j = (j + na - 1) u max(C_j, t)  (is_normalized: S = 1 exactly, B_j = j u max(C_j, t)).
  weighted_softmax walk: w_k = RN(e_k / se) has relative error rho_k = (1 + |d_k|) u + r_se + u, S = one(T):
    B_j = j u C_j + sum_{k <= j} rho_k p_k.
  eps-greedy, prob and the walk over dyadic weights are EXACT: budget 0.  UCB is Float64 on both sides: two scores are tied
  by construction (equal value, equal count: the same operations on the same operands) or must be separated by more than
  1e-9.  The largest bonus is c sqrt(log(2^32) / 1e-10) < 9.4e5 at c = 2; log within 1 ulp (halved by the square root), the
  square root, the product and the sum each within 2^-53 relative put a score within 4.5e-16 * 9.4e5 = 4.2e-10 of the exact
  one, so two evaluations (libm here, ocml on the device) differ by less than 1e-9 and never order separated scores differently.

NOT PINNED to the reference (listed like AcrobotRK4Env in tests/env_ref.py): a +Inf logit.  The reference delegates to
NNlib.logsoftmax / softmax, which may special-case Inf; this model, the oracle and the kernels use the plain formula, in which
Inf - Inf = NaN poisons the column: every log-probability is NaN and the first index (action 0) is returned.

`fault=` plants ONE misreading of the reference on purpose (tests/test_select_reference.py shows that each is caught):
    "last_max"             findmax / argmax: the last maximal index instead of the first
    "nan_not_max"          findmax: NaN is not maximal
    "nan_tie"              find_all_max: NaN == NaN counts as a tie
    "u_gt_eps"             `u > eps` instead of `u >= eps`
    "rand_all_under_mask"  the random action drawn from 1:n although a mask is given
    "mask_after_softmax"   categorical: the mask zeroes probabilities after the softmax instead of typemin before it
    "walk_le"              `cw <= t` in the walk
    "masked_weight_kept"   WeightedExplorer: values[.!mask] .= 0 forgotten
    "ignore_is_normalized" WeightedExplorer{true}: the sum computed anyway
    "index_mod"            index = w % n instead of (w * n) >> 32
    "shared_uniform"       (draws) actions 2j and 2j + 1 read the same uniform
    "gumbel_add"           log(-log(u)) added to the log-probabilities where the reference subtracts it
    "ucb_log_step"         log(step) instead of log(step + 1)
    "ucb_no_increment"     actioncounts[action] += 1 forgotten
"""
from types import SimpleNamespace

import numpy as np

F64 = np.float64
UNDEFINED = -1
U = 2.0 ** -24  # unit roundoff of Float32
SLACK = 1.0 + 2.0 ** -10  # second-order terms of the first-order bounds
TAG_EXPLORE, TAG_GUMBEL = 1, 2
FAULTS = ("last_max", "nan_not_max", "nan_tie", "u_gt_eps", "rand_all_under_mask", "mask_after_softmax", "walk_le",
          "masked_weight_kept", "ignore_is_normalized", "index_mod", "shared_uniform", "gumbel_add", "ucb_log_step",
          "ucb_no_increment")
LAW_FAULTS = ("shared_uniform", "gumbel_add", "index_mod")


def _f64(x):
    return np.asarray(x, dtype=F64)


def _quiet():
    return np.errstate(all="ignore")


# --------------------------------------------------------------------------------------------------- Philox -> arguments
def u01_f64(hi, lo):
    """rand(Float64) stand-in: the top 53 bits of (hi << 32 | lo), times 2^-53"""
    return float(((int(hi) << 32 | int(lo)) >> 11) * 2.0 ** -53)


def u01_f32(w):
    """rand(Float32) stand-in: the top 24 bits of w, times 2^-24"""
    return np.float32((int(w) >> 8) * 2.0 ** -24)


def index(w, n, fault=None):
    """rand(rng, 1:n) stand-in, 0-based: (w * n) >> 32"""
    w, n = np.asarray(w, dtype=np.uint64), np.asarray(n, dtype=np.uint64)
    if fault == "index_mod":
        return (w % np.maximum(n, 1)).astype(np.int64)
    return ((w * n) >> np.uint64(32)).astype(np.int64)


def draws(entry, seed, env_id_base, n, step, na, fault=None):
    """The random arguments of one launch of `entry` over n envs, from the draw layouts of include/rlhip.h:
    Philox(seed, idx = (env_id_base + i) mod 2^32, blk, t = step mod 2^32, tag)
      eps_greedy                  blk 0, EXPLORE: (w0, w1) -> u, w2 -> random index, w3 -> tie-break index
      categorical                 blk k // 2, GUMBEL: action k even -> (w0, w1), odd -> (w2, w3)
      weighted, weighted_softmax  blk 0, EXPLORE: (w0, w1) -> u
      gumbel_softmax              blk 0x8000 + k // 4, GUMBEL: action k -> Float32 uniform of w[k % 4]
      ucb                         blk 0, EXPLORE: w0 -> tie-break index"""
    import oracle

    ids = [(env_id_base + i) & 0xFFFFFFFF for i in range(n)]
    t = step & 0xFFFFFFFF
    if entry in ("eps_greedy", "weighted", "weighted_softmax", "ucb"):
        w = np.array([oracle.philox(seed, i, 0, t, TAG_EXPLORE) for i in ids], dtype=np.uint64).reshape(n, 4)
        if entry == "ucb":
            return dict(tie_w=w[:, 0])
        u = np.array([u01_f64(a, b) for a, b in w[:, :2]], dtype=F64)
        if entry == "eps_greedy":
            return dict(u=u, rand_w=w[:, 2], tie_w=w[:, 3])
        return dict(u=u)
    if entry == "categorical":
        u = np.empty((na, n), F64)
        for c, i in enumerate(ids):
            for b in range((na + 1) // 2):
                w = oracle.philox(seed, i, b, t, TAG_GUMBEL)
                u[2 * b, c] = u01_f64(w[0], w[1])
                if 2 * b + 1 < na:
                    u[2 * b + 1, c] = u[2 * b, c] if fault == "shared_uniform" else u01_f64(w[2], w[3])
        return dict(u=u)
    if entry == "gumbel_softmax":
        u = np.empty((na, n), np.float32)
        for c, i in enumerate(ids):
            for b in range((na + 3) // 4):
                w = oracle.philox(seed, i, 0x8000 + b, t, TAG_GUMBEL)
                for j in range(min(4, na - 4 * b)):
                    u[4 * b + j, c] = u01_f32(w[j])
        return dict(u32=u)
    raise KeyError(entry)


# ------------------------------------------------------------------------------------------------------- building blocks
def findmax(x, fault=None):
    """Base.findmax(x)[2] per column: the first maximal index, NaN greater than everything"""
    x = _f64(x)
    nan = np.isnan(x)
    xm = np.where(nan, -np.inf, x)
    idx = (x.shape[0] - 1 - xm[::-1].argmax(0)) if fault == "last_max" else xm.argmax(0)
    if fault == "nan_not_max":
        return idx.astype(np.int64)
    first_nan = (x.shape[0] - 1 - nan[::-1].argmax(0)) if fault == "last_max" else nan.argmax(0)
    return np.where(nan.any(0), first_nan, idx).astype(np.int64)


def find_all_max(x, mask=None, fault=None):
    """basic.jl:91-114: v = maximum(x) (of view(x, mask) :112), the indices with x[i] == v (and mask[i] :113).  Returns
    (v, ties (na, n) bool, defined (n,)): maximum over an empty view throws."""
    x = _f64(x)
    legal = np.ones(x.shape, bool) if mask is None else np.asarray(mask) != 0
    defined = legal.any(0)
    with _quiet():
        v = np.where(legal, x, -np.inf).max(0)  # np.max propagates NaN like Base.maximum
    v = np.where((np.isnan(x) & legal).any(0), np.nan, v)
    ties = legal & (x == v[None, :])
    if fault == "nan_tie":
        ties |= legal & np.isnan(x) & np.isnan(v)[None, :]
    return v, ties, defined


def pick(member, w, fault=None):
    """rand(rng, inds) for inds = findall(member) per column, from the word w: UNDEFINED where inds is empty"""
    member = np.asarray(member, bool)
    c = member.sum(0)
    j = index(w, c, fault)
    hit = member & (np.cumsum(member, 0) == (j + 1)[None, :])
    return np.where(c > 0, hit.argmax(0), UNDEFINED).astype(np.int64)


def _argmax_margin(g, B):
    """winner (first maximal index, NaN maximal), the gap to the runner-up and the allowance B_winner + max B"""
    na, n = g.shape
    a = findmax(g)
    cols = np.arange(n)
    gw = g[a, cols]
    rest = np.where(np.arange(na)[:, None] == a[None, :], -np.inf, np.where(np.isnan(g), -np.inf, g))
    with _quiet():
        margin = gw - rest.max(0)
    margin = np.where(np.isnan(gw) | (na == 1), np.inf, margin)  # a NaN decides by rule, not by arithmetic
    Bf = np.where(np.isfinite(B), B, 0.0)
    return a, margin, Bf[a, cols] + Bf.max(0)


def logsoftmax(x):
    """NNlib.logsoftmax over dim 1 in Float64 with the Float32 budget B (na, n) of the module docstring"""
    x = _f64(x)
    na = x.shape[0]
    with _quiet():
        mx = x.max(0)
        d = x - mx
        e = np.exp(d)
        se = e.sum(0)
        lse = np.log(se)
        lp = d - lse
        ad = np.where(e > 0, np.abs(d), 0.0)
        r_se = U * ((na - 1) + ((1 + ad) * e).sum(0) / se)
        B = (U * np.where(np.isfinite(d), np.abs(d), 0.0) + r_se + U * np.abs(lse) + U * np.where(np.isfinite(lp), np.abs(lp), 0.0)) * SLACK
    return lp, B, SimpleNamespace(d=d, e=e, se=se, lse=lse, r_se=r_se)


# ----------------------------------------------------------------------------------------------------------- eps-greedy
def eps_greedy(values, eps, u, rand_w, tie_w, mask=None, is_break_tie=False, fault=None):
    """plan!(::EpsilonGreedyExplorer{<:Any, is_break_tie}, values[, mask])  epsilon_greedy_explorer.jl:102-131:
    rand(rng) >= eps ? greedy : random, greedy = rand(rng, find_all_max(values[, mask])[2]) :105,:121 or
    findmax(values)[2] :111 / findmax_masked(values, mask)[2] :130 (= findmax(ifelse.(mask, A, typemin)) basic.jl:117-118);
    random = rand(rng, 1:length(values)) :105,:111 or rand(rng, findall(mask)) :122,:130."""
    x = _f64(values)
    na, n = x.shape
    legal = None if mask is None else np.asarray(mask) != 0
    greedy = (u > eps) if fault == "u_gt_eps" else (u >= eps)
    if is_break_tie:
        _, ties, _ = find_all_max(x, legal, fault)
        g = pick(ties, tie_w, fault)
    else:
        g = findmax(x if legal is None else np.where(legal, x, -np.inf), fault)
    if legal is None or fault == "rand_all_under_mask":
        r = index(rand_w, np.full(n, na), fault)
    else:
        r = pick(legal, rand_w, fault)
    return SimpleNamespace(decision=np.where(greedy, g, r), q=dict(greedy=greedy), margin=np.abs(_f64(u) - eps),
                           budget=np.zeros(n))


def eps_greedy_prob(values, eps, mask=None, is_break_tie=False, fault=None):
    """prob(::EpsilonGreedyExplorer, values[, mask])  :141-194 -> (probs (na, n) Float64, defined (n,))"""
    x = _f64(values)
    na, n = x.shape
    legal = np.ones(x.shape, bool) if mask is None else np.asarray(mask) != 0
    with _quiet():
        probs = np.where(legal, eps / legal.sum(0)[None, :], 0.0)  # :143,:163 fill(eps / n, n); :179-180,:190-191
    defined = np.ones(n, bool)
    if is_break_tie:
        _, ties, defined = find_all_max(x, None if mask is None else legal, fault)
        with _quiet():
            probs = probs + np.where(ties, (1 - eps) / ties.sum(0)[None, :], 0.0)  # :145-147,:181-184
    else:
        a = findmax(x if mask is None else np.where(legal, x, -np.inf), fault)
        probs[a, np.arange(n)] += 1 - eps  # :164,:192
    return probs, defined


# ---------------------------------------------------------------------------------------------------------- categorical
def categorical(logits, u, mask=None, fault=None):
    """sample_categorical networks.jl:425-432 on logits .+ ifelse.(mask, 0f0, typemin) (:468):
    log_probs = logsoftmax(logits, dims = 1); gumbels = -log.(-log.(rand(rng, size...))) .+ log_probs; argmax over dim 1."""
    l = np.asarray(logits, dtype=np.float32)
    legal = None if mask is None else np.asarray(mask) != 0
    if legal is not None and fault != "mask_after_softmax":
        with _quiet():
            l = l + np.where(legal, np.float32(0), np.float32(-np.inf))  # Float32 as written; NaN and +Inf become NaN
    lp, B, aux = logsoftmax(l)
    if legal is not None and fault == "mask_after_softmax":
        lp = np.where(legal, lp, -np.inf)
    with _quiet():
        gn = np.log(-np.log(_f64(u)))
        g = (lp + gn) if fault == "gumbel_add" else (lp - gn)
        Bg = B + 2.0 ** -51 * (1 + np.where(np.isfinite(gn), np.abs(gn), 0.0))
    a, margin, budget = _argmax_margin(g, Bg)
    if fault == "last_max":
        a = findmax(g, fault)
    cols = np.arange(l.shape[1])
    return SimpleNamespace(decision=a, q=dict(logp=lp, g=g, logp_a=lp[a, cols], logp_budget=np.where(np.isfinite(B), B, 0.0)[a, cols]),
                           margin=margin, budget=budget)


# ------------------------------------------------------------------------------------------------------------ explorers
def _walk(w, t, Bj, fault=None):
    """StatsBase.sample's walk: i = 1; cw = w[1]; while cw < t && i < n: i += 1; cw += w[i]"""
    na, n = w.shape
    with _quiet():
        C = np.cumsum(w, 0)
        go = (C <= t[None, :]) if fault == "walk_le" else (C < t[None, :])
    stop = ~go
    stop[na - 1] = True
    a = stop.argmax(0).astype(np.int64)
    if na == 1:
        return a, C, np.full(n, np.inf), np.zeros(n)
    with _quiet():
        dist = np.abs(t[None, :] - C[:-1])
        ok = np.isfinite(dist)
        slack = np.where(ok, dist - Bj[:-1], np.inf)
    j = slack.argmin(0)
    cols = np.arange(n)
    margin = np.where(ok[j, cols], dist[j, cols], np.inf)
    return a, C, margin, np.where(ok[j, cols], Bj[:-1][j, cols], 0.0)


def weighted(values, u, mask=None, is_normalized=False, fault=None, exact=False):
    """plan!(::WeightedExplorer{is_normalized}, values[, mask])  weighted_explorer.jl:25-34: values[.!mask] .= 0 :32;
    sample(rng, Weights(values)) :29 or Weights(values, one(T)) :26 (the sum is NOT computed).  exact=True: dyadic weights,
    every partial sum is exact in Float32, budget 0."""
    w = _f64(values).copy()
    na, n = w.shape
    if mask is not None and fault != "masked_weight_kept":
        w[np.asarray(mask) == 0] = 0.0
    with _quiet():
        S = np.ones(n) if (is_normalized and fault != "ignore_is_normalized") else w.sum(0)
        t = _f64(u) * S
        C = np.cumsum(w, 0)
        j = np.arange(na)[:, None]
        Bj = (j + (0 if is_normalized else na - 1)) * U * np.maximum(np.abs(C), np.abs(t)[None, :]) * SLACK
    if exact:
        Bj = np.zeros_like(Bj)
    a, C, margin, budget = _walk(w, t, np.where(np.isfinite(Bj), Bj, 0.0), fault)
    return SimpleNamespace(decision=a, q=dict(cum=C, t=t, total=S), margin=margin, budget=budget)


def weighted_softmax(values, u, mask=None, fault=None):
    """plan!(::WeightedSoftmaxExplorer, values[, mask])  weighted_softmax_explorer.jl:20-26: values[.!mask] .= typemin(T) :24;
    sample(rng, Weights(softmax(values), one(T))) :21"""
    x = _f64(values).copy()
    na, n = x.shape
    if mask is not None:
        x[np.asarray(mask) == 0] = -np.inf
    lp, _, aux = logsoftmax(x)
    with _quiet():
        p = aux.e / aux.se
        rho = (1 + np.where(aux.e > 0, np.abs(aux.d), 0.0)) * U + aux.r_se[None, :] + U
        C = np.cumsum(p, 0)
        Bj = (np.arange(na)[:, None] * U * C + np.cumsum(rho * p, 0)) * SLACK
    a, C, margin, budget = _walk(p, _f64(u), np.where(np.isfinite(Bj), Bj, 0.0), fault)
    return SimpleNamespace(decision=a, q=dict(cum=C, p=p, t=_f64(u)), margin=margin, budget=budget)


def gumbel_softmax(values, u32, mask=None, fault=None):
    """plan!(::GumbelSoftmaxExplorer, v[, mask])  gumbel_softmax_explorer.jl:12-24: v[.!mask] .= typemin(T) :22;
    argmax(logsoftmax(v) .- log.(-log.(rand(rng, T, n)))) :13-15"""
    x = _f64(values).copy()
    if mask is not None:
        x[np.asarray(mask) == 0] = -np.inf
    lp, B, _ = logsoftmax(x)
    with _quiet():
        gum = np.log(-np.log(_f64(u32)))
        g = (lp + gum) if fault == "gumbel_add" else (lp - gum)
        Bg = B + U * (1 + np.where(np.isfinite(gum), np.abs(gum), 0.0) + np.where(np.isfinite(g), np.abs(g), 0.0)) * SLACK
    a, margin, budget = _argmax_margin(g, Bg)
    if fault == "last_max":
        a = findmax(g, fault)
    return SimpleNamespace(decision=a, q=dict(logp=lp, g=g), margin=margin, budget=budget)


# ------------------------------------------------------------------------------------------------------------------ UCB
UCB_SEPARATION = 1e-9


def ucb(values, c, counts, step, tie_w, fault=None):
    """plan!(p::UCBExplorer, values)  UCB_explorer.jl:24-30, Float64: v, inds = find_all_max(@. values + c * sqrt(log(step + 1) /
    actioncounts)) :25; action = rand(rng, inds) :26; actioncounts[action] += 1 :27.  counts (na, n) is not modified; the
    namespace carries `counts` after the step (unchanged in an UNDEFINED column, where the reference throws at :26).
    margin = the winner's gap to the best score NOT tied with it; judged (exactly) iff it exceeds UCB_SEPARATION."""
    x = _f64(values)
    na, n = x.shape
    with _quiet():
        lg = np.log(F64(step if fault == "ucb_log_step" else step + 1))
        score = x + c * np.sqrt(lg / _f64(counts))
    v, ties, _ = find_all_max(score, None, fault)
    a = pick(ties, tie_w, fault)
    after = _f64(counts).copy()
    if fault != "ucb_no_increment":
        ok = a >= 0
        after[a[ok], np.arange(n)[ok]] += 1.0
    with _quiet():
        rest = np.where(ties | np.isnan(score), -np.inf, score).max(0)
        margin = np.where(np.isnan(v), np.inf, v - rest)
        margin = np.where(np.isnan(margin), np.inf, margin)  # Inf - Inf: ordered by value, not by arithmetic
    return SimpleNamespace(decision=a, q=dict(score=score, ties=ties), margin=margin, budget=np.full(n, UCB_SEPARATION),
                           counts=after)


# ------------------------------------------------------------------------------------------------------------------ laws
def law(kind, values, mask=None, eps=None, is_break_tie=False, is_normalized=False):
    """The exact Float64 probability vector of one column under each rule (random arguments uniform and independent)."""
    x = _f64(values).reshape(-1, 1)
    m = None if mask is None else (np.asarray(mask) != 0).reshape(-1, 1)
    if kind == "eps_greedy":
        return eps_greedy_prob(x, eps, m, is_break_tie)[0][:, 0]
    if kind in ("categorical", "weighted_softmax", "gumbel_softmax"):
        xm = x if m is None else np.where(m, x, -np.inf)
        lp, _, _ = logsoftmax(xm)  # P(argmax_k lp_k + Gumbel_k = a) = softmax_a; the walk over p draws a with p_a
        return np.exp(lp[:, 0])
    if kind == "weighted":
        w = x[:, 0].copy()
        if m is not None:
            w[~m[:, 0]] = 0.0
        if not is_normalized:
            return w / w.sum()
        C = np.minimum(np.cumsum(w), 1.0)  # t = u in [0, 1): action j owns [C_{j-1}, C_j), the last one the remainder
        C[-1] = 1.0
        return np.diff(np.concatenate([[0.0], C]))
    raise KeyError(kind)
