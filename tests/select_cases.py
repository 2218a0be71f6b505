"""Case grids for action selection, with a census (TEST INFRASTRUCTURE ONLY; a helper, not a test module).

Random logits never reach most of what a selection kernel decides by rule: exact ties, NaN and +-Inf, a column whose every
non-maximal exponential underflows, a legal maximum below a larger masked value, an empty tie set.  `cases(entry)` returns, per
entry point, deterministic grids whose COLUMNS are such classes: column i of a grid holds class (i + offset) mod #classes, so
that every class sits in every 64-lane wavefront position over the shapes.  `case.classes` maps the class name to its
columns; `census(case)` asserts that no class the grid is meant to hold is empty, so a grid can never silently miss one.

Shapes.  na over {1, 2, 3, 4, 5, 18, 63, 64, 65, 130} (the explorers: {1, 2, 3, 18, 63, 64}; 65 is their refusal) and n over
{1, 63, 64, 65, 257, 1000}, paired so that both lists are covered: na = 2 without a mask is the one-exponential shortcut,
64 / 65 the two sides of the short-log range, n = 63 / 64 / 65 / 257 the wavefront and block edges.

Run parameters rotate over the cases of an entry point and `coverage(entry)` asserts that each value occurs:
    addressing   "soa" (k_stride n, i_stride 1), "julia" (k_stride 1, i_stride na), "strided" (a non-contiguous view)
    mask_kind    "bool", "u8_2", "u8_255" -- the kernels test != 0
    step         0, 1, 2^32 - 1 (UCB, whose step is an Int64 >= 1: 1, 7, 2^32 - 1, 2^32 + 3 -- the counter is step mod 2^32)
    env_id_base  3, and 2^32 - 5 with n = 64: the env id wraps

`judge(case, got)` compares what the code under test returned with tests/select_ref.py under the margin rule.
"""
import functools
from types import SimpleNamespace

import numpy as np

import select_ref as R

F32 = np.float32
NA_FULL = (1, 2, 3, 4, 5, 18, 63, 64, 65, 130)
NA_EXPL = (1, 2, 3, 18, 63, 64)
N_ALL = (1, 63, 64, 65, 257, 1000)
SHAPES_FULL = ((1, 64), (2, 257), (3, 1000), (4, 65), (5, 63), (18, 257), (63, 65), (64, 1000), (65, 257), (130, 63), (3, 1))
SHAPES_EXPL = ((1, 63), (2, 257), (3, 1000), (18, 65), (63, 64), (64, 1000), (3, 1), (18, 257))
ADDRESSING = ("soa", "julia", "strided")
MASK_KINDS = ("bool", "u8_2", "u8_255")
STEPS_U32 = (0, 1, 2 ** 32 - 1)
STEPS_UCB = (1, 7, 2 ** 32 - 1, 2 ** 32 + 3)
WRAP_BASE = 2 ** 32 - 5
ENTRIES = ("eps_greedy", "prob", "categorical", "weighted", "weighted_softmax", "gumbel_softmax", "ucb")
EXCLUDED_CAP = 1e-3
assert {na for na, _ in SHAPES_FULL} == set(NA_FULL) and {n for _, n in SHAPES_FULL} == set(N_ALL)
assert {na for na, _ in SHAPES_EXPL} == set(NA_EXPL) and {n for _, n in SHAPES_EXPL} == set(N_ALL)


# ------------------------------------------------------------------------------------------------------- value classes
# builder(na, rng) -> (values (na,) Float32, mask (na,) bool or None = no requirement on the mask); min na
def _random(na, rng):
    return (rng.standard_normal(na) * 2).astype(F32), None


def _all_equal(na, rng):
    return np.full(na, 0.75, F32), None


def _ties(k):
    def build(na, rng):
        v = (rng.integers(-8, 4, na) / 4).astype(F32)  # dyadic, all below the maximum 1.5
        v[rng.choice(na, k, replace=False)] = 1.5
        return v, None
    return build


def _nan(k):
    def build(na, rng):
        v, _ = _random(na, rng)
        kk = na if k is None else k
        idx = rng.choice(np.arange(1, na) if (kk < na and na > 1) else na, kk, replace=False)  # not at index 0: a rule that
        v[idx] = np.nan                                                                         # ignores NaN must show
        return v, None
    return build


def _ninf(which):
    def build(na, rng):
        v, _ = _random(na, rng)
        if which == "one":
            v[rng.integers(0, na)] = -np.inf
        elif which == "all_but_one":
            keep = rng.integers(0, na)
            v[np.arange(na) != keep] = -np.inf
        else:
            v[:] = -np.inf
        return v, None
    return build


def _pinf(na, rng):
    v, _ = _random(na, rng)
    v[rng.integers(0, na)] = np.inf
    return v, None


def _spread_big(na, rng):
    v = (-105.0 - rng.random(na) * 20).astype(F32)  # exp(x - max) < exp(-104) < 2^-149: underflows to 0 in Float32
    v[rng.integers(0, na)] = 0.5
    return v, None


def _spread_ulp(na, rng):
    v = np.where(rng.random(na) < 0.5, F32(1.0), np.nextafter(F32(1.0), F32(2.0))).astype(F32)
    v[0], v[na - 1] = F32(1.0), np.nextafter(F32(1.0), F32(2.0))
    return v, None


def _one_legal(na, rng):
    v, _ = _random(na, rng)
    m = np.zeros(na, bool)
    m[rng.integers(0, na)] = True
    return v, m


def _legal_below_masked(na, rng):
    v, _ = _random(na, rng)
    m = np.ones(na, bool)
    m[np.argsort(v)[-max(1, na // 3):]] = False  # the largest values are illegal
    return v, m


def _masked_nan(na, rng):
    v, _ = _random(na, rng)
    m = rng.random(na) < 0.7
    k = rng.integers(1, na)
    v[k], m[k] = np.nan, False
    m[(k + 1) % na] = True
    return v, m


def _all_masked(na, rng):
    v, _ = _random(na, rng)
    return v, np.zeros(na, bool)


LOGIT_CLASSES = dict(random=(_random, 1), all_equal=(_all_equal, 1), tie2=(_ties(2), 2), tie3=(_ties(3), 3),
                     nan_one=(_nan(1), 1), nan_several=(_nan(2), 3), nan_all=(_nan(None), 1), ninf_one=(_ninf("one"), 1),
                     ninf_all_but_one=(_ninf("all_but_one"), 2), ninf_all=(_ninf("all"), 1), pinf=(_pinf, 1),
                     spread_big=(_spread_big, 2), spread_ulp=(_spread_ulp, 2))
MASK_CLASSES = dict(one_legal=(_one_legal, 2), legal_below_masked=(_legal_below_masked, 2), masked_nan=(_masked_nan, 2))
ALL_MASKED = dict(all_masked=(_all_masked, 1))


# weights (WeightedExplorer: "elements are assumed to be >= 0")
def _w_random(na, rng):
    return (rng.random(na) + F32(0.01)).astype(F32), None


def _w_dyadic(na, rng):
    return (rng.integers(0, 65, na) / 64).astype(F32), None  # multiples of 2^-6 below 2^7 na: every partial sum is exact


def _w_zeros(where):
    def build(na, rng, base=_w_random):
        v, _ = base(na, rng)
        k = max(1, na // 3)
        if where == "lead":
            v[:k] = 0
            v[k:] = np.maximum(v[k:], F32(1 / 64))
        elif where == "trail":
            v[na - k:] = 0
            v[:na - k] = np.maximum(v[:na - k], F32(1 / 64))
        else:
            v[:] = 0
        return v, None
    return build


def _dy(build):
    return lambda na, rng: build(na, rng, base=_w_dyadic)


def _w_nan(k):
    def build(na, rng):
        v, _ = _w_random(na, rng)
        v[rng.choice(na, na if k is None else k, replace=False)] = np.nan
        return v, None
    return build


def _w_pinf(na, rng):
    v, _ = _w_random(na, rng)
    v[rng.integers(0, na)] = np.inf
    return v, None


def _w_masked(build):
    def f(na, rng):
        v, m = build(na, rng)
        return np.abs(np.where(np.isfinite(v) | np.isnan(v), v, 1)).astype(F32), m
    return f


WEIGHT_CLASSES = dict(random=(_w_random, 1), all_equal=(_all_equal, 1), lead_zero=(_w_zeros("lead"), 2),
                      trail_zero=(_w_zeros("trail"), 2), all_zero=(_w_zeros("all"), 1), nan_one=(_w_nan(1), 1),
                      nan_all=(_w_nan(None), 1), pinf=(_w_pinf, 1))
WEIGHT_MASK_CLASSES = dict(one_legal=(_w_masked(_one_legal), 2), legal_below_masked=(_w_masked(_legal_below_masked), 2),
                           masked_nan=(_w_masked(_masked_nan), 2), all_masked=(_w_masked(_all_masked), 1))
DYADIC_CLASSES = dict(dyadic=(_w_dyadic, 1), lead_zero=(_dy(_w_zeros("lead")), 2), trail_zero=(_dy(_w_zeros("trail")), 2),
                      all_zero=(_w_zeros("all"), 1))


def _w_scaled(s):
    def build(na, rng):
        v, _ = _w_random(na, rng)
        return (v / v.sum() * s).astype(F32), None
    return build


NORMALIZED_CLASSES = dict(sum_below_one=(_w_scaled(0.3), 1), sum_above_one=(_w_scaled(3.0), 1), sum_near_one=(_w_scaled(1.0), 1))


def _grid(na, n, classes, masked, rng, offset):
    """(values (na, n), mask (na, n) bool or None, {class: columns}).  masked: columns whose class does not prescribe a mask get
    a random one with at least one legal action."""
    names = [c for c, (_, min_na) in classes.items() if na >= min_na]
    vals = np.empty((na, n), F32)
    mask = np.ones((na, n), bool) if masked else None
    cols = {c: [] for c in names}
    for i in range(n):
        c = names[(i + offset) % len(names)]
        v, m = classes[c][0](na, rng)
        vals[:, i] = v
        if masked:
            if m is None:
                m = rng.random(na) < 0.7
                m[rng.integers(0, na)] = True
            mask[:, i] = m
        else:
            assert m is None
        cols[c].append(i)
    return vals, mask, {c: np.array(ix, np.int64) for c, ix in cols.items()}


# --------------------------------------------------------------------------------------------------------------- cases
def _case(entry, tag, vals, mask, classes, ci, mi, **kw):
    na, n = vals.shape
    steps = STEPS_UCB if entry == "ucb" else STEPS_U32
    c = SimpleNamespace(entry=entry, na=na, n=n, values=vals, mask=mask, classes=classes, seed=1000 + 7 * ci,
                        step=steps[ci % len(steps)], env_id_base=3, addressing=ADDRESSING[ci % 3],
                        mask_kind=None if mask is None else MASK_KINDS[mi % 3], eps=None, is_break_tie=False,
                        is_normalized=False, exact=False, c=2.0, counts=None, steps=1)
    c.__dict__.update(kw)
    c.id = f"{entry}-{tag}{ci}-na{na}-n{n}-{c.addressing}" + ("" if mask is None else f"-{c.mask_kind}")  # ci: unique
    # a class can only be required where the grid has a column for it
    c.required = list(classes) if n >= len(classes) else [k for k, ix in classes.items() if len(ix)]
    return c


@functools.lru_cache(maxsize=None)
def cases(entry):
    out, ci, mi = [], 0, 0
    rng = np.random.default_rng(abs(hash_name(entry)))

    def add(tag, na, n, classes, masked, **kw):
        nonlocal ci, mi
        vals, mask, cols = _grid(na, n, classes, masked, rng, offset=ci)
        out.append(_case(entry, tag, vals, mask, cols, ci, mi, **kw))
        ci += 1
        mi += 1 if masked else 0

    if entry in ("eps_greedy", "prob"):
        eps_list = (0.3, 0.0, 1.0, 0.3)
        for k, (na, n) in enumerate(SHAPES_FULL):
            for masked in (False, True):
                cl = dict(LOGIT_CLASSES, **(dict(MASK_CLASSES, **ALL_MASKED) if masked else {}))
                add("grid", na, n, cl, masked, eps=eps_list[(k + masked) % 4], is_break_tie=bool((k + masked) % 2))
                add("grid", na, n, cl, masked, eps=0.3, is_break_tie=not bool((k + masked) % 2)) if n <= 257 else None
        add("wrap", 18, 64, LOGIT_CLASSES, False, eps=0.3, env_id_base=WRAP_BASE)
        if entry == "eps_greedy":  # eps equal to the uniform of one column: `>=` against `>`
            for tie in (False, True):
                add("epshit", 18, 65, dict(random=LOGIT_CLASSES["random"]), False, eps=0.5, is_break_tie=tie, step=1)
                c = out[-1]
                u = R.draws("eps_greedy", c.seed, c.env_id_base, c.n, c.step, c.na)["u"]
                c.eps = float(u[17])
                c.classes["eps_equals_u"] = np.array([17])
                c.required.append("eps_equals_u")
    elif entry == "categorical":
        for na, n in SHAPES_FULL:
            add("grid", na, n, LOGIT_CLASSES, False)
            add("grid", na, n, dict(LOGIT_CLASSES, **MASK_CLASSES), True)
        add("wrap", 5, 64, LOGIT_CLASSES, False, env_id_base=WRAP_BASE)
    elif entry in ("weighted_softmax", "gumbel_softmax"):
        for na, n in SHAPES_EXPL:
            add("grid", na, n, LOGIT_CLASSES, False)
            add("grid", na, n, dict(LOGIT_CLASSES, **MASK_CLASSES), True)
        add("wrap", 18, 64, LOGIT_CLASSES, False, env_id_base=WRAP_BASE)
    elif entry == "weighted":
        for na, n in SHAPES_EXPL:
            add("grid", na, n, WEIGHT_CLASSES, False)
            add("grid", na, n, dict(WEIGHT_CLASSES, **WEIGHT_MASK_CLASSES), True)
            add("dyadic", na, n, DYADIC_CLASSES, False, exact=True)
            add("dyadic", na, n, DYADIC_CLASSES, True, exact=True)
            add("normalized", na, n, NORMALIZED_CLASSES, False, is_normalized=True)
        add("wrap", 18, 64, WEIGHT_CLASSES, False, env_id_base=WRAP_BASE)
    elif entry == "ucb":
        ucb_cl = {k: LOGIT_CLASSES[k] for k in ("random", "all_equal", "tie2", "tie3", "nan_one", "nan_all", "pinf", "ninf_one")}
        for na, n in SHAPES_FULL:
            add("grid", na, n, ucb_cl, False)
            c = out[-1]
            c.counts = _ucb_counts(c, rng)
        add("wrap", 5, 64, ucb_cl, False, env_id_base=WRAP_BASE)
        out[-1].counts = _ucb_counts(out[-1], rng)
        add("seq40", 4, 65, dict(tie3=LOGIT_CLASSES["tie3"]), False, step=1, steps=40)  # three tied scores at step 1
        c = out[-1]
        c.counts = np.full((4, 65), 1e-10)
        c.more_values = [(rng.integers(-8, 9, (4, 65)) / 4).astype(F32) for _ in range(39)]  # dyadic: ties keep occurring
        c.classes["three_tied_scores"] = c.classes["tie3"]
        c.required.append("three_tied_scores")
    else:
        raise KeyError(entry)
    assert len({c.id for c in out}) == len(out)
    return tuple(out)


def hash_name(s):
    return sum((i + 1) * ord(ch) for i, ch in enumerate(s))


def _ucb_counts(c, rng):
    """per column: every count eps (the constructor's fill), one zero count, one huge count, small integer counts; a column whose
    class is a tie in value gets ONE count of its kind in every row (all eps / all zero: every score Inf / all huge / all 4), so
    that the SCORES tie"""
    cnt = np.empty((c.na, c.n))
    kinds = {k: [] for k in ("count_eps", "count_zero", "count_huge", "count_int")}
    for i in range(c.n):
        k = ("count_eps", "count_zero", "count_huge", "count_int")[(i // 3) % 4]
        col = np.full(c.na, 1e-10) if k == "count_eps" else rng.integers(1, 50, c.na).astype(np.float64)
        if k == "count_zero":
            col[rng.integers(0, c.na)] = 0.0
        if k == "count_huge":
            col[rng.integers(0, c.na)] = 1e300
        if any(i in c.classes.get(t, ()) for t in ("tie2", "tie3", "all_equal")):
            col[:] = dict(count_eps=1e-10, count_zero=0.0, count_huge=1e300, count_int=4.0)[k]
        cnt[:, i] = col
        kinds[k].append(i)
    for k, ix in kinds.items():
        c.classes[k] = np.array(ix, np.int64)
        if c.n >= 12:
            c.required.append(k)
    return cnt


def census(case):
    for k in case.required:
        assert len(case.classes[k]) > 0, (case.id, k)
    return {k: len(ix) for k, ix in case.classes.items()}


def coverage(entry):
    """every addressing, mask encoding, step, the wrapping env id and every shape occur among the cases of `entry`"""
    cs = cases(entry)
    full = entry in ("eps_greedy", "prob", "categorical", "ucb")
    assert {c.addressing for c in cs} == set(ADDRESSING), entry
    if entry != "ucb":
        assert {c.mask_kind for c in cs if c.mask is not None} == set(MASK_KINDS), entry
    assert {c.step for c in cs} >= set(STEPS_UCB if entry == "ucb" else STEPS_U32) or entry == "prob", entry
    assert any(c.env_id_base == WRAP_BASE and c.n == 64 for c in cs), entry
    assert {c.na for c in cs} >= set(NA_FULL if full else NA_EXPL) and {c.n for c in cs} >= set(N_ALL), entry
    want = set(LOGIT_CLASSES) if entry != "weighted" else set(WEIGHT_CLASSES) | set(DYADIC_CLASSES) | set(NORMALIZED_CLASSES)
    if entry == "ucb":
        want = {"random", "all_equal", "tie2", "tie3", "nan_one", "nan_all", "pinf", "ninf_one", "count_eps", "count_zero",
                "count_huge", "count_int", "three_tied_scores"}
    elif entry == "weighted":
        want |= set(WEIGHT_MASK_CLASSES)
    else:
        want |= set(MASK_CLASSES)
    if entry in ("eps_greedy", "prob"):
        want |= set(ALL_MASKED)
    have = {k for c in cs for k in c.required}
    assert want <= have, (entry, want - have)


# --------------------------------------------------------------------------------------------------------------- model
@functools.lru_cache(maxsize=None)
def _draws(entry, seed, base, n, step, na, shared):
    return R.draws(entry, seed, base, n, step, na, fault="shared_uniform" if shared else None)


def model(case, fault=None):
    """tests/select_ref.py on the case (the random arguments from the documented draw layout)"""
    e = case.entry
    if e == "prob":
        probs, defined = R.eps_greedy_prob(case.values, case.eps, case.mask, case.is_break_tie, fault)
        return SimpleNamespace(probs=probs, defined=defined)
    if e == "ucb":
        cnt, outs, vals = case.counts, [], [case.values] + list(getattr(case, "more_values", []))
        for s in range(case.steps):
            d = _draws(e, case.seed, case.env_id_base, case.n, case.step + s, case.na, False)
            r = R.ucb(vals[s], case.c, cnt, case.step + s, d["tie_w"], fault)
            cnt = r.counts.copy()
            und = r.decision == R.UNDEFINED
            cnt[0, und] += 1.0  # the project's pin for a column on which the reference throws: index 0, counted
            outs.append(r)
        return SimpleNamespace(steps=outs, counts=cnt)
    d = _draws(e, case.seed, case.env_id_base, case.n, case.step, case.na, fault == "shared_uniform")
    if e == "eps_greedy":
        return R.eps_greedy(case.values, case.eps, d["u"], d["rand_w"], d["tie_w"], case.mask, case.is_break_tie, fault)
    if e == "categorical":
        return R.categorical(case.values, d["u"], case.mask, fault)
    if e == "weighted":
        return R.weighted(case.values, d["u"], case.mask, case.is_normalized, fault, exact=case.exact)
    if e == "weighted_softmax":
        return R.weighted_softmax(case.values, d["u"], case.mask, fault)
    if e == "gumbel_softmax":
        return R.gumbel_softmax(case.values, d["u32"], case.mask, fault)
    raise KeyError(e)


def _decisions(r, got_actions):
    """judged columns and mismatches among them; an UNDEFINED model decision is the pinned index 0"""
    want = np.where(r.decision == R.UNDEFINED, 0, r.decision)
    judged = (r.margin > r.budget) | (r.budget == 0)  # budget 0: the rule's arithmetic is exact, every column is judged
    return judged, int(np.sum(judged & (want != got_actions)))


def judge(case, got, fault=None):
    """got: what the code under test returned -- dict(actions[, logp]) / dict(probs) / dict(actions = [per step], counts).
    Returns mismatch (judged columns that disagree with the model), excluded (share of columns left out by the margin rule),
    and for categorical the largest |logp - model| and its budget."""
    m = model(case, fault)
    e = case.entry
    if e == "prob":
        want = np.where(m.defined[None, :], m.probs, 0.0)  # find_all_max over an empty mask throws: the project returns zeros
        bad = ~((want == got["probs"]) | (np.isnan(want) & np.isnan(got["probs"])))
        return SimpleNamespace(mismatch=int(bad.any(0).sum()), excluded=0.0)
    if e == "ucb":
        mism, excl = 0, 0
        for r, a in zip(m.steps, got["actions"]):
            judged, k = _decisions(r, a)
            mism, excl = mism + k, excl + int((~judged).sum())
        mism += int((m.counts != got["counts"]).any(0).sum()) if excl == 0 else 0
        return SimpleNamespace(mismatch=mism, excluded=excl / (case.n * case.steps))
    judged, mism = _decisions(m, got["actions"])
    out = SimpleNamespace(mismatch=mism, excluded=float((~judged).mean()), logp_err=0.0, logp_budget=0.0)
    if e == "categorical" and got.get("logp") is not None:
        # judged on the model's own action: the log-probability of the action the code returned, where they agree
        same = np.where(m.decision == R.UNDEFINED, 0, m.decision) == got["actions"]
        want, have = m.q["logp_a"], got["logp"].astype(np.float64)
        both_nan = np.isnan(want) & np.isnan(have)
        with np.errstate(all="ignore"):
            err = np.where(both_nan | (want == have), 0.0, np.abs(want - have))
        err = np.where(np.isnan(err), np.inf, err)
        bad = same & (err > m.q["logp_budget"])
        out.mismatch += int(bad.sum())
        fin = same & np.isfinite(err)
        if fin.any():
            k = np.argmax(np.where(fin, err, -1.0))
            out.logp_err, out.logp_budget = float(err[k]), float(m.q["logp_budget"][k])
    return out


# -------------------------------------------------------------------------------------------------------------- oracle
EXACT_ENTRIES = ("eps_greedy", "prob", "ucb")


def is_exact(case):
    """the grids whose arithmetic is exact take no allowance: no column may be left out"""
    return case.entry in EXACT_ENTRIES or case.exact


def mask_u8(case):
    """the mask as the C ABI takes it: one byte per entry, any non-zero value is `true`"""
    if case.mask is None:
        return None
    one = {"bool": 1, "u8_2": 2, "u8_255": 255}[case.mask_kind]
    return (case.mask.astype(np.uint8) * one).astype(np.uint8)


def run_oracle(case):
    import oracle

    e, m = case.entry, mask_u8(case)
    if e == "eps_greedy":
        return dict(actions=oracle.eps_greedy_select(case.values, case.eps, case.seed, case.step, case.env_id_base, m, case.is_break_tie))
    if e == "prob":
        v = case.values.astype(np.float64)
        cols = [oracle.eps_greedy_prob(v[:, i], case.eps, None if m is None else m[:, i], case.is_break_tie) for i in range(case.n)]
        return dict(probs=np.stack(cols, 1))
    if e == "categorical":
        a, lp = oracle.categorical_sample(case.values, case.seed, case.step, case.env_id_base, m)
        return dict(actions=a, logp=lp)
    if e == "ucb":
        cnt = np.ascontiguousarray(case.counts.copy())
        vals = [case.values] + list(getattr(case, "more_values", []))
        acts = [oracle.ucb_select(vals[s], case.c, cnt, case.step + s, case.seed, case.env_id_base) for s in range(case.steps)]
        return dict(actions=acts, counts=cnt)
    return dict(actions=oracle.explorer_select(e, case.values, case.seed, case.step, case.env_id_base, m, case.is_normalized))


def law_oracle(c, n=None, step=None):
    import oracle

    n = LAW_N if n is None else n
    v = tile(c.column, n)
    m = None if getattr(c, "mask_column", None) is None else tile(c.mask_column.astype(np.uint8), n)
    step = c.step if step is None else step
    if c.entry == "categorical":
        return oracle.categorical_sample(v, c.seed, step, c.env_id_base, m)[0]
    if c.entry == "eps_greedy":
        return oracle.eps_greedy_select(v, c.eps, c.seed, step, c.env_id_base, m, c.is_break_tie)
    return oracle.explorer_select(c.entry, v, c.seed, step, c.env_id_base, m, c.is_normalized)



# ---------------------------------------------------------------------------------------------------------- statistics
LAW_N = 1 << 17
LAW_ALPHA = 1e-6
MIN_EXPECTED = 100


def chi2_bar(dof):
    from scipy.stats import chi2

    return float(chi2.ppf(1 - LAW_ALPHA, dof)) if dof > 0 else 0.0


def chi2_counts(actions, p, na):
    """Pearson's statistic of the action counts against p over the cells with p > 0; +inf if a cell with p = 0 was hit.
    Returns (statistic, degrees of freedom, counts)."""
    cnt = np.bincount(np.asarray(actions, np.int64), minlength=na).astype(np.float64)
    n = cnt.sum()
    live = p > 0
    if cnt[~live].sum() > 0:
        return np.inf, int(live.sum()) - 1, cnt
    if live.sum() == 1:
        return -1.0, 0, cnt  # a single possible action and nothing else drawn: below the bar 0 of dof 0
    E = n * p[live]
    return float(((cnt[live] - E) ** 2 / E).sum()), int(live.sum()) - 1, cnt


def chi2_independence(a, b, k=3):
    """Pearson's statistic of the k x k contingency table of (a, b) against the product of its margins; dof (k - 1)^2"""
    tab = np.zeros((k, k))
    np.add.at(tab, (np.asarray(a, np.int64), np.asarray(b, np.int64)), 1.0)
    E = tab.sum(1, keepdims=True) * tab.sum(0, keepdims=True) / tab.sum()
    return float(((tab - E) ** 2 / E).sum()), (k - 1) ** 2, tab


@functools.lru_cache(maxsize=None)
def law_cases():
    """One column repeated LAW_N times per case; every expected count is >= MIN_EXPECTED (logit spread 2.5 at na >= 64)."""
    out = []
    rng = np.random.default_rng(20240)

    def add(entry, na, v, mask=None, **kw):
        c = SimpleNamespace(entry=entry, na=na, n=LAW_N, column=np.asarray(v, F32), mask_column=mask, seed=4000 + 13 * len(out),
                            step=5 + len(out), env_id_base=11, eps=None, is_break_tie=False, is_normalized=False)
        c.__dict__.update(kw)
        kind = "eps_greedy" if entry == "eps_greedy" else entry
        c.p = R.law(kind, c.column, mask, eps=c.eps, is_break_tie=c.is_break_tie, is_normalized=c.is_normalized)
        assert abs(c.p.sum() - 1) < 1e-12 and (c.p[c.p > 0] * LAW_N).min() >= MIN_EXPECTED, (entry, na)
        c.id = f"{entry}-na{na}" + ("" if mask is None else "-masked")
        out.append(c)

    def mask_of(na):
        m = np.ones(na, bool)
        m[1::3] = False
        return m

    for na in (2, 3, 5, 64, 65):
        v = rng.permutation(np.linspace(0.0, 2.5 if na >= 64 else 2.0, na))
        add("categorical", na, v)
        add("categorical", na, v, mask_of(na))
    for entry in ("weighted", "weighted_softmax", "gumbel_softmax"):
        for na in (3, 64):
            v = rng.permutation(np.linspace(0.5, 1.5, na)) if entry == "weighted" else rng.permutation(np.linspace(0.0, 2.5, na))
            add(entry, na, v)
    v = np.array([1.0, 0.25, 1.0, -1.0, 1.0])  # a three-way tie
    add("eps_greedy", 5, v, eps=0.3, is_break_tie=True)
    add("eps_greedy", 5, v, np.array([True, True, False, True, True]), eps=0.3, is_break_tie=True)
    return tuple(out)


def tile(column, n):
    return np.ascontiguousarray(np.repeat(np.asarray(column)[:, None], n, 1))


INDEPENDENCE = (SimpleNamespace(id="categorical", entry="categorical", column=np.array([0.3, -0.4, 0.9], F32), eps=None,
                                is_break_tie=False, seed=77, step=9, env_id_base=5),
                SimpleNamespace(id="eps_greedy", entry="eps_greedy", column=np.array([0.5, 0.5, 0.0], F32), eps=0.3,
                                is_break_tie=True, seed=78, step=2, env_id_base=5))
