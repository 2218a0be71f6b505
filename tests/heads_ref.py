"""The Gaussian heads' log-probabilities as a float64 model with a derived error budget (plain numpy; no oracle, no GPU).

csrc/heads.hip and the oracle are built with -ffp-contract=off and Float32 division is the IEEE sequence, so every + - * / of the
kernel is correctly rounded: replayed in numpy float32 in the kernel's order it is bit-identical given equal inputs.  Only the libm
calls (ocml on the device, glibc in the oracle) differ.  A quantity of the kernel is carried here as `Q(c, e)`: a float64 centre and
an absolute error bound.
  * e == 0: the quantity is an exact replay (c holds a float32 value); an operation on exact operands is done in float32, e stays 0
  * a libm call f: c = f evaluated in float64 on the centre, e = |f'(c)| e_in + E_f ulp(c), with E_f the OpenCL full-profile
    single-precision bounds that ocml is written to meet (E below; OpenCL C specification, "Relative error as ULPs")
  * an operation with an inexact operand: c in float64, e = first-order propagation + half an ulp of the rounded Float32 result
  * a scaling by a power of two is exact
The outputs are the expected value in float64 and a per-sample budget; the bar is 2 x budget (the factor covers the dropped
second-order terms and the ulp changes at binade edges).  Where the expected value is not finite (log of an exact 0, Inf - Inf) the
non-finite pattern must match exactly.  On the (state, action) path z = atanhf(a) is not observable: its centre is float64
atanh(a), and a component whose u = 1 - t^2 is within 4 of its own error bound makes the sample unconstrained: it is left out and
counted (`left`), against a cap set by the caller.
Shared by tests/test_heads_reference.py (CPU, the oracle and planted faults), tests/test_gpu_heads.py and tests/test_gpu_parity.py."""
import numpy as np

E = {"log": 3.0, "exp": 3.0, "log1p": 2.0, "tanh": 5.0, "atanh": 5.0}
F32, F64 = np.float32, np.float64
LOG2PI = F32(1.8378770664093453)   # log(2f0 * pi) as Float32 (distributions.jl:9)
LN2 = F32(0.6931472)               # log(2f0)
EPS = F32(1.0e-8)


def ulp(x):
    """the Float32 spacing at |x| (x a float64 centre); NaN where x is not finite"""
    with np.errstate(all="ignore"):
        return np.spacing(np.abs(np.asarray(x, F64)).astype(F32)).astype(F64)


class Q:
    def __init__(self, c, e=0.0):
        c = np.asarray(c)
        self.c = c.astype(F64)
        self.e = np.broadcast_to(np.asarray(e, F64), c.shape).copy()

    def _op(self, o, f, prop):
        o = o if isinstance(o, Q) else Q(F32(o))
        with np.errstate(all="ignore"):
            r64 = f(self.c, o.c)
            r32 = f(self.c.astype(F32), o.c.astype(F32)).astype(F64)
            exact = (self.e == 0) & (o.e == 0)
            return Q(np.where(exact, r32, r64), np.where(exact, 0.0, prop(self, o) + 0.5 * ulp(r64)))

    def __add__(self, o):
        return self._op(o, np.add, lambda a, b: a.e + b.e)

    def __sub__(self, o):
        return self._op(o, np.subtract, lambda a, b: a.e + b.e)

    def __mul__(self, o):
        return self._op(o, np.multiply, lambda a, b: np.abs(a.c) * b.e + np.abs(b.c) * a.e)

    def __truediv__(self, o):
        return self._op(o, np.divide, lambda a, b: a.e / np.abs(b.c) + np.abs(a.c) * b.e / (b.c * b.c))

    def scale(self, k):                     # k a power of two (or -1): exact
        return Q(self.c * k, self.e * abs(k))

    def abs(self):
        return Q(np.abs(self.c), self.e)

    def relu(self):
        return Q(np.where(self.c > 0, self.c, 0.0), np.where(self.c > -self.e, self.e, 0.0))

    def libm(self, name):
        with np.errstate(all="ignore"):
            c = getattr(np, {"atanh": "arctanh"}.get(name, name))(self.c)
            if name == "log":               # d(log u) = du / (u - du)
                room = self.c - self.e
                p = np.where(self.e == 0, 0.0, np.where(room > 0, self.e / room, np.inf))
            elif name == "exp":
                p = c * self.e
            elif name == "log1p":
                p = self.e / (1.0 + self.c)
            elif name == "tanh":
                p = (1.0 - c * c) * self.e
            else:
                assert name == "atanh" and not self.e.any()
                p = 0.0
            return Q(c, p + E[name] * ulp(c))


def clamp(x, lo, hi):
    """clamp(x, lo, hi) of the reference = clampj of the kernel: a NaN passes through"""
    x = np.asarray(x, F32)
    return np.where(x > F32(hi), F32(hi), np.where(x < F32(lo), F32(lo), x)).astype(F32)


def _like(x, z):
    """(d, n) head input -> broadcastable against (d, K, n) samples"""
    x = np.asarray(x, F32)
    return x[:, None, :] if np.ndim(z) == 3 else x


def _gaussian(mu, sg, z, t):
    """GaussianNetwork (:74): diagnormlogpdf(mu, sigma, z) .+ logpdfcorrection(z, squash); z, t are Q over (d, ...) or t None"""
    mu, sg = Q(mu), Q(sg)
    d = z.c.shape[0]
    one = np.ones(z.c.shape[1:], F32)
    prod, total, corr = Q(one), Q(0 * one), Q(0 * one)
    left = np.zeros(one.shape, bool)
    for k in range(d):
        s = Q(sg.c[k]) + EPS
        v = s * s
        dx = Q(z.c[k], z.e[k]) - Q(mu.c[k])
        prod = prod * v
        total = total + (dx * dx) / v
        if t is not None:
            tk = Q(t.c[k], t.e[k])
            u = Q(one) - tk * tk
            left |= (u.e > 0) & ~(u.c > 4 * u.e)
            corr = corr + u.libm("log")
    lp = ((prod.libm("log") + total) + Q(F32(d)) * LOG2PI).scale(-0.5)
    return (lp + corr.scale(-1)) if t is not None else lp, left


def _soft(mu, sg, z):
    """SoftGaussianNetwork (:156): sum(normlogpdf(mu, sigma, z) .- 2 (log 2 - z - softplus(-2 z)), dims = 1)"""
    acc = Q(np.zeros(z.c.shape[1:], F32))
    for k in range(z.c.shape[0]):
        zk = Q(z.c[k], z.e[k])
        nl = _normlogpdf(Q(mu[k]), Q(sg[k]), zk)
        x = zk.scale(-2)
        sp = x.abs().scale(-1).libm("exp").libm("log1p") + x.relu()
        acc = acc + (nl - ((Q(LN2) - zk) - sp).scale(2))
    return acc


def _normlogpdf(mu, sg, x):
    se = sg + EPS
    zz = (x - mu) / se
    return (zz * zz + LOG2PI).scale(-0.5) - se.libm("log")


def _out(q, left=None):
    left = np.zeros(q.c.shape, bool) if left is None else left
    return q.c, q.e, left & np.isfinite(q.c)


def gaussian_sample(mu, sg, z, t=None):
    """sampling: z the pre-squash sample (Float32, exact), t the implementation's own tanh action (or None: identity);
    mu, sg (d, n), sg already clamped; z, t (d, K, n) -> expected, budget, left (K, n); left is empty on this path"""
    return _out(*_gaussian(_like(mu, z), _like(sg, z), Q(np.asarray(z, F32)), None if t is None else Q(np.asarray(t, F32))))


def gaussian_eval(mu, sg, a, squash):
    """(model)(state, action): a (d, K, n) Float32"""
    a = Q(np.asarray(a, F32))
    if not squash:
        return _out(*_gaussian(_like(mu, a.c), _like(sg, a.c), a, None))
    z = a.libm("atanh")
    return _out(*_gaussian(_like(mu, a.c), _like(sg, a.c), z, z.libm("tanh")))


def soft_sample(mu, sg, z):
    return _out(_soft(_like(mu, z), _like(sg, z), Q(np.asarray(z, F32))))


def soft_eval(mu, sg, a):
    return _out(_soft(_like(mu, a), _like(sg, a), Q(np.asarray(a, F32)).libm("atanh")))


def normlogpdf(mu, sg, x):
    """normlogpdf(mu, sigma, x) elementwise (distributions.jl:18-21): one term of the soft branch"""
    return _out(_normlogpdf(Q(np.asarray(mu, F32)), Q(np.asarray(sg, F32)), Q(np.asarray(x, F32))))


def diagnormlogpdf(mu, sg, x):
    """diagnormlogpdf over dims = 1 of (d, n) arrays (distributions.jl:31-34): the identity branch of the head"""
    return _out(*_gaussian(np.asarray(mu, F32), np.asarray(sg, F32), Q(np.asarray(x, F32)), None))


def tanh_ulps(t, z):
    """|t - tanh(z)| in Float32 ulps of the float64 value, elementwise; NaN in must give NaN out (then 0), else Inf"""
    t, z = np.asarray(t, F32), np.asarray(z, F32)
    with np.errstate(all="ignore"):
        ref = np.tanh(z.astype(F64))
        r = np.abs(t.astype(F64) - ref) / ulp(ref)
    return np.where(np.isnan(ref), np.where(np.isnan(t), 0.0, np.inf), np.where(np.isnan(r), np.inf, r))


# ------------------------------------------------------------------------------------------------ the cases both suites run
FAMILIES = ("identity", "tanh", "soft")            # GaussianNetwork identity / tanh, SoftGaussianNetwork
SQUASH_SOFT = {"identity": (0, 0), "tanh": (1, 0), "soft": (1, 1)}
# (d, n, K): the four the suite had, then odd d with K > 1 (a Philox pair (q / 2, q & 1) of draw q = k + d j straddles two
# samples), d = 64 with odd K, K > 256 with n = 1 (one state across two blocks), 257 states (one lane in the second block)
SHAPES = [(1, 4099, 1), (10, 3, 5), (6, 1000, 3), (64, 17, 2), (3, 700, 4), (5, 33, 3), (1, 50, 7), (64, 5, 3), (2, 1, 300),
          (7, 257, 1)]
SCALED_SHAPES = [(6, 1000, 3), (3, 700, 4)]         # run once more with mu x 3: tanhf saturates, +Inf log-probabilities
LO, HI = 0.2, 1.7
EVAL_CAP = 0.005                                    # left-out share on sampled actions at sigma in [LO, HI], unit-normal mu


def inputs(d, n, seed=0, scale=1.0):
    rng = np.random.default_rng(seed)
    mu = (rng.normal(size=(d, n)) * scale).astype(F32)
    raw = np.log1p(np.exp(rng.normal(size=(d, n)))).astype(F32)
    return mu, raw


def grid_actions(d, K, n, emax, seed=0):
    """|a| = 1 - 2^-e, e = 1 ... emax, every e present, with random signs"""
    rng = np.random.default_rng(seed)
    e = (np.arange(d * K * n) % emax + 1).reshape(d, K, n)
    return (rng.choice([-1.0, 1.0], size=e.shape) * (1.0 - 2.0 ** -e)).astype(F32)


def edge_cases():
    """name -> dict(mu, raw (d, n), lo, hi, K): saturation and the sigma edges"""
    rng = np.random.default_rng(7)
    nx = np.nextafter
    out = {}
    d, n = 4, 40                                   # |z| ~ 12 +- 0.2: tanhf(z) rounds to +-1, 1 - t^2 is an exact 0
    out["saturated"] = dict(mu=(12.0 * rng.choice([-1.0, 1.0], size=(d, n))).astype(F32), raw=np.ones((d, n), F32), lo=0.05,
                            hi=0.05, K=2)
    lo, hi = F32(0.5), F32(1.25)                   # raw sigma below, at and above both clamp limits (and negative, and +Inf)
    vals = np.array([-1.0, 0.1, nx(lo, F32(0)), lo, nx(lo, F32(1)), 0.8, nx(hi, F32(0)), hi, nx(hi, F32(2)), 3.0, np.inf], F32)
    d, n = 3, 2 * len(vals)
    out["clamp_limits"] = dict(mu=rng.normal(size=(d, n)).astype(F32), raw=rng.permutation(np.tile(vals, 2 * d)).reshape(d, n),
                               lo=float(lo), hi=float(hi), K=2)
    d, n = 5, 21
    out["min_eq_max"] = dict(mu=rng.normal(size=(d, n)).astype(F32), raw=inputs(d, n, 1)[1], lo=0.7, hi=0.7, K=3)
    raw = inputs(d, n, 2)[1]
    raw.reshape(-1)[::8] = np.nan                  # clamp passes a NaN through (reference and clampj): that component's z and
                                                   # action and the state's logp are NaN; states i % 8 in (2, 5, 7) stay clean
    out["nan_sigma"] = dict(mu=rng.normal(size=(d, n)).astype(F32), raw=raw, lo=LO, hi=HI, K=2)
    for d in (1, 3):                               # sigma = 0: s = 1e-8, v = 1e-16 finite at d = 1, prod = 1e-48 -> 0 at d = 3
        out[f"sigma0_d{d}"] = dict(mu=rng.normal(size=(d, 33)).astype(F32), raw=np.zeros((d, 33), F32), lo=0.0, hi=np.inf, K=2)
    d, n = 8, 65                                   # v^8 ~ 1e-42 ... 4e-42: prod is a Float32 subnormal, the reference stays finite
    out["subnormal_prod"] = dict(mu=rng.normal(size=(d, n)).astype(F32), raw=rng.uniform(1e-3, 4e-3, size=(d, n)).astype(F32),
                                 lo=2.4e-3, hi=2.6e-3, K=2)
    return out


def tanh_sweep():
    """mu for `min_sigma = max_sigma = 0` (action = tanhf(mu) exactly): +-0, subnormals, 2^-126 ... 2^4 on a log grid, the Float32
    neighbours of the saturation point, +-Inf, NaN; every finite value with both signs"""
    sat = F32(9.010913)                            # atanh(1 - 2^-25): float64 tanh rounds to 1.0f from about here on
    near = [sat]
    for _ in range(40):
        near = [np.nextafter(near[0], F32(0))] + near + [np.nextafter(near[-1], F32(np.inf))]
    pos = np.concatenate([np.array([0.0, 1e-45, 3e-42, 1e-39, 1.1754942e-38], F32),
                          np.exp2(np.linspace(-126.0, 4.0, 4001)).astype(F32), np.array(near, F32), np.array([np.inf], F32)])
    return np.concatenate([pos, -pos, np.array([np.nan], F32)]).astype(F32)


def check_tanh_sweep(x, t):
    """-> the worst ulp distance from float64 tanh; asserts the bound, odd symmetry, |t| <= 1 and NaN -> NaN"""
    x, t = np.asarray(x, F32), np.asarray(t, F32)
    ul = tanh_ulps(t, x)
    assert ul.max() <= E["tanh"], f"tanhf is {ul.max():.2f} ulps from float64 tanh at x = {x[ul.argmax()]!r} (bound {E['tanh']})"
    fin = ~np.isnan(x)
    assert np.isnan(t[~fin]).all() and not np.isnan(t[fin]).any() and (np.abs(t[fin]) <= 1).all()
    h = (x.size - 1) // 2                           # x = [pos, -pos, NaN]
    # (mu = -0 reaches tanhf as mu + 0 * noise = +-0 by the sign of the draw: the sign is asserted away from 0 only)
    assert np.array_equal(x[:h], -x[h:2 * h]) and np.array_equal(t[:h], -t[h:2 * h])
    assert (np.signbit(t) == np.signbit(x))[fin & (x != 0)].all()
    assert (t[x == np.inf] == 1).all() and (t[x == -np.inf] == -1).all()
    return float(ul.max())


def judge_sampling(family, mu, raw, lo, hi, z, a, lp, tag=""):
    """an implementation's sampled actions a (d, K, n) and log-probabilities lp (K, n) against the model; z is the pre-squash
    sample (the oracle's identity-mode action for the same seed, env_id_base and step)"""
    sg = clamp(raw, lo, hi)
    a, z = np.asarray(a, F32), np.asarray(z, F32)
    res = {}
    if family == "identity":
        assert np.array_equal(a, z, equal_nan=True), f"{tag}: mu + sigma * noise is Float32 arithmetic on the same draws"
        model = gaussian_sample(mu, sg, z)
    else:
        ul = tanh_ulps(a, z)
        res["tanh_ulps"] = float(ul.max())
        assert ul.max() <= E["tanh"], f"{tag}: tanhf is {ul.max():.2f} ulps from float64 tanh (bound {E['tanh']})"
        assert (np.abs(a) <= 1)[~np.isnan(z)].all(), tag
        model = gaussian_sample(mu, sg, z, t=a) if family == "tanh" else soft_sample(mu, sg, z)
    res.update(judge(lp, *model, cap=0.0, tag=tag))
    return res


def judge_eval(family, mu, raw, lo, hi, a, lp, cap, tag=""):
    """(model)(state, action): lp (K, n) for actions a (d, K, n)"""
    sg = clamp(raw, lo, hi)
    model = soft_eval(mu, sg, a) if family == "soft" else gaussian_eval(mu, sg, a, family == "tanh")
    return judge(lp, *model, cap=0.0 if family == "identity" else cap, tag=tag)


# An implementation `impl` (the oracle's binding on the CPU, the device heads on the GPU) offers
#   impl.sample(mu, raw, K, lo, hi, family, seed, env_id_base, step) -> a (d, K, n), lp (K, n)
#   impl.logp(mu, raw, a, lo, hi, family) -> lp (K, n)
# and `ref` is the oracle's: its identity-mode action is the pre-squash sample z, its squashed action the evaluation point.
SEED, BASE, STEP = 11, 5, 4


def run_shape(impl, ref, family, d, n, K, scale=1.0):
    """one shape, sampling and (scale = 1) evaluation on the oracle's sampled actions -> [sampling result, evaluation result].
    The 0.5 % cap is a share: a case of fewer than 200 samples cannot resolve it (one sample is more than the cap), so there the
    left-out samples are only counted -- the caller pools them over all shapes of the family and applies the cap to the pool."""
    mu, raw = inputs(d, n, seed=d, scale=scale)
    tag = f"{family} d={d} n={n} K={K} mu x {scale:g}"
    z, _ = ref.sample(mu, raw, K, LO, HI, "identity", SEED, BASE, STEP)
    a, lp = impl.sample(mu, raw, K, LO, HI, family, SEED, BASE, STEP)
    assert a.shape == (d, K, n) and lp.shape == (K, n)
    out = [judge_sampling(family, mu, raw, LO, HI, z, a, lp, tag="sample " + tag)]
    if scale == 1.0:
        ao, _ = ref.sample(mu, raw, K, LO, HI, family, SEED, BASE, STEP)
        lp2 = impl.logp(mu, raw, ao, LO, HI, family)
        out.append(judge_eval(family, mu, raw, LO, HI, ao, lp2, EVAL_CAP if K * n >= 200 else 1.0, tag="eval " + tag))
    return out


def pooled_left_out(results):
    ev = [r for r in results if r["tag"].startswith("eval")]
    return sum(round(r["left_out"] * r["n"]) for r in ev) / max(1, sum(r["n"] for r in ev))


def run_grid(impl, family):
    """evaluation on |a| = 1 - 2^-e: e <= 12 for GaussianNetwork tanh (beyond, 1 - t^2 is within its own error), e <= 23 for
    SoftGaussianNetwork (well-conditioned in z); nothing may be left out"""
    d, K, n = 4, 3, 23
    mu, raw = inputs(d, n, seed=17)
    a = grid_actions(d, K, n, 12 if family == "tanh" else 23, seed=3)
    return judge_eval(family, mu, raw, LO, HI, a, impl.logp(mu, raw, a, LO, HI, family), 0.0, tag=f"grid {family}")


def run_edge(impl, ref, family, name, case):
    """saturation / sigma edges: sampling for every family; evaluation where it is constrained everywhere (identity; soft unless
    sigma = 0, where dz / 1e-8 leaves a budget of hundreds of nats) and, for `saturated`, the model's non-finite pattern at a = +-1"""
    mu, raw, lo, hi, K = case["mu"], case["raw"], case["lo"], case["hi"], case["K"]
    tag = f"{name} {family}"
    z, _ = ref.sample(mu, raw, K, lo, hi, "identity", SEED, BASE, STEP)
    a, lp = impl.sample(mu, raw, K, lo, hi, family, SEED, BASE, STEP)
    out = [judge_sampling(family, mu, raw, lo, hi, z, a, lp, tag="sample " + tag)]
    bad = np.isnan(raw)[:, None, :] | np.zeros(a.shape, bool)
    assert np.array_equal(np.isnan(a), bad) and np.array_equal(np.isnan(lp), bad.any(0)), tag
    if name == "saturated":
        if family != "identity":
            assert np.array_equal(a, np.sign(mu)[:, None, :] * np.ones_like(a)), tag
        assert (lp == np.inf).all() if family == "tanh" else np.isfinite(lp).all(), tag
    if name == "sigma0_d1":
        assert np.isfinite(lp).all(), tag
    if name == "sigma0_d3":
        assert np.isfinite(lp).all() if family == "soft" else (lp == np.inf).all(), tag
    if name == "subnormal_prod":
        v = (clamp(raw, lo, hi) + EPS) ** 2
        p = np.multiply.reduce(v, axis=0, dtype=F32)           # (order-free check of the case itself; the model replays in order)
        assert ((p > 0) & (p < F32(2.0 ** -126))).all() and np.isfinite(lp).all(), tag
    if name == "saturated" or family == "identity" or (family == "soft" and not name.startswith("sigma0")):
        ao, _ = ref.sample(mu, raw, K, lo, hi, family, SEED, BASE, STEP)
        lp2 = impl.logp(mu, raw, ao, lo, hi, family)
        out.append(judge_eval(family, mu, raw, lo, hi, ao, lp2, 0.0, tag="eval " + tag))
        if name == "saturated" and family != "identity":
            assert np.isnan(lp2).all(), tag                   # atanh(+-1) = +-Inf: -Inf from the density, +Inf from the correction
    return out


def judge(got, expected, budget, left, cap=0.0, tag=""):
    """assert `got` against the model and return what was measured: the non-finite pattern matches exactly, every finite sample
    that is not left out lies within 2 x budget, and at most `cap` of the samples are left out"""
    got, expected = np.asarray(got, F64), np.asarray(expected, F64)
    assert got.shape == expected.shape, (tag, got.shape, expected.shape)
    fin = np.isfinite(expected)
    share = float(left.mean())
    assert share <= cap, f"{tag}: {left.sum()} of {left.size} samples left out ({share:.4%} > cap {cap:.2%})"
    keep = fin & ~left
    assert np.isfinite(budget[keep]).all() and (budget[keep] > 0).all(), tag
    # where the model is not finite and the sample is constrained: the same Inf (with its sign) or NaN
    nf = ~fin & ~left
    same = np.where(np.isnan(expected), np.isnan(got), got == expected)
    assert same[nf].all(), f"{tag}: non-finite pattern differs at {int((~same & nf).sum())} samples"
    assert np.isfinite(got[keep]).all(), f"{tag}: {int((~np.isfinite(got[keep])).sum())} non-finite outputs where the model is finite"
    ratio = np.abs(got[keep] - expected[keep]) / (2.0 * budget[keep])
    worst = float(ratio.max()) if ratio.size else 0.0
    res = {"tag": tag, "worst_over_bar": worst, "median_budget": float(np.median(budget[keep])) if ratio.size else 0.0,
           "left_out": share, "non_finite": int(nf.sum()), "n": int(got.size)}
    assert worst <= 1.0, f"{tag}: |got - model| reaches {worst:.3g} x the bar (2 x budget) at {int((ratio > 1).sum())} samples"
    return res
