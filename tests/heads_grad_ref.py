"""The pullbacks of csrc/heads_grad.hip as a numpy model (plain numpy; no oracle, no GPU), in the reference's shapes: mu, raw_sigma and
both gradients (d, n), actions / draws / dact (d, K, n), dlogp (K, n).

Every + - * / of the kernels is a correctly rounded Float32 operation in the order include/rlhip.h states (-ffp-contract=off), so
  * normlogpdf_bwd, diagnormlogpdf_bwd, the sampling pullbacks (`sample_bwd`) and the identity-squash evaluation pullback are exact
    numpy-Float32 replays, compared bit for bit, the +-0 and the non-finite patterns included (`same`).  The draws eps are an input:
    the forward entry's own actions at mu = 0, raw_sigma = 1, min = max = 1, identity squash (0 + 1 * eps is exact; `draws`), and
    t = tanhf(z) is the forward entry's own SoftGaussianNetwork action at the same (seed, env_id_base, step): exact inputs, as the
    Cov suite takes the implementation's own L.
  * the evaluation pullbacks with squash = 1 or soft = 1 contain one unobservable libm call, z = atanhf(a).  They are carried as `Q`s of
    tests/heads_ref.py (E["atanh"] ulp, first-order propagation) and judged at the project's bar of 2 x budget; no sample is left out (these
    formulas have no log(1 - t^2) singularity).  Where the expected value is not finite (a = +-1) the pattern must match exactly.
`logp_bwd` is written on Qs for all three families: on exact operands a Q operation IS the Float32 operation with error 0, so the identity
family comes out exact (`judge_grad` compares an element with budget 0 bit for bit).

Every function takes keyword switches that plant a fault; tests/test_heads_grad_reference.py shows that each one is caught.
Shared by tests/test_heads_grad_reference.py (CPU) and tests/test_gpu_heads_grad.py."""
import numpy as np

from heads_ref import EPS, F32, F64, Q, SQUASH_SOFT, clamp
from mvnorm_grad_ref import cotangent, same  # noqa: F401  (re-exported: the suites use G.same / G.cotangent)

ONE, TWO, ZERO = F32(1.0), F32(2.0), F32(0.0)


def _f(a):
    return np.ascontiguousarray(np.asarray(a, F32))


def passes(raw, lo, hi, strict=False):
    """the reference's clamp rule: the cotangent passes where !(raw > hi) && !(raw < lo) -- inclusive bounds, and a NaN passes"""
    raw = _f(raw)
    with np.errstate(invalid="ignore"):
        if strict:                                  # FAULT: a gradient is lost at raw == lo and raw == hi
            return ~(raw >= F32(hi)) & ~(raw <= F32(lo))
        return ~(raw > F32(hi)) & ~(raw < F32(lo))


def _select(dsg, ok, product=False):
    """draw_sigma = pass ? dsg : +0 on Float32 arrays.  FAULT `product`: dsg * pass, which leaks a NaN / Inf and gives -0"""
    with np.errstate(all="ignore"):
        return (dsg * ok.astype(F32)).astype(F32) if product else np.where(ok, dsg, ZERO).astype(F32)


def _sum_j(terms, descending=False):
    """0 + sum over the K samples (axis 1 of (d, K, n)) in ascending j, sequentially.  FAULT `descending`"""
    K = terms.shape[1]
    acc = np.zeros((terms.shape[0], terms.shape[2]), F32)
    with np.errstate(all="ignore"):
        for j in (range(K - 1, -1, -1) if descending else range(K)):
            acc = acc + terms[:, j, :]
    return acc


def normlogpdf_bwd(mu, sigma, x, g):
    """elementwise -> dmu, dsigma, dx"""
    mu, sigma, x, g = _f(mu), _f(sigma), _f(x), _f(g)
    with np.errstate(all="ignore"):
        s = sigma + EPS
        z = (x - mu) / s
        w = z / s
        return g * w, g * ((z * z - ONE) / s), -(g * w)


def diagnormlogpdf_bwd(mu, sigma, x, g):
    """(d, n) arrays, g (n,) -> dmu, dsigma, dx"""
    mu, sigma, x, g = _f(mu), _f(sigma), _f(x), _f(g)[None, :]
    with np.errstate(all="ignore"):
        s = sigma + EPS
        v = s * s
        e = x - mu
        w = e / v
        return g * w, g * (((e * e) / v - ONE) / s), -(g * w)


def logp_bwd(family, mu, raw, a, g, lo, hi, descending=False, strict_pass=False, clamp_product=False):
    """the pullback of (model)(state, action) -> (centre, error) of dmu and of draw_sigma, each (d, n); error 0 = an exact replay"""
    squash, soft = SQUASH_SOFT[family]
    mu, raw, a, g = _f(mu), _f(raw), _f(a), _f(g)
    d, K, n = a.shape
    with np.errstate(all="ignore"):
        s = Q(clamp(raw, lo, hi) + EPS)
    m = Q(mu)
    z = Q(a).libm("atanh") if (squash or soft) else Q(a)
    am, asg = Q(np.zeros((d, n), F32)), Q(np.zeros((d, n), F32))
    for j in (range(K - 1, -1, -1) if descending else range(K)):
        zj, gj = Q(z.c[:, j], z.e[:, j]), Q(g[j][None, :])
        if soft:
            zz = (zj - m) / s
            tm, ts = gj * (zz / s), gj * ((zz * zz - ONE) / s)
        else:
            e, v = zj - m, s * s
            tm, ts = gj * (e / v), gj * (((e * e) / v - ONE) / s)
        am, asg = am + tm, asg + ts
    ok = passes(raw, lo, hi, strict_pass)
    with np.errstate(all="ignore"):
        if clamp_product:
            return (am.c, am.e), (asg.c * ok, asg.e * ok)
        return (am.c, am.e), (np.where(ok, asg.c, 0.0), np.where(ok, asg.e, 0.0))


def sample_bwd(family, mu, raw, eps, lo, hi, g=None, dact=None, t=None, descending=False, strict_pass=False, clamp_product=False,
               drop_dz_eps=False, unsquashed_correction=False, dact_without_jacobian=False):
    """the pullback of the sampling calls -> dmu, draw_sigma (d, n), exact.  eps (d, K, n): the regenerated draws; g (K, n) or None;
    soft: t = the forward's own tanhf(z) (d, K, n), dact (d, K, n) or None"""
    squash, soft = SQUASH_SOFT[family]
    mu, raw, eps = _f(mu), _f(raw), _f(eps)
    g3 = None if g is None else _f(g)[None, :, :]
    with np.errstate(all="ignore"):
        sg = clamp(raw, lo, hi)
        m3, sg3, s3 = mu[:, None, :], sg[:, None, :], (sg + EPS)[:, None, :]
        z = m3 + sg3 * eps
        if not soft:
            assert dact is None and g3 is not None, "a GaussianNetwork's actions carry no gradient; dlogp is required"
            e, v = z - m3, s3 * s3
            tm, ts = g3 * (e / v), g3 * (((e * e) / v - ONE) / s3)
        else:
            assert t is not None and (g3 is not None or dact is not None)
            t = _f(t)
            zz = (z - m3) / s3
            w = zz / s3
            dz = np.zeros(z.shape, F32)
            if g3 is not None:
                dz = g3 * ((TWO * z if unsquashed_correction else TWO * t) - w)     # FAULT: 2 z, the correction without the squash
            if dact is not None:
                dz = dz + _f(dact) * (ONE if dact_without_jacobian else (ONE - t * t))
            tm = (g3 * w if g3 is not None else ZERO) + dz
            ts = (g3 * ((zz * zz - ONE) / s3) if g3 is not None else ZERO) + (np.zeros_like(dz) if drop_dz_eps else dz * eps)
    return _sum_j(tm.astype(F32), descending), _select(_sum_j(ts.astype(F32), descending), passes(raw, lo, hi, strict_pass), clamp_product)


def draws(sample, d, n, K, seed, base, step):
    """randn(rng, Float32, d, K, n) of the shared stream from an implementation's UNCHANGED forward entry: mu = 0, sigma clamped to
    exactly 1, identity squash, so z = 0 + 1 * eps = eps.  `sample` has the signature of tests/heads_ref.py's `impl.sample`"""
    a, _ = sample(np.zeros((d, n), F32), np.ones((d, n), F32), K, 1.0, 1.0, "identity", seed, base, step)
    return _f(a)


def misindexed(eps):
    """FAULT: the draws as a kernel would regenerate them with the index j + K k in place of k + d j"""
    d, K, n = eps.shape
    flat = eps.transpose(1, 0, 2).reshape(K * d, n)             # flat[k + d j] = eps[k, j]
    return np.ascontiguousarray(flat.reshape(d, K, n))          # [k, j] = flat[j + K k]


def judge_grad(got, c, e, tag=""):
    """an implementation's gradient against a (centre, error) pair: where the model is not finite the same Inf (with its sign) or
    NaN; where its error is 0 bit for bit (+-0 included); elsewhere within 2 x budget.  Nothing is left out."""
    got, c, e = np.asarray(got, F32), np.asarray(c, F64), np.asarray(e, F64)
    assert got.shape == c.shape, (tag, got.shape, c.shape)
    fin = np.isfinite(c)
    with np.errstate(invalid="ignore"):
        nf_same = np.where(np.isnan(c), np.isnan(got), got.astype(F64) == c)
    assert nf_same[~fin].all(), f"{tag}: non-finite pattern differs at {int((~nf_same & ~fin).sum())} elements"
    exact = fin & (e == 0)
    assert same(got[exact], c[exact].astype(F32)), f"{tag}: {int((got[exact] != c[exact].astype(F32)).sum())} exact elements differ"
    rest = fin & ~exact
    res = {"tag": tag, "n": int(got.size), "exact": int(exact.sum()), "non_finite": int((~fin).sum()), "worst_over_bar": 0.0,
           "median_budget": 0.0}
    if rest.any():
        assert np.isfinite(e[rest]).all() and (e[rest] > 0).all(), f"{tag}: an unconstrained element"
        assert np.isfinite(got[rest]).all(), f"{tag}: non-finite outputs where the model is finite"
        ratio = np.abs(got[rest].astype(F64) - c[rest]) / (2.0 * e[rest])
        res["worst_over_bar"], res["median_budget"] = float(ratio.max()), float(np.median(e[rest]))
        assert ratio.max() <= 1.0, f"{tag}: |got - model| reaches {ratio.max():.3g} x the bar (2 x budget) at {int((ratio > 1).sum())} elements"
    return res


def approx(a, b, rtol=1e-5):
    """relative 1e-5 over the whole tensor (2-norm), the comparison with float64 autograd on Float32 inputs: the Float32 replay's own
    rounding is 6e-8 per operation, and a single element of a sum that cancels is not constrained by a relative bound of its own"""
    a, b = np.asarray(a, F64).ravel(), np.asarray(b, F64).ravel()
    return bool(np.linalg.norm(a - b) <= rtol * max(np.linalg.norm(a), np.linalg.norm(b)))
