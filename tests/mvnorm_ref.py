"""CovGaussianNetwork, mvnormlogpdf and the Gaussian KL divergences (csrc/cov_heads.hip) as a float64 model with a per-sample error
budget (plain numpy; no oracle, no GPU).  Built on `Q` (with its `E` and `ulp`) and `judge` of tests/heads_ref.py; the bar stays 2 x budget and a
non-finite expected value must be matched exactly in pattern.  Nothing is left out (cap 0 everywhere).

The kernels' + - * / are correctly rounded Float32 operations in the order include/rlhip.h states, so on exact Float32 operands they
are replayed bit for bit (`Q` with e == 0 computes in Float32); only expf / logf carry a budget (the OpenCL ulp bounds of `E`).
Everything downstream of vec_to_tril takes the implementation's own L as an exact input -- the head entry points return L_out for that
reason -- and L itself is judged by `judge_tril`: the diagonal against float64 softplusbeta + 1e-5 within the propagated expf / logf
budget, the entries below the diagonal and the zeros above it bit for bit.

Two refinements of `Q` that the diagonal needs:
  * expf beyond the Float32 range is +Inf exactly (`_f32_range`)
  * `expf(x / 10) + 1.0f`: the sum is ROUNDED to Float32.  Where every value the operand may take (c - e ... c + e) gives the same
    Float32 sum, the sum is that Float32 exactly and the error is gone (rounding is monotonic).  That is what makes the naive form
    distinguishable from a log1p form at x = -200 (sum = 1.0f exactly, logf(1.0f) = 0, diagonal = 1e-5f exactly) -- `_plus_one`.

Array shapes are the reference's: mu (da, n), chol_vec (nv, n), L (da, da, n), x / actions (da, K, n) or (da, n), logp (K, n) or (n,).
Shared by tests/test_mvnorm_reference.py (CPU: closed forms, planted faults) and tests/test_gpu_cov_heads.py."""
import numpy as np

from heads_ref import F32, F64, LOG2PI, Q, judge

BETA = F32(10.0)
FLOOR = F32(1.0e-5)
RTOL = float(np.sqrt(np.finfo(F32).eps))      # Julia's `≈` default for Float32: rtol = sqrt(eps(Float32))


def tril_index(i, j, da):
    """cholesky_matrix_to_vector_index(i, j, da), 1-based (networks.jl:359)"""
    return ((2 * da - j) * (j - 1)) // 2 + i


def nvec(da):
    return da * (da + 1) // 2


def _zero(shape):
    return Q(np.zeros(shape, F32))


def _f32_range(q):
    """a centre beyond the Float32 range is +-Inf exactly"""
    with np.errstate(all="ignore"):
        c32 = q.c.astype(F32).astype(F64)
    over = np.isinf(c32) & np.isfinite(q.c)
    return Q(np.where(over, c32, q.c), np.where(over, 0.0, q.e))


def _plus_one(q):
    s = q + F32(1.0)
    with np.errstate(all="ignore"):
        lo, hi = ((q.c - q.e) + 1.0).astype(F32), ((q.c + q.e) + 1.0).astype(F32)
    same = lo == hi
    return Q(np.where(same, lo.astype(F64), s.c), np.where(same, 0.0, s.e))


def softplusbeta(x):
    """logf(expf(x / 10.0f) + 1.0f) * 10.0f (networks.jl:360) of exact Float32 x -> Q"""
    return _plus_one(_f32_range((Q(np.asarray(x, F32)) / BETA).libm("exp"))).libm("log") * BETA


def chol_diag(x):
    return softplusbeta(x) + FLOOR


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, F32)).view(np.uint32)


def judge_tril(L, chol_vec, tag=""):
    """an implementation's L (da, da, n) for chol_vec (nv, n) -> what `judge` measured on the diagonal"""
    L, v = np.asarray(L, F32), np.asarray(chol_vec, F32)
    da = L.shape[0]
    assert L.shape == (da, da, v.shape[1]) and v.shape[0] == nvec(da), (tag, L.shape, v.shape)
    for i in range(1, da + 1):
        for j in range(1, da + 1):
            got = L[i - 1, j - 1]
            if i > j:
                want = v[tril_index(i, j, da) - 1]
                assert np.array_equal(_bits(got), _bits(want)), f"{tag}: L[{i},{j}] is not vector element {tril_index(i, j, da)} bit for bit"
            elif i < j:
                assert not _bits(got).any(), f"{tag}: L[{i},{j}] above the diagonal is not +0"
    dg = chol_diag(np.stack([v[tril_index(i, i, da) - 1] for i in range(1, da + 1)]))
    got = np.stack([L[i, i] for i in range(da)])
    return judge(got, dg.c, dg.e, np.zeros(dg.c.shape, bool), cap=0.0, tag=f"{tag} diagonal")


def sample_replay(mu, L, eps):
    """z = mu + L eps in the stated order, numpy Float32 (bit for bit): mu (da, n), L (da, da, n), eps (da, K, n) -> (da, K, n)"""
    mu, L, eps = np.asarray(mu, F32), np.asarray(L, F32), np.asarray(eps, F32)
    z = np.empty_like(eps)
    with np.errstate(all="ignore"):
        for i in range(mu.shape[0]):
            acc = L[i, 0][None, :] * eps[0]
            for j in range(1, i + 1):
                acc = acc + L[i, j][None, :] * eps[j]
            z[i] = mu[i][None, :] + acc
    return z


def _rows(L, r, c, like):
    a = np.asarray(L, F32)[r, c]
    return Q(a[None, :] if like == 2 else a)


def _solve_sq(L, t, frm, ss, nd):
    """t (a list of Q rows) := L \\ t from row `frm` on; -> ss + the squares of the solved rows, ascending"""
    da = len(t)
    for c in range(frm, da):
        y = t[c] / _rows(L, c, c, nd)
        ss = ss + y * y
        for r in range(c + 1, da):
            t[r] = t[r] - _rows(L, r, c, nd) * y
    return ss


def _sum_log_diag(L):
    L = np.asarray(L, F32)
    ld = _zero(L.shape[2:])
    for c in range(L.shape[0]):
        ld = ld + Q(L[c, c]).libm("log")
    return ld


def _out(q):
    return q.c, q.e, np.zeros(q.c.shape, bool)


def _mvnormlogpdf(mu, L, x, order=range, logdet_factor=2):
    mu, x = np.asarray(mu, F32), np.asarray(x, F32)
    da, nd = mu.shape[0], x.ndim - 1
    m = mu[:, None, :] if nd == 2 else mu
    t = [Q(x[r]) - Q(m[r]) for r in range(da)]
    if order is range:
        ss = _solve_sq(L, t, 0, _zero(x.shape[1:]), nd)
    else:                                      # (a planted fault: the squares summed in another order)
        ys = []
        for c in range(da):
            y = t[c] / _rows(L, c, c, nd)
            ys.append(y * y)
            for r in range(c + 1, da):
                t[r] = t[r] - _rows(L, r, c, nd) * y
        ss = _zero(x.shape[1:])
        for c in order(da):
            ss = ss + ys[c]
    logdet = _sum_log_diag(L).scale(logdet_factor)
    return ((Q(F32(da)) * LOG2PI + logdet) + ss).scale(-0.5)


def mvnormlogpdf(mu, L, x):
    """mvnormlogpdf(mu, L, x) (distributions.jl:46-66): x (da, K, n) -> (K, n), x (da, n) -> (n,); expected, budget, left"""
    return _out(_mvnormlogpdf(mu, L, x))


def mvnormkldivergence(mu1, L1, mu2, L2):
    """mvnormkldivergence (distributions.jl:88-109) in the closed form of include/rlhip.h -> (n,)"""
    mu1, mu2, L1 = np.asarray(mu1, F32), np.asarray(mu2, F32), np.asarray(L1, F32)
    da, n = mu1.shape
    logdet = _sum_log_diag(L2).scale(2) - _sum_log_diag(L1).scale(2)
    trace = _zero((n,))
    for c in range(da):
        t = [Q(L1[r, c]) if r >= c else None for r in range(da)]
        trace = _solve_sq(L2, t, c, trace, 1)
    t = [Q(mu2[r]) - Q(mu1[r]) for r in range(da)]
    sq = _solve_sq(L2, t, 0, _zero((n,)), 1)
    return _out((((logdet - F32(da)) + trace) + sq).scale(0.5))


def diagnormkldivergence(mu1, s1, mu2, s2):
    """diagnormkldivergence (distributions.jl:117-124) over dims = 1 of (d, n) arrays -> (n,)"""
    mu1, s1, mu2, s2 = (np.asarray(a, F32) for a in (mu1, s1, mu2, s2))
    d, n = mu1.shape
    l1, l2, trace, sq = _zero((n,)), _zero((n,)), _zero((n,)), _zero((n,))
    for k in range(d):
        a, b, dm = Q(s1[k]), Q(s2[k]), Q(mu2[k]) - Q(mu1[k])
        v1, v2 = a * a, b * b
        l2 = l2 + v2.libm("log")
        l1 = l1 + v1.libm("log")
        trace = trace + v1 / v2
        sq = sq + (dm * dm) / v2
    return _out(((((l2 - l1) - F32(d)) + trace) + sq).scale(0.5))


def normkldivergence(mu1, s1, mu2, s2):
    """normkldivergence (distributions.jl:137-139) elementwise"""
    a, b = Q(np.asarray(s1, F32)), Q(np.asarray(s2, F32))
    dm = Q(np.asarray(mu1, F32)) - Q(np.asarray(mu2, F32))
    return _out(((b.libm("log") - a.libm("log")) + (a * a + dm * dm) / (Q(F32(2.0)) * (b * b))) - F32(0.5))


# ------------------------------------------------------------------------------------------------ float64 closed forms (the golden cases)
def normal_logpdf64(mu, s, x):
    return -0.5 * (((x - mu) / s) ** 2 + np.log(2 * np.pi)) - np.log(s)


def normal_kl64(mu1, s1, mu2, s2):
    return np.log(s2 / s1) + (s1 * s1 + (mu1 - mu2) ** 2) / (2 * s2 * s2) - 0.5


def mvnormal_logpdf64(mu, S, x):
    mu, S, x = (np.asarray(a, F64) for a in (mu, S, x))
    dx = x - mu
    return -0.5 * (mu.size * np.log(2 * np.pi) + np.linalg.slogdet(S)[1] + dx @ np.linalg.solve(S, dx))


def mvnormal_kl64(mu1, S1, mu2, S2):
    mu1, S1, mu2, S2 = (np.asarray(a, F64) for a in (mu1, S1, mu2, S2))
    dm = mu2 - mu1
    return 0.5 * (np.trace(np.linalg.solve(S2, S1)) + dm @ np.linalg.solve(S2, dm) - mu1.size
                  + np.linalg.slogdet(S2)[1] - np.linalg.slogdet(S1)[1])


def approx(a, b):
    """Julia's isapprox with the Float32 default: |a - b| <= sqrt(eps(Float32)) max(|a|, |b|)"""
    a, b = np.asarray(a, F64), np.asarray(b, F64)
    return bool((np.abs(a - b) <= RTOL * np.maximum(np.abs(a), np.abs(b))).all())


# ------------------------------------------------------------------------------------------------ the cases both suites run
# (da, n, K): the golden shape; one lane in a second block; odd da with odd K (a Philox pair straddles two samples); the reference's
# own shape; da = 16; one state across two blocks; more than 16 blocks at K = 1
SHAPES = [(2, 2, 1), (1, 257, 1), (3, 700, 4), (5, 33, 3), (10, 3, 5), (16, 17, 2), (16, 1, 300), (7, 4099, 1)]
SEED, BASE, STEP = 11, 5, 4


def inputs(da, n, seed=0):
    """mu and chol_vec unit-normal: the diagonals sit near 5 ... 9, every case is well-conditioned"""
    rng = np.random.default_rng(1000 + seed)
    return rng.normal(size=(da, n)).astype(F32), rng.normal(size=(nvec(da), n)).astype(F32)


def edge_vectors():
    """da = 3, n = 40: diagonal inputs in {-1000, -200, 0, 880, 900, NaN}, an Inf and a NaN below the diagonal"""
    da, n = 3, 40
    rng = np.random.default_rng(7)
    mu, vec = rng.normal(size=(da, n)).astype(F32), rng.normal(size=(nvec(da), n)).astype(F32)
    vals = np.array([-1000.0, -200.0, 0.0, 880.0, 900.0, np.nan], F32)
    for s in range(18):                        # state s: diagonal (s % 3) takes value vals[s // 3]
        vec[tril_index(s % 3 + 1, s % 3 + 1, da) - 1, s] = vals[s // 3]
    vec[tril_index(2, 1, da) - 1, 20] = np.inf
    vec[tril_index(3, 2, da) - 1, 21] = -np.inf
    vec[tril_index(3, 1, da) - 1, 22] = np.nan
    return mu, vec
