"""The pullbacks of csrc/cov_heads_grad.hip as a numpy model (plain numpy; no oracle, no GPU), in the reference's shapes: mu (da, n),
chol_vec (nv, n), L / dL (da, da, n), x / dx (da, K, n), dlogp (K, n), KL cotangents (n,).

Apart from one expf every operation of the kernels is a correctly rounded Float32 + - * / in the order include/rlhip.h states, so the
expected values are an exact numpy-Float32 replay and are compared bit for bit, the +-0 and the non-finite patterns included
(`same`; a NaN matches a NaN).  The expf sits in the derivative of softplusbeta on the diagonal of the vec_to_tril pullback,
dvec = dL[c,c] * (1.0f / (1.0f + expf(-(v / 10.0f)))): that factor is carried as a `Q` of tests/heads_ref.py (OpenCL ulp bound of expf,
first-order propagation, the `_f32_range` / `_plus_one` refinements of tests/mvnorm_ref.py) and the diagonal of dvec is judged at the
project's bar of 2 x budget with cap 0 (`judge_dvec`); where the factor is exact (expf overflowed: 1 / Inf = 0; expf vanished: 1 / 1 = 1)
the diagonal is bit for bit as well.  The fused head pullback takes the implementation's own L as an exact input, as the forward suite does.

Every function takes keyword switches that plant a fault; tests/test_mvnorm_grad_reference.py shows that each one is caught.
Shared by tests/test_mvnorm_grad_reference.py (CPU) and tests/test_gpu_cov_heads_grad.py."""
import numpy as np

import mvnorm_ref as M
from heads_ref import F32, F64, Q, judge

ONE = F32(1.0)


def _f(a):
    return np.ascontiguousarray(np.asarray(a, F32))


def same(a, b):
    """bit for bit, +-0 included; a NaN matches a NaN (the payload of a NaN that arithmetic produced is the platform's)"""
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    ok = ~np.isnan(a)
    return np.array_equal(M._bits(a)[ok], M._bits(b)[ok])


def _solve(L, t, frm=0):
    """t (a list of Float32 arrays) := L \\ t from row `frm` on: row i takes t = t - L[i,j] y[j] in ascending j, then y[i] = t / L[i,i]"""
    da = len(t)
    for c in range(frm, da):
        t[c] = t[c] / L[c][c]
        for r in range(c + 1, da):
            t[r] = t[r] - L[r][c] * t[c]
    return t


def _solve_t(L, t):
    """t := L^T \\ t: columns c = da ... 1: u[c] = t[c] / L[c,c], then t[r] = t[r] - L[c,r] u[c] for r < c"""
    for c in range(len(t) - 1, -1, -1):
        t[c] = t[c] / L[c][c]
        for r in range(c):
            t[r] = t[r] - L[c][r] * t[c]
    return t


def _rows(L, lead=None):
    """L (da, da, n) -> L[r][c] as (n,) arrays, or (1, n) to broadcast against (K, n)"""
    L = _f(L)
    return [[L[r, c] if lead is None else L[r, c][None, :] for c in range(L.shape[1])] for r in range(L.shape[0])]


def mvnormlogpdf_bwd(mu, L, x, g, descending_k=False, drop_gs=False, full_outer=False):
    """-> dmu (da, n), dL (da, da, n), dx (da, K, n): exact Float32"""
    mu, x, g = _f(mu), _f(x), _f(g)
    flat = x.ndim == 2
    if flat:
        x, g = x[:, None, :], g[None, :]
    da, K, n = x.shape
    Lr, Ln = _rows(L, lead=1), _rows(L)
    with np.errstate(all="ignore"):
        y = _solve(Lr, [x[r] - mu[r][None, :] for r in range(da)])
        u = _solve_t(Lr, list(y))
        gu = [g * u[r] for r in range(da)]
        dx = np.stack([-gu[r] for r in range(da)])
        zero = np.zeros(n, F32)
        dmu = [zero.copy() for _ in range(da)]
        S = [[zero.copy() for _ in range(da)] for _ in range(da)]
        gs = zero.copy()
        for k in (range(K - 1, -1, -1) if descending_k else range(K)):
            for r in range(da):
                dmu[r] = dmu[r] + gu[r][k]
                for c in range(da if full_outer else r + 1):
                    S[r][c] = S[r][c] + gu[r][k] * y[c][k]
            gs = gs + g[k]
        if not drop_gs:
            for c in range(da):
                S[c][c] = S[c][c] - gs / Ln[c][c]
    return np.stack(dmu), np.stack([np.stack(row) for row in S]), (dx[:, 0, :] if flat else dx)


def softplusbeta_grad(v):
    """1.0f / (1.0f + expf(-(v / 10.0f))) of exact Float32 v -> Q"""
    e = M._f32_range((Q(np.asarray(v, F32)) / M.BETA).scale(-1).libm("exp"))
    return Q(np.full(np.shape(v), ONE)) / M._plus_one(e)


def vec_to_tril_bwd(vec, dL, sigmoid_one=False):
    """-> centre (nv, n) float64 and error bound (nv, n): 0 wherever the value is an exact Float32 (everything below the diagonal)"""
    vec, dL = _f(vec), _f(dL)
    da = dL.shape[0]
    c, e = np.zeros(vec.shape, F64), np.zeros(vec.shape, F64)
    with np.errstate(all="ignore"):
        for i in range(1, da + 1):
            for j in range(1, i + 1):
                at = M.tril_index(i, j, da) - 1
                if i > j:
                    c[at] = dL[i - 1, j - 1]
                else:
                    q = Q(dL[i - 1, j - 1]) * (Q(np.full(vec.shape[1], ONE)) if sigmoid_one else softplusbeta_grad(vec[at]))
                    c[at], e[at] = q.c, q.e
    return c, e


def judge_dvec(got, c, e, tag=""):
    """an implementation's dvec against `vec_to_tril_bwd`: bit for bit where the model is exact, else within 2 x budget (cap 0)"""
    got = np.asarray(got, F32)
    assert got.shape == c.shape, (tag, got.shape, c.shape)
    exact = e == 0
    assert same(got[exact], c[exact].astype(F32)), f"{tag}: an exact element of dvec differs"
    rest = ~exact
    if not rest.any():
        return {"tag": tag, "worst_over_bar": 0.0, "n": 0}
    return judge(got[rest], c[rest], e[rest], np.zeros(int(rest.sum()), bool), cap=0.0, tag=tag)


def head_logp_bwd(mu, vec, L, a, g, **faults):
    """(model)(state, action) pulled back onto mu and the Cholesky vector, L the implementation's own -> dmu, (centre, error) of dvec"""
    sig = faults.pop("sigmoid_one", False)
    dmu, dL, _ = mvnormlogpdf_bwd(mu, L, a, g, **faults)
    return dmu, vec_to_tril_bwd(vec, dL, sigmoid_one=sig)


def mvnormkl_bwd(mu1, L1, mu2, L2, g, drop_pa=False):
    """-> dmu1, dL1, dmu2, dL2: exact Float32"""
    mu1, mu2, L1, g = _f(mu1), _f(mu2), _f(L1), _f(g)
    da, n = mu1.shape
    R2 = _rows(L2)
    zero = np.zeros(n, F32)
    with np.errstate(all="ignore"):
        m = _solve(R2, [mu2[r] - mu1[r] for r in range(da)])
        q = _solve_t(R2, list(m))
        dmu2 = np.stack([g * q[r] for r in range(da)])
        dmu1 = np.stack([-(g * q[r]) for r in range(da)])
        W = [[q[r] * m[j] if r >= j else None for j in range(da)] for r in range(da)]
        dL1 = np.zeros((da, da, n), F32)
        for c in range(da):
            a = _solve(R2, [L1[r, c] if r >= c else zero.copy() for r in range(da)], frm=c)
            p = _solve_t(R2, list(a))
            for r in range(c, da):
                dL1[r, c] = g * p[r] if r > c else g * (p[c] - ONE / L1[c, c])
            if not drop_pa:
                for j in range(c, da):
                    for r in range(j, da):
                        W[r][j] = W[r][j] + p[r] * a[j]
        dL2 = np.zeros((da, da, n), F32)
        for j in range(da):
            for r in range(j, da):
                dL2[r, j] = g * (-W[r][j]) if r > j else g * (ONE / R2[j][j] - W[j][j])
    return dmu1, dL1, dmu2, dL2


def diagnormkl_bwd(mu1, s1, mu2, s2, g):
    """(d, n) arguments, g (n,) -> dmu1, ds1, dmu2, ds2: exact Float32"""
    mu1, a, mu2, b, g = _f(mu1), _f(s1), _f(mu2), _f(s2), _f(g)[None, :]
    with np.errstate(all="ignore"):
        dm = mu2 - mu1
        v1, v2 = a * a, b * b
        w = dm / v2
        return -(g * w), g * (a / v2 - ONE / a), g * w, g * (ONE / b - (v1 + dm * dm) / (v2 * b))


def normkl_bwd(mu1, s1, mu2, s2, g):
    """elementwise -> dmu1, ds1, dmu2, ds2: exact Float32"""
    mu1, a, mu2, b, g = _f(mu1), _f(s1), _f(mu2), _f(s2), _f(g)
    with np.errstate(all="ignore"):
        dm = mu1 - mu2
        v2 = b * b
        w = dm / v2
        return g * w, g * (a / v2 - ONE / a), -(g * w), g * (ONE / b - (a * a + dm * dm) / (v2 * b))


def approx_tensor(a, b):
    """Julia's array `≈` with the Float32 default: |a - b|_2 <= sqrt(eps(Float32)) max(|a|_2, |b|_2) over the whole tensor"""
    a, b = np.asarray(a, F64).ravel(), np.asarray(b, F64).ravel()
    return bool(np.linalg.norm(a - b) <= M.RTOL * max(np.linalg.norm(a), np.linalg.norm(b)))


def cotangent(shape, seed):
    """a unit-normal cotangent: every output is weighted differently, both signs"""
    return np.random.default_rng(5000 + seed).normal(size=shape).astype(F32)
