"""CovGaussianNetwork, mvnormlogpdf and the Gaussian KL kernels on the device (csrc/cov_heads.hip) against the float64 model with a
derived error budget (tests/mvnorm_ref.py), through the C ABI and the Python host."""
import json
import os

import numpy as np
import pytest
import torch

import mvnorm_ref as M
from heads_ref import F32, F64, judge

pytestmark = pytest.mark.gpu
KAT = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "mvnorm_kat.json")))


@pytest.fixture(scope="module")
def dev():
    import rlhip  # noqa: F401
    return Device()


def _same(a, b):
    """bit for bit; a NaN matches a NaN (the payload of a NaN that arithmetic produced is the platform's)"""
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    ok = ~np.isnan(a)
    return np.array_equal(M._bits(a)[ok], M._bits(b)[ok])


class Device:
    """the entry points of csrc/cov_heads.hip on numpy arrays in the reference's shapes (mu (da, n), chol_vec (nv, n), L (da, da, n),
    actions (da, K, n), logp (K, n)); the storage handed to the library is the column-major array"""

    def __init__(self):
        from rlhip._lib import call
        from rlhip.ops import ptr, stream_ptr

        self.call, self.ptr, self.sp = call, ptr, stream_ptr

    @staticmethod
    def up(a):
        """Julia-shaped numpy array -> device tensor holding its column-major storage"""
        a = np.asarray(a, F32)
        return torch.tensor(np.ascontiguousarray(a.transpose(*range(a.ndim - 1, -1, -1))), device="cuda")

    @staticmethod
    def down(t):
        a = t.cpu().numpy()
        return np.ascontiguousarray(a.transpose(*range(a.ndim - 1, -1, -1)))

    def empty(self, *shape):
        return torch.empty(shape, dtype=torch.float32, device="cuda")

    def noise(self, da, n, K, seed, base, step):
        """randn(rng, Float32, da, K, n) of the shared stream, from the UNCHANGED Gaussian head: mu = 0, sigma clamped to exactly 1,
        identity squash, so z = 0 + 1 * eps = eps"""
        mu, raw, act = torch.zeros((n, da), device="cuda"), torch.ones((n, da), device="cuda"), self.empty(n, K, da)
        self.call("rlhip_gaussian_head_sample_f32", self.ptr(mu), self.ptr(raw), da, n, K, 1.0, 1.0, 0, 0, seed, base, step,
                  self.ptr(act), None, self.sp())
        return self.down(act)

    def vec_to_tril(self, vec):
        nv, n = vec.shape
        da = next(d for d in range(1, 17) if M.nvec(d) == nv)
        v, L = self.up(vec), self.empty(n, da, da)
        self.call("rlhip_vec_to_tril_f32", self.ptr(v), da, n, self.ptr(L), self.sp())
        return self.down(L)

    def sample(self, mu, vec, K, seed=M.SEED, base=M.BASE, step=M.STEP, want_logp=True, want_L=True):
        da, n = mu.shape
        m, v, act = self.up(mu), self.up(vec), self.empty(n, K, da)
        lp = self.empty(n, K) if want_logp else None
        L = self.empty(n, da, da) if want_L else None
        self.call("rlhip_cov_gaussian_head_sample_f32", self.ptr(m), self.ptr(v), da, n, K, seed, base, step, self.ptr(act),
                  self.ptr(lp), self.ptr(L), self.sp())
        return self.down(act), None if lp is None else self.down(lp), None if L is None else self.down(L)

    def logp(self, mu, vec, a, want_L=True):
        da, K, n = a.shape
        m, v, x, lp = self.up(mu), self.up(vec), self.up(a), self.empty(n, K)
        L = self.empty(n, da, da) if want_L else None
        self.call("rlhip_cov_gaussian_head_logp_f32", self.ptr(m), self.ptr(v), self.ptr(x), da, n, K, self.ptr(lp), self.ptr(L),
                  self.sp())
        return self.down(lp), None if L is None else self.down(L)

    def mvnormlogpdf(self, mu, L, x):
        from rlhip import ops

        return self.down(ops.mvnormlogpdf(self.up(mu), self.up(L), self.up(x)))

    def mvnormkl(self, mu1, L1, mu2, L2):
        from rlhip import ops

        return ops.mvnormkldivergence(self.up(mu1), self.up(L1), self.up(mu2), self.up(L2)).cpu().numpy()

    def diagkl(self, mu1, s1, mu2, s2):
        from rlhip import ops

        return ops.diagnormkldivergence(self.up(mu1), self.up(s1), self.up(mu2), self.up(s2)).cpu().numpy()

    def normkl(self, mu1, s1, mu2, s2):
        from rlhip import ops

        return self.down(ops.normkldivergence(self.up(mu1), self.up(s1), self.up(mu2), self.up(s2)))


def _show(res):
    print({k: (f"{v:.3g}" if isinstance(v, float) else v) for k, v in res.items()})
    return res


@pytest.mark.parametrize("da,n,K", M.SHAPES)
def test_head_sampling_and_evaluation(dev, da, n, K):
    """L judged entry by entry; actions = the numpy Float32 replay of mu + L_dev eps, bit for bit; logp within the bar; (model)(state,
    action) on those actions within the bar and bit-equal to the sampling logp; the fused calls byte for byte the three-call
    composition; outputs independent of which optional outputs are asked for; a second call (step + 1) differs"""
    mu, vec = M.inputs(da, n, seed=da)
    tag = f"da={da} n={n} K={K}"
    eps = dev.noise(da, n, K, M.SEED, M.BASE, M.STEP)
    a, lp, L = dev.sample(mu, vec, K)
    assert a.shape == (da, K, n) and lp.shape == (K, n) and L.shape == (da, da, n)
    _show(M.judge_tril(L, vec, tag="L " + tag))
    diag = np.stack([L[i, i] for i in range(da)])
    assert (diag > 3).all() and (diag < 11).all()                         # well-conditioned, as the inputs promise
    assert _same(a, M.sample_replay(mu, L, eps)), f"{tag}: actions are not mu + L eps in the stated order"
    model = M.mvnormlogpdf(mu, L, a)
    _show(judge(lp, *model, cap=0.0, tag="sample " + tag))
    lp2, L2 = dev.logp(mu, vec, a)
    _show(judge(lp2, *model, cap=0.0, tag="eval " + tag))
    assert _same(lp2, lp) and _same(L2, L)
    # the composition: vec_to_tril -> (the product, replayed above on the same draws) -> mvnormlogpdf
    Lc = dev.vec_to_tril(vec)
    assert _same(Lc, L), f"{tag}: fused L differs from rlhip_vec_to_tril_f32"
    assert _same(dev.mvnormlogpdf(mu, Lc, a), lp), f"{tag}: fused logp differs from rlhip_mvnormlogpdf_f32"
    a0, none, noL = dev.sample(mu, vec, K, want_logp=False, want_L=False)
    assert none is None and noL is None and _same(a0, a)
    assert _same(dev.logp(mu, vec, a, want_L=False)[0], lp)
    a1, lp1, _ = dev.sample(mu, vec, K, step=M.STEP + 1)
    assert not np.array_equal(a1, a) and not np.array_equal(lp1, lp)
    assert _same(a1, M.sample_replay(mu, L, dev.noise(da, n, K, M.SEED, M.BASE, M.STEP + 1)))


def test_head_edge_diagonals_and_non_finite_entries(dev):
    """da = 3, n = 40, K = 2: diagonal inputs -1000 and -200 give the floor 1e-5 exactly, 880 stays finite, 900 overflows expf (Inf
    diagonal, -Inf log-probability of a finite action), NaN stays NaN; an Inf and a NaN below the diagonal; the model's non-finite
    pattern is matched exactly (`judge`)"""
    mu, vec = M.edge_vectors()
    da, n, K = 3, 40, 2
    a, lp, L = dev.sample(mu, vec, K)
    _show(M.judge_tril(L, vec, tag="edge L"))
    d0 = L[0, 0]
    assert d0[0] == F32(1e-5) and d0[3] == F32(1e-5) and np.isfinite(d0[9]) and abs(d0[9] - 880) < 1e-3
    assert d0[12] == np.inf and np.isnan(d0[15]) and L[1, 1, 13] == np.inf and L[2, 2, 14] == np.inf
    assert L[1, 0, 20] == np.inf and L[2, 1, 21] == -np.inf and np.isnan(L[2, 0, 22])
    assert _same(a, M.sample_replay(mu, L, dev.noise(da, n, K, M.SEED, M.BASE, M.STEP)))
    r = _show(judge(lp, *M.mvnormlogpdf(mu, L, a), cap=0.0, tag="edge sample"))
    assert r["non_finite"] >= 2 * 7
    # finite actions: the Inf diagonals give -Inf
    x = np.random.default_rng(5).normal(size=(da, K, n)).astype(F32)
    lp2, L2 = dev.logp(mu, vec, x)
    assert _same(L2, L)
    _show(judge(lp2, *M.mvnormlogpdf(mu, L, x), cap=0.0, tag="edge eval"))
    assert (lp2[:, 12:15] == -np.inf).all() and np.isnan(lp2[:, 15:18]).all() and np.isnan(lp2[:, 22]).all()
    assert np.isfinite(lp2[:, :12]).all() and np.isfinite(lp2[:, 23:]).all()
    assert _same(dev.mvnormlogpdf(mu, dev.vec_to_tril(vec), x), lp2)


@pytest.mark.parametrize("da,n,K", M.SHAPES)
def test_kl_divergences_and_mvnormlogpdf(dev, da, n, K):
    """the three KLs and the stand-alone mvnormlogpdf on two independent input sets; KL(p, p) within the budget of 0"""
    tag = f"da={da} n={n} K={K}"
    mu1, vec1 = M.inputs(da, n, seed=100 + da)
    mu2, vec2 = M.inputs(da, n, seed=200 + da)
    L1, L2 = dev.vec_to_tril(vec1), dev.vec_to_tril(vec2)
    rng = np.random.default_rng(da)
    x = (mu1[:, None, :] + 3 * rng.normal(size=(da, K, n))).astype(F32)
    _show(judge(dev.mvnormlogpdf(mu1, L1, x), *M.mvnormlogpdf(mu1, L1, x), cap=0.0, tag="mvnormlogpdf " + tag))
    _show(judge(dev.mvnormkl(mu1, L1, mu2, L2), *M.mvnormkldivergence(mu1, L1, mu2, L2), cap=0.0, tag="mvn KL " + tag))
    s1 = (np.abs(rng.normal(size=(da, n))) + 0.1).astype(F32)
    s2 = (np.abs(rng.normal(size=(da, n))) + 0.1).astype(F32)
    _show(judge(dev.diagkl(mu1, s1, mu2, s2), *M.diagnormkldivergence(mu1, s1, mu2, s2), cap=0.0, tag="diag KL " + tag))
    _show(judge(dev.normkl(mu1, s1, mu2, s2), *M.normkldivergence(mu1, s1, mu2, s2), cap=0.0, tag="1-D KL " + tag))
    for name, got, model in (("mvn", dev.mvnormkl(mu1, L1, mu1, L1), M.mvnormkldivergence(mu1, L1, mu1, L1)),
                             ("diag", dev.diagkl(mu1, s1, mu1, s1), M.diagnormkldivergence(mu1, s1, mu1, s1))):
        judge(got, *model, cap=0.0, tag=f"{name} KL(p, p) " + tag)
        assert (np.abs(model[0]) <= 2 * model[1]).all() and (np.abs(got.astype(F64)) <= 2 * model[1]).all(), f"{name} KL(p, p) {tag}"


def test_golden_cases_on_the_device(dev):
    """RLCore/test/utils/distributions.jl:20-126 and networks.jl:174-196 on the kernels, against the closed forms of Normal / MvNormal
    in float64 at the reference's own tolerance (Julia's `≈`: rtol = sqrt(eps(Float32)))"""
    c = KAT["normal_1d"]
    one = lambda k: np.array([[c[k]]], F32)                                                  # noqa: E731
    assert M.approx(dev.normkl(one("mu1"), one("sigma1"), one("mu2"), one("sigma2")), np.log(6 / 5) + 26 / 72 - 0.5)
    assert M.approx(dev.normkl(one("mu2"), one("sigma2"), one("mu1"), one("sigma1")),
                    M.normal_kl64(c["mu2"], c["sigma2"], c["mu1"], c["sigma1"]))
    for case in ("diag_2d", "diag_3d"):
        g = {k: np.asarray(v, F32) for k, v in KAT[case].items() if not k.startswith("_")}
        if case == "diag_3d":
            g = {k: v[:, 0, :] for k, v in g.items()}
        for p, q in (("1", "2"), ("2", "1")):
            got = dev.diagkl(g["mu" + p], g["sigma" + p], g["mu" + q], g["sigma" + q])
            for i in range(2):
                assert M.approx(got[i], M.mvnormal_kl64(g["mu" + p][:, i], np.diag(g["sigma" + p][:, i].astype(F64) ** 2),
                                                        g["mu" + q][:, i], np.diag(g["sigma" + q][:, i].astype(F64) ** 2)))
    f = KAT["full_cov"]
    mu1, mu2, x = (np.asarray(f[k], F32) for k in ("mu1", "mu2", "x"))
    chol = lambda S: np.repeat(np.linalg.cholesky(np.asarray(S, F64)).astype(F32)[:, :, None], 2, axis=2)   # noqa: E731
    L1, L2 = chol(f["Sigma1"]), chol(f["Sigma2"])
    lp = dev.mvnormlogpdf(mu1[:, 0, :], L1, x)
    assert lp.shape == (1, 2)
    for i in range(2):
        assert M.approx(lp[0, i], M.mvnormal_logpdf64(mu1[:, 0, i], f["Sigma1"], x[:, 0, i]))
    assert M.approx(dev.mvnormkl(mu1[:, 0, :], L1, mu2[:, 0, :], L2), 1.0)
    assert M.approx(dev.mvnormkl(mu2[:, 0, :], L2, mu1[:, 0, :], L1), 1.0)
    v = KAT["vec_to_tril"]
    vec = np.repeat(np.asarray(v["cholesky_vec"], F32)[:, None], v["batch"], axis=1)
    want = np.array(v["cholesky_mat_raw"], F64)
    for i, j in v["softplusbeta_at"]:
        want[i - 1, j - 1] = np.log(np.exp(want[i - 1, j - 1] / 10.0) + 1.0) * 10.0
    L = dev.vec_to_tril(vec)
    for b in range(v["batch"]):
        assert np.linalg.norm(L[:, :, b] - want) <= M.RTOL * max(np.linalg.norm(L[:, :, b]), np.linalg.norm(want))


def test_sigma_zero_patterns_of_the_kls(dev):
    """sigma = 0 on either side, on both, and a negative sigma: logf(0) = -Inf, 0 / 0, Inf - Inf -- the model's pattern, exactly"""
    rng = np.random.default_rng(11)
    d, n = 3, 48
    mu1, mu2 = rng.normal(size=(d, n)).astype(F32), rng.normal(size=(d, n)).astype(F32)
    s1, s2 = (np.abs(rng.normal(size=(d, n))) + 0.1).astype(F32), (np.abs(rng.normal(size=(d, n))) + 0.1).astype(F32)
    s1[0, 0:12], s2[1, 12:24] = 0.0, 0.0
    s1[2, 24:36], s2[2, 24:36] = 0.0, 0.0
    s1[1, 36:40] = -1.0
    mu2[:, 30:36] = mu1[:, 30:36]
    r = _show(judge(dev.normkl(mu1, s1, mu2, s2), *M.normkldivergence(mu1, s1, mu2, s2), cap=0.0, tag="1-D KL sigma = 0"))
    assert r["non_finite"] >= 36
    r = _show(judge(dev.diagkl(mu1, s1, mu2, s2), *M.diagnormkldivergence(mu1, s1, mu2, s2), cap=0.0, tag="diag KL sigma = 0"))
    assert r["non_finite"] >= 36
    got = dev.diagkl(mu1, s1, mu2, s2)
    assert (got[0:12] == np.inf).all() and np.isfinite(got[40:]).all()


def _mlp_net(rl, ns, da, n, seed):
    """pre / mu / Sigma as closures over ops.mlp2_forward.  The forward kernel takes at most 16 inputs and 32 outputs, so the 20 state
    components enter `pre` through two nets (16 + 4 inputs) and the 55-element Cholesky vector leaves `Sigma` through two (32 + 23)"""
    from rlhip import ops

    feat, h, nv = 15, 32, M.nvec(da)
    p = [ops.mlp2_init(16, h, feat, seed, 0), ops.mlp2_init(ns - 16, h, feat, seed, 1), ops.mlp2_init(feat, h, da, seed, 2),
         ops.mlp2_init(feat, h, 32, seed, 3), ops.mlp2_init(feat, h, nv - 32, seed, 4)]
    pre = lambda s: ops.mlp2_forward(p[0], 16, h, feat, 1, s[:16]) + ops.mlp2_forward(p[1], ns - 16, h, feat, 1, s[16:])   # noqa: E731
    mu = lambda x: ops.mlp2_forward(p[2], feat, h, da, 1, x)                                                                # noqa: E731
    Sigma = lambda x: torch.cat([ops.mlp2_forward(p[3], feat, h, 32, 1, x), ops.mlp2_forward(p[4], feat, h, nv - 32, 1, x)])  # noqa: E731
    return rl.CovGaussianNetwork(pre, mu, Sigma, seed=3, env_id_base=1)


def test_network_end_to_end_in_the_reference_test_shapes():
    """RLCore/test/utils/networks.jl:206-230 on rlhip.CovGaussianNetwork at (ns, da, n) = (20, 10, 3)"""
    import rlhip as rl
    from rlhip import ops

    ns, da, n = 20, 10, 3
    gn = _mlp_net(rl, ns, da, n, seed=5)
    state = torch.rand((ns, n), device="cuda")
    m, L = gn(state)
    assert m.shape == (da, n) and L.shape == (da, da, n)
    a, logp = gn(state, is_sampling=True, is_return_log_prob=True)
    assert a.shape == (da, n) and logp.shape == (1, n) and gn.step == 1
    logp2d = gn(state, a)
    assert logp2d.shape == (1, n) and torch.equal(logp2d, logp)
    s3 = state.unsqueeze(1)
    m, L = gn(s3)
    assert m.shape == (da, 1, n) and L.shape == (da, da, n)
    a, logp = gn(s3, is_sampling=True, is_return_log_prob=True)
    assert a.shape == (da, 1, n) and logp.shape == (1, 1, n) and gn.step == 2
    only = gn(s3, is_sampling=True)
    assert only.shape == (da, 1, n) and not torch.equal(only, a) and gn.step == 3
    # logp ≈ mvnormlogpdf(m, L, a)  (here: the same kernel arithmetic, so bit for bit) and logp ≈ gn(state, a)
    st = lambda t: t.permute(*range(t.dim() - 1, -1, -1)).contiguous()                        # noqa: E731  Julia shape -> storage
    ref = ops.mvnormlogpdf(st(m[:, 0, :]), st(L), st(a))
    assert torch.equal(ref.t().unsqueeze(0), logp)
    assert M.approx(logp.cpu().numpy(), gn(s3, a).cpu().numpy()) and torch.equal(gn(s3, a), logp)
    acts, logps = gn.sample(s3, 5)
    assert acts.shape == (da, 5, n) and logps.shape == (1, 5, n) and gn.step == 4
    logps2 = gn(s3, acts)
    assert logps2.shape == (1, 5, n) and M.approx(logps2.cpu().numpy(), logps.cpu().numpy())
    # against the ground truth of :231-234: MvNormal(m, L L') in float64
    mh, Lh, ah, lh = (t.cpu().numpy().astype(F64) for t in (m[:, 0, :], L, acts, logps[0]))
    for i in range(n):
        S = Lh[:, :, i] @ Lh[:, :, i].T
        for j in range(5):
            assert M.approx(lh[j, i], M.mvnormal_logpdf64(mh[:, i], S, ah[:, j, i]))
    # and the model's bar on the whole thing
    judge(lh, *M.mvnormlogpdf(mh.astype(F32), Lh.astype(F32), ah.astype(F32)), cap=0.0, tag="network")


def test_bad_arguments_launch_nothing(dev):
    """da = 0, 17 and NULL outputs: RLHIP_EINVAL, and the output buffers keep their contents; n = 0 is a no-op"""
    from rlhip import _lib

    n, K = 4, 2
    canary = lambda *s: torch.full(s, 7.0, device="cuda")                                     # noqa: E731
    act, lp, L, src = canary(n * K * 17), canary(n * K), canary(n * 17 * 17), canary(n * 17 * 17)
    P = dev.ptr
    for da in (0, 17):
        for name, args in (("rlhip_vec_to_tril_f32", (P(src), da, n, P(L), dev.sp())),
                           ("rlhip_mvnormlogpdf_f32", (P(src), P(src), P(src), da, K, n, P(lp), dev.sp())),
                           ("rlhip_cov_gaussian_head_sample_f32", (P(src), P(src), da, n, K, 1, 0, 0, P(act), P(lp), P(L), dev.sp())),
                           ("rlhip_cov_gaussian_head_logp_f32", (P(src), P(src), P(src), da, n, K, P(lp), P(L), dev.sp())),
                           ("rlhip_mvnormkldivergence_f32", (P(src), P(src), P(src), P(src), da, n, P(lp), dev.sp()))):
            with pytest.raises(_lib.RLHipArgumentError, match="da must be in 1 ... 16"):
                dev.call(name, *args)
    with pytest.raises(_lib.RLHipArgumentError, match="NULL"):
        dev.call("rlhip_cov_gaussian_head_sample_f32", P(src), P(src), 3, n, K, 1, 0, 0, None, P(lp), P(L), dev.sp())
    with pytest.raises(_lib.RLHipArgumentError, match="NULL"):
        dev.call("rlhip_cov_gaussian_head_logp_f32", P(src), P(src), P(src), 3, n, K, None, P(L), dev.sp())
    with pytest.raises(_lib.RLHipArgumentError, match="NULL"):
        dev.call("rlhip_vec_to_tril_f32", P(src), 3, n, None, dev.sp())
    with pytest.raises(_lib.RLHipArgumentError):
        dev.call("rlhip_cov_gaussian_head_sample_f32", P(src), P(src), 3, n, 0, 1, 0, 0, P(act), P(lp), P(L), dev.sp())
    dev.call("rlhip_cov_gaussian_head_sample_f32", P(src), P(src), 3, 0, K, 1, 0, 0, P(act), P(lp), P(L), dev.sp())
    dev.call("rlhip_cov_gaussian_head_logp_f32", P(src), P(src), P(src), 3, 0, K, P(lp), P(L), dev.sp())
    dev.call("rlhip_mvnormkldivergence_f32", P(src), P(src), P(src), P(src), 3, 0, P(lp), dev.sp())
    torch.cuda.synchronize()
    assert (act == 7).all() and (lp == 7).all() and (L == 7).all()
