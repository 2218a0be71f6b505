"""The pullbacks of CovGaussianNetwork, mvnormlogpdf, vec_to_tril and the Gaussian KL divergences on the device
(csrc/cov_heads_grad.hip) against the model (tests/mvnorm_grad_ref.py), through the C ABI and through rlhip/grad.py.  Everything but
the diagonal of the vec_to_tril pullback is an exact Float32 replay and is compared bit for bit."""
import numpy as np
import pytest
import torch

import mvnorm_grad_ref as G
import mvnorm_ref as M
from heads_ref import F32
from test_gpu_cov_heads import Device
from test_mvnorm_grad_reference import _case, mvnormlogpdf64, vec_to_tril64

pytestmark = pytest.mark.gpu
SENTINEL = 7.0


class GradDevice(Device):
    """the entry points of csrc/cov_heads_grad.hip on numpy arrays in the reference's shapes; an output that is not asked for is handed
    over as NULL and its buffer, filled with a sentinel, is returned as it is"""

    def _outs(self, shapes, need):
        outs = [torch.full(s, SENTINEL, dtype=torch.float32, device="cuda") for s in shapes]
        return outs, [self.ptr(o) if w else None for o, w in zip(outs, need)]

    def logpdf_bwd(self, mu, L, x, g, need=(1, 1, 1)):
        da, K, n = x.shape
        ins = [self.up(a) for a in (mu, L, x, g)]
        outs, ptrs = self._outs([(n, da), (n, da, da), (n, K, da)], need)
        self.call("rlhip_mvnormlogpdf_bwd_f32", *(self.ptr(t) for t in ins), da, K, n, *ptrs, self.sp())
        return [self.down(o) for o in outs]

    def tril_bwd(self, vec, dL):
        da, n = dL.shape[0], vec.shape[1]
        v, d, out = self.up(vec), self.up(dL), self.empty(n, M.nvec(da))
        self.call("rlhip_vec_to_tril_bwd_f32", self.ptr(v), self.ptr(d), da, n, self.ptr(out), self.sp())
        return self.down(out)

    def head_bwd(self, mu, vec, a, g, need=(1, 1)):
        da, K, n = a.shape
        ins = [self.up(t) for t in (mu, vec, a, g)]
        outs, ptrs = self._outs([(n, da), (n, M.nvec(da))], need)
        self.call("rlhip_cov_gaussian_head_logp_bwd_f32", *(self.ptr(t) for t in ins), da, n, K, *ptrs, self.sp())
        return [self.down(o) for o in outs]

    def mvnkl_bwd(self, mu1, L1, mu2, L2, g, need=(1, 1, 1, 1)):
        da, n = mu1.shape
        ins = [self.up(t) for t in (mu1, L1, mu2, L2, g)]
        outs, ptrs = self._outs([(n, da), (n, da, da), (n, da), (n, da, da)], need)
        self.call("rlhip_mvnormkldivergence_bwd_f32", *(self.ptr(t) for t in ins), da, n, *ptrs, self.sp())
        return [self.down(o) for o in outs]

    def diagkl_bwd(self, mu1, s1, mu2, s2, g):
        d, n = mu1.shape
        ins = [self.up(t) for t in (mu1, s1, mu2, s2, g)]
        outs, ptrs = self._outs([(n, d)] * 4, (1, 1, 1, 1))
        self.call("rlhip_diagnormkldivergence_bwd_f32", *(self.ptr(t) for t in ins), d, n, *ptrs, self.sp())
        return [self.down(o) for o in outs]

    def normkl_bwd(self, mu1, s1, mu2, s2, g):
        ins = [self.up(t) for t in (mu1, s1, mu2, s2, g)]
        outs, ptrs = self._outs([tuple(ins[0].shape)] * 4, (1, 1, 1, 1))
        self.call("rlhip_normkldivergence_bwd_f32", *(self.ptr(t) for t in ins), mu1.size, *ptrs, self.sp())
        return [self.down(o) for o in outs]


@pytest.fixture(scope="module")
def dev():
    import rlhip  # noqa: F401
    return GradDevice()


def _show(res):
    print({k: (f"{v:.3g}" if isinstance(v, float) else v) for k, v in res.items()})
    return res


@pytest.mark.parametrize("da,n,K", M.SHAPES)
def test_every_pullback_matches_the_model(dev, da, n, K):
    """the six entry points through the C ABI: bit for bit the Float32 replay (the diagonal of dvec within its expf budget), and the
    fused head pullback byte for byte the three-call composition"""
    tag = f"da={da} n={n} K={K}"
    mu1, vec1, mu2, vec2, x, s1, s2 = _case(da, n, K)
    _, L1 = dev.logp(mu1, vec1, x)                       # the implementation's own L, an exact input of everything downstream
    L2 = dev.vec_to_tril(vec2)
    g = G.cotangent((K, n), 1)
    got = dev.logpdf_bwd(mu1, L1, x, g)
    for name, a, b in zip(("dmu", "dL", "dx"), got, G.mvnormlogpdf_bwd(mu1, L1, x, g)):
        assert G.same(a, b), f"mvnormlogpdf_bwd {name} {tag}"
    # vec_to_tril_bwd on a dense cotangent whose upper triangle is NaN: it must not be read
    dL = G.cotangent((da, da, n), 2)
    dL[np.triu_indices(da, 1)] = np.nan
    _show(G.judge_dvec(dev.tril_bwd(vec1, dL), *G.vec_to_tril_bwd(vec1, dL), tag="vec_to_tril_bwd " + tag))
    # the head: against the model, and against the composition
    dmu, dvec = dev.head_bwd(mu1, vec1, x, g)
    want_dmu, (c, e) = G.head_logp_bwd(mu1, vec1, L1, x, g)
    assert G.same(dmu, want_dmu), f"head dmu {tag}"
    _show(G.judge_dvec(dvec, c, e, tag="head dvec " + tag))
    assert G.same(dmu, got[0]) and G.same(dvec, dev.tril_bwd(vec1, got[1])), f"{tag}: the fused pullback is not the composition"
    # the KLs
    gk = G.cotangent((n,), 3)
    for name, a, b in zip(("dmu1", "dL1", "dmu2", "dL2"), dev.mvnkl_bwd(mu1, L1, mu2, L2, gk), G.mvnormkl_bwd(mu1, L1, mu2, L2, gk)):
        assert G.same(a, b), f"mvnormkldivergence_bwd {name} {tag}"
    for name, a, b in zip(("dmu1", "ds1", "dmu2", "ds2"), dev.diagkl_bwd(mu1, s1, mu2, s2, gk), G.diagnormkl_bwd(mu1, s1, mu2, s2, gk)):
        assert G.same(a, b), f"diagnormkldivergence_bwd {name} {tag}"
    ge = G.cotangent((da, n), 4)
    for name, a, b in zip(("dmu1", "ds1", "dmu2", "ds2"), dev.normkl_bwd(mu1, s1, mu2, s2, ge), G.normkl_bwd(mu1, s1, mu2, s2, ge)):
        assert G.same(a, b), f"normkldivergence_bwd {name} {tag}"


def test_every_combination_of_nullable_outputs(dev):
    """(5, 33, 3): an output that is not asked for is untouched (the sentinel), the others are what the full call gives"""
    da, n, K = 5, 33, 3
    mu1, vec1, mu2, vec2, x, _, _ = _case(da, n, K)
    L1, L2 = dev.vec_to_tril(vec1), dev.vec_to_tril(vec2)
    g, gk = G.cotangent((K, n), 1), G.cotangent((n,), 3)
    for full, run, k in ((dev.logpdf_bwd(mu1, L1, x, g), lambda need: dev.logpdf_bwd(mu1, L1, x, g, need), 3),
                         (dev.mvnkl_bwd(mu1, L1, mu2, L2, gk), lambda need: dev.mvnkl_bwd(mu1, L1, mu2, L2, gk, need), 4),
                         (dev.head_bwd(mu1, vec1, x, g), lambda need: dev.head_bwd(mu1, vec1, x, g, need), 2)):
        for mask in range(2 ** k):
            need = [(mask >> b) & 1 for b in range(k)]
            for b, (got, want) in enumerate(zip(run(need), full)):
                if need[b]:
                    assert G.same(got, want), (k, need, b)
                else:
                    assert (got == SENTINEL).all(), (k, need, b)


def test_edge_diagonals_and_non_finite_entries(dev):
    """da = 3, n = 40, K = 2 (tests/mvnorm_ref.py edge_vectors): diagonal inputs -1000 / -200 (L = the floor, the sigmoid factor is 0 at
    -1000 exactly), 880, 900 (an Inf diagonal), NaN, and an Inf and a NaN below the diagonal -- the model's patterns, exactly"""
    mu, vec = M.edge_vectors()
    da, n, K = 3, 40, 2
    x = np.random.default_rng(5).normal(size=(da, K, n)).astype(F32)
    g = G.cotangent((K, n), 1)
    _, L = dev.logp(mu, vec, x)
    for name, a, b in zip(("dmu", "dL", "dx"), dev.logpdf_bwd(mu, L, x, g), G.mvnormlogpdf_bwd(mu, L, x, g)):
        assert G.same(a, b), f"edge mvnormlogpdf_bwd {name}"
    dmu, dvec = dev.head_bwd(mu, vec, x, g)
    want_dmu, (c, e) = G.head_logp_bwd(mu, vec, L, x, g)
    assert G.same(dmu, want_dmu)
    _show(G.judge_dvec(dvec, c, e, tag="edge head dvec"))
    assert np.isnan(dvec[:, 15:18]).any() and np.isnan(dvec[:, 22]).any() and np.isfinite(dvec[:, 23:]).all()
    mu2, vec2 = M.inputs(da, n, seed=9)
    L2, gk = dev.vec_to_tril(vec2), G.cotangent((n,), 3)
    for (a1, b1, a2, b2) in ((mu, L, mu2, L2), (mu2, L2, mu, L)):
        for name, a, b in zip(("dmu1", "dL1", "dmu2", "dL2"), dev.mvnkl_bwd(a1, b1, a2, b2, gk), G.mvnormkl_bwd(a1, b1, a2, b2, gk)):
            assert G.same(a, b), f"edge mvnormkldivergence_bwd {name}"
    # sigma = 0 on either side of the small KLs: 1 / 0, 0 / 0, Inf - Inf
    rng = np.random.default_rng(11)
    s1, s2 = (np.abs(rng.normal(size=(da, n))) + 0.1).astype(F32), (np.abs(rng.normal(size=(da, n))) + 0.1).astype(F32)
    s1[0, 0:12], s2[1, 12:24], s1[2, 24:36], s2[2, 24:36] = 0.0, 0.0, 0.0, 0.0
    for a, b in zip(dev.diagkl_bwd(mu, s1, mu2, s2, gk), G.diagnormkl_bwd(mu, s1, mu2, s2, gk)):
        assert G.same(a, b)
    ge = G.cotangent((da, n), 4)
    for a, b in zip(dev.normkl_bwd(mu, s1, mu2, s2, ge), G.normkl_bwd(mu, s1, mu2, s2, ge)):
        assert G.same(a, b)


def test_k_sum_is_bit_identical_from_run_to_run(dev):
    da, n, K = 16, 1, 300
    mu1, vec1, _, _, x, _, _ = _case(da, n, K)
    g = G.cotangent((K, n), 1)
    first = dev.head_bwd(mu1, vec1, x, g)
    for _ in range(3):
        again = dev.head_bwd(mu1, vec1, x, g)
        assert G.same(again[0], first[0]) and G.same(again[1], first[1])


def test_autograd_through_ops_on_the_device(dev):
    """rlhip/grad.py on device tensors: values bit-identical to the plain call, gradients bit-identical to the ABI calls"""
    from rlhip import ops

    da, n, K = 5, 33, 3
    mu1, vec1, mu2, vec2, x, s1, s2 = _case(da, n, K)
    g = G.cotangent((K, n), 1)
    tm, tv, tx = (dev.up(a).requires_grad_(True) for a in (mu1, vec1, x))
    with torch.no_grad():
        plain = ops.mvnormlogpdf(tm, ops.vec_to_tril(tv, da), tx)
    out = ops.mvnormlogpdf(tm, ops.vec_to_tril(tv, da), tx)
    assert out.grad_fn is not None and torch.equal(out, plain)
    (out * dev.up(g)).sum().backward()
    L1 = dev.vec_to_tril(vec1)
    dmu, dL, dx = dev.logpdf_bwd(mu1, L1, x, g)
    assert G.same(dev.down(tm.grad), dmu) and G.same(dev.down(tx.grad), dx) and G.same(dev.down(tv.grad), dev.tril_bwd(vec1, dL))
    gk = G.cotangent((n,), 3)
    L2 = dev.vec_to_tril(vec2)
    a = [dev.up(t).requires_grad_(w) for t, w in zip((mu1, L1, mu2, L2), (False, False, True, True))]
    (ops.mvnormkldivergence(*a) * dev.up(gk)).sum().backward()
    want = dev.mvnkl_bwd(mu1, L1, mu2, L2, gk)
    assert a[0].grad is None and G.same(dev.down(a[2].grad), want[2]) and G.same(dev.down(a[3].grad), want[3])
    a = [dev.up(t).requires_grad_(True) for t in (mu1, s1, mu2, s2)]
    (ops.diagnormkldivergence(*a) * dev.up(gk)).sum().backward()
    for t, w in zip(a, dev.diagkl_bwd(mu1, s1, mu2, s2, gk)):
        assert G.same(dev.down(t.grad), w)
    a = [dev.up(t).requires_grad_(True) for t in (mu1, s1, mu2, s2)]
    ops.normkldivergence(*a).sum().backward()
    for t, w in zip(a, dev.normkl_bwd(mu1, s1, mu2, s2, np.ones((da, n), F32))):
        assert G.same(dev.down(t.grad), w)


def test_bad_arguments_launch_nothing(dev):
    """da = 0, 17, K = 0 and NULL inputs: RLHIP_EINVAL, and the output buffers keep their contents; n = 0 is a no-op"""
    from rlhip import _lib

    n, K = 4, 2
    canary = lambda *s: torch.full(s, 7.0, device="cuda")                                     # noqa: E731
    out, src = canary(n * K * 17 * 17), canary(n * K * 17 * 17)
    P, sp = dev.ptr, dev.sp
    for da in (0, 17):
        for name, args in (("rlhip_mvnormlogpdf_bwd_f32", (P(src), P(src), P(src), P(src), da, K, n, P(out), P(out), P(out), sp())),
                           ("rlhip_vec_to_tril_bwd_f32", (P(src), P(src), da, n, P(out), sp())),
                           ("rlhip_cov_gaussian_head_logp_bwd_f32", (P(src), P(src), P(src), P(src), da, n, K, P(out), P(out), sp())),
                           ("rlhip_mvnormkldivergence_bwd_f32", (P(src), P(src), P(src), P(src), P(src), da, n, P(out), P(out), P(out),
                                                                 P(out), sp()))):
            with pytest.raises(_lib.RLHipArgumentError, match="da must be in 1 ... 16"):
                dev.call(name, *args)
    with pytest.raises(_lib.RLHipArgumentError):
        dev.call("rlhip_mvnormlogpdf_bwd_f32", P(src), P(src), P(src), P(src), 3, 0, n, P(out), P(out), P(out), sp())
    with pytest.raises(_lib.RLHipArgumentError, match="NULL"):
        dev.call("rlhip_cov_gaussian_head_logp_bwd_f32", P(src), P(src), P(src), None, 3, n, K, P(out), P(out), sp())
    with pytest.raises(_lib.RLHipArgumentError, match="NULL"):
        dev.call("rlhip_vec_to_tril_bwd_f32", P(src), P(src), 3, n, None, sp())
    dev.call("rlhip_mvnormlogpdf_bwd_f32", P(src), P(src), P(src), P(src), 3, K, 0, P(out), P(out), P(out), sp())
    dev.call("rlhip_cov_gaussian_head_logp_bwd_f32", P(src), P(src), P(src), P(src), 3, 0, K, P(out), P(out), sp())
    dev.call("rlhip_mvnormkldivergence_bwd_f32", P(src), P(src), P(src), P(src), P(src), 3, n, None, None, None, None, sp())
    dev.call("rlhip_normkldivergence_bwd_f32", P(src), P(src), P(src), P(src), P(src), 0, P(out), P(out), P(out), P(out), sp())
    torch.cuda.synchronize()
    assert (out == 7).all()


# the training test: measured once on one MI355X (profiles/cov_heads_grad.md), |final Float32 device loss - final float64 CPU loss| =
# 2.8e-7 at a loss of 5.33 (0.6 ulp of the Float32 loss; 1e-8 ... 7.7e-7 over the steps on the way).  The bar is ten times the measured
# gap: Float32 rounding enters every step and compounds through Adam's normalised update
TRAIN_STEPS, TRAIN_LR = 40, 0.05
TRAIN_GAP_MEASURED = 2.8e-7
TRAIN_BAR = 10 * TRAIN_GAP_MEASURED


def train_head(steps=TRAIN_STEPS, lr=TRAIN_LR):
    """-> (initial loss, final loss) of the device run and of the float64 CPU run from the same weights and data"""
    import rlhip

    ns, da, n = 3, 2, 512
    rng = np.random.default_rng(2024)
    state = rng.normal(size=(ns, n))
    A, C = np.array([[0.5, -1.0, 0.25], [1.5, 0.0, -0.75]]), np.array([[1.0, 0.0], [0.8, 0.6]])      # a fixed correlated Gaussian
    action = A @ state + C @ rng.normal(size=(da, n))
    torch.manual_seed(7)
    lin_mu, lin_S = torch.nn.Linear(ns, da), torch.nn.Linear(ns, M.nvec(da))
    init = [p.detach().clone() for p in (lin_mu.weight, lin_mu.bias, lin_S.weight, lin_S.bias)]

    # float64, CPU: the reference's formulas in torch
    ps = [p.double().requires_grad_(True) for p in init]
    s64, a64 = torch.tensor(state.T), torch.tensor(action.T[:, None, :])
    opt = torch.optim.Adam(ps, lr=lr)
    ref = []
    for _ in range(steps + 1):
        mu, vec = s64 @ ps[0].t() + ps[1], s64 @ ps[2].t() + ps[3]
        loss = -mvnormlogpdf64(mu, vec_to_tril64(vec, da), a64).mean()
        ref.append(float(loss.detach()))
        opt.zero_grad()
        loss.backward()
        opt.step()

    # Float32, device: rlhip.CovGaussianNetwork over torch.nn.Linear sub-networks, through rlhip/grad.py
    lin_mu, lin_S = lin_mu.cuda(), lin_S.cuda()
    net = rlhip.CovGaussianNetwork(mu=lambda s: lin_mu(s.t()).t(), Sigma=lambda s: lin_S(s.t()).t())
    s32 = torch.tensor(state, dtype=torch.float32, device="cuda")
    a32 = torch.tensor(action, dtype=torch.float32, device="cuda")
    opt = torch.optim.Adam(list(lin_mu.parameters()) + list(lin_S.parameters()), lr=lr)
    got = []
    for _ in range(steps + 1):
        loss = -net(s32, a32).mean()
        got.append(float(loss.detach()))
        opt.zero_grad()
        loss.backward()
        opt.step()
    return got, ref


def test_the_head_trains_with_a_torch_optimiser():
    got, ref = train_head()
    gap = abs(got[-1] - ref[-1])
    print(f"device loss {got[0]:.6f} -> {got[-1]:.6f}; float64 loss {ref[0]:.6f} -> {ref[-1]:.6f}; gap {gap:.3e} (bar {TRAIN_BAR})")
    assert got[-1] < got[0], "the loss did not fall"
    assert ref[-1] < ref[0]
    assert gap <= TRAIN_BAR, f"final loss {got[-1]!r} is {gap:.3e} from the float64 run's {ref[-1]!r} (bar {TRAIN_BAR:.3e})"
