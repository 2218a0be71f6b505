"""The model of csrc/cov_heads_grad.hip (tests/mvnorm_grad_ref.py) against float64 autograd of the reference's formulas, against the
reference's own gradient-test inputs and against planted faults; the host wrappers' shape handling with the C calls stubbed; the six
entry points in the built library; and the wiring of rlhip/grad.py with the model standing in for the C calls.  CPU only."""
import json
import math
import os
import re

import numpy as np
import pytest
import torch

import mvnorm_grad_ref as G
import mvnorm_ref as M
from heads_ref import F32, F64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KAT = json.load(open(os.path.join(ROOT, "tests", "golden", "mvnorm_grad_kat.json")))
SYMS = ["rlhip_mvnormlogpdf_bwd_f32", "rlhip_vec_to_tril_bwd_f32", "rlhip_cov_gaussian_head_logp_bwd_f32",
        "rlhip_mvnormkldivergence_bwd_f32", "rlhip_diagnormkldivergence_bwd_f32", "rlhip_normkldivergence_bwd_f32"]


def J(a):
    """Julia-shaped array <-> its column-major storage as a C-ordered array (all axes reversed); works both ways"""
    a = np.asarray(a)
    return np.ascontiguousarray(a.transpose(*range(a.ndim - 1, -1, -1)))


def tril_f32(vec, da):
    """vec_to_tril with the model's centre rounded to Float32: a valid 'implementation's own L'"""
    vec = np.asarray(vec, F32)
    L = np.zeros((da, da, vec.shape[1]), F32)
    for i in range(1, da + 1):
        for j in range(1, i + 1):
            x = vec[M.tril_index(i, j, da) - 1]
            L[i - 1, j - 1] = M.chol_diag(x).c.astype(F32) if i == j else x
    return L


# ------------------------------------------------------------------- the reference's formulas in float64 torch, written independently
# storages: mu (n, da), L (n, da, da) indexed [state, column, row], x (n, K, da), vec (n, nv)
def t64(a, grad=True):
    return torch.tensor(J(a), dtype=torch.float64, requires_grad=grad)


def _mat(Ls):
    """storage [state, column, row] -> lower-triangular matrices [state, row, column]"""
    return torch.tril(Ls.transpose(1, 2))


def vec_to_tril64(vec, da):
    """networks.jl:359-381: softplusbeta(x) = log(exp(x / 10) + 1) * 10 on the diagonal, + 1e-5 -> storage [state, column, row]"""
    n = vec.shape[0]
    L = torch.zeros((n, da, da), dtype=torch.float64)
    for i in range(1, da + 1):
        for j in range(1, i + 1):
            x = vec[:, M.tril_index(i, j, da) - 1]
            L[:, j - 1, i - 1] = torch.log(torch.exp(x / 10.0) + 1.0) * 10.0 + float(F32(1e-5)) if i == j else x
    return L


def mvnormlogpdf64(mu, Ls, x):
    """distributions.jl:46-50: -((d log2pi + 2 sum(log(diag(L)))) + sum(abs2, L \\ (x - mu))) / 2 -> (n, K)"""
    L = _mat(Ls)
    da = mu.shape[1]
    y = torch.linalg.solve_triangular(L, (x - mu[:, None, :]).transpose(1, 2), upper=False)      # (n, da, K)
    logdet = 2.0 * torch.log(torch.diagonal(L, dim1=1, dim2=2)).sum(1)
    return -((da * math.log(2.0 * math.pi) + logdet)[:, None] + (y * y).sum(1)) / 2.0


def mvnormkl64(mu1, L1s, mu2, L2s):
    """distributions.jl:88-103, with its dense inverses and products"""
    L1, L2 = _mat(L1s), _mat(L2s)
    d = mu1.shape[1]
    logdet = 2.0 * torch.log(torch.diagonal(L2, dim1=1, dim2=2)).sum(1) - 2.0 * torch.log(torch.diagonal(L1, dim1=1, dim2=2)).sum(1)
    M1 = L1 @ L1.transpose(1, 2)
    L2i = torch.linalg.inv(L2)
    X = (L2i.transpose(1, 2) @ L2i) @ M1
    trace = torch.diagonal(X, dim1=1, dim2=2).sum(1)
    sq = ((L2i @ (mu2 - mu1)[:, :, None])[:, :, 0] ** 2).sum(1)
    return (logdet - d + trace + sq) / 2.0


def diagnormkl64(mu1, s1, mu2, s2):
    v1, v2 = s1 ** 2, s2 ** 2
    return (torch.log(v2).sum(1) - torch.log(v1).sum(1) - mu1.shape[1] + (v1 / v2).sum(1) + ((mu2 - mu1) ** 2 / v2).sum(1)) / 2.0


def normkl64(mu1, s1, mu2, s2):
    return torch.log(s2) - torch.log(s1) + (s1 ** 2 + (mu1 - mu2) ** 2) / (2.0 * s2 ** 2) - 0.5


def grads64(out, g, *wrt):
    """gradients of sum(g * out) in Julia shapes"""
    return [J(t.numpy()) for t in torch.autograd.grad((out * torch.tensor(J(g), dtype=torch.float64)).sum(), wrt)]


def _case(da, n, K):
    mu1, vec1 = M.inputs(da, n, seed=100 + da)
    mu2, vec2 = M.inputs(da, n, seed=200 + da)
    rng = np.random.default_rng(da)
    x = (mu1[:, None, :] + 3 * rng.normal(size=(da, K, n))).astype(F32)
    s1 = (np.abs(rng.normal(size=(da, n))) + 0.1).astype(F32)
    s2 = (np.abs(rng.normal(size=(da, n))) + 0.1).astype(F32)
    return mu1, vec1, mu2, vec2, x, s1, s2


# ------------------------------------------------------------------------------------------------ (a) the model against autograd
@pytest.mark.parametrize("da,n,K", M.SHAPES)
def test_model_matches_float64_autograd_of_the_reference_formulas(da, n, K):
    """every gradient tensor by Julia's array `≈` over the whole tensor (at da = 1 the diagonal term g (u y - 1 / L) cancels: a single
    state reaches 1e-3 relative, the tensor does not)"""
    mu1, vec1, mu2, vec2, x, s1, s2 = _case(da, n, K)
    L1, L2 = tril_f32(vec1, da), tril_f32(vec2, da)
    g = G.cotangent((K, n), 1)
    # mvnormlogpdf
    tm, tL, tx = t64(mu1), t64(L1), t64(x)
    want = grads64(mvnormlogpdf64(tm, tL, tx), g, tm, tL, tx)
    got = G.mvnormlogpdf_bwd(mu1, L1, x, g)
    for name, a, b in zip(("dmu", "dL", "dx"), got, want):
        assert a.shape == b.shape and G.approx_tensor(a, b), f"mvnormlogpdf {name}"
    assert not got[1][np.triu_indices(da, 1)].any()
    # the head: vec_to_tril chained in
    tm, tv = t64(mu1), t64(vec1)
    want = grads64(mvnormlogpdf64(tm, vec_to_tril64(tv, da), t64(x, False)), g, tm, tv)
    dmu, (c, e) = G.head_logp_bwd(mu1, vec1, L1, x, g)
    assert G.approx_tensor(dmu, want[0]) and G.approx_tensor(c, want[1]), "head"
    assert (e[[M.tril_index(k, k, da) - 1 for k in range(1, da + 1)]] > 0).all() and (e >= 0).all()
    # vec_to_tril alone
    dL = G.cotangent((da, da, n), 2)
    tv = t64(vec1)
    want = grads64(vec_to_tril64(tv, da), np.tril(dL.transpose(2, 0, 1)).transpose(1, 2, 0), tv)
    assert G.approx_tensor(G.vec_to_tril_bwd(vec1, dL)[0], want[0]), "vec_to_tril"
    # the KLs
    gk = G.cotangent((n,), 3)
    ts = [t64(a) for a in (mu1, L1, mu2, L2)]
    for name, a, b in zip(("dmu1", "dL1", "dmu2", "dL2"), G.mvnormkl_bwd(mu1, L1, mu2, L2, gk), grads64(mvnormkl64(*ts), gk, *ts)):
        assert a.shape == b.shape and G.approx_tensor(a, b), f"mvnormkl {name}"
    ts = [t64(a) for a in (mu1, s1, mu2, s2)]
    for name, a, b in zip(("dmu1", "ds1", "dmu2", "ds2"), G.diagnormkl_bwd(mu1, s1, mu2, s2, gk), grads64(diagnormkl64(*ts), gk, *ts)):
        assert G.approx_tensor(a, b), f"diagnormkl {name}"
    ge = G.cotangent((da, n), 4)
    ts = [t64(a) for a in (mu1, s1, mu2, s2)]
    for name, a, b in zip(("dmu1", "ds1", "dmu2", "ds2"), G.normkl_bwd(mu1, s1, mu2, s2, ge), grads64(normkl64(*ts), ge, *ts)):
        assert G.approx_tensor(a, b), f"normkl {name}"


# ------------------------------------------------------------------------------------------------ (b) the reference's own inputs
def test_reference_gradient_test_inputs():
    """gradient(...) of sum(f) as RLCore/test/utils/distributions.jl takes it (cotangent 1), against the float64 closed forms"""
    c = KAT["normal_1d"]
    one = lambda k: np.array([c[k]], F32)                                                    # noqa: E731
    d = G.normkl_bwd(one("mu1"), one("sigma1"), one("mu2"), one("sigma2"), np.ones(1, F32))
    assert G.approx_tensor(d[0], c["d_kl_d_mu1"]) and G.approx_tensor(d[2], -c["d_kl_d_mu1"])
    for case in ("diag_2d", "diag_3d"):
        k = {key: np.asarray(v, F32) for key, v in KAT[case].items() if not key.startswith("_")}
        if case == "diag_3d":
            k = {key: v[:, 0, :] for key, v in k.items()}
        d = G.diagnormkl_bwd(k["mu1"], k["sigma1"], k["mu2"], k["sigma2"], np.ones(2, F32))
        assert G.approx_tensor(d[0], k["d_kl_d_mu1"]) and G.approx_tensor(d[2], -k["d_kl_d_mu1"])
    f = KAT["full_cov"]
    mu1, mu2, x = (np.asarray(f[k], F32) for k in ("mu1", "mu2", "x"))
    chol = lambda S: np.repeat(np.linalg.cholesky(np.asarray(S, F64)).astype(F32)[:, :, None], 2, axis=2)   # noqa: E731
    L1, L2 = chol(f["Sigma1"]), chol(f["Sigma2"])
    _, _, dx = G.mvnormlogpdf_bwd(mu1[:, 0, :], L1, x, np.ones((1, 2), F32))
    assert dx.shape == (2, 1, 2) and G.approx_tensor(dx, f["d_logpdf_d_x"])
    dmu1 = G.mvnormkl_bwd(mu1[:, 0, :], L1, mu2[:, 0, :], L2, np.ones(2, F32))[0]
    assert G.approx_tensor(dmu1, np.asarray(f["d_kl_d_mu1"])[:, 0, :])


# ------------------------------------------------------------------------------------------------ (c) planted faults must not pass
def test_fault_descending_k_sum():
    da, n, K = 16, 1, 300
    mu, vec, _, _, x, _, _ = _case(da, n, K)
    L, g = tril_f32(vec, da), G.cotangent((K, n), 1)
    good, bad = G.mvnormlogpdf_bwd(mu, L, x, g), G.mvnormlogpdf_bwd(mu, L, x, g, descending_k=True)
    assert G.same(bad[2], good[2])                                  # dx has no sum
    assert not G.same(bad[0], good[0]) and not G.same(bad[1], good[1])
    assert G.approx_tensor(bad[1], good[1])                         # ... a fault that only the bit-for-bit judge sees


def test_fault_missing_gs_term_and_full_outer_product():
    da, n, K = 5, 33, 3
    mu, vec, _, _, x, _, _ = _case(da, n, K)
    L, g = tril_f32(vec, da), G.cotangent((K, n), 1)
    good = G.mvnormlogpdf_bwd(mu, L, x, g)
    no_gs = G.mvnormlogpdf_bwd(mu, L, x, g, drop_gs=True)
    assert G.same(no_gs[0], good[0]) and not G.same(no_gs[1], good[1]) and not G.approx_tensor(no_gs[1], good[1])
    full = G.mvnormlogpdf_bwd(mu, L, x, g, full_outer=True)
    assert not G.same(full[1], good[1]) and full[1][np.triu_indices(da, 1)].any()
    # through the head: the judge of dvec sees the missing term on the diagonal
    c, e = G.head_logp_bwd(mu, vec, L, x, g)[1]
    G.judge_dvec(c.astype(F32), c, e, tag="good")
    with pytest.raises(AssertionError):
        G.judge_dvec(G.head_logp_bwd(mu, vec, L, x, g, drop_gs=True)[1][0].astype(F32), c, e, tag="no gs")


def test_fault_sigmoid_replaced_by_one():
    da, n, K = 3, 700, 4
    mu, vec, _, _, x, _, _ = _case(da, n, K)
    L, g = tril_f32(vec, da), G.cotangent((K, n), 1)
    c, e = G.head_logp_bwd(mu, vec, L, x, g)[1]
    r = G.judge_dvec(c.astype(F32), c, e, tag="sigmoid")
    assert r["n"] == da * n and r["worst_over_bar"] <= 0.5          # rounding the centre costs half an ulp, inside the bar
    bad = G.head_logp_bwd(mu, vec, L, x, g, sigmoid_one=True)[1][0].astype(F32)
    with pytest.raises(AssertionError):
        G.judge_dvec(bad, c, e, tag="sigmoid = 1")


def test_fault_kl_without_the_p_a_term():
    da, n = 5, 33
    mu1, vec1, mu2, vec2, _, _, _ = _case(da, n, 1)
    L1, L2, g = tril_f32(vec1, da), tril_f32(vec2, da), G.cotangent((n,), 3)
    good, bad = G.mvnormkl_bwd(mu1, L1, mu2, L2, g), G.mvnormkl_bwd(mu1, L1, mu2, L2, g, drop_pa=True)
    assert all(G.same(bad[k], good[k]) for k in (0, 1, 2))
    assert not G.same(bad[3], good[3]) and not G.approx_tensor(bad[3], good[3])


def test_model_non_finite_and_zero_patterns():
    """the edge vectors of the forward suite: diagonals at -1000 / -200 (the floor), 880, 900 (expf overflows: an Inf diagonal),
    NaN; the sigmoid factor is exactly 0 at -1000 (expf(100) = Inf) and exactly 1 at 880 / 900"""
    mu, vec = M.edge_vectors()
    s = G.softplusbeta_grad(np.array([-1000.0, -200.0, 0.0, 880.0, 900.0, np.nan], F32))
    assert s.c[0] == 0 and s.e[0] == 0 and s.c[3] == 1 and s.e[3] == 0 and s.c[4] == 1 and s.e[4] == 0
    assert 0 < s.c[1] < 1e-8 and s.e[1] > 0 and s.c[2] == 0.5 and np.isnan(s.c[5])
    L = tril_f32(vec, 3)
    x = np.random.default_rng(5).normal(size=(3, 2, 40)).astype(F32)
    dmu, dL, dx = G.mvnormlogpdf_bwd(mu, L, x, G.cotangent((2, 40), 1))
    assert np.isfinite(dmu[:, :12]).all() and np.isnan(dmu[:, 15:18]).any() and np.isnan(dL[:, :, 22]).any()
    assert not dL[np.triu_indices(3, 1)].any() and not M._bits(dL[np.triu_indices(3, 1)]).any()     # +0, not -0


# ------------------------------------------------------------------------------------------------ (d) the host wrappers, C calls stubbed
class _Stub:
    def __init__(self):
        self.calls = []

    def call(self, name, *args):
        self.calls.append((name, args))
        return 0


def _patch(monkeypatch, call):
    from rlhip import heads, ops

    for mod in (heads, ops):
        monkeypatch.setattr(mod, "call", call)
        monkeypatch.setattr(mod, "ptr", lambda t: t if t is None else (t.is_contiguous() or pytest.fail("not contiguous")) and t)
        monkeypatch.setattr(mod, "stream_ptr", lambda: None)


@pytest.fixture
def stub(monkeypatch):
    s = _Stub()
    _patch(monkeypatch, s.call)
    return s


def test_backward_wrappers_shapes_and_nullable_outputs(stub):
    from rlhip import _lib, ops

    n, da, K = 6, 4, 3
    nv = M.nvec(da)
    mu, L, x, vec = torch.zeros((n, da)), torch.zeros((n, da, da)), torch.zeros((n, K, da)), torch.zeros((n, nv))
    dmu, dL, dx = ops.mvnormlogpdf_backward(mu, L, x, torch.zeros((n, K)))
    assert dmu.shape == (n, da) and dL.shape == (n, da, da) and dx.shape == (n, K, da)
    name, args = stub.calls[-1]
    assert name == "rlhip_mvnormlogpdf_bwd_f32" and args[4:7] == (da, K, n) and args[7] is dmu and args[8] is dL and args[9] is dx
    dmu, dL, dx = ops.mvnormlogpdf_backward(mu, L, x[:, 0, :].contiguous(), torch.zeros(n), need=(False, True, False))
    assert dmu is None and dx is None and dL.shape == (n, da, da)
    assert stub.calls[-1][1][4:7] == (da, 1, n) and stub.calls[-1][1][7] is None and stub.calls[-1][1][9] is None
    assert ops.vec_to_tril_backward(vec, L, da).shape == (n, nv)
    assert stub.calls[-1][0] == "rlhip_vec_to_tril_bwd_f32" and stub.calls[-1][1][2:4] == (da, n)
    dmu, dvec = ops.cov_gaussian_head_logp_backward(mu, vec, x, torch.zeros((n, K)))
    assert dmu.shape == (n, da) and dvec.shape == (n, nv)
    assert stub.calls[-1][0] == "rlhip_cov_gaussian_head_logp_bwd_f32" and stub.calls[-1][1][4:7] == (da, n, K)
    outs = ops.mvnormkldivergence_backward(mu, L, mu, L, torch.zeros(n), need=(False, False, True, True))
    assert outs[0] is None and outs[1] is None and outs[2].shape == (n, da) and outs[3].shape == (n, da, da)
    name, args = stub.calls[-1]
    assert name == "rlhip_mvnormkldivergence_bwd_f32" and args[5:7] == (da, n) and args[7] is None and args[8] is None and args[10] is outs[3]
    outs = ops.diagnormkldivergence_backward(mu, mu, mu, mu, torch.zeros(n))
    assert [o.shape for o in outs] == [(n, da)] * 4 and stub.calls[-1][1][5:7] == (da, n)
    e = torch.zeros((5, 7))
    outs = ops.normkldivergence_backward(e, e, e, e, e, need=(True, False, False, False))
    assert outs[0].shape == (5, 7) and outs[1:] == (None, None, None) and stub.calls[-1][1][5] == 35
    for bad in (lambda: ops.mvnormlogpdf_backward(mu, L, x, torch.zeros((n, K + 1))),
                lambda: ops.vec_to_tril_backward(vec, torch.zeros((n, da, da + 1)), da),
                lambda: ops.cov_gaussian_head_logp_backward(mu, vec, x, torch.zeros((n,))),
                lambda: ops.mvnormkldivergence_backward(mu, L, mu, L, torch.zeros(n + 1)),
                lambda: ops.diagnormkldivergence_backward(mu, mu, mu, mu, torch.zeros((n, da))),
                lambda: ops.normkldivergence_backward(e, e, e, e, mu)):
        with pytest.raises(_lib.RLHipArgumentError):
            bad()


def test_grad_module_is_bypassed_when_nothing_requires_grad(stub, monkeypatch):
    import rlhip
    from rlhip import grad, ops

    def boom(*a, **k):
        raise AssertionError("rlhip/grad.py was entered although nothing requires a gradient")

    for cls in (grad.VecToTril, grad.MvNormLogPdf, grad.CovHeadLogp, grad.CovHeadSample, grad.MvNormKL, grad.DiagNormKL, grad.NormKL):
        monkeypatch.setattr(cls, "apply", boom)
    n, da, K = 3, 2, 2
    mu, L, x, vec = torch.zeros((n, da)), torch.zeros((n, da, da)), torch.zeros((n, K, da)), torch.zeros((n, 3))
    net = rlhip.CovGaussianNetwork(mu=lambda s: mu.t(), Sigma=lambda s: vec.t())
    run = lambda: (ops.vec_to_tril(vec, da), ops.mvnormlogpdf(mu, L, x), ops.mvnormkldivergence(mu, L, mu, L),   # noqa: E731
                   ops.diagnormkldivergence(mu, mu, mu, mu), ops.normkldivergence(mu, mu, mu, mu), net(torch.zeros((4, n))),
                   net(torch.zeros((4, n)), torch.zeros((da, n))), net(torch.zeros((4, n)), is_sampling=True, is_return_log_prob=True),
                   net.sample(torch.zeros((4, 1, n)), K))
    run()
    assert len(stub.calls) == 9
    for t in (mu, L, x, vec):
        t.requires_grad_(True)
    with torch.no_grad():                                           # inputs that require grad, but grad mode is off
        run()
    assert len(stub.calls) == 18
    with pytest.raises(AssertionError, match="grad.py was entered"):
        ops.mvnormlogpdf(mu, L, x)
    with pytest.raises(AssertionError, match="grad.py was entered"):
        net(torch.zeros((4, n)), torch.zeros((da, n)))


# ------------------------------------------------------------------------------------------------ the built library
def test_the_six_entry_points_are_exported_with_prototypes():
    from rlhip import _lib

    syms = _lib.declared_symbols()
    for s in SYMS:
        assert s in syms and s in _lib._PROTOS and hasattr(_lib.lib, s), s
    assert _lib.lib.rlhip_abi_version() == 2
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert int(re.search(r"\((\d+) `extern \"C\"` entry points", text).group(1)) == len(syms)
    glue = open(os.path.join(ROOT, "reinforcementlearning.jl_amd", "julia", "RLHip.jl")).read()
    for s in SYMS:
        assert s in text, s
        assert f"ccall((:{s}, LIB)" in glue, s
    for fn in ("mvnormlogpdf", "mvnormkldivergence", "diagnormkldivergence", "normkldivergence", "vec_to_tril"):
        assert f"function ChainRulesCore.rrule(::typeof(ReinforcementLearningCore.{fn})," in glue, fn
    # the (state, action) call is the sub-networks followed by the head function that carries the rule
    assert "function ChainRulesCore.rrule(::typeof(cov_gaussian_logp), μ::DevMatrix, v::DevMatrix, action::DevArray3)" in glue
    call = glue[glue.index("function (m::HipCovGaussianNetwork)(state::DevArray3, action::DevArray3)"):]
    assert "cov_gaussian_logp(μ, v, action)" in call[:call.index("\nend")]


@pytest.mark.parametrize("da", [0, 17, -1])
def test_bad_arguments_are_refused_before_any_device_work(da):
    """argument checks come before any HIP call: RLHIP_EINVAL with a message, no device needed"""
    from rlhip import _lib

    one = (np.zeros(4096, F32)).ctypes.data            # a non-NULL host address: never dereferenced
    L = _lib.lib
    assert L.rlhip_mvnormlogpdf_bwd_f32(one, one, one, one, da, 1, 4, one, one, one, None) == -1 and b"da" in L.rlhip_last_error()
    assert L.rlhip_vec_to_tril_bwd_f32(one, one, da, 4, one, None) == -1
    assert L.rlhip_cov_gaussian_head_logp_bwd_f32(one, one, one, one, da, 4, 1, one, one, None) == -1
    assert L.rlhip_mvnormkldivergence_bwd_f32(one, one, one, one, one, da, 4, one, one, one, one, None) == -1
    # K < 1 and NULL inputs, with a good da
    assert L.rlhip_mvnormlogpdf_bwd_f32(one, one, one, one, 3, 0, 4, one, one, one, None) == -1
    assert L.rlhip_cov_gaussian_head_logp_bwd_f32(one, one, one, one, 3, 4, 0, one, one, None) == -1
    assert L.rlhip_mvnormlogpdf_bwd_f32(one, one, one, None, 3, 1, 4, one, one, one, None) == -1 and b"NULL" in L.rlhip_last_error()
    assert L.rlhip_mvnormlogpdf_bwd_f32(None, one, one, one, 3, 1, 4, one, one, one, None) == -1
    assert L.rlhip_vec_to_tril_bwd_f32(one, None, 3, 4, one, None) == -1
    assert L.rlhip_vec_to_tril_bwd_f32(one, one, 3, 4, None, None) == -1
    assert L.rlhip_cov_gaussian_head_logp_bwd_f32(one, one, None, one, 3, 4, 1, one, one, None) == -1
    assert L.rlhip_mvnormkldivergence_bwd_f32(one, one, one, one, None, 3, 4, one, one, one, one, None) == -1
    assert L.rlhip_diagnormkldivergence_bwd_f32(one, one, one, None, one, 2, 4, one, one, one, one, None) == -1
    assert L.rlhip_diagnormkldivergence_bwd_f32(one, one, one, one, one, 0, 4, one, one, one, one, None) == -1
    assert L.rlhip_normkldivergence_bwd_f32(one, None, one, one, one, 4, one, one, one, one, None) == -1
    assert L.rlhip_normkldivergence_bwd_f32(one, one, one, one, one, -1, one, one, one, one, None) == -1
    # n = 0 and "no output asked for" are no-ops that need no device either
    assert L.rlhip_mvnormlogpdf_bwd_f32(one, one, one, one, 3, 1, 0, one, one, one, None) == 0
    assert L.rlhip_vec_to_tril_bwd_f32(one, one, 3, 0, one, None) == 0
    assert L.rlhip_cov_gaussian_head_logp_bwd_f32(one, one, one, one, 3, 0, 1, one, one, None) == 0
    assert L.rlhip_mvnormkldivergence_bwd_f32(one, one, one, one, one, 3, 0, one, one, one, one, None) == 0
    assert L.rlhip_mvnormkldivergence_bwd_f32(one, one, one, one, one, 3, 4, None, None, None, None, None) == 0
    assert L.rlhip_diagnormkldivergence_bwd_f32(one, one, one, one, one, 2, 0, one, one, one, one, None) == 0
    assert L.rlhip_normkldivergence_bwd_f32(one, one, one, one, one, 0, one, one, one, one, None) == 0


# ------------------------------------------------------------------------------------------------ (e) the wiring of rlhip/grad.py
class _ModelLibrary:
    """a CPU stand-in for the C calls: every entry point of csrc/cov_heads.hip / cov_heads_grad.hip computed by the models on the
    storages it is handed (pointers are the tensors themselves), outputs written in place, NULL outputs skipped"""

    def __init__(self):
        self.calls = []

    @staticmethod
    def _put(out, a):
        if out is not None:
            out.copy_(torch.tensor(J(np.asarray(a, F32))))

    def call(self, name, *a):
        self.calls.append(name)
        n_ = lambda t: J(t.detach().numpy())                                                 # noqa: E731  storage -> Julia shape
        if name == "rlhip_vec_to_tril_f32":
            self._put(a[3], tril_f32(n_(a[0]), a[1]))
        elif name == "rlhip_mvnormlogpdf_f32":
            self._put(a[6], M.mvnormlogpdf(n_(a[0]), n_(a[1]), n_(a[2]))[0].reshape(J(a[6].numpy()).shape))
        elif name == "rlhip_cov_gaussian_head_logp_f32":
            self._put(a[6], M.mvnormlogpdf(n_(a[0]), tril_f32(n_(a[1]), a[3]), n_(a[2]))[0])
        elif name == "rlhip_cov_gaussian_head_sample_f32":
            da, n, K = a[2:5]
            eps = np.random.default_rng(a[7]).normal(size=(da, K, n)).astype(F32)
            L = tril_f32(n_(a[1]), da)
            z = M.sample_replay(n_(a[0]), L, eps)
            self._put(a[8], z)
            self._put(a[9], M.mvnormlogpdf(n_(a[0]), L, z)[0])
            self._put(a[10], L)
        elif name == "rlhip_mvnormkldivergence_f32":
            self._put(a[6], M.mvnormkldivergence(*(n_(t) for t in a[:4]))[0])
        elif name == "rlhip_diagnormkldivergence_f32":
            self._put(a[6], M.diagnormkldivergence(*(n_(t) for t in a[:4]))[0])
        elif name == "rlhip_normkldivergence_f32":
            self._put(a[5], M.normkldivergence(*(n_(t) for t in a[:4]))[0])
        elif name == "rlhip_mvnormlogpdf_bwd_f32":
            g = n_(a[3])
            for out, val in zip(a[7:10], G.mvnormlogpdf_bwd(n_(a[0]), n_(a[1]), n_(a[2]), g)):
                self._put(out, val)
        elif name == "rlhip_vec_to_tril_bwd_f32":
            self._put(a[4], G.vec_to_tril_bwd(n_(a[0]), n_(a[1]))[0])
        elif name == "rlhip_cov_gaussian_head_logp_bwd_f32":
            mu, vec = n_(a[0]), n_(a[1])
            dmu, (c, _) = G.head_logp_bwd(mu, vec, tril_f32(vec, a[4]), n_(a[2]), n_(a[3]))
            self._put(a[7], dmu)
            self._put(a[8], c)
        elif name == "rlhip_mvnormkldivergence_bwd_f32":
            for out, val in zip(a[7:11], G.mvnormkl_bwd(*(n_(t) for t in a[:5]))):
                self._put(out, val)
        elif name == "rlhip_diagnormkldivergence_bwd_f32":
            for out, val in zip(a[7:11], G.diagnormkl_bwd(*(n_(t) for t in a[:5]))):
                self._put(out, val)
        elif name == "rlhip_normkldivergence_bwd_f32":
            for out, val in zip(a[6:10], G.normkl_bwd(*(n_(t) for t in a[:5]))):
                self._put(out, val)
        else:
            pytest.fail(f"unexpected call {name}")
        return 0


@pytest.fixture
def model_lib(monkeypatch):
    lib = _ModelLibrary()
    _patch(monkeypatch, lib.call)
    return lib


def _leaf(a, grad=True):
    return torch.tensor(J(a), dtype=torch.float32, requires_grad=grad)


def _close(t, want):
    return G.approx_tensor(J(t.detach().numpy()), want)


def test_autograd_functions_agree_with_the_model_and_with_float64_autograd(model_lib):
    """saved tensors, the K reshapes and the nullable outputs of every Function: gradients of sum(g * f) through rlhip/grad.py are the
    model's, bit for bit where the model is exact, and `≈` float64 autograd of the reference's formulas; values are the plain call's"""
    from rlhip import ops

    da, n, K = 3, 7, 4
    mu1, vec1, mu2, vec2, x, s1, s2 = _case(da, n, K)
    L1, L2 = tril_f32(vec1, da), tril_f32(vec2, da)
    g = torch.tensor(J(G.cotangent((K, n), 1)))
    # mvnormlogpdf, all three gradients, 3-D and 2-D x
    tm, tL, tx = _leaf(mu1), _leaf(L1), _leaf(x)
    out = ops.mvnormlogpdf(tm, tL, tx)
    with torch.no_grad():
        assert torch.equal(out, ops.mvnormlogpdf(tm, tL, tx)) and out.grad_fn is not None
    (out * g).sum().backward()
    want = G.mvnormlogpdf_bwd(mu1, L1, x, J(g.numpy()))
    for t, w in zip((tm, tL, tx), want):
        assert G.same(J(t.grad.numpy()), w)
    tm2, tx2 = _leaf(mu1), _leaf(x[:, 0, :], False)
    ops.mvnormlogpdf(tm2, _leaf(L1, False), tx2).sum().backward()                     # sum(): an expanded (non-contiguous) cotangent
    assert model_lib.calls[-1] == "rlhip_mvnormlogpdf_bwd_f32" and tx2.grad is None
    assert G.same(J(tm2.grad.numpy()), G.mvnormlogpdf_bwd(mu1, L1, x[:, 0, :], np.ones(n, F32))[0])
    # vec_to_tril -> mvnormlogpdf chained by autograd = the head's pullback
    tv, tm = _leaf(vec1), _leaf(mu1)
    (ops.mvnormlogpdf(tm, ops.vec_to_tril(tv, da), _leaf(x, False)) * g).sum().backward()
    dmu, (c, e) = G.head_logp_bwd(mu1, vec1, L1, x, J(g.numpy()))
    assert G.same(J(tm.grad.numpy()), dmu) and G.same(J(tv.grad.numpy()), c.astype(F32))
    t64m, t64v = t64(mu1), t64(vec1)
    w64 = grads64(mvnormlogpdf64(t64m, vec_to_tril64(t64v, da), t64(x, False)), J(g.numpy()), t64m, t64v)
    assert _close(tm.grad, w64[0]) and _close(tv.grad, w64[1])
    # the KLs, with only some inputs requiring a gradient (NULL outputs)
    gk = torch.tensor(G.cotangent((n,), 3))
    a = [_leaf(mu1, False), _leaf(L1, False), _leaf(mu2), _leaf(L2)]
    (ops.mvnormkldivergence(*a) * gk).sum().backward()
    want = G.mvnormkl_bwd(mu1, L1, mu2, L2, gk.numpy())
    assert a[0].grad is None and a[1].grad is None and G.same(J(a[2].grad.numpy()), want[2]) and G.same(J(a[3].grad.numpy()), want[3])
    ts = [t64(v) for v in (mu1, L1, mu2, L2)]
    assert _close(a[3].grad, grads64(mvnormkl64(*ts), gk.numpy(), ts[3])[0])
    a = [_leaf(v) for v in (mu1, s1, mu2, s2)]
    (ops.diagnormkldivergence(*a) * gk).sum().backward()
    for t, w in zip(a, G.diagnormkl_bwd(mu1, s1, mu2, s2, gk.numpy())):
        assert G.same(J(t.grad.numpy()), w)
    ge = torch.tensor(J(G.cotangent((da, n), 4)))
    a = [_leaf(v) for v in (mu1, s1, mu2, s2)]
    (ops.normkldivergence(*a) * ge).sum().backward()
    for t, w in zip(a, G.normkl_bwd(mu1, s1, mu2, s2, J(ge.numpy()))):
        assert G.same(J(t.grad.numpy()), w)


def test_network_log_probabilities_are_differentiable_through_torch_modules(model_lib):
    """rlhip.CovGaussianNetwork with torch.nn.Linear heads: (state, action), the sampling log-probability and net.sample pull back to
    the modules' weights through ONE fused launch; sampled actions carry no gradient; the float64 torch model gives the same gradients"""
    import rlhip

    torch.manual_seed(0)
    ns, da, n, K = 5, 3, 6, 4
    lin_mu, lin_S = torch.nn.Linear(ns, da), torch.nn.Linear(ns, M.nvec(da))
    col = lambda lin: (lambda s: lin(s.t()).t())                                       # noqa: E731  (ns, n) -> (d, n)
    net = rlhip.CovGaussianNetwork(mu=col(lin_mu), Sigma=col(lin_S), seed=3)
    state, action = torch.randn(ns, n), torch.randn(da, K, n)

    def want(act_julia):
        """the same loss on the float64 torch model -> gradients of the four parameter tensors"""
        ps = [p.detach().double().requires_grad_(True) for p in (lin_mu.weight, lin_mu.bias, lin_S.weight, lin_S.bias)]
        s = state.double().t()
        mu, vec = s @ ps[0].t() + ps[1], s @ ps[2].t() + ps[3]
        lp = mvnormlogpdf64(mu, vec_to_tril64(vec, da), torch.tensor(J(act_julia), dtype=torch.float64))
        return torch.autograd.grad(-lp.mean(), ps)

    def check(loss, act_julia):
        params = (lin_mu.weight, lin_mu.bias, lin_S.weight, lin_S.bias)
        got = torch.autograd.grad(loss, params)
        assert model_lib.calls[-1] == "rlhip_cov_gaussian_head_logp_bwd_f32"
        for a, b in zip(got, want(act_julia)):
            assert G.approx_tensor(a.numpy(), b.numpy())

    lp = net(state.unsqueeze(1), action)
    assert lp.shape == (1, K, n) and lp.requires_grad
    check(-lp.mean(), action.numpy())
    lp2 = net(state, action[:, 0, :])
    assert lp2.shape == (1, n)
    check(-lp2.mean(), action[:, :1, :].numpy())
    a, lp3 = net(state, is_sampling=True, is_return_log_prob=True)
    assert a.shape == (da, n) and not a.requires_grad and lp3.requires_grad and net.step == 1
    check(-lp3.mean(), a.numpy()[:, None, :])
    acts, lps = net.sample(state.unsqueeze(1), K)
    assert acts.shape == (da, K, n) and not acts.requires_grad and lps.shape == (1, K, n) and net.step == 2
    check(-lps.mean(), acts.numpy())
    only = net(state, is_sampling=True)
    assert not only.requires_grad and net.step == 3
    # a gradient for the actions too: the composition (vec_to_tril -> mvnormlogpdf), whose pullback has dx
    act = action.clone().requires_grad_(True)
    net(state.unsqueeze(1), act).sum().backward()
    assert act.grad.shape == (da, K, n) and "rlhip_mvnormlogpdf_bwd_f32" in model_lib.calls[-2:]
    mu, L = net(state)
    assert L.requires_grad and L.shape == (da, da, n)
