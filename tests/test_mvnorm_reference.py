"""The float64 model of csrc/cov_heads.hip (tests/mvnorm_ref.py) against the reference's own test inputs and against planted faults, the
host wrappers' shape handling with the C calls stubbed, and the seven entry points in the built library.  CPU only."""
import json
import os
import re

import numpy as np
import pytest
import torch

import mvnorm_ref as M
from heads_ref import F32, F64, judge

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KAT = json.load(open(os.path.join(ROOT, "tests", "golden", "mvnorm_kat.json")))
SYMS = ["rlhip_vec_to_tril_f32", "rlhip_mvnormlogpdf_f32", "rlhip_cov_gaussian_head_sample_f32", "rlhip_cov_gaussian_head_logp_f32",
        "rlhip_normkldivergence_f32", "rlhip_diagnormkldivergence_f32", "rlhip_mvnormkldivergence_f32"]


def _a(x):
    return np.asarray(x, F32)


def _chol(S):
    """cholesky(S).L as Float32, repeated over a batch of 2: (da, da, 2)"""
    L = np.linalg.cholesky(np.asarray(S, F64)).astype(F32)
    return np.stack([L, L], axis=2)


# ---------------------------------------------------------------------------------------------- the model against the closed forms
def test_hand_checked_closed_forms():
    c = KAT["normal_1d"]
    assert abs(M.normal_kl64(c["mu1"], c["sigma1"], c["mu2"], c["sigma2"]) - (np.log(6 / 5) + 26 / 72 - 0.5)) < 1e-15
    f = KAT["full_cov"]
    m1, m2 = _a(f["mu1"])[:, 0, 0], _a(f["mu2"])[:, 0, 0]
    assert abs(M.mvnormal_kl64(m1, f["Sigma1"], m2, f["Sigma2"]) - 1.0) < 1e-14
    assert abs(M.mvnormal_kl64(m2, f["Sigma2"], m1, f["Sigma1"]) - 1.0) < 1e-14


def test_model_normkldivergence_matches_normal():
    c = KAT["normal_1d"]
    for a, b in (("1", "2"), ("2", "1")):
        got, budget, _ = M.normkldivergence(_a([c["mu" + a]]), _a([c["sigma" + a]]), _a([c["mu" + b]]), _a([c["sigma" + b]]))
        assert M.approx(got, M.normal_kl64(c["mu" + a], c["sigma" + a], c["mu" + b], c["sigma" + b]))
        assert 0 < budget[0] < 1e-6


@pytest.mark.parametrize("case", ["diag_2d", "diag_3d"])
def test_model_diagnormkldivergence_matches_mvnormal(case):
    c = {k: _a(v) for k, v in KAT[case].items() if not k.startswith("_")}
    if case == "diag_3d":                                        # dropdims(..., dims = 2)  (distributions.jl:126-129)
        c = {k: v[:, 0, :] for k, v in c.items()}
    for a, b in (("1", "2"), ("2", "1")):
        got, _, _ = M.diagnormkldivergence(c["mu" + a], c["sigma" + a], c["mu" + b], c["sigma" + b])
        assert got.shape == (2,)
        for i in range(2):
            want = M.mvnormal_kl64(c["mu" + a][:, i], np.diag(c["sigma" + a][:, i].astype(F64) ** 2), c["mu" + b][:, i],
                                   np.diag(c["sigma" + b][:, i].astype(F64) ** 2))
            assert M.approx(got[i], want)
            # a diagonal covariance is a full one with L = Diagonal(sigma)
            L1 = np.stack([np.diag(c["sigma" + a][:, k]) for k in range(2)], axis=2)
            L2 = np.stack([np.diag(c["sigma" + b][:, k]) for k in range(2)], axis=2)
            assert M.approx(M.mvnormkldivergence(c["mu" + a], L1, c["mu" + b], L2)[0][i], want)


def test_model_full_covariance_matches_mvnormal():
    f = KAT["full_cov"]
    mu1, mu2, x = _a(f["mu1"]), _a(f["mu2"]), _a(f["x"])
    L1, L2 = _chol(f["Sigma1"]), _chol(f["Sigma2"])
    lp, budget, _ = M.mvnormlogpdf(mu1[:, 0, :], L1, x)
    assert lp.shape == (1, 2) and (budget > 0).all() and (budget < 1e-5).all()
    for i in range(2):
        assert M.approx(lp[0, i], M.mvnormal_logpdf64(mu1[:, 0, i], f["Sigma1"], x[:, 0, i]))
    assert np.array_equal(M.mvnormlogpdf(mu1[:, 0, :], L1, x[:, 0, :])[0], lp[0])        # the 2-D form is the K = 1 form
    for (ma, La, Sa), (mb, Lb, Sb) in (((mu1, L1, f["Sigma1"]), (mu2, L2, f["Sigma2"])), ((mu2, L2, f["Sigma2"]), (mu1, L1, f["Sigma1"]))):
        kl, _, _ = M.mvnormkldivergence(ma[:, 0, :], La, mb[:, 0, :], Lb)
        assert kl.shape == (2,) and M.approx(kl, np.full(2, M.mvnormal_kl64(ma[:, 0, 0], Sa, mb[:, 0, 0], Sb))) and M.approx(kl, 1.0)


def test_model_vec_to_tril_matches_the_reference_test():
    v = KAT["vec_to_tril"]
    da = v["da"]
    for i in range(1, da + 1):
        for j in range(1, i + 1):
            assert M.tril_index(i, j, da) == v["inds_mat"][i - 1][j - 1]
    vec = np.repeat(_a(v["cholesky_vec"])[:, None], v["batch"], axis=1)
    want = np.array(v["cholesky_mat_raw"], F64)
    for i, j in v["softplusbeta_at"]:
        want[i - 1, j - 1] = np.log(np.exp(want[i - 1, j - 1] / 10.0) + 1.0) * 10.0     # the reference test leaves the 1e-5 to `≈`
    L = _model_tril(vec, da)
    assert L.shape == (da, da, v["batch"])
    for b in range(v["batch"]):
        assert np.linalg.norm(L[:, :, b] - want) <= M.RTOL * max(np.linalg.norm(L[:, :, b]), np.linalg.norm(want))
    M.judge_tril(L, vec, tag="model")


def _model_tril(vec, da, index=M.tril_index, diag=lambda x: M.chol_diag(x).c.astype(F32)):
    """vec_to_tril built from the model (its centre rounded to Float32); `index` / `diag` are where faults are planted"""
    vec = np.asarray(vec, F32)
    L = np.zeros((da, da, vec.shape[1]), F32)
    for i in range(1, da + 1):
        for j in range(1, i + 1):
            x = vec[index(i, j, da) - 1]
            L[i - 1, j - 1] = diag(x) if i == j else x
    return L


# ---------------------------------------------------------------------------------------------- planted faults must not pass
def test_fault_swapped_index_in_the_vector_to_matrix_map():
    mu, vec = M.inputs(4, 9, seed=1)
    M.judge_tril(_model_tril(vec, 4), vec)
    row_major = lambda i, j, da: (i * (i - 1)) // 2 + j                       # noqa: E731  the row-wise packing
    with pytest.raises(AssertionError):
        M.judge_tril(_model_tril(vec, 4, index=row_major), vec)
    pair = {(4, 2): (3, 2), (3, 2): (4, 2)}                                   # two entries of one column exchanged
    swapped = lambda i, j, da: M.tril_index(*pair.get((i, j), (i, j)), da)    # noqa: E731
    with pytest.raises(AssertionError):
        M.judge_tril(_model_tril(vec, 4, index=swapped), vec)


def test_fault_log1p_form_and_missing_floor_at_minus_200():
    vec = np.full((1, 3), -200.0, F32)
    vec[0, 1], vec[0, 2] = -1000.0, 0.5
    naive = lambda x: (np.log(np.exp(x / F32(10)) + F32(1)) * F32(10) + F32(1e-5)).astype(F32)      # noqa: E731  numpy Float32 ops
    good = _model_tril(vec, 1, diag=naive)
    assert good[0, 0, 0] == F32(1e-5) and good[0, 0, 1] == F32(1e-5)              # the floor, exactly
    M.judge_tril(good, vec)
    log1p = lambda x: (np.log1p(np.exp(x / F32(10))) * F32(10) + F32(1e-5)).astype(F32)              # noqa: E731
    assert log1p(vec)[0, 0] != F32(1e-5)
    with pytest.raises(AssertionError):
        M.judge_tril(_model_tril(vec, 1, diag=log1p), vec)
    no_floor = lambda x: (np.log(np.exp(x / F32(10)) + F32(1)) * F32(10)).astype(F32)                # noqa: E731
    with pytest.raises(AssertionError):
        M.judge_tril(_model_tril(vec, 1, diag=no_floor), vec)
    with pytest.raises(AssertionError):                                            # ... and at an ordinary input
        M.judge_tril(_model_tril(np.full((1, 2), 0.5, F32), 1, diag=no_floor), np.full((1, 2), 0.5, F32))


def test_fault_descending_summation():
    """y^2 = [2^24, 1, 1, ...] on a unit L: ascending, every + 1 is absorbed; descending, the fifteen ones arrive as 15"""
    da, n = 16, 3
    mu = np.zeros((da, n), F32)
    L = np.repeat(np.eye(da, dtype=F32)[:, :, None], n, axis=2)
    x = np.ones((da, n), F32)
    x[0] = 4096.0
    good = M._mvnormlogpdf(mu, L, x).c.astype(F32)
    judge(good, *M.mvnormlogpdf(mu, L, x), tag="ascending")
    desc = M._mvnormlogpdf(mu, L, x, order=lambda d: range(d - 1, -1, -1)).c.astype(F32)
    assert not np.array_equal(desc, good)
    with pytest.raises(AssertionError):
        judge(desc, *M.mvnormlogpdf(mu, L, x), tag="descending")


def test_fault_missing_factor_two_on_the_log_determinant():
    mu, vec = M.inputs(5, 11, seed=2)
    L = _model_tril(vec, 5)
    x = (mu + np.random.default_rng(3).normal(size=mu.shape)).astype(F32)
    judge(M._mvnormlogpdf(mu, L, x).c.astype(F32), *M.mvnormlogpdf(mu, L, x), tag="2 ld")
    with pytest.raises(AssertionError):
        judge(M._mvnormlogpdf(mu, L, x, logdet_factor=1).c.astype(F32), *M.mvnormlogpdf(mu, L, x), tag="1 ld")


def test_model_non_finite_patterns():
    """expf overflow -> Inf diagonal -> -Inf log-probability of a finite action; NaN and Inf below the diagonal propagate"""
    mu, vec = M.edge_vectors()
    d = M.chol_diag(vec[[M.tril_index(k, k, 3) - 1 for k in (1, 2, 3)]])
    assert (d.c[0, [0, 3]] == F64(F32(1e-5))).all() and (d.e[0, [0, 3]] < 1e-12).all()      # -1000, -200: the floor, exactly
    assert d.c[0, 12] == np.inf and np.isnan(d.c[0, 15]) and np.isfinite(d.c[0, 9]) and abs(d.c[0, 9] - 880.0) < 1e-3
    L = _model_tril(vec, 3)
    x = np.zeros_like(mu)
    lp, _, _ = M.mvnormlogpdf(mu, L, x)
    assert (lp[12:15] == -np.inf).all() and np.isnan(lp[15:18]).all() and np.isfinite(lp[:12]).all()
    # an Inf below the diagonal makes the rows after it Inf (ss = Inf), a NaN makes them NaN
    assert (lp[[20, 21]] == -np.inf).all() and np.isnan(lp[22]) and np.isfinite(lp[18:20]).all() and np.isfinite(lp[23:]).all()


# ---------------------------------------------------------------------------------------------- the host wrappers, C calls stubbed
class _Stub:
    """records (name, args) of every ABI call the wrappers make; pointers are the tensors themselves"""

    def __init__(self):
        self.calls = []

    def call(self, name, *args):
        self.calls.append((name, args))
        return 0


@pytest.fixture
def stub(monkeypatch):
    from rlhip import heads, ops

    s = _Stub()
    for mod in (heads, ops):
        monkeypatch.setattr(mod, "call", s.call)
        monkeypatch.setattr(mod, "ptr", lambda t: t if t is None else (t.is_contiguous() or pytest.fail("not contiguous")) and t)
        monkeypatch.setattr(mod, "stream_ptr", lambda: None)
    return s


def _net(da, n, **kw):
    import rlhip

    mu, vec = torch.zeros((da, n)), torch.zeros((M.nvec(da), n))
    seen = []
    net = rlhip.CovGaussianNetwork(pre=lambda s: seen.append(tuple(s.shape)) or s, mu=lambda x: mu, Sigma=lambda x: vec, **kw)
    return net, seen


def test_wrapper_call_forms_and_shapes(stub):
    da, n, ns = 10, 3, 20
    net, seen = _net(da, n, seed=9, env_id_base=2)
    state = torch.zeros((ns, n))
    m, L = net(state)
    assert m.shape == (da, n) and L.shape == (da, da, n)
    name, args = stub.calls[-1]
    assert name == "rlhip_vec_to_tril_f32" and args[0].shape == (n, M.nvec(da)) and args[1:3] == (da, n) and args[3].shape == (n, da, da)
    m, L = net(state.unsqueeze(1))
    assert m.shape == (da, 1, n) and L.shape == (da, da, n) and seen[-1] == (ns, n)
    assert net.step == 0
    a, lp = net(state, is_sampling=True, is_return_log_prob=True)
    assert a.shape == (da, n) and lp.shape == (1, n) and net.step == 1
    name, args = stub.calls[-1]
    assert name == "rlhip_cov_gaussian_head_sample_f32"
    assert args[0].shape == (n, da) and args[1].shape == (n, M.nvec(da)) and args[2:8] == (da, n, 1, 9, 2, 0)
    assert args[8].shape == (n, 1, da) and args[9].shape == (n, 1) and args[10] is None
    only = net(state, is_sampling=True)
    assert only.shape == (da, n) and stub.calls[-1][1][9] is None and stub.calls[-1][1][7] == 1 and net.step == 2
    a3, lp3 = net(state.unsqueeze(1), is_sampling=True, is_return_log_prob=True)
    assert a3.shape == (da, 1, n) and lp3.shape == (1, 1, n) and net.step == 3
    acts, lps = net.sample(state.unsqueeze(1), 5)
    assert acts.shape == (da, 5, n) and lps.shape == (1, 5, n) and net.step == 4
    assert stub.calls[-1][1][2:5] == (da, n, 5) and stub.calls[-1][1][8].shape == (n, 5, da)
    out = net(state, a)
    assert out.shape == (1, n) and net.step == 4
    name, args = stub.calls[-1]
    assert name == "rlhip_cov_gaussian_head_logp_f32" and args[2].shape == (n, 1, da) and args[3:6] == (da, n, 1) and args[7] is None
    out = net(state.unsqueeze(1), acts)
    assert out.shape == (1, 5, n) and stub.calls[-1][1][3:6] == (da, n, 5)
    # the storage handed over is the reference's column-major array: element (k, j, i) at (i K + j) da + k
    marked = torch.arange(da * 5 * n, dtype=torch.float32).reshape(da, 5, n)
    net(state.unsqueeze(1), marked)
    flat = stub.calls[-1][1][2].reshape(-1)
    assert flat[(2 * 5 + 3) * da + 7] == marked[7, 3, 2]
    act, lp, Lo = net._sample(torch.zeros((da, n)), torch.zeros((M.nvec(da), n)), 2, True, want_L=True)
    assert act.shape == (n, 2, da) and lp.shape == (n, 2) and Lo.shape == (n, da, da)
    with pytest.raises(ValueError):
        bad, _ = _net(da, n)
        bad.Sigma = lambda x: torch.zeros((da * da, n))
        bad(state)
    with pytest.raises(ValueError):
        net(state, torch.zeros((da + 1, n)))


def test_ops_wrappers_shapes(stub):
    from rlhip import _lib, ops

    n, da, K = 6, 4, 3
    mu, L = torch.zeros((n, da)), torch.zeros((n, da, da))
    assert ops.vec_to_tril(torch.zeros((n, M.nvec(da))), da).shape == (n, da, da)
    assert stub.calls[-1][0] == "rlhip_vec_to_tril_f32" and stub.calls[-1][1][1:3] == (da, n)
    assert ops.mvnormlogpdf(mu, L, torch.zeros((n, K, da))).shape == (n, K)
    assert stub.calls[-1][0] == "rlhip_mvnormlogpdf_f32" and stub.calls[-1][1][3:6] == (da, K, n)
    assert ops.mvnormlogpdf(mu, L, torch.zeros((n, da))).shape == (n,) and stub.calls[-1][1][3:6] == (da, 1, n)
    assert ops.mvnormkldivergence(mu, L, mu, L).shape == (n,) and stub.calls[-1][1][4:6] == (da, n)
    assert ops.diagnormkldivergence(mu, mu, mu, mu).shape == (n,) and stub.calls[-1][1][4:6] == (da, n)
    e = torch.zeros((5, 7))
    assert ops.normkldivergence(e, e, e, e).shape == (5, 7) and stub.calls[-1][1][4] == 35
    for bad in (lambda: ops.vec_to_tril(torch.zeros((n, 9)), da), lambda: ops.mvnormlogpdf(mu, L, torch.zeros((n, K, da + 1))),
                lambda: ops.mvnormkldivergence(mu, L, mu, torch.zeros((n, da, da + 1))),
                lambda: ops.diagnormkldivergence(mu, mu, mu, torch.zeros((n, da + 1))), lambda: ops.normkldivergence(e, e, e, mu)):
        with pytest.raises(_lib.RLHipArgumentError):
            bad()


# ---------------------------------------------------------------------------------------------- the built library
def test_the_seven_entry_points_are_exported_with_prototypes():
    import rlhip
    from rlhip import _lib

    syms = _lib.declared_symbols()
    for s in SYMS:
        assert s in syms and s in _lib._PROTOS and hasattr(_lib.lib, s), s
    assert rlhip.CovGaussianNetwork is rlhip.heads.CovGaussianNetwork
    assert _lib.lib.rlhip_abi_version() == 2
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert int(re.search(r"\((\d+) `extern \"C\"` entry points", text).group(1)) == len(syms)
    for s in SYMS:
        assert s in text, s
    glue = open(os.path.join(ROOT, "reinforcementlearning.jl_amd", "julia", "RLHip.jl")).read()
    for s in SYMS:
        assert f"ccall((:{s}, LIB)" in glue, s
    assert "mutable struct HipCovGaussianNetwork" in glue


@pytest.mark.parametrize("da", [0, 17, -1])
def test_bad_da_and_null_outputs_are_refused_before_any_device_work(da):
    """argument checks come before any HIP call: RLHIP_EINVAL with a message, no device needed"""
    from rlhip import _lib

    one = (np.zeros(4096, F32)).ctypes.data            # a non-NULL host address: never dereferenced
    L = _lib.lib
    assert L.rlhip_vec_to_tril_f32(one, da, 4, one, None) == -1 and b"da" in L.rlhip_last_error()
    assert L.rlhip_mvnormlogpdf_f32(one, one, one, da, 1, 4, one, None) == -1
    assert L.rlhip_cov_gaussian_head_sample_f32(one, one, da, 4, 1, 0, 0, 0, one, one, one, None) == -1
    assert L.rlhip_cov_gaussian_head_logp_f32(one, one, one, da, 4, 1, one, one, None) == -1
    assert L.rlhip_mvnormkldivergence_f32(one, one, one, one, da, 4, one, None) == -1
    # NULL outputs / inputs and K < 1, with a good da
    assert L.rlhip_vec_to_tril_f32(one, 3, 4, None, None) == -1 and b"NULL" in L.rlhip_last_error()
    assert L.rlhip_mvnormlogpdf_f32(one, one, one, 3, 1, 4, None, None) == -1
    assert L.rlhip_cov_gaussian_head_sample_f32(one, one, 3, 4, 1, 0, 0, 0, None, one, one, None) == -1
    assert L.rlhip_cov_gaussian_head_sample_f32(one, one, 3, 4, 0, 0, 0, 0, one, one, one, None) == -1
    assert L.rlhip_cov_gaussian_head_logp_f32(one, one, one, 3, 4, 1, None, one, None) == -1
    assert L.rlhip_normkldivergence_f32(one, one, one, one, 4, None, None) == -1
    assert L.rlhip_diagnormkldivergence_f32(one, one, one, one, 0, 4, one, None) == -1
    assert L.rlhip_diagnormkldivergence_f32(one, one, one, one, 2, 4, None, None) == -1
    assert L.rlhip_mvnormkldivergence_f32(one, one, one, one, 3, 4, None, None) == -1
    # n = 0 is a no-op that needs no device either
    assert L.rlhip_cov_gaussian_head_sample_f32(one, one, 3, 0, 1, 0, 0, 0, one, None, None, None) == 0
    assert L.rlhip_mvnormkldivergence_f32(one, one, one, one, 3, 0, one, None) == 0
