"""The quantile-regression (QR-DQN) learner as include/rlhip.h states it (its QR-DQN section is the specification), twice, with no GPU:

  (a) `replay`: the per-sample lines replayed in numpy Float32 in the header's order -- layer 1 and every output row one fmaf chain (an
      fmaf is the exact Float64 product and sum, rounded once more to Float32), Q the ascending sum of an action's quantiles over
      (float)N, T_j one fmaf, then per (k, j) the Huber value and slope over kappa and the two fmaf chains rho_k, d_k over j ascending.
      There is no libm call on the path.  The batch sums (loss, every gradient element) are accumulated in Float64: the device's fixed
      Float32 order is judged against them.
  (b) `torch_model`: the mathematics alone in float64 torch -- rho^kappa_tau(u) = |tau - 1{u < 0}| L_kappa(u) / kappa with
      tau_k = (2 k + 1) / (2 N), summed over k, mean over j, mean over the batch; the target and the selection without gradient --
      differentiated by autograd, no hand pullback.  The ReLU masks are taken from (a) (the census of tests/qrdqn_cases.py keeps every
      pre-activation off zero), a* is the model's OWN decision.  `fault=` plants a misreading of the text.

`budgets` bounds Q, T and ql of a Float32 evaluation against exact arithmetic: sac_ref.net_error for the rows, then first order through
the mean, the target line and the pairwise term (whose slope in u is at most min(|u|, kappa) / kappa <= 1, and which is continuous at
u = 0 although its weight jumps there) plus half an ulp per rounded operation; the bar is 2 x budget (`within`).
Shared by tests/test_qrdqn_reference.py (CPU), tests/test_gpu_qrdqn_kernels.py and tests/test_gpu_qrdqn_learner.py."""
import numpy as np

from c51_ref import _net64, _t, chain_sum, discount, gamma_pow, rel, within  # noqa: F401
from heads_ref import F32, F64
from sac_ref import U32, act_der, fma, forward, join, net_error, nparams, split  # noqa: F401


def taus(N):
    """tau_k = (float)(2 k + 1) / (float)(2 N)"""
    return (np.arange(N).astype(F32) * F32(2) + F32(1)).astype(F32) / F32(2 * N)


def mean_q(l, na, N):
    """rows (na N, B), row k + N o -> th (na, N, B), Q (na, B) = (sum_k th, k ascending) / (float)N"""
    th = np.asarray(l, F32).reshape(na, N, -1)
    return th, (chain_sum(th.transpose(1, 0, 2)) / F32(N)).astype(F32)


def huber(u, kappa):
    """-> (hub / kappa, dhub / kappa) in Float32, every operation rounded, as the header writes them"""
    kappa = F32(kappa)
    au = np.abs(u)
    with np.errstate(all="ignore"):
        inside = ((F32(0.5) * u).astype(F32) * u).astype(F32)
        outside = (kappa * (au - (F32(0.5) * kappa).astype(F32)).astype(F32)).astype(F32)
        hub = np.where(au <= kappa, inside, outside).astype(F32)
        dhub = np.minimum(np.maximum(u, -kappa), kappa).astype(F32)
        return (hub / kappa).astype(F32), (dhub / kappa).astype(F32)


def pairwise(T, th, kappa):
    """T (Nj, B), th (Nk, B) -> rho (Nk, B), d (Nk, B): the two fmaf chains over j ascending; u (Nj, Nk, B)"""
    N = th.shape[0]
    tau = taus(N)[:, None]
    one_minus = (F32(1) - tau).astype(F32)
    rho, d = np.zeros(th.shape, F32), np.zeros(th.shape, F32)
    us = np.zeros((T.shape[0],) + th.shape, F32)
    for j in range(T.shape[0]):
        u = (T[j][None, :] - th).astype(F32)
        hk, dk = huber(u, kappa)
        w = np.where(u < 0, one_minus, tau).astype(F32)
        rho, d = fma(w, hk, rho), fma(w, dk, d)
        us[j] = u
    return rho, d, us


def replay(c):
    """-> dict(qt, qo, sel, T, ql, loss, grad, hid*, z1*, u, ...) for a case of tests/qrdqn_cases.py"""
    ns, h, na, N, act, B = c["ns"], c["h"], c["na"], c["N"], c["act"], c["batch"]
    M = na * N
    s, sn, a, r = (np.asarray(c[k]) for k in ("s", "sn", "a", "r"))
    r = r.astype(F32)
    cols = np.arange(B)
    lt, hid_t, z1_t = forward(c["target"], ns, h, M, act, sn)
    tht, qt = mean_q(lt, na, N)
    out = dict(lt=lt, tht=tht, qt=qt, hid_t=hid_t, z1_t=z1_t, qo=None, z1_o=None, hid_o=None, lo=None)
    qsel = qt
    if c["double"]:
        lo, hid_o, z1_o = forward(c["params"], ns, h, M, act, sn)
        _, qo = mean_q(lo, na, N)
        out.update(qo=qo, z1_o=z1_o, hid_o=hid_o, lo=lo)
        qsel = qo
    sel = np.argmax(qsel, axis=0).astype(np.int32)  # the first maximum
    cc = discount(c)
    thn = tht[sel, :, cols].T.copy()  # (N, B)
    T = fma(cc[None, :], thn, r[None, :])
    l, hid, z1 = forward(c["params"], ns, h, M, act, s)
    known = (a >= 0) & (a < na)
    ac = np.where(known, a, 0)
    tha = l.reshape(na, N, B)[ac, :, cols].T.copy()  # (N, B)
    rho, d, u = pairwise(T, tha, c["kappa"])
    L = (chain_sum(rho) / F32(N)).astype(F32)
    with np.errstate(all="ignore"):
        g = ((-d).astype(F32) / (F32(N) * F32(B)).astype(F32)).astype(F32)
    Lw = L
    if c.get("weights") is not None:
        w = np.asarray(c["weights"], F32)
        g = (g * w[None, :]).astype(F32)
        Lw = (L * w).astype(F32)
    g[:, ~known] = 0
    ql = np.where(known, L, F32(0)).astype(F32)
    loss = float(Lw[known].astype(F64).sum() / float(F32(B)))
    # back-propagation through rows k + N a_i only
    W1, b1, W2, b2 = split(np.asarray(c["params"], F32), ns, h, M)
    dh = np.zeros((h, B), F32)
    dl = np.zeros((M, B), F32)
    for k in range(N):
        rows = k + N * ac
        dh = fma(g[k][None, :], W2[rows, :].T, dh)
        dl[rows, cols] = g[k]
    dz = (dh * act_der(act, hid)).astype(F32)
    dz[:, ~known] = 0
    gW2 = dl.astype(F64) @ hid.astype(F64).T
    gW1 = dz.astype(F64) @ np.asarray(s, F64).T
    grad = join(gW1, dz.astype(F64).sum(1), gW2, dl.astype(F64).sum(1))
    out.update(sel=sel, cc=cc, thn=thn, T=T, l=l, tha=tha, rho=rho, d=d, u=u, g=g, ql=ql, loss=loss, grad=grad, hid=hid, z1=z1, known=known)
    return out


def forward_replay(c, obs):
    """rlhip_qrdqn_forward_f32 on obs (ns, n) -> (q (na, n), quantiles (na N, n))"""
    l, _, _ = forward(c["params"], c["ns"], c["h"], c["na"] * c["N"], c["act"], obs)
    return mean_q(l, c["na"], c["N"])[1], l


# ------------------------------------------------------------------------------------------------ (b) float64 autograd
FAULTS = ("tau_low", "indicator", "transposed", "no_kappa", "rows", "wrong_net_argmax", "no_cont", "gamma_not_pow", "target_differentiated",
          "weighted_ql")


def torch_model(c, rp, fault=None):
    """-> dict(grad, loss, ql, T, sel, gap, qt, qo) in float64; rp = replay(c) gives the ReLU masks"""
    import torch

    ns, h, na, N, act, B = c["ns"], c["h"], c["na"], c["N"], c["act"], c["batch"]
    M = na * N
    relu = lambda hv: (np.asarray(hv) > 0).astype(F64)  # noqa: E731
    kappa = float(F32(c["kappa"]))

    def shaped(l):  # (M, B) -> (na, N, B)
        return l.reshape(N, na, B).permute(1, 0, 2) if fault == "rows" else l.reshape(na, N, B)

    params, target = _t(c["params"], True), _t(c["target"])
    if fault == "target_differentiated":
        target = params
    s, sn = _t(c["s"]), _t(c["sn"])
    tht = shaped(_net64(target, ns, h, M, act, sn, relu(rp["hid_t"])))
    qt = tht.mean(1)
    qo = None
    if c["double"]:
        qo = shaped(_net64(params, ns, h, M, act, sn, relu(rp["hid_o"]))).mean(1).detach()
    qsel = qo if (c["double"] and fault != "wrong_net_argmax") else qt.detach()
    if fault == "wrong_net_argmax" and not c["double"]:
        raise ValueError("wrong_net_argmax needs a double_dqn case")
    sel = torch.argmax(qsel, 0)
    top = torch.sort(qsel, 0, descending=True).values
    gap = (top[0] - top[1]).numpy() if na > 1 else np.full(B, np.inf)
    cols = torch.arange(B)
    cc = _t(discount(dict(c, _fault_gamma=fault == "gamma_not_pow")))
    if fault == "no_cont":
        cc = torch.full((B,), float(F32(c["gamma"])), dtype=torch.float64) if c.get("n_used") is None else \
            _t(discount(dict(c, term=np.zeros(B, np.uint8))))
    T = _t(c["r"])[:, None] + cc[:, None] * tht[sel, :, cols]  # (B, Nj)
    if fault != "target_differentiated":
        T = T.detach()
    a = np.asarray(c["a"])
    known = torch.tensor((a >= 0) & (a < na))
    ac = torch.tensor(np.where((a >= 0) & (a < na), a, 0))
    th = shaped(_net64(params, ns, h, M, act, s, relu(rp["hid"])))[ac, :, cols]  # (B, Nk)
    u = T[:, None, :] - th[:, :, None]  # (B, k, j)
    au = u.abs()
    hub = torch.where(au <= kappa, 0.5 * u * u, kappa * (au - 0.5 * kappa))
    k = torch.arange(N, dtype=torch.float64)
    tau = k / N if fault == "tau_low" else (2.0 * k + 1.0) / (2.0 * N)
    tau = tau[None, None, :] if fault == "transposed" else tau[None, :, None]
    below = (u > 0) if fault == "indicator" else (u < 0)
    rho = (tau - below.to(torch.float64)).abs() * hub
    if fault != "no_kappa":
        rho = rho / kappa
    ql = rho.sum(1).mean(1)
    ql = torch.where(known, ql, torch.zeros_like(ql))
    w_is = _t(c["weights"]) if c.get("weights") is not None else torch.ones(B, dtype=torch.float64)
    loss = (w_is * ql).sum() / B
    loss.backward()
    ql_out = (w_is * ql) if fault == "weighted_ql" else ql
    return dict(grad=params.grad.numpy().copy(), loss=float(loss.detach()), ql=ql_out.detach().numpy(), T=T.detach().numpy().T.copy(),
                sel=sel.numpy().astype(np.int32), gap=gap, qt=qt.detach().numpy(), qo=None if qo is None else qo.numpy())


# ---------------------------------------------------------------------------------------------- per-sample error budgets
def mean_budget(l, e_l, na, N):
    """-> budget of Q (na, B) from rows l (M, B) with error bound e_l (M, B): the rows' errors averaged, N adds and one division"""
    al = np.abs(np.asarray(l, F64)).reshape(na, N, -1)
    return np.asarray(e_l, F64).reshape(na, N, -1).sum(1) / N + (N + 1) * U32 * al.sum(1) / N


def budgets(c, rp):
    """-> dict(q_t, q_o (na, B), T (N, B), ql (B,)) of absolute error bounds for the values of replay `rp`"""
    ns, h, na, N, act, B = c["ns"], c["h"], c["na"], c["N"], c["act"], c["batch"]
    M = na * N
    cols = np.arange(B)
    kappa = float(F32(c["kappa"]))
    e_lt = net_error(c["target"], ns, h, M, act, c["sn"])
    out = dict(q_t=mean_budget(rp["lt"], e_lt, na, N), q_o=None)
    if c["double"]:
        out["q_o"] = mean_budget(rp["lo"], net_error(c["params"], ns, h, M, act, c["sn"]), na, N)
    cc, r = rp["cc"].astype(F64), np.asarray(c["r"], F64)
    e_thn = e_lt.reshape(na, N, B)[rp["sel"], :, cols].T  # (N, B)
    b_T = np.abs(cc)[None, :] * e_thn + U32 * (np.abs(cc[None, :] * rp["thn"].astype(F64)) + np.abs(r)[None, :])
    out["T"] = b_T
    e_l = net_error(c["params"], ns, h, M, act, c["s"])
    ac = np.where(rp["known"], np.asarray(c["a"]), 0)
    e_th = e_l.reshape(na, N, B)[ac, :, cols].T  # (Nk, B)
    u = rp["u"].astype(F64)  # (Nj, Nk, B)
    e_u = b_T[:, None, :] + e_th[None, :, :] + U32 * np.abs(u)
    au = np.abs(u)
    hub = np.where(au <= kappa, 0.5 * u * u, kappa * (au - 0.5 * kappa)) / kappa  # <= the term: the weight is at most 1
    e_pair = e_u * np.minimum(au + e_u, kappa) / kappa + 8.0 * U32 * hub
    rho = rp["rho"].astype(F64)
    b_rho = e_pair.sum(0) + (N + 1) * U32 * rho
    L = rho.sum(0) / N
    out["ql"] = np.where(rp["known"], (b_rho.sum(0) + (N + 1) * U32 * rho.sum(0)) / N + U32 * L, 0.0)
    return out
