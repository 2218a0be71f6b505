"""The categorical (C51) learner as include/rlhip.h states it (its C51 section is the specification), twice, with no GPU:

  (a) `replay`: the per-sample lines replayed in numpy Float32 in the header's order -- layer 1 and every logit one fmaf chain (an fmaf
      is the exact Float64 product and sum, rounded once more to Float32), the softmax sums, Q, the projection and the cross-entropy
      chains in ascending order.  numpy's Float32 exp / log stand in for expf / logf (the budgets below carry their error).  The batch
      sums (loss, every gradient element) are accumulated in Float64: the device's fixed Float32 order is judged against them.
  (b) `torch_model`: the mathematics in float64 torch -- softmax, the dense projection, cross-entropy; the target and the selection
      without gradient -- differentiated by autograd, no hand pullback.  The ReLU masks are taken from (a) (the census of
      tests/c51_cases.py keeps every pre-activation off zero), a* is the model's OWN decision.  `fault=` plants a misreading of the text.

`budgets` bounds q, probs, proj and ce of a Float32 evaluation against exact arithmetic: sac_ref.net_error for the logits, then first
order through softmax / projection / cross-entropy plus half an ulp per rounded operation (4 ulp for exp and log); the bar is 2 x
budget (`within`).  `project` is the general projection helper of the model (Dopamine's project_distribution).
Shared by tests/test_c51_reference.py (CPU), tests/test_gpu_c51_kernels.py and tests/test_gpu_c51_learner.py."""
import numpy as np

from heads_ref import F32, F64, ulp
from sac_ref import U32, act_der, fma, forward, join, net_error, nparams, split  # noqa: F401

GPOW_MAX = 32


def gamma_pow(gamma, n):
    """rlhip_gamma_pow: evaluated in Float64 and rounded once"""
    return F32(F64(F32(gamma)) ** int(n))


def support(c):
    """-> (Delta, z (n_atoms,)) as the header rounds them"""
    K = c["n_atoms"]
    delta = F32((F32(c["v_max"]) - F32(c["v_min"])) / F32(K - 1))
    return delta, fma(np.arange(K).astype(F32), delta, F32(c["v_min"]))


def chain_sum(x):
    """adds along axis 0 in ascending order, from +0, in Float32"""
    acc = np.zeros(x.shape[1:], F32)
    for k in range(x.shape[0]):
        acc = (acc + x[k]).astype(F32)
    return acc


def dist(logits, na, K, z):
    """logits (na K, B), row k + K o -> p (na, K, B), Q (na, B), mx, S, e"""
    l = np.asarray(logits, F32).reshape(na, K, -1)
    mx = l.max(1)
    with np.errstate(all="ignore"):
        e = np.exp((l - mx[:, None, :]).astype(F32)).astype(F32)
    S = chain_sum(e.transpose(1, 0, 2))
    p = (e / S[:, None, :]).astype(F32)
    q = np.zeros(S.shape, F32)
    for k in range(K):
        q = fma(z[k], p[:, k, :], q)
    return p, q, mx, S, e


def discount(c):
    """c_i = disc * cont per sample (Float32)"""
    B = c["batch"]
    cont = np.where(np.asarray(c["term"]) != 0, F32(0), F32(1)).astype(F32)
    if c.get("n_used") is not None and not c.get("_fault_gamma"):
        pw = np.array([gamma_pow(c["gamma"], n) for n in range(GPOW_MAX + 1)], F32)
        disc = pw[np.clip(np.asarray(c["n_used"]), 0, GPOW_MAX)]
    else:
        disc = np.full(B, F32(c["gamma"]), F32)
    return (disc * cont).astype(F32)


def projection(z, delta, v_min, v_max, r, cc, pt):
    """the dense projection: pt (K, B) over the atoms j -> m (K, B), Tz (K, B)"""
    K = z.shape[0]
    tz = np.clip((r[None, :] + (cc[None, :] * z[:, None]).astype(F32)).astype(F32), F32(v_min), F32(v_max)).astype(F32)
    m = np.zeros(pt.shape, F32)
    for j in range(K):
        w = np.clip((F32(1) - (np.abs((tz[j][None, :] - z[:, None]).astype(F32)) / delta).astype(F32)).astype(F32), F32(0), F32(1))
        m = fma(w.astype(F32), pt[j][None, :], m)
    return m, tz


def replay(c):
    """-> dict(q_t, q_o, sel, proj, tz, ce, loss, grad, hid*, z1*, ...) for a case of tests/c51_cases.py"""
    ns, h, na, K, act, B = c["ns"], c["h"], c["na"], c["n_atoms"], c["act"], c["batch"]
    M = na * K
    delta, z = support(c)
    s, sn, a, r = (np.asarray(c[k]) for k in ("s", "sn", "a", "r"))
    r = r.astype(F32)
    cols = np.arange(B)
    lt, hid_t, z1_t = forward(c["target"], ns, h, M, act, sn)
    pt, qt, _, _, _ = dist(lt, na, K, z)
    out = dict(delta=delta, z=z, lt=lt, pt=pt, qt=qt, hid_t=hid_t, z1_t=z1_t, qo=None, z1_o=None, hid_o=None, lo=None)
    qsel = qt
    if c["double"]:
        lo, hid_o, z1_o = forward(c["params"], ns, h, M, act, sn)
        po, qo, _, _, _ = dist(lo, na, K, z)
        out.update(qo=qo, z1_o=z1_o, hid_o=hid_o, lo=lo, po=po)
        qsel = qo
    sel = np.argmax(qsel, axis=0).astype(np.int32)  # the first maximum
    cc = discount(c)
    ptj = pt[sel, :, cols].T.copy()  # (K, B)
    m, tz = projection(z, delta, c["v_min"], c["v_max"], r, cc, ptj)
    if c.get("m_scale") is not None:
        m = (m * F32(c["m_scale"])).astype(F32)
    l, hid, z1 = forward(c["params"], ns, h, M, act, s)
    known = (a >= 0) & (a < na)
    ac = np.where(known, a, 0)
    la = l.reshape(na, K, B)[ac, :, cols].T.copy()  # (K, B)
    mx = la.max(0)
    with np.errstate(all="ignore"):
        e = np.exp((la - mx[None, :]).astype(F32)).astype(F32)
        S = chain_sum(e)
        logS = np.log(S).astype(F32)
    lp = ((la - mx[None, :]).astype(F32) - logS[None, :]).astype(F32)
    acc = np.zeros(B, F32)
    for k in range(K):
        acc = fma(m[k], lp[k], acc)
    L = (-acc).astype(F32)
    Sm = chain_sum(m)
    p = (e / S[None, :]).astype(F32)
    g = (((p * Sm[None, :]).astype(F32) - m).astype(F32) / F32(B)).astype(F32)
    Lw = L
    if c.get("weights") is not None:
        w = np.asarray(c["weights"], F32)
        g = (g * w[None, :]).astype(F32)
        Lw = (L * w).astype(F32)
    g[:, ~known] = 0
    ce = np.where(known, L, F32(0)).astype(F32)
    loss = float(Lw[known].astype(F64).sum() / float(F32(B)))
    # back-propagation through rows k + K a_i only
    W1, b1, W2, b2 = split(np.asarray(c["params"], F32), ns, h, M)
    dh = np.zeros((h, B), F32)
    d = np.zeros((M, B), F32)
    for k in range(K):
        rows = k + K * ac
        dh = fma(g[k][None, :], W2[rows, :].T, dh)
        d[rows, cols] = g[k]
    dz = (dh * act_der(act, hid)).astype(F32)
    dz[:, ~known] = 0
    gW2 = d.astype(F64) @ hid.astype(F64).T
    gW1 = dz.astype(F64) @ np.asarray(s, F64).T
    grad = join(gW1, dz.astype(F64).sum(1), gW2, d.astype(F64).sum(1))
    out.update(sel=sel, cc=cc, ptj=ptj, proj=m, tz=tz, l=l, la=la, lp=lp, p=p, mx=mx, S=S, logS=logS, Sm=Sm, g=g, ce=ce, loss=loss,
               grad=grad, hid=hid, z1=z1, known=known)
    return out


def forward_replay(c, obs):
    """rlhip_c51_forward_f32 on obs (ns, n) -> (q (na, n), probs (na K, n), logits (na K, n))"""
    na, K = c["na"], c["n_atoms"]
    _, z = support(c)
    l, _, _ = forward(c["params"], c["ns"], c["h"], na * K, c["act"], obs)
    p, q, _, _, _ = dist(l, na, K, z)
    return q, p.reshape(na * K, -1), l


# ------------------------------------------------------------------------------------------------ (b) float64 autograd
FAULTS = ("rows", "scatter", "no_clamp", "wrong_net_argmax", "no_cont", "sm_one", "weighted_ce", "gamma_not_pow", "target_differentiated")


def _t(x, grad=False):
    import torch

    return torch.tensor(np.asarray(x, F64), dtype=torch.float64, requires_grad=grad)


def _net64(p, ni, h, no, act, x, mask):
    import torch

    o1, o2, o3 = h * ni, h * ni + h, h * ni + h + no * h
    W1, b1, W2, b2 = p[:o1].reshape(ni, h).t(), p[o1:o2], p[o2:o3].reshape(h, no).t(), p[o3:]
    zz = W1 @ x + b1[:, None]
    hv = zz * _t(mask) if act == 0 else torch.tanh(zz)
    return W2 @ hv + b2[:, None]


def project(supports, weights, target_support):
    """the model's general projection helper (Dopamine's project_distribution / the Zoo's): mass `weights` (..., n) sitting at `supports`
    (..., n) onto the equally spaced `target_support` (K,): clip the supports into the target's range, then every source point gives
    clamp(1 - |x - z_k| / Delta, 0, 1) of its mass to atom k.  torch float64 in, (..., K) out."""
    import torch

    zt = torch.as_tensor(target_support, dtype=torch.float64)
    delta = (zt[-1] - zt[0]) / (zt.numel() - 1)
    x = torch.clamp(torch.as_tensor(supports, dtype=torch.float64), float(zt[0]), float(zt[-1]))
    w = torch.clamp(1.0 - (x[..., :, None] - zt).abs() / delta, 0.0, 1.0)  # (..., n, K)
    return (w * torch.as_tensor(weights, dtype=torch.float64)[..., :, None]).sum(-2)


def _scatter(x, weights, zt, v_min, delta):
    """the floor / ceil scatter form (a MISREADING here): a point exactly on an atom has l = u and loses its mass"""
    import torch

    b = (x - v_min) / delta
    lo, up = torch.floor(b), torch.ceil(b)
    K = zt.numel()
    m = torch.zeros(x.shape[:-1] + (K,), dtype=torch.float64)
    m.scatter_add_(-1, lo.long().clamp(0, K - 1), weights * (up - b))
    m.scatter_add_(-1, up.long().clamp(0, K - 1), weights * (b - lo))
    return m


def torch_model(c, rp, fault=None):
    """-> dict(grad, loss, ce, proj, sel, gap, qt, qo, probs_t) in float64; rp = replay(c) gives the ReLU masks and the Float32
    constants (Delta, z) of the support"""
    import torch

    ns, h, na, K, act, B = c["ns"], c["h"], c["na"], c["n_atoms"], c["act"], c["batch"]
    M = na * K
    relu = lambda hv: (np.asarray(hv) > 0).astype(F64)  # noqa: E731
    z, delta = _t(rp["z"]), float(rp["delta"])
    v_min, v_max = float(F32(c["v_min"])), float(F32(c["v_max"]))

    def shaped(l):  # (M, B) -> (na, K, B)
        return l.reshape(K, na, B).permute(1, 0, 2) if fault == "rows" else l.reshape(na, K, B)

    params, target = _t(c["params"], True), _t(c["target"])
    if fault == "target_differentiated":
        target = params
    s, sn = _t(c["s"]), _t(c["sn"])
    pt = torch.softmax(shaped(_net64(target, ns, h, M, act, sn, relu(rp["hid_t"]))), 1)
    qt = (pt * z[None, :, None]).sum(1)
    qo = None
    if c["double"]:
        po = torch.softmax(shaped(_net64(params, ns, h, M, act, sn, relu(rp["hid_o"]))), 1)
        qo = (po * z[None, :, None]).sum(1).detach()
    qsel = qo if (c["double"] and fault != "wrong_net_argmax") else qt.detach()
    if fault == "wrong_net_argmax" and not c["double"]:
        raise ValueError("wrong_net_argmax needs a double_dqn case")
    sel = torch.argmax(qsel, 0)
    top = torch.sort(qsel, 0, descending=True).values
    gap = (top[0] - top[1]).numpy() if na > 1 else np.full(B, np.inf)
    cols = torch.arange(B)
    ptj = pt[sel, :, cols]  # (B, K)
    cc = _t(discount(dict(c, _fault_gamma=fault == "gamma_not_pow")))
    if fault == "no_cont":
        cc = torch.full((B,), float(F32(c["gamma"])), dtype=torch.float64) if c.get("n_used") is None else \
            _t(discount(dict(c, term=np.zeros(B, np.uint8))))
    tz = _t(c["r"])[:, None] + cc[:, None] * z[None, :]  # (B, K)
    if fault == "scatter":
        m = _scatter(torch.clamp(tz, v_min, v_max), ptj, z, v_min, delta)
    elif fault == "no_clamp":
        w = torch.clamp(1.0 - (tz[:, :, None] - z).abs() / delta, 0.0, 1.0)
        m = (w * ptj[:, :, None]).sum(1)
    else:
        w = torch.clamp(1.0 - (torch.clamp(tz, v_min, v_max)[:, :, None] - z).abs() / delta, 0.0, 1.0)
        m = (w * ptj[:, :, None]).sum(1)
    if c.get("m_scale") is not None:
        m = m * float(F32(c["m_scale"]))
    if fault != "target_differentiated":
        m = m.detach()
    a = np.asarray(c["a"])
    known = torch.tensor((a >= 0) & (a < na))
    ac = torch.tensor(np.where((a >= 0) & (a < na), a, 0))
    l = shaped(_net64(params, ns, h, M, act, s, relu(rp["hid"])))
    la = l[ac, :, cols]  # (B, K)
    if fault == "sm_one":  # the gradient p - m: the loss whose log-partition term is not weighted by sum(m)
        ce = -(m * la).sum(1) + torch.logsumexp(la, 1)
    else:
        ce = -(m * torch.log_softmax(la, 1)).sum(1)
    ce = torch.where(known, ce, torch.zeros_like(ce))
    w_is = _t(c["weights"]) if c.get("weights") is not None else torch.ones(B, dtype=torch.float64)
    loss = (w_is * ce).sum() / B
    loss.backward()
    ce_out = (w_is * ce) if fault == "weighted_ce" else ce
    return dict(grad=params.grad.numpy().copy(), loss=float(loss.detach()), ce=ce_out.detach().numpy(), proj=m.detach().numpy().T.copy(),
                sel=sel.numpy().astype(np.int32), gap=gap, qt=qt.detach().numpy(), qo=None if qo is None else qo.numpy(),
                probs_t=pt.detach().numpy(), tz=tz.detach().numpy().T.copy())


# ---------------------------------------------------------------------------------------------- per-sample error budgets
LIBM = 4.0  # exp and log: at most 4 ulp (ocml's expf / logf and numpy's Float32 forms both stay far inside)


def softmax_budget(l, e_l, na, K, z):
    """-> (budget of p (na, K, B), budget of Q (na, B)) from logits l (M, B) with error bound e_l (M, B)"""
    p, q, _, _, _ = dist(l, na, K, z)
    emax = np.asarray(e_l, F64).reshape(na, K, -1).max(1)
    rel = 2.0 * emax[:, None, :] + 2.0 * ulp(F32(1)) * np.abs(np.asarray(l, F64).reshape(na, K, -1)) + (K + 2 * LIBM + 4) * 2.0 * U32
    b_p = p.astype(F64) * rel
    az = np.abs(z.astype(F64))[None, :, None]
    b_q = (az * b_p).sum(1) + (K + 2) * U32 * (az * p.astype(F64)).sum(1)
    return b_p, b_q


def budgets(c, rp):
    """-> dict(q_t, q_o, proj (K, B), ce (B,)) of absolute error bounds for the values of replay `rp`"""
    ns, h, na, K, act, B = c["ns"], c["h"], c["na"], c["n_atoms"], c["act"], c["batch"]
    M = na * K
    z, delta = rp["z"], F64(rp["delta"])
    cols = np.arange(B)
    e_lt = net_error(c["target"], ns, h, M, act, c["sn"])
    b_pt, b_qt = softmax_budget(rp["lt"], e_lt, na, K, z)
    out = dict(q_t=b_qt, p_t=b_pt, q_o=None)
    if c["double"]:
        out["q_o"] = softmax_budget(rp["lo"], net_error(c["params"], ns, h, M, act, c["sn"]), na, K, z)[1]
    b_ptj = b_pt[rp["sel"], :, cols].T  # (K, B)
    r, cc, tz = np.asarray(c["r"], F64), rp["cc"].astype(F64), rp["tz"].astype(F64)
    z64 = z.astype(F64)
    e_tz = 3.0 * U32 * (np.abs(r)[None, :] + np.abs(cc[None, :] * z64[:, None]))  # (Kj, B)
    dist_jk = np.abs(tz[:, None, :] - z64[None, :, None])                           # (Kj, Kk, B)
    near = dist_jk <= delta * (1.0 + 1e-3)
    e_w = np.where(near, (e_tz[:, None, :] + 2.0 * U32 * (np.abs(tz)[:, None, :] + np.abs(z64)[None, :, None])) / delta + 4.0 * U32, 0.0)
    w = np.clip(1.0 - dist_jk / delta, 0.0, 1.0)
    ptj = rp["ptj"].astype(F64)
    b_m = (e_w * ptj[:, None, :] + w * b_ptj[:, None, :]).sum(0) + (K + 1) * U32 * rp["proj"].astype(F64)
    if c.get("m_scale") is not None:
        b_m = b_m * float(c["m_scale"]) + U32 * rp["proj"].astype(F64)
    out["proj"] = b_m
    e_l = net_error(c["params"], ns, h, M, act, c["s"])
    ac = np.where(rp["known"], np.asarray(c["a"]), 0)
    e_la = e_l.reshape(na, K, B)[ac, :, cols].T.max(0)  # (B,)
    lp = rp["lp"].astype(F64)
    b_lp = 2.0 * e_la[None, :] + U32 * (4.0 * np.abs(rp["la"].astype(F64) - rp["mx"].astype(F64)[None, :]) +
                                         (2 * LIBM + 2) * np.abs(rp["logS"].astype(F64))[None, :] + (K + 2 * LIBM + 4))
    m = rp["proj"].astype(F64)
    out["ce"] = np.where(rp["known"], (b_m * np.abs(lp) + m * b_lp).sum(0) + (K + 1) * U32 * (m * np.abs(lp)).sum(0), 0.0)
    return out


def within(got, centre, budget, tag=""):
    """|got - centre| <= 2 x budget everywhere (both finite; never tighter than one ulp of the centre) -> the worst ratio"""
    got, centre, budget = np.asarray(got, F64), np.asarray(centre, F64), np.asarray(budget, F64)
    assert np.isfinite(got).all() and np.isfinite(centre).all() and np.isfinite(budget).all(), f"{tag}: non-finite value or budget"
    bar = 2.0 * np.maximum(budget, 0.5 * ulp(centre.astype(F32)).astype(F64))
    ratio = np.abs(got - centre) / bar
    assert ratio.max() <= 1.0, f"{tag}: |got - model| reaches {ratio.max():.3g} x the bar (2 x budget) at {int((ratio > 1).sum())} of {got.size}"
    return float(ratio.max())


def rel(a, b):
    a, b = np.asarray(a, F64).ravel(), np.asarray(b, F64).ravel()
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))
