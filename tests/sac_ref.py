"""Soft Actor-Critic as include/rlhip.h states it (the SAC section is the specification), twice, with no oracle code and no GPU:

  (a) `critic_replay` / `actor_replay`: the per-sample lines replayed in numpy Float32 in the header's order -- every forward pass the
      chain z = b1[j], fmaf over k ascending; out = b2, fmaf over j ascending (an fmaf is the exact Float64 product and sum, rounded once
      more to Float32) -- with the draws `eps` as an ARGUMENT (heads_grad_ref.draws regenerates them from an implementation's unchanged
      forward entry).  The batch sums (losses, statistics, every gradient element) are accumulated in Float64: the device's fixed
      Float32 order is judged against them at the project's F32_GRAD_TOL.
  (b) `torch_model`: the three losses in float64 torch, differentiated by autograd -- no hand pullback.  `sel`, the clamp's `pass` and
      the ReLU masks are taken from (a), so no decision can differ between the two.  `fault=` plants a misreading of the text.

`head_budget` / `target_budget` carry the per-sample outputs (raw sigma, logp, y) as heads_ref.Q quantities: the first-order propagation
of heads_ref.E's libm bounds plus half an ulp per rounded operation, as tests/heads_ref.py derives its budgets; the bar is 2 x budget.
Shared by tests/test_sac_reference.py (CPU), tests/test_gpu_sac_kernels.py and tests/test_gpu_sac_learner.py."""
import numpy as np

import heads_grad_ref as G
from heads_ref import EPS, F32, F64, LN2, LOG2PI, Q, _normlogpdf, clamp, ulp

U32 = 2.0 ** -24  # half an ulp, relative


def nparams(ni, h, no):
    return h * ni + h + no * h + no


def split(p, ni, h, no):
    """flat mlp2 vector -> W1 (h, ni), b1 (h), W2 (no, h), b2 (no): W1[j, k] = p[j + h k], W2[o, j] = p[o + no j]"""
    p = np.asarray(p)
    o1, o2, o3 = h * ni, h * ni + h, h * ni + h + no * h
    return p[:o1].reshape(ni, h).T, p[o1:o2], p[o2:o3].reshape(h, no).T, p[o3:]


def join(W1, b1, W2, b2):
    return np.concatenate([np.asarray(W1).T.ravel(), np.asarray(b1).ravel(), np.asarray(W2).T.ravel(), np.asarray(b2).ravel()])


def fma(a, b, c):
    with np.errstate(all="ignore"):
        return (np.asarray(a, F64) * np.asarray(b, F64) + np.asarray(c, F64)).astype(F32)


def act_fwd(act, z):
    return np.maximum(z, F32(0)) if act == 0 else np.tanh(z).astype(F32)


def act_der(act, hv):
    return (hv > 0).astype(F32) if act == 0 else (F32(1) - hv * hv).astype(F32)


def forward(p, ni, h, no, act, x):
    """x (ni, B) Float32 -> out (no, B), hidden (h, B), z (h, B): the chain of rlhip_mlp2_forward_f32"""
    W1, b1, W2, b2 = split(np.asarray(p, F32), ni, h, no)
    x = np.asarray(x, F32)
    z = np.repeat(b1[:, None], x.shape[1], 1).astype(F32)
    for k in range(ni):
        z = fma(W1[:, k:k + 1], x[k:k + 1, :], z)
    hv = act_fwd(act, z)
    out = np.repeat(b2[:, None], x.shape[1], 1).astype(F32)
    for j in range(h):
        out = fma(W2[:, j:j + 1], hv[j:j + 1, :], out)
    return out, hv, z


def softplus(x):
    x = np.asarray(x, F32)
    with np.errstate(all="ignore"):
        return (np.log1p(np.exp(-np.abs(x))) + np.maximum(x, F32(0))).astype(F32)


def normlogpdf1(mu, sg, x):
    with np.errstate(all="ignore"):
        se = sg + EPS
        z = (x - mu) / se
        return (-(z * z + LOG2PI) / F32(2) - np.log(se)).astype(F32)


def head(mu, rho, eps, lo, hi, scale, tanh_correction=True):
    """the actor head of the header on Float32 vectors -> dict(raw, sg, ok, z, a, u, logp)"""
    mu, rho, eps = (np.asarray(t, F32) for t in (mu, rho, eps))
    with np.errstate(all="ignore"):
        raw = softplus(rho)
        sg = clamp(raw, lo, hi)
        z = (mu + sg * eps).astype(F32)
        a = np.tanh(z).astype(F32)
        logp = normlogpdf1(mu, sg, z)
        if tanh_correction:
            logp = (logp - F32(2) * ((LN2 - z) - softplus(F32(-2) * z))).astype(F32)
    return dict(raw=raw, sg=sg, ok=G.passes(raw, lo, hi), z=z, a=a, u=(F32(scale) * a).astype(F32), logp=logp)


def draw_pair(sample, n, seed, step, base=0):
    """normal_draw(seed, base + i, step, 0) and (.., 1) for i < n, from an implementation's unchanged forward entry"""
    e = G.draws(sample, 2, n, 1, seed, base, step)
    return np.ascontiguousarray(e[0, 0]), np.ascontiguousarray(e[1, 0])


# ------------------------------------------------------------------------------------------------------------ (a) the replay
def _backprop(ni, h, no, act, p, x, hv, d):
    """gradient of sum_i sum_o d[o, i] out[o, i] -> flat Float64 vector; per-sample terms as the header writes them, sums in Float64"""
    W1, b1, W2, b2 = split(np.asarray(p, F32), ni, h, no)
    d = np.asarray(d, F32)
    dh = np.zeros(hv.shape, F32)
    for o in range(no):
        dh = fma(d[o:o + 1, :], W2[o][:, None], dh) if no > 1 else (d[o:o + 1, :] * W2[o][:, None]).astype(F32)
    dz = (dh * act_der(act, hv)).astype(F32)
    gW2 = d.astype(F64) @ hv.astype(F64).T                      # (no, h)
    gW1 = dz.astype(F64) @ np.asarray(x, F64).T                 # (h, ni)
    return join(gW1, dz.astype(F64).sum(1), gW2, d.astype(F64).sum(1))


def critic_replay(c, eps):
    """-> dict(y, sel_t, logp_n, loss (2,), grad, masks...) for case `c` (tests/sac_cases.py) and the draws eps (batch,) of index 0"""
    ns, h, act, B = c["ns"], c["h"], c["act"], c["batch"]
    nq = nparams(ns + 1, h, 1)
    s, a, r, t, sn = c["records"]()
    alpha, gamma, fb = F32(c["alpha"]), F32(c["gamma"]), F32(B)
    o, hv_a, _ = forward(c["actor"], ns, h, 2, act, sn)
    hd = head(o[0], o[1], eps, c["lo"], c["hi"], c["scale"])
    xn = np.vstack([sn, hd["u"][None, :]]).astype(F32)
    qt, hvt, zt = zip(*(forward(c["targets"][k * nq:(k + 1) * nq], ns + 1, h, 1, act, xn) for k in range(2)))
    qt1, qt2 = qt[0][0], qt[1][0]
    second = qt2 < qt1
    qmin = np.where(second, qt2, qt1).astype(F32)
    cont = np.where(t != 0, F32(0), F32(1)).astype(F32)
    y = (r + (gamma * cont) * (qmin - alpha * hd["logp"])).astype(F32)
    x = np.vstack([s, a[None, :]]).astype(F32)
    out = dict(y=y, eps=eps, sel_t=np.where(second, 2, 1), head=hd, x=x, xn=xn, hid_actor=hv_a, hid_t=hvt, z_t=zt, qt=(qt1, qt2), loss=[], q=[],
               hid=[], g=[])
    grads = []
    for k in range(2):
        p = c["critics"][k * nq:(k + 1) * nq]
        q, hv, _ = forward(p, ns + 1, h, 1, act, x)
        d = (q[0] - y).astype(F32)
        g = ((F32(2) * d) / fb).astype(F32)
        out["loss"].append(float((d * d).astype(F32).astype(F64).sum() / float(fb)))
        out["q"].append(q[0]), out["hid"].append(hv), out["g"].append(g)
        grads.append(_backprop(ns + 1, h, 1, act, p, x, hv, g[None, :]))
    out["grad"] = np.concatenate(grads)
    return out


def actor_replay(c, eps, critics=None):
    """-> dict(sel, logp, q, stats (3,), grad, alpha_new, ...) for the draws eps (batch,) of index 1; critics: the stepped vector"""
    ns, h, act, B = c["ns"], c["h"], c["act"], c["batch"]
    nq = nparams(ns + 1, h, 1)
    critics = c["critics"] if critics is None else critics
    s = c["records"]()[0]
    alpha, fb, scale = F32(c["alpha"]), F32(B), F32(c["scale"])
    o, hv_a, _ = forward(c["actor"], ns, h, 2, act, s)
    mu, rho = o[0], o[1]
    hd = head(mu, rho, eps, c["lo"], c["hi"], c["scale"])
    x = np.vstack([s, hd["u"][None, :]]).astype(F32)
    dlogp, dq = F32(alpha / fb), F32(F32(-1.0) / fb)
    qs, dus, hvs, zs = [], [], [], []
    for k in range(2):
        p = np.asarray(critics[k * nq:(k + 1) * nq], F32)
        W1, _, W2, _ = split(p, ns + 1, h, 1)
        q, hv, z = forward(p, ns + 1, h, 1, act, x)
        dzj = ((dq * W2[0][:, None]).astype(F32) * act_der(act, hv)).astype(F32)
        du = np.zeros(B, F32)
        for j in range(h):
            du = fma(dzj[j], W1[j, ns], du)
        qs.append(q[0]), dus.append(du), hvs.append(hv), zs.append(z)
    second = qs[1] < qs[0]
    q = np.where(second, qs[1], qs[0]).astype(F32)
    dact = (scale * np.where(second, dus[1], dus[0])).astype(F32)
    with np.errstate(all="ignore"):
        sd = hd["sg"] + EPS
        zz = ((hd["z"] - mu) / sd).astype(F32)
        w = (zz / sd).astype(F32)
        tt = hd["a"]
        dz = (dlogp * (F32(2) * tt - w)).astype(F32)
        dz = (dz + dact * (F32(1) - tt * tt)).astype(F32)
        dmu = (dlogp * w + dz).astype(F32)
        dsg = (dlogp * ((zz * zz - F32(1)) / sd) + dz * eps).astype(F32)
        draw = np.where(hd["ok"], dsg, F32(0)).astype(F32)
        drho = (draw * (F32(1) / (F32(1) + np.exp(-rho)))).astype(F32)
    li = (alpha * hd["logp"] - q).astype(F32)
    stats = np.array([t.astype(F64).sum() / float(fb) for t in (li, q, hd["logp"])])
    grad = _backprop(ns, h, 2, act, c["actor"], s, hv_a, np.vstack([dmu, drho]))
    alpha_new = F32(alpha - F32(c["alpha_lr"]) * (F32(-F32(stats[2])) - F32(c["target_entropy"])))
    return dict(eps=eps, sel=np.where(second, 2, 1), logp=hd["logp"], q=q, qs=qs, stats=stats, grad=grad, alpha_new=alpha_new, head=hd, x=x,
                hid_actor=hv_a, hid=hvs, z=zs, drho=drho, dmu=dmu, mu=mu, rho=rho)


# ------------------------------------------------------------------------------------------------ (b) float64 autograd
FAULTS = ("max", "no_cont", "no_alpha_target", "no_alpha_actor", "no_scale_dact", "no_tanh_correction", "y_differentiated")


def _t(x, grad=False):
    import torch

    return torch.tensor(np.asarray(x, F64), dtype=torch.float64, requires_grad=grad)


def _net64(p, ni, h, no, act, x, mask):
    """float64 forward from a flat torch vector; relu through the mask of (a): h = z * mask"""
    import torch

    o1, o2, o3 = h * ni, h * ni + h, h * ni + h + no * h
    W1, b1, W2, b2 = p[:o1].reshape(ni, h).t(), p[o1:o2], p[o2:o3].reshape(h, no).t(), p[o3:]
    z = W1 @ x + b1[:, None]
    hv = z * _t(mask) if act == 0 else torch.tanh(z)
    return W2 @ hv + b2[:, None]


def _head64(o, eps, c, ok, tanh_correction=True):
    import math

    import torch

    mu, raw = o[0], torch.nn.functional.softplus(o[1])
    lo, hi = float(F32(c["lo"])), float(F32(c["hi"]))
    okt = torch.tensor(np.asarray(ok))
    bound = torch.where(raw.detach() > hi, torch.full_like(raw, hi if math.isfinite(hi) else 0.0), torch.full_like(raw, lo))
    sg = torch.where(okt, raw, bound)
    z = mu + sg * _t(eps)
    se = sg + float(EPS)
    zz = (z - mu) / se
    logp = -(zz * zz + float(LOG2PI)) / 2.0 - torch.log(se)
    if tanh_correction:
        logp = logp - 2.0 * ((float(LN2) - z) - torch.nn.functional.softplus(-2.0 * z))
    return float(F32(c["scale"])) * torch.tanh(z), logp


def torch_model(c, eps0, eps1, ra, rc, critics=None, fault=None):
    """the three losses in float64 with the decisions of the replays rc = critic_replay, ra = actor_replay -> dict(critic_grad,
    critic_loss (2,), y, actor_grad, actor_stats (3,), alpha_new, logp).  `critics`: the vector the actor step reads (default c's)"""
    import torch

    ns, h, act, B = c["ns"], c["h"], c["act"], c["batch"]
    nq = nparams(ns + 1, h, 1)
    s, a, r, t, sn = c["records"]()
    alpha, gamma = float(F32(c["alpha"])), float(F32(c["gamma"]))
    relu = lambda hv: (np.asarray(hv) > 0).astype(F64)  # noqa: E731
    # ---- critic loss
    actor, crit, targ = _t(c["actor"]), _t(c["critics"], True), _t(c["targets"])
    if fault == "y_differentiated":
        targ = crit  # the target is read off the trained vector and not held constant
    u_n, logp_n = _head64(_net64(actor, ns, h, 2, act, _t(sn), relu(rc["hid_actor"])), eps0, c, rc["head"]["ok"])
    xn = torch.cat([_t(sn), u_n[None, :]])
    qt = [_net64(targ[k * nq:(k + 1) * nq], ns + 1, h, 1, act, xn, relu(rc["hid_t"][k]))[0] for k in range(2)]
    second = torch.tensor(rc["sel_t"] == 2)
    if fault == "max":
        second = ~second
    qmin = torch.where(second, qt[1], qt[0])
    cont = _t(np.where(t != 0, 0.0, 1.0)) if fault != "no_cont" else torch.ones(B, dtype=torch.float64)
    y = _t(r) + gamma * cont * (qmin - (0.0 if fault == "no_alpha_target" else alpha) * logp_n)
    if fault != "y_differentiated":
        y = y.detach()
    x = torch.cat([_t(s), _t(a)[None, :]])
    losses = [((_net64(crit[k * nq:(k + 1) * nq], ns + 1, h, 1, act, x, relu(rc["hid"][k]))[0] - y) ** 2).mean() for k in range(2)]
    (losses[0] + losses[1]).backward()
    out = dict(critic_grad=crit.grad.numpy().copy(), critic_loss=np.array([float(v.detach()) for v in losses]), y=y.detach().numpy())
    # ---- actor loss
    actor = _t(c["actor"], True)
    crit2 = _t(c["critics"] if critics is None else critics)
    u, logp = _head64(_net64(actor, ns, h, 2, act, _t(s), relu(ra["hid_actor"])), eps1, c, ra["head"]["ok"],
                      tanh_correction=fault != "no_tanh_correction")
    if fault == "no_scale_dact":  # the action reaches the critic, its gradient comes back without action_scale
        k = float(F32(c["scale"]))
        u = u.detach() + (u - u.detach()) / k
    xa = torch.cat([_t(s), u[None, :]])
    qa = [_net64(crit2[k * nq:(k + 1) * nq], ns + 1, h, 1, act, xa, relu(ra["hid"][k]))[0] for k in range(2)]
    q = torch.where(torch.tensor(ra["sel"] == 2), qa[1], qa[0])
    li = (0.0 if fault == "no_alpha_actor" else alpha) * logp - q
    li.mean().backward()
    out.update(actor_grad=actor.grad.numpy().copy(), logp=logp.detach().numpy(),
               actor_stats=np.array([float(v.detach().mean()) for v in (li, q, logp)]))
    # ---- the entropy coefficient: gradient descent on alpha * (mean(-logp) - target_entropy)
    al = _t([alpha], True)
    (al * (-logp.detach().mean() - float(F32(c["target_entropy"])))).sum().backward()
    out["alpha_new"] = float(alpha - float(F32(c["alpha_lr"])) * float(al.grad[0]))
    return out


# ---------------------------------------------------------------------------------------------- per-sample error budgets
def softplus_q(x):
    """softplus_nnlib on a Q: log1p(exp(-|x|)) + relu(x)"""
    return x.abs().scale(-1).libm("exp").libm("log1p") + x.relu()


def net_error(p, ni, h, no, act, x, e_last=None):
    """absolute error bound of `forward` (no, B) against exact arithmetic, plus the first-order effect of an error e_last (B,) of the
    LAST input row: every fmaf rounds once, to at most half an ulp of the sum of magnitudes it has reached"""
    W1, b1, W2, b2 = (np.asarray(t, F64) for t in split(np.asarray(p, F32), ni, h, no))
    x = np.asarray(x, F64)
    z = W1 @ x + b1[:, None]
    e_z = ni * U32 * (np.abs(W1) @ np.abs(x) + np.abs(b1)[:, None])
    if e_last is not None:
        e_z = e_z + np.abs(W1[:, -1:]) * np.asarray(e_last, F64)[None, :]
    if act == 0:
        hv, e_h = np.maximum(z, 0.0), np.where(z > -e_z, e_z, 0.0)
    else:
        hv = np.tanh(z)
        e_h = (1.0 - hv * hv) * e_z + 5.0 * ulp(hv)
    return np.abs(W2) @ e_h + h * U32 * (np.abs(W2) @ np.abs(hv) + np.abs(b2)[:, None])


def head_budget(mu, rho, eps, lo, hi, scale, e_mu=0.0, e_rho=0.0):
    """the head as Q quantities from the actor outputs (with their error bounds) -> dict of Q: raw, u, logp"""
    mu_q, rho_q = Q(np.asarray(mu, F32), e_mu), Q(np.asarray(rho, F32), e_rho)
    raw = softplus_q(rho_q)
    hi32, lo32 = F64(F32(hi)), F64(F32(lo))
    above, below = raw.c > hi32, raw.c < lo32   # (the census keeps raw 1e-4 away from both bounds: no decision inside the budget)
    sg = Q(np.where(above, hi32, np.where(below, lo32, raw.c)), np.where(above | below, 0.0, raw.e))
    z = mu_q + sg * Q(np.asarray(eps, F32))
    logp = _normlogpdf(mu_q, sg, z) - ((Q(LN2) - z) - softplus_q(z.scale(-2))).scale(2)
    return dict(raw=raw, u=z.libm("tanh") * Q(F32(scale)), logp=logp, z=z)


def target_budget(c, rc):
    """y of the critic step as a Q (centre: the replay's value): the errors of the actor at s', of the head, of both target critics at
    x' (with the error of u'), through the target line"""
    ns, h, act = c["ns"], c["h"], c["act"]
    nq = nparams(ns + 1, h, 1)
    s, a, r, t, sn = c["records"]()
    e_o = net_error(c["actor"], ns, h, 2, act, sn)
    o, _, _ = forward(c["actor"], ns, h, 2, act, sn)
    hb = head_budget(o[0], o[1], rc["eps"], c["lo"], c["hi"], c["scale"], e_o[0], e_o[1])
    e_qt = [net_error(c["targets"][k * nq:(k + 1) * nq], ns + 1, h, 1, act, rc["xn"], hb["u"].e)[0] for k in range(2)]
    qsel = Q(np.where(rc["sel_t"] == 2, rc["qt"][1], rc["qt"][0]), np.where(rc["sel_t"] == 2, e_qt[1], e_qt[0]))
    cont = np.where(t != 0, F32(0), F32(1)).astype(F32)
    y = Q(np.asarray(r, F32)) + Q((F32(c["gamma"]) * cont).astype(F32)) * (qsel - Q(F32(c["alpha"])) * hb["logp"])
    return y, hb


def within(got, q, tag=""):
    """|got - centre| <= 2 x budget everywhere (both finite)"""
    got = np.asarray(got, F64)
    assert np.isfinite(got).all() and np.isfinite(q.c).all() and np.isfinite(q.e).all(), f"{tag}: non-finite value or budget"
    bar = 2.0 * np.maximum(q.e, 0.5 * ulp(q.c))
    ratio = np.abs(got - q.c) / bar
    assert ratio.max() <= 1.0, f"{tag}: |got - model| reaches {ratio.max():.3g} x the bar (2 x budget) at {int((ratio > 1).sum())} of {got.size}"
    return float(ratio.max())
