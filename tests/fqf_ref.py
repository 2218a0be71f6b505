"""The mathematics of the FQF section of include/rlhip.h as a plain torch model: fraction stage, forward, quantile-Huber loss and the
fraction loss, gradients by autograd.  The quantile network is tests/iqn_ref.py's.  The levels are the model's own fraction stage or,
teacher-forced, GIVEN (`tau`, (N + 1, B): tests hand the kernel's tau_out over, so that cospi's sensitivity to a last-bit level
difference does not blur the comparison of everything behind the levels).  The dtype is the dtype of the parameters: float64 is the
reference, float32 gives the Float32 floor from which the tests' bars are derived."""
import numpy as np
import torch

from iqn_ref import net, split


def fractions(p, pf, dims, N, act, x):
    """-> tau (N + 1, B), q (N, B), the entropy H (B); psi is a constant of the fraction net's gradient"""
    ns, h, na, nc = dims
    W1, b1 = split(p, *dims)[:2]
    z = (W1 @ x + b1[:, None]).detach()
    psi = torch.relu(z) if act == 0 else torch.tanh(z)
    l = pf[:N * h].view(h, N).T @ psi + pf[N * h:, None]
    lq = torch.log_softmax(l, 0)
    q = lq.exp()
    edge = torch.ones((1, x.shape[1]), dtype=p.dtype)
    return torch.cat([0 * edge, q.cumsum(0)[:-1], edge]), q, -(q * lq).sum(0)


def mids(tau):
    return 0.5 * (tau[:-1] + tau[1:]), tau[1:] - tau[:-1]


def forward(p, pf, dims, N, act, x, tau=None):
    """-> dict(q (na, B), th (N, na, B), tau, that)"""
    tau = fractions(p, pf, dims, N, act, x)[0] if tau is None else tau
    that, d = mids(tau)
    th = net(p, dims, act, x, that)[0]
    return dict(q=(d[:, None, :] * th).sum(0), th=th, tau=tau, that=that)


def loss(p, pt, pf, dims, N, act, kappa, ent_coef, s, a, r, term, sn, gamma, n_used=None, weights=None, double=False, tau=None):
    """-> dict(loss: the quantile-Huber loss (differentiate by p), frac_loss: the fraction surrogate (differentiate by pf), ql (B),
    target (N, B), sel (B), tau, that, ent (B), margin: the smallest a* margin, zs: the pre-activations (psi where act is relu, phi
    always) of every network evaluation in the loss, zmin: the smallest |z| among them)"""
    na, B, dt = dims[2], s.shape[1], p.dtype
    g32 = np.float64(np.float32(gamma))
    disc = torch.full((B,), float(g32), dtype=dt)
    if n_used is not None:  # the 33 host-computed powers, Float32
        disc = torch.tensor((g32 ** np.arange(33)).astype(np.float32), dtype=dt)[n_used.clamp(0, 32).long()]
    c = disc * (1.0 - term.to(dt))
    tau_own, _, H = fractions(p, pf, dims, N, act, s)
    tau = tau_own.detach() if tau is None else tau
    that, d = mids(tau)
    cols = torch.arange(B)
    with torch.no_grad():
        tht, zp_t, zf_t = net(pt, dims, act, sn, that)
        zs = [zf_t] + ([zp_t] if act == 0 else [])
        tho = tht
        if double:
            tho, zp_o, zf_o = net(p, dims, act, sn, that)
            zs += [zf_o] + ([zp_o] if act == 0 else [])
        qsel = (d[:, None, :] * tho).sum(0)
        sel = qsel.argmax(0)
        top = qsel.topk(2, 0).values if na > 1 else None
        T = r[None] + c[None] * tht[:, sel, cols]
    valid = (a >= 0) & (a < na)
    ac = a.clamp(0, na - 1).long()
    th, zp, zf = net(p, dims, act, s, that)
    zs += [zf.detach()] + ([zp.detach()] if act == 0 else [])
    th = th[:, ac, cols]
    u = T[None, :, :] - th[:, None, :]
    hub = torch.where(u.abs() <= kappa, 0.5 * u * u, kappa * (u.abs() - 0.5 * kappa)) / kappa
    w = torch.where(u < 0, 1.0 - that[:, None, :], that[:, None, :])
    ql = torch.where(valid, (w * hub).sum((0, 1)) / N, torch.zeros((), dtype=dt))
    wts = (weights if weights is not None else torch.ones(B, dtype=dt)) * valid.to(dt)
    # the paper's fraction gradient as a surrogate: d/dtau_i of the 1-Wasserstein distance is gf[i], i = 1 .. N - 1
    with torch.no_grad():
        thi, _, zf_i = net(p, dims, act, s, tau[1:-1])  # (psi(s) is in zs already)
        zs.append(zf_i)
        gf = 2.0 * thi[:, ac, cols] - th[1:] - th[:-1]
    frac = (wts * ((gf * tau_own[1:-1]).sum(0) - ent_coef * H)).sum() / B
    return dict(loss=(ql * wts).sum() / B, frac_loss=frac, ql=ql.detach(), target=T, sel=sel.to(torch.int32), tau=tau, that=that,
                ent=H.detach(), margin=float((top[0] - top[1]).min()) if top is not None else np.inf, zs=zs,
                zmin=min(float(z.abs().min()) for z in zs))
