"""The mathematics of the IQN section of include/rlhip.h as a plain torch model: forward, quantile-Huber loss, autograd gradient.
The quantile levels are ARGUMENTS (tests read them back from the kernels or map Philox words with `levels`).  The dtype is the dtype of
the parameters: float64 is the reference, float32 gives the Float32 floor from which the tests' bar is derived."""
import math

import numpy as np
import torch


def nparams(ns, h, na, nc):
    return h * ns + h + h * nc + h + na * h + na


def split(p, ns, h, na, nc):
    """the flat vector -> W1 (h, ns), b1, Wphi (h, nc), bphi, W2 (na, h), b2   (every matrix column-major)"""
    out, o = [], 0
    for rows, cols in ((h, ns), (h, 1), (h, nc), (h, 1), (na, h), (na, 1)):
        blk = p[o:o + rows * cols]
        out.append(blk.view(cols, rows).T if cols > 1 else blk)
        o += rows * cols
    return out


def levels(words):
    """tau = (w >> 15) * 2^-17 of uint32 Philox words"""
    return (np.asarray(words, np.uint64) >> np.uint64(15)).astype(np.float64) * 2.0 ** -17


def net(p, dims, act, x, tau):
    """x (ns, B), tau (L, B) -> th (L, na, B), and the pre-activations of psi (h, B) and phi (h, L, B)"""
    ns, h, na, nc = dims
    W1, b1, Wp, bp, W2, b2 = split(p, *dims)
    zpsi = W1 @ x + b1[:, None]
    psi = torch.relu(zpsi) if act == 0 else torch.tanh(zpsi)
    e = torch.arange(1, nc + 1, dtype=p.dtype)
    # cospi of the EXACT product (e tau is exact in Float32 too: tau sits on a 2^-17 grid): the period is taken off before the
    # multiplication by pi, as a cospi does
    c = torch.cos(math.pi * torch.remainder(e[:, None, None] * tau[None], 2.0))
    zphi = torch.einsum("je,elb->jlb", Wp, c) + bp[:, None, None]
    m = psi[:, None, :] * torch.relu(zphi)
    return torch.einsum("oj,jlb->lob", W2, m) + b2[None, :, None], zpsi, zphi


def loss(p, pt, dims, act, kappa, s, a, r, term, sn, gamma, tau, taup, n_used=None, weights=None, double=False):
    """-> dict(loss, ql (B), target (N', B), sel (B), zmin: the smallest |pre-activation| of a relu, margin: the smallest a* margin)"""
    na, B, dt = dims[2], s.shape[1], p.dtype
    g32 = np.float64(np.float32(gamma))
    disc = torch.full((B,), float(g32), dtype=dt)
    if n_used is not None:  # the 33 host-computed powers, Float32
        pw = torch.tensor((g32 ** np.arange(33)).astype(np.float32), dtype=dt)
        disc = pw[n_used.clamp(0, 32).long()]
    c = disc * (1.0 - term.to(dt))
    with torch.no_grad():
        tht, zp_t, zf_t = net(pt, dims, act, sn, taup)
        zs = [zf_t] + ([zp_t] if act == 0 else [])
        qsel = tht.mean(0)
        if double:
            tho, zp_o, zf_o = net(p, dims, act, sn, taup)
            zs += [zf_o] + ([zp_o] if act == 0 else [])
            qsel = tho.mean(0)
        sel = qsel.argmax(0)
        top = qsel.topk(2, 0).values if na > 1 else None
        T = r[None] + c[None] * tht[:, sel, torch.arange(B)]
    valid = (a >= 0) & (a < na)
    th, zp, zf = net(p, dims, act, s, tau)
    zs += [zf] + ([zp] if act == 0 else [])
    th = th[:, a.clamp(0, na - 1).long(), torch.arange(B)]
    u = T[None, :, :] - th[:, None, :]
    hub = torch.where(u.abs() <= kappa, 0.5 * u * u, kappa * (u.abs() - 0.5 * kappa)) / kappa
    w = torch.where(u < 0, 1.0 - tau[:, None, :], tau[:, None, :])
    ql = torch.where(valid, (w * hub).sum((0, 1)) / T.shape[0], torch.zeros((), dtype=dt))
    L = (ql * (weights if weights is not None else 1.0)).sum() / B
    return dict(loss=L, ql=ql.detach(), target=T, sel=sel.to(torch.int32), zmin=min(float(z.detach().abs().min()) for z in zs),
                margin=float((top[0] - top[1]).min()) if top is not None else math.inf)
