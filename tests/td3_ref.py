"""A plain torch model of the TD3 / DDPG section of include/rlhip.h: the networks, the gathered records and the clipped noise `e` in,
targets, losses, statistics and -- by autograd -- both gradients out.  dtype = torch.float64 is the reference; the same model in
torch.float32 gives the Float32 floor of each output (tests/test_gpu_td3.py, profiles/td3.md).  No order of summation is modelled."""
import numpy as np
import torch


def mlp(p, ni, h, act, x):
    """mlp2(ni, h, 1) on x (ni, B) from the flat vector p -> (out (B,), z (h, B))"""
    W1, b1 = p[:h * ni].reshape(ni, h), p[h * ni:h * ni + h]
    W2, b2 = p[h * ni + h:h * ni + 2 * h], p[h * ni + 2 * h]
    z = W1.t() @ x + b1[:, None]
    return W2 @ (torch.relu(z) if act == 0 else torch.tanh(z)) + b2, z


def _t(x, dtype):
    return torch.tensor(np.asarray(x), dtype=dtype)


def critic(c, rec, e, dtype=torch.float64):
    """the critic launch: c holds ns, h, act, nc, gamma, scale, lo, hi and the flat vectors actor_t, critics, targets; rec = (s, a, r,
    t, s'); e the clipped noise -> dict(y, loss, grad, u_raw (u' before its clamp), qt (nc, B), z: every layer-1 pre-activation)"""
    ns, h, act, nc = c["ns"], c["h"], c["act"], c["nc"]
    s, a, r, t, sn = (_t(x, dtype) for x in rec)
    npq = (ns + 1) * h + 2 * h + 1
    critics = _t(c["critics"], dtype).requires_grad_()
    targets, gamma, scale = _t(c["targets"], dtype), _t(c["gamma"], dtype), _t(c["scale"], dtype)
    mu, z_a = mlp(_t(c["actor_t"], dtype), ns, h, act, sn)
    u_raw = scale * torch.tanh(mu) + _t(e, dtype)
    xn = torch.cat([sn, u_raw.clamp(c["lo"], c["hi"])[None]])
    qt, z_t = zip(*(mlp(targets[k * npq:(k + 1) * npq], ns + 1, h, act, xn) for k in range(nc)))
    y = r + (gamma * (1 - t)) * torch.stack(qt).min(0).values
    q, z_q = zip(*(mlp(critics[k * npq:(k + 1) * npq], ns + 1, h, act, torch.cat([s, a[None]])) for k in range(nc)))
    loss = torch.stack([((qk - y) ** 2).mean() for qk in q])
    loss.sum().backward()
    out = dict(y=y, loss=loss, grad=critics.grad, u_raw=u_raw, qt=torch.stack(qt), z=torch.cat([z_a, *z_t, *z_q]))
    return {k: v.detach().numpy() for k, v in out.items()}


def actor(c, rec, critics=None, dtype=torch.float64):
    """the actor launch against `critics` (default c's): -> dict(stats (mean -Q1, mean Q1), grad, z)"""
    ns, h, act = c["ns"], c["h"], c["act"]
    s = _t(rec[0], dtype)
    p = _t(c["actor"], dtype).requires_grad_()
    q1 = _t(c["critics"] if critics is None else critics, dtype)[:(ns + 1) * h + 2 * h + 1]
    mu, z_a = mlp(p, ns, h, act, s)
    q, z_q = mlp(q1, ns + 1, h, act, torch.cat([s, (_t(c["scale"], dtype) * torch.tanh(mu))[None]]))
    loss = -q.mean()
    loss.backward()
    out = dict(stats=torch.stack([loss, q.mean()]), grad=p.grad, z=torch.cat([z_a, z_q]))
    return {k: v.detach().numpy() for k, v in out.items()}
