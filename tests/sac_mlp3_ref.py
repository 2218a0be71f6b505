"""A plain torch model of the "SAC with two hidden layers" section of include/rlhip.h, built as tests/td3_mlp3_ref.py is: the networks,
the gathered records and the regenerated draws in; targets, losses, statistics, `sel`, `pass`, the alpha step and -- by autograd --
both gradients out.  dtype = torch.float64 is the reference, torch.float32 gives the Float32 floor of each output.  No order of
summation is modelled.  `actor_by_the_header` pulls the actor loss back through the head by the header's own lines (dmu, dsg, draw,
drho), for the CPU check that they are the derivative of the plain formulas.  Also the case list of tests/test_gpu_sac_mlp3.py."""
import numpy as np
import torch

import sac_cases as SC
import td3_mlp3_ref as T
from heads_ref import F32

BASE = dict(ns=3, h=64, act=0, batch=65, alpha=0.2, alpha_lr=3e-3, target_entropy=-1.0, scale=2.0, lo=0.0, hi=np.inf, gamma=0.99)
# `carry`: at h = 256 a partial row of [Q1 | Q2] is 526 KB, 16 MiB hold 31 of them, so the 32nd tile is a workgroup's second
# (tests/test_gpu_sac_mlp3.py reads it off the workspace function); `carry2`: the same for the actor's row (62 of 263 KB)
CASES = {"base": dict(), "ns2": dict(ns=2), "ns4": dict(ns=4), "tanh": dict(act=1), "h32": dict(h=32), "h96": dict(h=96), "h160": dict(h=160),
         "h256": dict(h=256), "b1": dict(batch=1), "b32": dict(batch=32), "carry": dict(h=256, batch=31 * 32 + 1),
         "carry2": dict(h=256, batch=62 * 32 + 1), "clamp": dict(lo=0.55, hi=0.8), "alpha": dict(alias=True)}
SEEDS = {"b32": 1}  # walked on the CPU until the Float32 and Float64 models take the same decisions (tests/test_sac_mlp3_reference.py)


def nparams(ni, h, no=1):
    return h * ni + h + h * h + h + no * h + no


def _actor(rng, ns, h):
    """mlp3(ns, h, 2): T._net's layers 1 and 2, then W3 (2 x h, column-major) and b3 (2)"""
    p, s3 = T._net(rng, ns, h), 2.0 * np.sqrt(6.0 / (h + 2))
    return np.concatenate([p[:-h - 1], rng.uniform(-s3, s3, 2 * h), rng.uniform(-0.3, 0.3, 2)]).astype(F32)


def build(name):
    c = dict(BASE, name=name, **CASES[name])
    rng = np.random.default_rng(8000 + 10 * list(CASES).index(name) + SEEDS.get(name, 0))
    ns, h = c["ns"], c["h"]
    c["actor"] = _actor(rng, ns, h)
    q1 = T._net(rng, ns + 1, h)  # (Q2 near Q1: two independent nets differ by a constant larger than their spread over the samples)
    c["critics"] = np.concatenate([q1, (q1 + rng.normal(0, 0.05, q1.shape)).astype(F32)])
    c["targets"] = (c["critics"] + rng.normal(0, 0.02, c["critics"].shape)).astype(F32)
    c["S"] = rng.normal(0, 1, (SC.PUSHES + 1, ns, SC.N_ENV)).astype(F32)
    c["A"] = rng.uniform(-c["scale"], c["scale"], (SC.PUSHES, SC.N_ENV)).astype(F32)
    c["Rw"] = rng.normal(0, 1, (SC.PUSHES, SC.N_ENV)).astype(F32)
    c["T"] = (rng.uniform(size=(SC.PUSHES, SC.N_ENV)) < 0.15).astype(np.uint8)
    c["idx"] = rng.integers(0, SC.CAP * SC.N_ENV, c["batch"]).astype(np.int64)
    li, e = np.argwhere(c["T"][SC.PUSHES - SC.CAP:] != 0)[0]
    c["idx"][0] = li * SC.N_ENV + e  # every case holds a terminal transition, batch 1 too
    return c


def mlp2o(p, ni, h, act, x):
    """mlp3(ni, h, 2) on x (ni, B) from the flat vector p -> out (2, B): row 0 mu, row 1 rho"""
    f = torch.relu if act == 0 else torch.tanh
    o = np.cumsum([0, h * ni, h, h * h, h, 2 * h])
    W1, b1, W2, b2, W3, b3 = p[:o[1]].reshape(ni, h), p[o[1]:o[2]], p[o[2]:o[3]].reshape(h, h), p[o[3]:o[4]], p[o[4]:o[5]].reshape(h, 2), p[o[5]:]
    return W3.t() @ f(W2.t() @ f(W1.t() @ x + b1[:, None]) + b2[:, None]) + b3[:, None]


def head(mu, rho, eps, c):
    """the actor head of the SAC section -> (a = tanh(z), logp, pass, sg, z)"""
    sp = torch.nn.functional.softplus
    raw = sp(rho)
    sg = raw.clamp(c["lo"], c["hi"])  # (autograd: zero outside the bounds, as the select of `pass`)
    z = mu + sg * eps
    zz = (z - mu) / (sg + 1e-8)
    logp = -(zz * zz + np.log(2 * np.pi)) / 2 - torch.log(sg + 1e-8) - 2 * ((np.log(2.0) - z) - sp(-2 * z))
    return torch.tanh(z), logp, (raw <= c["hi"]) & (raw >= c["lo"]), sg, z


_t = lambda x, dtype: torch.tensor(np.asarray(x), dtype=dtype)  # noqa: E731
_np = lambda d: {k: v.detach().numpy() for k, v in d.items()}  # noqa: E731


def critic(c, rec, eps0, dtype=torch.float64):
    """the critic update -> dict(y, loss (2,), grad, sel_t, ok: `pass` of the head at s')"""
    ns, h, act = c["ns"], c["h"], c["act"]
    s, a, r, t, sn = (_t(x, dtype) for x in rec)
    npq = nparams(ns + 1, h)
    critics, targets = _t(c["critics"], dtype).requires_grad_(), _t(c["targets"], dtype)
    o = mlp2o(_t(c["actor"], dtype), ns, h, act, sn)
    an, lpn, ok, _, _ = head(o[0], o[1], _t(eps0, dtype), c)
    xn = torch.cat([sn, (_t(c["scale"], dtype) * an)[None]])
    qt = torch.stack([T.mlp(targets[k * npq:(k + 1) * npq], ns + 1, h, act, xn)[0] for k in range(2)])
    y = r + (_t(c["gamma"], dtype) * (1 - t)) * (qt.min(0).values - _t(c["alpha"], dtype) * lpn)
    x = torch.cat([s, a[None]])
    loss = torch.stack([((T.mlp(critics[k * npq:(k + 1) * npq], ns + 1, h, act, x)[0] - y) ** 2).mean() for k in range(2)])
    loss.sum().backward()
    return _np(dict(y=y, loss=loss, grad=critics.grad, sel_t=1 + (qt[1] < qt[0]).long(), ok=ok))


def _actor_forward(c, rec, eps1, critics, dtype, p):
    ns, h, act = c["ns"], c["h"], c["act"]
    s, npq = _t(rec[0], dtype), nparams(ns + 1, h)
    q12 = _t(c["critics"] if critics is None else critics, dtype)
    o = mlp2o(p, ns, h, act, s)
    a, logp, ok, sg, z = head(o[0], o[1], _t(eps1, dtype), c)
    u = _t(c["scale"], dtype) * a
    q = torch.stack([T.mlp(q12[k * npq:(k + 1) * npq], ns + 1, h, act, torch.cat([s, u[None]]))[0] for k in range(2)])
    return o, a, logp, ok, sg, z, u, q


def actor(c, rec, eps1, critics=None, dtype=torch.float64):
    """the actor update against `critics` (default c's) -> dict(stats (3,), grad, sel, logp, ok, alpha_new)"""
    p, alpha = _t(c["actor"], dtype).requires_grad_(), _t(c["alpha"], dtype)
    o, a, logp, ok, sg, z, u, q = _actor_forward(c, rec, eps1, critics, dtype, p)
    qmin = torch.minimum(q[0], q[1])  # (no |Q1 - Q2| of a case is zero: autograd takes the smaller critic alone)
    li = alpha * logp - qmin
    li.mean().backward()
    alpha_new = alpha - _t(c["alpha_lr"], dtype) * ((-logp.mean()) - _t(c["target_entropy"], dtype))
    return _np(dict(stats=torch.stack([li.mean(), qmin.mean(), logp.mean()]), grad=p.grad, sel=1 + (q[1] < q[0]).long(), logp=logp, ok=ok,
                    alpha_new=alpha_new.reshape(1)))


def actor_by_the_header(c, rec, eps1):
    """the actor gradient in Float64 with the head pulled back by the header's lines: du of the selected critic by autograd through
    that critic alone, then dact, dz, dmu, dsg, draw, drho as written, then (dmu, drho) through the actor"""
    dtype = torch.float64
    p, fb = _t(c["actor"], dtype).requires_grad_(), float(c["batch"])
    o, a, logp, ok, sg, z, u, q = _actor_forward(c, rec, eps1, None, dtype, p)
    eps, mu, rho = _t(eps1, dtype), o[0].detach(), o[1].detach()
    du = torch.autograd.grad(torch.where(q[1] < q[0], q[1], q[0]).sum() * (-1.0 / fb), u, retain_graph=True)[0]
    a, sg, z = a.detach(), sg.detach(), z.detach()
    dlogp, dact, s = c["alpha"] / fb, c["scale"] * du, sg + 1e-8
    zz = (z - mu) / s
    w = zz / s
    dz = dlogp * (2 * a - w) + dact * (1 - a * a)
    dmu, dsg = dlogp * w + dz, dlogp * ((zz * zz - 1) / s) + dz * eps
    drho = torch.where(ok, dsg, torch.zeros_like(dsg)) * (1 / (1 + torch.exp(-rho)))
    return torch.autograd.grad(o, p, torch.stack([dmu, drho]))[0].numpy()


def floors(c, rec, eps0, eps1):
    """-> (Float64 critic run, Float64 actor run, {output: distance of the Float32 model from them, relative to max |reference|},
    whether both precisions take the same decisions: sel, the smaller target critic, `pass` of both heads)"""
    rc, ra = critic(c, rec, eps0), actor(c, rec, eps1)
    rc32, ra32 = critic(c, rec, eps0, torch.float32), actor(c, rec, eps1, dtype=torch.float32)
    fl = {k: T.rel(rc32[k], rc[k]) for k in ("y", "loss", "grad")}
    fl = dict(y=fl["y"], closs=fl["loss"], cgrad=fl["grad"], **{k: T.rel(ra32[v], ra[v]) for k, v in
                                                               (("logp", "logp"), ("stats", "stats"), ("agrad", "grad"), ("alpha", "alpha_new"))})
    same = all(np.array_equal(x[k], y[k]) for x, y, ks in ((rc, rc32, ("sel_t", "ok")), (ra, ra32, ("sel", "ok"))) for k in ks)
    return rc, ra, fl, same
