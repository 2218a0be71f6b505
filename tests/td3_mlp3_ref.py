"""A plain torch model of the "TD3 and DDPG with two hidden layers" section of include/rlhip.h, built as tests/td3_ref.py is: the
networks, the gathered records and the clipped noise `e` in; targets, losses, statistics and -- by autograd -- both gradients out.
dtype = torch.float64 is the reference, torch.float32 gives the Float32 floor of each output.  No order of summation is modelled.
Also the case list of tests/test_gpu_td3_mlp3.py, shared with the CPU check of its decision margins."""
import numpy as np
import torch

import sac_cases as SC
from heads_ref import F32

CARRY = 256 * 32 + 1  # the smallest batch at which a workgroup carries a second tile (asserted from the workspace function)
BASE = dict(ns=3, h=64, act=0, nc=2, batch=65, tn=0.2, clip=0.5, scale=2.0, lo=-1.2, hi=1.2, terminal=0.15, gamma=0.99)
CASES = {"base": dict(), "h32": dict(h=32), "h96": dict(h=96), "h256": dict(h=256), "ns2": dict(ns=2), "ns4": dict(ns=4),
         "tanh": dict(act=1), "ddpg": dict(nc=1, tn=0.0), "b1": dict(batch=1), "b63": dict(batch=63), "b64": dict(batch=64),
         "carry": dict(batch=CARRY), "corner": dict(h=256, ns=4, act=1)}
SEEDS = {"carry": 2}  # walked on the CPU until the Float32 and Float64 models take the same decisions (test_td3_mlp3_reference.py)


def nparams(ni, h):
    return h * ni + h + h * h + h + h + 1


def _net(rng, ni, h):
    s1, s2, s3 = 2.0 * np.sqrt(6.0 / (ni + h)), np.sqrt(6.0 / (2 * h)), 4.0 * np.sqrt(6.0 / (h + 1))
    return np.concatenate([rng.uniform(-s1, s1, h * ni), rng.uniform(-0.3, 0.3, h), rng.uniform(-s2, s2, h * h), rng.uniform(-0.3, 0.3, h),
                           rng.uniform(-s3, s3, h), rng.uniform(-0.3, 0.3, 1)]).astype(F32)


def build(name):
    c = dict(BASE, name=name, **CASES[name])
    rng = np.random.default_rng(7000 + 10 * list(CASES).index(name) + SEEDS.get(name, 0))
    ns, h = c["ns"], c["h"]
    c["actor"], c["actor_t"] = _net(rng, ns, h), _net(rng, ns, h)
    c["critics"] = np.concatenate([_net(rng, ns + 1, h) for _ in range(c["nc"])])
    c["targets"] = (c["critics"] + rng.normal(0, 0.02, c["critics"].shape)).astype(F32)
    c["S"] = rng.normal(0, 1, (SC.PUSHES + 1, ns, SC.N_ENV)).astype(F32)
    c["A"] = rng.uniform(-c["scale"], c["scale"], (SC.PUSHES, SC.N_ENV)).astype(F32)
    c["Rw"] = rng.normal(0, 1, (SC.PUSHES, SC.N_ENV)).astype(F32)
    c["T"] = (rng.uniform(size=(SC.PUSHES, SC.N_ENV)) < c["terminal"]).astype(np.uint8)
    c["idx"] = rng.integers(0, SC.CAP * SC.N_ENV, c["batch"]).astype(np.int64)
    return c


def records(c, idx):
    p, e = idx // SC.N_ENV + (SC.PUSHES - SC.CAP), idx % SC.N_ENV  # logical transition li is push li + (PUSHES - CAP)
    return (np.ascontiguousarray(c["S"][p, :, e].T), c["A"][p, e], c["Rw"][p, e], c["T"][p, e], np.ascontiguousarray(c["S"][p + 1, :, e].T))


def clipped(c, draws):
    return np.clip(F32(c["tn"]) * draws, F32(-c["clip"]), F32(c["clip"])).astype(F32) if c["tn"] else np.zeros_like(draws)


def mlp(p, ni, h, act, x):
    """mlp3(ni, h, 1) on x (ni, B) from the flat vector p -> (out (B,), z1 and z2 stacked (2 h, B))"""
    f = torch.relu if act == 0 else torch.tanh
    o = np.cumsum([0, h * ni, h, h * h, h, h])
    W1, b1, W2, b2, W3, b3 = p[:o[1]].reshape(ni, h), p[o[1]:o[2]], p[o[2]:o[3]].reshape(h, h), p[o[3]:o[4]], p[o[4]:o[5]], p[o[5]]
    z1 = W1.t() @ x + b1[:, None]
    z2 = W2.t() @ f(z1) + b2[:, None]
    return W3 @ f(z2) + b3, torch.cat([z1, z2])


def _t(x, dtype):
    return torch.tensor(np.asarray(x), dtype=dtype)


def critic(c, rec, e, dtype=torch.float64):
    """the critic update -> dict(y, loss, grad, u_raw (u' before its clamp), qt (nc, B), z: every pre-activation of both layers)"""
    ns, h, act, nc = c["ns"], c["h"], c["act"], c["nc"]
    s, a, r, t, sn = (_t(x, dtype) for x in rec)
    npq = nparams(ns + 1, h)
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
    """the actor update against `critics` (default c's) -> dict(stats (mean -Q1, mean Q1), grad, z)"""
    ns, h, act = c["ns"], c["h"], c["act"]
    s = _t(rec[0], dtype)
    p = _t(c["actor"], dtype).requires_grad_()
    q1 = _t(c["critics"] if critics is None else critics, dtype)[:nparams(ns + 1, h)]
    mu, z_a = mlp(p, ns, h, act, s)
    q, z_q = mlp(q1, ns + 1, h, act, torch.cat([s, (_t(c["scale"], dtype) * torch.tanh(mu))[None]]))
    loss = -q.mean()
    loss.backward()
    out = dict(stats=torch.stack([loss, q.mean()]), grad=p.grad, z=torch.cat([z_a, z_q]))
    return {k: v.detach().numpy() for k, v in out.items()}


def decisions(c, rc, ra):
    """every decision of an update: the smaller target critic, whether u' clamps (and where), the sign of every relu pre-activation"""
    d = [rc["u_raw"] > c["hi"], rc["u_raw"] < c["lo"]]
    if c["nc"] == 2:
        d.append(rc["qt"][1] < rc["qt"][0])
    if c["act"] == 0:
        d += [rc["z"] > 0, ra["z"] > 0]
    return [np.asarray(x) for x in d]


rel = lambda got, want: float(np.abs(np.asarray(got, np.float64) - want).max() / max(np.abs(want).max(), 1e-30))  # noqa: E731


def floors(c, rec, e):
    """-> (Float64 critic run, Float64 actor run, {output: distance of the Float32 model from them, relative to max |reference|},
    whether both precisions take the same decisions)"""
    rc, ra, rc32, ra32 = critic(c, rec, e), actor(c, rec), critic(c, rec, e, torch.float32), actor(c, rec, dtype=torch.float32)
    fl = dict(y=rel(rc32["y"], rc["y"]), closs=rel(rc32["loss"], rc["loss"]), cgrad=rel(rc32["grad"], rc["grad"]),
              stats=rel(ra32["stats"], ra["stats"]), agrad=rel(ra32["grad"], ra["grad"]))
    same = all(np.array_equal(a, b) for a, b in zip(decisions(c, rc, ra), decisions(c, rc32, ra32)))
    return rc, ra, fl, same
