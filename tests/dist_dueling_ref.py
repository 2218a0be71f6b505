"""The dueling distributional section of include/rlhip.h as plain models, with no GPU:

  `fold` / `unfold`   the header's lines in numpy; dtype Float32 is the bit-exact replay (each line one rounded operation, the sum
                      left-folded, a true division), Float64 the same mathematics
  `combine`           the output-domain form, val .+ adv .- mean(adv, dims = 1) per atom, on rows (M', n)
  `noisy_forward`     tests/noisy_ref.py's per-env forward on the M' rows, then `combine`, softmax and Q
  `torch_model`       float64 torch: the dueling network in the reference's own form -> softmax -> Q -> a* -> projection -> the C51 loss,
                      differentiated by autograd with respect to the DUELING vector (the target and the selection without gradient)
  `case`              a seeded gradient case; at the fixed seed the float64 model's top-two target-Q gap exceeds 1e-3 and every ReLU
                      pre-activation stays 1e-6 off zero at every sample (tests/test_dist_dueling_reference.py asserts both)
Everything else (the C51 replay, the supports, the projection helper, the noisy draws) is tests/c51_ref.py's and tests/noisy_ref.py's."""
import numpy as np

import c51_ref as C
import noisy_ref as N
from heads_ref import F32, F64

SHAPES = [(2, 4, 1, 2), (3, 8, 3, 5), (4, 128, 2, 51), (4, 256, 4, 51)]  # (ns, h, na, K); (4, 8, 4, 64) is refused
REFUSED = (4, 8, 4, 64)
V_MIN, V_MAX = -2.0, 3.0


def _head(v, ns, h, rows):
    """the head of an mlp2 vector as (h + 1, rows): column j of W2, the bias as the last column"""
    return v[h * ns + h:].reshape(h + 1, rows)


def fold(duel, ns, h, na, K, dtype=F32):
    d = np.asarray(duel, dtype)
    head = _head(d, ns, h, (1 + na) * K)
    adv, val = head[:, :na * K].reshape(h + 1, na, K), head[:, na * K:]
    s = adv[:, 0]
    for o in range(1, na):
        s = (s + adv[:, o]).astype(dtype)
    mean = (s / dtype(na)).astype(dtype)
    eff = ((val[:, None, :] + adv).astype(dtype) - mean[:, None, :]).astype(dtype)
    return np.concatenate([d[:h * ns + h], eff.ravel()])


def unfold(grad_eff, ns, h, na, K, dtype=F32):
    g = np.asarray(grad_eff, dtype)
    x = _head(g, ns, h, na * K).reshape(h + 1, na, K)
    s = x[:, 0]
    for o in range(1, na):
        s = (s + x[:, o]).astype(dtype)
    adv = (x - (s / dtype(na)).astype(dtype)[:, None, :]).astype(dtype)
    return np.concatenate([g[:h * ns + h], np.concatenate([adv.reshape(h + 1, na * K), s], 1).ravel()])


def combine(rows, na, K, dtype=F64):
    """rows (M', n) -> (M, n): per atom (v + a_o) - ((a_0 + a_1) + ...) / na"""
    r = np.asarray(rows, dtype)
    adv, val = r[:na * K].reshape(na, K, -1), r[na * K:]
    s = adv[0]
    for o in range(1, na):
        s = (s + adv[o]).astype(dtype)
    return ((val[None] + adv).astype(dtype) - (s / dtype(na)).astype(dtype)[None]).astype(dtype).reshape(na * K, -1)


def noisy_forward(noisy, ns, h, na, K, act, obs, seed, env_id_base, step, dtype=F64):
    """-> logits (M, n), probs (M, n), q (na, n) of a noisy dueling vector, every operand in `dtype`"""
    raw = N.forward(noisy, ns, h, 1 + na, K, act, V_MIN, V_MAX, obs, seed, env_id_base, step, dtype=dtype)[0]
    l = combine(raw, na, K, dtype)
    z = (dtype(V_MIN) + np.arange(K).astype(dtype) * dtype((V_MAX - V_MIN) / (K - 1))).astype(dtype)
    e = np.exp(l.reshape(na, K, -1) - l.reshape(na, K, -1).max(1, keepdims=True))
    p = (e / e.sum(1, keepdims=True)).astype(dtype)
    return l, p.reshape(na * K, -1), np.einsum("k,okn->on", z, p).astype(dtype)


def case(ns, h, na, K, batch, double=False, extras=False, seed=0):
    """a C51 case of tests/c51_ref.py whose networks are dueling vectors (`duel`, `duel_t`); `params` / `target` are their Float32 folds"""
    rng = np.random.default_rng([seed, ns, h, na, K, batch, int(double), int(extras)])
    nd = C.nparams(ns, h, (1 + na) * K)
    duel, duel_t = (rng.normal(0, 0.4, nd).astype(F32) for _ in range(2))
    c = dict(ns=ns, h=h, na=na, n_atoms=K, act=0 if h > 8 else 1, batch=batch, v_min=V_MIN, v_max=V_MAX, gamma=0.9, double=double,
             duel=duel, duel_t=duel_t, params=fold(duel, ns, h, na, K), target=fold(duel_t, ns, h, na, K),
             s=rng.normal(0, 1, (ns, batch)).astype(F32), sn=rng.normal(0, 1, (ns, batch)).astype(F32),
             a=rng.integers(0, na, batch).astype(np.int32), r=rng.normal(0.2, 1.0, batch).astype(F32),
             term=(rng.uniform(size=batch) < 0.2).astype(np.uint8), n_used=None, weights=None)
    if extras:
        c.update(n_used=rng.integers(1, 4, batch).astype(np.int32), weights=rng.uniform(0.3, 1.0, batch).astype(F32))
    return c


def torch_model(c):
    """-> dict(grad (dueling length), loss, sel, gap, zmin): float64 autograd of the dueling C51 loss"""
    import torch

    ns, h, na, K, act, B = c["ns"], c["h"], c["na"], c["n_atoms"], c["act"], c["batch"]
    t = lambda x: torch.tensor(np.asarray(x, F64), dtype=torch.float64)  # noqa: E731
    z = t(C.support(c)[1])
    zmin = [np.inf]

    def logits(p, x):  # the reference's own form: val .+ adv .- mean(adv, dims = 1), (na, K, B)
        o1, o2, rows = h * ns, h * ns + h, (1 + na) * K
        pre = p[:o1].reshape(ns, h).t() @ x + p[o1:o2, None]
        zmin[0] = min(zmin[0], float(pre.detach().abs().min()))
        out = p[o2:o2 + rows * h].reshape(h, rows).t() @ (torch.relu(pre) if act == 0 else torch.tanh(pre)) + p[o2 + rows * h:, None]
        adv, val = out[:na * K].reshape(na, K, B), out[na * K:]
        return val[None] + adv - adv.mean(0, keepdim=True)

    duel, duel_t, cols = t(c["duel"]).requires_grad_(True), t(c["duel_t"]), torch.arange(B)
    with torch.no_grad():
        pt = torch.softmax(logits(duel_t, t(c["sn"])), 1)
        qsel = (torch.softmax(logits(duel, t(c["sn"])), 1) * z[None, :, None]).sum(1) if c["double"] else (pt * z[None, :, None]).sum(1)
        sel = torch.argmax(qsel, 0)
        top = torch.sort(qsel, 0, descending=True).values
        tz = t(c["r"])[:, None] + t(C.discount(c))[:, None] * z[None, :]
        m = C.project(tz, pt[sel, :, cols], z)  # (B, K)
    la = logits(duel, t(c["s"]))[torch.tensor(c["a"].astype(np.int64)), :, cols]
    w = t(c["weights"]) if c["weights"] is not None else torch.ones(B, dtype=torch.float64)
    loss = (w * -(m * torch.log_softmax(la, 1)).sum(1)).sum() / B
    loss.backward()
    return dict(grad=duel.grad.numpy().copy(), loss=float(loss.detach()), sel=sel.numpy().astype(np.int32),
                gap=float((top[0] - top[1]).min()) if na > 1 else np.inf, zmin=zmin[0] if act == 0 else np.inf)


def replay_grad(c):
    """the Float32 replay of the update path: C51's replay on the folded vectors, then the unfold -> (grad (dueling length), replay)"""
    rp = C.replay(c)
    return unfold(rp["grad"].astype(F32), c["ns"], c["h"], c["na"], c["n_atoms"]), rp
