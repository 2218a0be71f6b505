"""DuelingNetwork(base, val, adv) (RLCore/src/utils/networks.jl:510-522, Q = val .+ adv .- mean(adv, dims = 1)) restated for the tests
of csrc/dueling.hip -- no new oracle code:

  fold / unfold     numpy Float32 in exactly the order of the kernels (left-folded sum over the na rows, a true division by
                    float(na), (Wval + Wadv) - mean): the device results are compared BIT FOR BIT against these;
  literal_q         Float32 `val + adv - mean` from two plain oracle forwards (the network as the reference writes it);
  torch_f64_grad    Float64 autograd of the literal two-layer network under Huber -- independent of the fold identity;
  composed          fold -> oracle.dqn_loss_grad / oracle.dqn3_loss_grad on the effective vectors -> unfold: what the device computes.

Flat dueling vector: [plain layout with (Wadv, badv) as its last Dense | Wval (h) | bval (1)]; the last Dense is W (na x h,
column-major: element (a, j) at j * na + a) followed by b (na).
Shared by tests/test_dueling_reference.py (CPU) and tests/test_gpu_dueling.py."""
import numpy as np

import oracle

F = np.float32


def plain_nparams(ns, h, na, layers):
    return oracle.mlp2_nparams(ns, h, na) if layers == 2 else oracle.mlp3_nparams(ns, h, na)


def nparams(ns, h, na, layers):
    return plain_nparams(ns, h, na, layers) + h + 1


def offsets(ns, h, na, layers):
    """{tensor: (offset, size)} of the dueling vector, in storage order"""
    sizes = [("W1", h * ns), ("b1", h)] + ([("W2", h * h), ("b2", h)] if layers == 3 else []) + \
            [("Wadv", na * h), ("badv", na), ("Wval", h), ("bval", 1)]
    out, o = {}, 0
    for name, n in sizes:
        out[name] = (o, n)
        o += n
    assert o == nparams(ns, h, na, layers)
    return out


def _left_sum(x):  # x (rows, na) Float32 -> ((x0 + x1) + x2) + x3, every partial sum rounded to Float32
    s = x[:, 0].copy()
    for a in range(1, x.shape[1]):
        s = (s + x[:, a]).astype(F)
    return s


def fold(duel, ns, h, na, layers):
    """dueling vector -> effective plain vector, Float32, the kernel's order"""
    duel = np.ascontiguousarray(duel, F)
    assert duel.size == nparams(ns, h, na, layers)
    nb = plain_nparams(ns, h, na, layers) - na * h - na
    # rows 0 .. h - 1: the columns of Wadv with Wval; row h: badv with bval -- the same expressions
    adv = duel[nb:nb + na * h + na].reshape(h + 1, na)
    val = duel[nb + na * h + na:]
    mean = (_left_sum(adv) / F(na)).astype(F)
    head = ((val[:, None] + adv).astype(F) - mean[:, None]).astype(F)
    return np.concatenate([duel[:nb], head.reshape(-1)]).astype(F)


def unfold(grad_eff, ns, h, na, layers):
    """gradient of the effective vector -> gradient of the dueling vector, Float32, the kernel's order"""
    g = np.ascontiguousarray(grad_eff, F)
    assert g.size == plain_nparams(ns, h, na, layers)
    nb = g.size - na * h - na
    ge = g[nb:].reshape(h + 1, na)
    s = _left_sum(ge)
    gadv = (ge - (s / F(na)).astype(F)[:, None]).astype(F)
    return np.concatenate([g[:nb], gadv.reshape(-1), s]).astype(F)


def unfold_f64(grad_eff, ns, h, na, layers):
    """the chain rule of the fold evaluated in Float64 (no statement about summation order)"""
    g = np.asarray(grad_eff, np.float64)
    nb = g.size - na * h - na
    ge = g[nb:].reshape(h + 1, na)
    return np.concatenate([g[:nb], (ge - ge.mean(1, keepdims=True)).reshape(-1), ge.sum(1)])


def make(ns, h, na, layers, plain, rng, bval_scale=0.1):
    """a dueling vector from a plain one (its last Dense becomes adv) and a Glorot-uniform Dense(h, 1) val head with a bias"""
    lim = np.sqrt(6.0 / (h + 1))
    wval = rng.uniform(-lim, lim, h).astype(F)
    return np.concatenate([np.asarray(plain, F), wval, [F(rng.normal() * bval_scale)]]).astype(F)


def literal_q(duel, ns, h, na, act, x, layers=2):
    """Float32 `val .+ adv .- mean(adv, dims = 1)`: the adv and val heads as two plain networks on the shared base"""
    duel = np.ascontiguousarray(duel, F)
    n = plain_nparams(ns, h, na, layers)
    nb = n - na * h - na
    fwd = oracle.mlp2_forward if layers == 2 else oracle.mlp3_forward
    adv = fwd(np.ascontiguousarray(duel[:n]), ns, h, na, act, x)
    val = fwd(np.concatenate([duel[:nb], duel[n:]]).astype(F), ns, h, 1, act, x)
    mean = (_left_sum(np.ascontiguousarray(adv.T)) / F(na)).astype(F)
    return ((val + adv).astype(F) - mean[None, :]).astype(F)


def torch_f64_grad(duel, duel_t, ns, h, na, act, s, a, r, t, sn, gamma, delta=1.0):
    """(loss, gradient in the flat dueling layout, Q(s) Float64) of the LITERAL two-layer dueling network: torch Float64 autograd of
    mean(huber(Q(s)[a] - (r + gamma (1 - t) max Qt(s'))))"""
    import torch

    off = offsets(ns, h, na, 2)

    def tensors(p, grad):
        p = np.asarray(p, np.float64)
        shapes = {"W1": (ns, h), "b1": (h,), "Wadv": (h, na), "badv": (na,), "Wval": (h,), "bval": (1,)}
        return {k: torch.tensor(p[o:o + n].reshape(shapes[k]), dtype=torch.float64, requires_grad=grad) for k, (o, n) in off.items()}

    def q(P, x):
        z = P["W1"].T @ x + P["b1"][:, None]  # W1 is stored column-major (h x ns): the (ns, h) view is its transpose
        hh = torch.relu(z) if act == 0 else torch.tanh(z)
        adv = P["Wadv"].T @ hh + P["badv"][:, None]
        val = (P["Wval"] @ hh + P["bval"])[None, :]
        return val + adv - adv.mean(0, keepdim=True)

    P, PT = tensors(duel, True), tensors(duel_t, False)
    T = lambda x: torch.tensor(np.asarray(x, np.float64))  # noqa: E731
    b = len(r)
    qs = q(P, T(s))
    with torch.no_grad():
        y = T(r) + gamma * (1 - T(t)) * q(PT, T(sn)).max(0).values
    e = qs[torch.tensor(np.asarray(a, np.int64)), torch.arange(b)] - y
    loss = torch.nn.functional.huber_loss(e, torch.zeros_like(e), delta=delta)
    loss.backward()
    g = np.concatenate([P[k].grad.numpy().reshape(-1) for k in off])
    return float(loss.detach()), g, qs.detach().numpy()


def composed(layers, ns, h, na, act, duel, duel_t, s, a, r, t, sn, gamma, delta=1.0, weights=None):
    """what the device computes: fold both nets, the oracle's plain loss / gradient on the effective vectors, unfold.
    -> (loss, dueling gradient, effective online vector, effective target vector)"""
    pe, pte = fold(duel, ns, h, na, layers), fold(duel_t, ns, h, na, layers)
    if layers == 2:
        loss, g = oracle.dqn_loss_grad(ns, h, na, act, pe, pte, s, a, r, t, sn, gamma, delta, weights=weights)
    else:
        loss, g, _ = oracle.dqn3_loss_grad(ns, h, na, act, pe, pte, s, a, r, t, sn, gamma, delta, weights=weights)
    return loss, unfold(g, ns, h, na, layers), pe, pte
