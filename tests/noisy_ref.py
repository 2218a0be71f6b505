"""The NoisyDense section of include/rlhip.h as a plain numpy model, Float64 unless a dtype is handed in: the factor draws (Philox words
from the oracle's binding, the Box-Muller lines here), f, the fold, the unfold and the per-env forward up to Q."""
import numpy as np

from oracle.binding import philox

QA, QB, QC, QD = 0, 16, 272, 528
TAG_ACT, TAG_ONLINE, TAG_TARGET = 12, 13, 14


def normal_draws(seed, idx, step, q0, count, tag):
    """e_q for q = q0 .. q0 + count - 1 (q0 even): one Philox block and one Box-Muller transform per pair"""
    out = np.empty(count + (count & 1))
    for p in range(len(out) // 2):
        w = philox(seed, idx & 0xFFFFFFFF, (q0 >> 1) + p, step, tag)
        u1, u2 = ((w[0] >> 8) + 1) * 2.0 ** -24, (w[1] >> 8) * 2.0 ** -24
        r, a = np.sqrt(-2.0 * np.log(u1)), 6.283185307179586 * u2
        out[2 * p], out[2 * p + 1] = r * np.cos(a), r * np.sin(a)
    return out[:count]


def f(e):
    return np.copysign(np.sqrt(np.abs(e)), e)


def factors(seed, idx, step, tag, ns, h, M):
    """-> a (ns), b (h), c (h), d (M)"""
    return tuple(f(normal_draws(seed, idx, step, q0, n, tag)) for q0, n in ((QA, ns), (QB, h), (QC, h), (QD, M)))


def xi(seed, counter, tag, ns, h, M):
    """the noise of every element of the mlp2 layout W1 (h x ns, column-major) | b1 | W2 (M x h, column-major) | b2"""
    a, b, c, d = factors(seed, 0, counter, tag, ns, h, M)
    return np.concatenate([np.outer(a, b).ravel(), b, np.outer(c, d).ravel(), d])


def fold(noisy, x):
    noisy = np.asarray(noisy, np.float64)
    n = noisy.size // 2
    return noisy[:n] + noisy[n:] * x


def unfold(g, x):
    g = np.asarray(g, np.float64)
    return np.concatenate([g, g * x])


def forward(noisy, ns, h, na, n_atoms, act, v_min, v_max, obs, seed, env_id_base, step, dtype=np.float64):
    """obs (ns, n) -> logits (M, n), probs (M, n), q (na, n); every operand is cast to `dtype` first and stays there"""
    M, n = na * n_atoms, obs.shape[1]
    P = np.asarray(noisy, np.float64).astype(dtype)
    half = P.size // 2

    def split(v):
        o1, o2, o3 = h * ns, h * ns + h, h * ns + h + M * h
        return v[:o1].reshape(ns, h).T, v[o1:o2], v[o2:o3].reshape(h, M).T, v[o3:]

    (W1m, b1m, W2m, b2m), (W1s, b1s, W2s, b2s) = split(P[:half]), split(P[half:])
    z = (dtype(v_min) + np.arange(n_atoms).astype(dtype) * dtype((v_max - v_min) / (n_atoms - 1))).astype(dtype)
    logits, probs, q = np.empty((M, n), dtype), np.empty((M, n), dtype), np.empty((na, n), dtype)
    for i in range(n):
        a, b, c, d = (v.astype(dtype) for v in factors(seed, env_id_base + i, step, TAG_ACT, ns, h, M))
        x = np.asarray(obs[:, i]).astype(dtype)
        pre = (W1m @ x + b1m) + b * (W1s @ (a * x) + b1s)
        hid = np.maximum(pre, dtype(0)) if act == 0 else np.tanh(pre)
        l = (W2m @ hid + b2m) + d * (W2s @ (c * hid) + b2s)
        e = np.exp(l.reshape(na, n_atoms) - l.reshape(na, n_atoms).max(1, keepdims=True))
        p = e / e.sum(1, keepdims=True)
        logits[:, i], probs[:, i], q[:, i] = l, p.ravel(), p @ z
    return logits, probs, q
