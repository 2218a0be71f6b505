"""Thin functional layer over the C ABI: torch device tensors in, torch device tensors out.

Every function here is a direct call into librlhip.so (HIP kernels); torch only owns the memory and
the stream.  Names follow the reference (RLCore/src/utils/basic.jl, .../distributions.jl, ...).
Matrix arguments follow Julia's column-major convention: pass tensors whose *storage* is the
column-major matrix, i.e. a torch tensor of shape (n2, n1) C-contiguous == Julia (n1, n2).  The
helpers `from_julia` / `to_julia` convert from/to the mathematical (n1, n2) view.
"""
import ctypes as C

import torch

from . import _lib
from ._lib import call

_DT = {torch.float32: "f32", torch.float64: "f64"}


def stream_ptr():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def ptr(t):
    if t is None:
        return None
    if not t.is_cuda:
        raise _lib.RLHipError("rlhip ops need CUDA/HIP device tensors (there is no CPU fallback)")
    if not t.is_contiguous():
        raise _lib.RLHipArgumentError("tensor must be contiguous")
    return C.c_void_p(t.data_ptr())


def from_julia(a, dtype=None, device="cuda"):
    """(n1, n2) mathematical matrix -> tensor holding its column-major storage (shape (n2, n1))."""
    t = torch.as_tensor(a, dtype=dtype, device=device)
    return t.t().contiguous() if t.dim() == 2 else t.contiguous()


def to_julia(t):
    return t.t() if t.dim() == 2 else t


def _dims_shape(t):
    """tensor holding column-major storage of an n1 x n2 matrix (shape (n2, n1)) or a vector."""
    if t.dim() == 1:
        return t.shape[0], 1
    if t.dim() == 2:
        return t.shape[1], t.shape[0]
    raise _lib.RLHipArgumentError("expected a vector or a matrix")


def _u8(t):
    if t is None:
        return None
    if t.dtype == torch.bool:
        t = t.view(torch.uint8)
    if t.dtype != torch.uint8:
        raise _lib.RLHipArgumentError("terminal / mask must be bool or uint8")
    return t


# --------------------------------------------------------------------------------------- scans
def discount_rewards(rewards, gamma, terminal=None, init=None, dims=0):
    """discount_rewards(rewards, gamma; terminal, init, dims)  RLCore/src/utils/basic.jl:138-235."""
    sfx = _DT[rewards.dtype]
    n1, n2 = _dims_shape(rewards)
    out = torch.empty_like(rewards)
    if init is not None and not torch.is_tensor(init):
        init = torch.tensor([init], dtype=rewards.dtype, device=rewards.device)
    call(f"rlhip_discount_rewards_{sfx}", ptr(out), ptr(rewards), n1, n2, gamma, ptr(_u8(terminal)),
         ptr(init), dims, stream_ptr())
    return out


def discount_rewards_reduced(rewards, gamma, terminal=None, init=None, dims=0):
    """discount_rewards_reduced  RLCore/src/utils/basic.jl:237-319."""
    sfx = _DT[rewards.dtype]
    n1, n2 = _dims_shape(rewards)
    if rewards.dim() == 2 and dims not in (1, 2):
        raise _lib.RLHipArgumentError("matrix input requires dims = 1 or 2")
    n_out = 1 if rewards.dim() == 1 else (n2 if dims == 1 else n1)
    out = torch.empty(n_out, dtype=rewards.dtype, device=rewards.device)
    if init is not None and not torch.is_tensor(init):
        init = torch.tensor([init], dtype=rewards.dtype, device=rewards.device)
    call(f"rlhip_discount_rewards_reduced_{sfx}", ptr(out), ptr(rewards), n1, n2, gamma,
         ptr(_u8(terminal)), ptr(init), dims, stream_ptr())
    return out


def generalized_advantage_estimation(rewards, values, gamma, lam, terminal=None, dims=0):
    """generalized_advantage_estimation  RLCore/src/utils/basic.jl:334-417."""
    sfx = _DT[rewards.dtype]
    n1, n2 = _dims_shape(rewards)
    out = torch.empty_like(rewards)
    call(f"rlhip_gae_{sfx}", ptr(out), ptr(rewards), ptr(values), n1, n2, gamma, lam,
         ptr(_u8(terminal)), dims, stream_ptr())
    return out


def gae_returns(rewards, values, terminal, gamma, lam):
    """PPO fusion on time-major (T, n) tensors: returns (advantages, returns)."""
    T, n = rewards.shape
    adv = torch.empty_like(rewards)
    ret = torch.empty_like(rewards)
    call("rlhip_gae_returns_f32", ptr(adv), ptr(ret), ptr(rewards), ptr(values), ptr(_u8(terminal)), n, T,
         gamma, lam, stream_ptr())
    return adv, ret


# ----------------------------------------------------------------------------------- selection
def get_eps(kind, eps_stable, eps_init, warmup_steps, decay_steps, step):
    return _lib.lib.rlhip_get_eps({"linear": 0, "exp": 1}[kind], eps_stable, eps_init, warmup_steps,
                                  decay_steps, step)


def eps_greedy_select(values, eps, seed, step, env_id_base=0, mask=None, is_break_tie=False, soa=True):
    """values: (na, n) tensor.  soa=True: C-contiguous (na, n) (component-major, this library's layout);
    soa=False: storage of a Julia (na, N) column-major matrix, i.e. torch shape (n, na)."""
    if soa:
        na, n = values.shape
        ks, is_ = n, 1
    else:
        n, na = values.shape
        ks, is_ = 1, na
    out = torch.empty(n, dtype=torch.int32, device=values.device)
    call("rlhip_eps_greedy_select_f32", ptr(values), na, n, ks, is_, ptr(_u8(mask)), float(eps),
         int(is_break_tie), seed, env_id_base, step, ptr(out), stream_ptr())
    return out


def eps_greedy_prob(values, eps, mask=None, is_break_tie=False, soa=True):
    """prob(::EpsilonGreedyExplorer, values[, mask]) for every env of a (na, n) device tensor: Float64 probabilities in the
    layout of `values` (epsilon_greedy_explorer.jl:141-194)."""
    if soa:
        na, n = values.shape
        ks, is_ = n, 1
    else:
        n, na = values.shape
        ks, is_ = 1, na
    out = torch.empty(values.shape, dtype=torch.float64, device=values.device)
    m8 = _u8(mask)
    call("rlhip_eps_greedy_prob_f32", ptr(values), na, n, ks, is_, ptr(m8), float(eps), int(is_break_tie), ptr(out),
         stream_ptr())
    return out


def categorical_sample(logits, seed, step, env_id_base=0, mask=None, soa=True):
    if soa:
        na, n = logits.shape
        ks, is_ = n, 1
    else:
        n, na = logits.shape
        ks, is_ = 1, na
    a = torch.empty(n, dtype=torch.int32, device=logits.device)
    lp = torch.empty(n, dtype=torch.float32, device=logits.device)
    call("rlhip_categorical_sample_f32", ptr(logits), na, n, ks, is_, ptr(_u8(mask)), seed, env_id_base,
         step, ptr(a), ptr(lp), stream_ptr())
    return a, lp


# ------------------------------------------------------------------------------------- updates
def polyak_(dst, src, rho):
    call("rlhip_polyak_f32", ptr(dst), ptr(src), dst.numel(), rho, stream_ptr())
    return dst


def clip_by_global_norm_(grad, clip_norm):
    """clip_by_global_norm!(gs, ps, clip_norm)  RLCore/src/utils/basic.jl:21-29 -> device scalar gn."""
    gn = torch.empty(1, dtype=torch.float32, device=grad.device)
    call("rlhip_clip_by_global_norm_f32", ptr(grad), grad.numel(), clip_norm, ptr(gn), stream_ptr())
    return gn


def adam_(params, grad, m, v, beta_pow, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8):
    call("rlhip_adam_f32", ptr(params), ptr(grad), ptr(m), ptr(v), ptr(beta_pow), params.numel(), lr, beta1,
         beta2, eps, stream_ptr())


def clip_adam_(params, grad, m, v, beta_pow, grad_scale=1.0, clip_norm=0.0, lr=1e-3, beta1=0.9,
               beta2=0.999, eps=1e-8, gn_out=None):
    call("rlhip_clip_adam_f32", ptr(params), ptr(grad), ptr(m), ptr(v), ptr(beta_pow), params.numel(),
         grad_scale, clip_norm, lr, beta1, beta2, eps, ptr(gn_out), stream_ptr())


def normlogpdf(mu, sigma, x):
    if _wants_grad(mu, sigma, x):
        from . import grad

        return grad.NormLogPdf.apply(mu, sigma, x)
    out = torch.empty_like(x)
    call("rlhip_normlogpdf_f32", ptr(mu), ptr(sigma), ptr(x), ptr(out), x.numel(), stream_ptr())
    return out


def diagnormlogpdf(mu, sigma, x):
    """arrays are storages of Julia (d, n) matrices: torch shape (n, d)."""
    if _wants_grad(mu, sigma, x):
        from . import grad

        return grad.DiagNormLogPdf.apply(mu, sigma, x)
    n, d = mu.shape
    out = torch.empty(n, dtype=torch.float32, device=mu.device)
    call("rlhip_diagnormlogpdf_f32", ptr(mu), ptr(sigma), ptr(x), d, n, ptr(out), stream_ptr())
    return out


def _wants_grad(*tensors):
    """autograd is recording and an input asks for a gradient: the call goes through rlhip/grad.py (same kernels, same values)"""
    return torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors)


def vec_to_tril(chol_vec, da):
    """vec_to_tril(cholesky_vec, da)  RLCore/src/utils/networks.jl:359-381.  chol_vec: storage of a Julia (nv, n) matrix, torch shape
    (n, nv) with nv = da (da + 1) / 2 -> storage of the Julia (da, da, n) array L: torch shape (n, da, da) indexed [state, column, row]."""
    if _wants_grad(chol_vec):
        from . import grad

        return grad.VecToTril.apply(chol_vec, da)
    n, nv = chol_vec.shape
    if nv != da * (da + 1) // 2:
        raise _lib.RLHipArgumentError(f"a Cholesky vector for da = {da} has {da * (da + 1) // 2} elements, got {nv}")
    out = torch.empty((n, da, da), dtype=torch.float32, device=chol_vec.device)
    call("rlhip_vec_to_tril_f32", ptr(chol_vec), da, n, ptr(out), stream_ptr())
    return out


def mvnormlogpdf(mu, L, x):
    """mvnormlogpdf(mu, L, x), the batch form  RLCore/src/utils/distributions.jl:46-66.  Storages of the Julia arrays: mu (n, da)
    [Julia (da, 1, n)], L (n, da, da) [Julia (da, da, n)], x (n, K, da) [Julia (da, K, n)] -> (n, K) [Julia (1, K, n)]; x (n, da) is
    K = 1 and gives (n,)."""
    if _wants_grad(mu, L, x):
        from . import grad

        return grad.MvNormLogPdf.apply(mu, L, x)
    n, da = mu.shape
    flat = x.dim() == 2
    K = 1 if flat else x.shape[1]
    if tuple(L.shape) != (n, da, da) or tuple(x.shape) != ((n, da) if flat else (n, K, da)):
        raise _lib.RLHipArgumentError(f"mvnormlogpdf: mu {tuple(mu.shape)}, L {tuple(L.shape)}, x {tuple(x.shape)} do not agree")
    out = torch.empty((n,) if flat else (n, K), dtype=torch.float32, device=mu.device)
    call("rlhip_mvnormlogpdf_f32", ptr(mu), ptr(L), ptr(x), da, K, n, ptr(out), stream_ptr())
    return out


def normkldivergence(mu1, sigma1, mu2, sigma2):
    """normkldivergence(mu1, sigma1, mu2, sigma2) elementwise  RLCore/src/utils/distributions.jl:137-139"""
    if _wants_grad(mu1, sigma1, mu2, sigma2):
        from . import grad

        return grad.NormKL.apply(mu1, sigma1, mu2, sigma2)
    if not (mu1.shape == sigma1.shape == mu2.shape == sigma2.shape):
        raise _lib.RLHipArgumentError("normkldivergence: the four arguments must have one shape")
    out = torch.empty_like(mu1)
    call("rlhip_normkldivergence_f32", ptr(mu1), ptr(sigma1), ptr(mu2), ptr(sigma2), mu1.numel(), ptr(out), stream_ptr())
    return out


def diagnormkldivergence(mu1, sigma1, mu2, sigma2):
    """diagnormkldivergence  RLCore/src/utils/distributions.jl:117-129.  arrays are storages of Julia (d, n) matrices: torch shape
    (n, d) -> (n,)."""
    if _wants_grad(mu1, sigma1, mu2, sigma2):
        from . import grad

        return grad.DiagNormKL.apply(mu1, sigma1, mu2, sigma2)
    if not (mu1.dim() == 2 and mu1.shape == sigma1.shape == mu2.shape == sigma2.shape):
        raise _lib.RLHipArgumentError("diagnormkldivergence: the four arguments must be (n, d) tensors of one shape")
    n, d = mu1.shape
    out = torch.empty(n, dtype=torch.float32, device=mu1.device)
    call("rlhip_diagnormkldivergence_f32", ptr(mu1), ptr(sigma1), ptr(mu2), ptr(sigma2), d, n, ptr(out), stream_ptr())
    return out


def mvnormkldivergence(mu1, L1, mu2, L2):
    """mvnormkldivergence(mu1, L1, mu2, L2), the batch form  RLCore/src/utils/distributions.jl:88-109.  mu (n, da), L (n, da, da) as in
    `mvnormlogpdf` -> (n,)."""
    if _wants_grad(mu1, L1, mu2, L2):
        from . import grad

        return grad.MvNormKL.apply(mu1, L1, mu2, L2)
    n, da = mu1.shape
    if mu2.shape != mu1.shape or tuple(L1.shape) != (n, da, da) or tuple(L2.shape) != (n, da, da):
        raise _lib.RLHipArgumentError("mvnormkldivergence: mu (n, da) and L (n, da, da) do not agree")
    out = torch.empty(n, dtype=torch.float32, device=mu1.device)
    call("rlhip_mvnormkldivergence_f32", ptr(mu1), ptr(L1), ptr(mu2), ptr(L2), da, n, ptr(out), stream_ptr())
    return out


def _like(t, want):
    return torch.empty_like(t) if want else None


def vec_to_tril_backward(chol_vec, dL, da):
    """pullback of `vec_to_tril`: chol_vec (n, nv), dL (n, da, da) [only its lower triangle is read] -> dvec (n, nv)"""
    n, nv = chol_vec.shape
    if nv != da * (da + 1) // 2 or tuple(dL.shape) != (n, da, da):
        raise _lib.RLHipArgumentError(f"vec_to_tril_backward: chol_vec {tuple(chol_vec.shape)}, dL {tuple(dL.shape)}, da = {da}")
    out = torch.empty_like(chol_vec)
    call("rlhip_vec_to_tril_bwd_f32", ptr(chol_vec), ptr(dL), da, n, ptr(out), stream_ptr())
    return out


def mvnormlogpdf_backward(mu, L, x, dlogp, need=(True, True, True)):
    """pullback of `mvnormlogpdf`: the forward arguments and dlogp shaped like the forward output -> (dmu (n, da), dL (n, da, da) with
    zeros above the diagonal, dx like x); `need` skips outputs (None in their place).  The sums over K run in ascending order."""
    n, da = mu.shape
    flat = x.dim() == 2
    K = 1 if flat else x.shape[1]
    if (tuple(L.shape) != (n, da, da) or tuple(x.shape) != ((n, da) if flat else (n, K, da))
            or tuple(dlogp.shape) != ((n,) if flat else (n, K))):
        raise _lib.RLHipArgumentError(f"mvnormlogpdf_backward: mu {tuple(mu.shape)}, L {tuple(L.shape)}, x {tuple(x.shape)}, "
                                      f"dlogp {tuple(dlogp.shape)} do not agree")
    dmu, dL, dx = _like(mu, need[0]), _like(L, need[1]), _like(x, need[2])
    call("rlhip_mvnormlogpdf_bwd_f32", ptr(mu), ptr(L), ptr(x), ptr(dlogp), da, K, n, ptr(dmu), ptr(dL), ptr(dx), stream_ptr())
    return dmu, dL, dx


def cov_gaussian_head_logp_backward(mu, chol_vec, action, dlogp, need=(True, True)):
    """pullback of (model::CovGaussianNetwork)(state, action) onto the heads' outputs, one launch: mu (n, da), chol_vec (n, nv),
    action (n, K, da), dlogp (n, K) -> (dmu (n, da), dvec (n, nv))"""
    n, da = mu.shape
    K = action.shape[1] if action.dim() == 3 else 0
    if tuple(chol_vec.shape) != (n, da * (da + 1) // 2) or tuple(action.shape) != (n, K, da) or tuple(dlogp.shape) != (n, K):
        raise _lib.RLHipArgumentError(f"cov_gaussian_head_logp_backward: mu {tuple(mu.shape)}, chol_vec {tuple(chol_vec.shape)}, "
                                      f"action {tuple(action.shape)}, dlogp {tuple(dlogp.shape)} do not agree")
    dmu, dvec = _like(mu, need[0]), _like(chol_vec, need[1])
    call("rlhip_cov_gaussian_head_logp_bwd_f32", ptr(mu), ptr(chol_vec), ptr(action), ptr(dlogp), da, n, K, ptr(dmu), ptr(dvec),
         stream_ptr())
    return dmu, dvec


def mvnormkldivergence_backward(mu1, L1, mu2, L2, dout, need=(True, True, True, True)):
    """pullback of `mvnormkldivergence`: dout (n,) -> (dmu1, dL1, dmu2, dL2) shaped like the arguments"""
    n, da = mu1.shape
    if mu2.shape != mu1.shape or tuple(L1.shape) != (n, da, da) or tuple(L2.shape) != (n, da, da) or tuple(dout.shape) != (n,):
        raise _lib.RLHipArgumentError("mvnormkldivergence_backward: mu (n, da), L (n, da, da) and dout (n,) do not agree")
    outs = tuple(_like(t, w) for t, w in zip((mu1, L1, mu2, L2), need))
    call("rlhip_mvnormkldivergence_bwd_f32", ptr(mu1), ptr(L1), ptr(mu2), ptr(L2), ptr(dout), da, n, *(ptr(o) for o in outs),
         stream_ptr())
    return outs


def diagnormkldivergence_backward(mu1, sigma1, mu2, sigma2, dout, need=(True, True, True, True)):
    """pullback of `diagnormkldivergence`: (n, d) arguments, dout (n,) -> (dmu1, dsigma1, dmu2, dsigma2)"""
    if not (mu1.dim() == 2 and mu1.shape == sigma1.shape == mu2.shape == sigma2.shape) or tuple(dout.shape) != (mu1.shape[0],):
        raise _lib.RLHipArgumentError("diagnormkldivergence_backward: four (n, d) tensors of one shape and dout (n,)")
    n, d = mu1.shape
    outs = tuple(_like(t, w) for t, w in zip((mu1, sigma1, mu2, sigma2), need))
    call("rlhip_diagnormkldivergence_bwd_f32", ptr(mu1), ptr(sigma1), ptr(mu2), ptr(sigma2), ptr(dout), d, n,
         *(ptr(o) for o in outs), stream_ptr())
    return outs


def normkldivergence_backward(mu1, sigma1, mu2, sigma2, dout, need=(True, True, True, True)):
    """pullback of `normkldivergence`, elementwise: five tensors of one shape -> (dmu1, dsigma1, dmu2, dsigma2)"""
    if not (mu1.shape == sigma1.shape == mu2.shape == sigma2.shape == dout.shape):
        raise _lib.RLHipArgumentError("normkldivergence_backward: the five arguments must have one shape")
    outs = tuple(_like(t, w) for t, w in zip((mu1, sigma1, mu2, sigma2), need))
    call("rlhip_normkldivergence_bwd_f32", ptr(mu1), ptr(sigma1), ptr(mu2), ptr(sigma2), ptr(dout), mu1.numel(),
         *(ptr(o) for o in outs), stream_ptr())
    return outs


def normlogpdf_backward(mu, sigma, x, dout, need=(True, True, True)):
    """pullback of `normlogpdf`, elementwise: four tensors of one shape -> (dmu, dsigma, dx); `need` skips outputs (None in their place)"""
    if not (mu.shape == sigma.shape == x.shape == dout.shape):
        raise _lib.RLHipArgumentError("normlogpdf_backward: the four arguments must have one shape")
    outs = tuple(_like(t, w) for t, w in zip((mu, sigma, x), need))
    call("rlhip_normlogpdf_bwd_f32", ptr(mu), ptr(sigma), ptr(x), ptr(dout), x.numel(), *(ptr(o) for o in outs), stream_ptr())
    return outs


def diagnormlogpdf_backward(mu, sigma, x, dout, need=(True, True, True)):
    """pullback of `diagnormlogpdf`: three (n, d) tensors of one shape, dout (n,) -> (dmu, dsigma, dx); d <= 64, the heads' bound"""
    if not (mu.dim() == 2 and mu.shape == sigma.shape == x.shape) or tuple(dout.shape) != (mu.shape[0],):
        raise _lib.RLHipArgumentError("diagnormlogpdf_backward: three (n, d) tensors of one shape and dout (n,)")
    n, d = mu.shape
    outs = tuple(_like(t, w) for t, w in zip((mu, sigma, x), need))
    call("rlhip_diagnormlogpdf_bwd_f32", ptr(mu), ptr(sigma), ptr(x), ptr(dout), d, n, *(ptr(o) for o in outs), stream_ptr())
    return outs


def gaussian_head_logp_backward(mu, raw_sigma, action, dlogp, min_sigma, max_sigma, squash, soft, need=(True, True)):
    """pullback of (model::GaussianNetwork / SoftGaussianNetwork)(state, action) onto the heads' outputs, one launch: mu, raw_sigma (n, d),
    action (n, K, d) [data: no gradient], dlogp (n, K) -> (dmu, draw_sigma), both (n, d).  The sums over K run in ascending order."""
    n, d = mu.shape
    K = action.shape[1] if action.dim() == 3 else 0
    if raw_sigma.shape != mu.shape or tuple(action.shape) != (n, K, d) or tuple(dlogp.shape) != (n, K):
        raise _lib.RLHipArgumentError(f"gaussian_head_logp_backward: mu {tuple(mu.shape)}, raw_sigma {tuple(raw_sigma.shape)}, "
                                      f"action {tuple(action.shape)}, dlogp {tuple(dlogp.shape)} do not agree")
    dmu, draw = _like(mu, need[0]), _like(raw_sigma, need[1])
    call("rlhip_gaussian_head_logp_bwd_f32", ptr(mu), ptr(raw_sigma), ptr(action), ptr(dlogp), d, n, K, float(min_sigma),
         float(max_sigma), int(squash), int(soft), ptr(dmu), ptr(draw), stream_ptr())
    return dmu, draw


def gaussian_head_sample_backward(mu, raw_sigma, K, min_sigma, max_sigma, squash, soft, seed, env_id_base, step, dact=None, dlogp=None,
                                  need=(True, True)):
    """pullback of the sampling calls, one launch that regenerates the draws of (seed, env_id_base, step): mu, raw_sigma (n, d), dact
    (n, K, d) or None [SoftGaussianNetwork only: a GaussianNetwork's actions carry no gradient], dlogp (n, K) or None
    -> (dmu, draw_sigma), both (n, d)"""
    n, d = mu.shape
    if (raw_sigma.shape != mu.shape or (dact is not None and tuple(dact.shape) != (n, K, d))
            or (dlogp is not None and tuple(dlogp.shape) != (n, K))):
        raise _lib.RLHipArgumentError(f"gaussian_head_sample_backward: mu {tuple(mu.shape)}, raw_sigma {tuple(raw_sigma.shape)}, K = {K}, "
                                      f"dact {None if dact is None else tuple(dact.shape)}, "
                                      f"dlogp {None if dlogp is None else tuple(dlogp.shape)} do not agree")
    dmu, draw = _like(mu, need[0]), _like(raw_sigma, need[1])
    call("rlhip_gaussian_head_sample_bwd_f32", ptr(mu), ptr(raw_sigma), d, n, K, float(min_sigma), float(max_sigma), int(squash),
         int(soft), seed, env_id_base, step, ptr(dact), ptr(dlogp), ptr(dmu), ptr(draw), stream_ptr())
    return dmu, draw


def huber_loss(q, target, delta=1.0, with_grad=True):
    loss = torch.empty(1, dtype=torch.float32, device=q.device)
    dq = torch.empty_like(q) if with_grad else None
    call("rlhip_huber_f32", ptr(q), ptr(target), q.numel(), delta, ptr(loss), ptr(dq), stream_ptr())
    return loss, dq


def td_target(qt_next, reward, terminal, gamma):
    """qt_next: SoA (na, n)."""
    na, n = qt_next.shape
    out = torch.empty(n, dtype=torch.float32, device=qt_next.device)
    call("rlhip_td_target_f32", ptr(qt_next), na, n, n, 1, ptr(reward), ptr(_u8(terminal)), gamma, ptr(out),
         stream_ptr())
    return out


# ----------------------------------------------------------------------------------------- misc
def fill_uniform(n, seed, t, tag, device="cuda"):
    out = torch.empty(n, dtype=torch.float32, device=device)
    call("rlhip_fill_uniform_f32", ptr(out), n, seed, t, tag, stream_ptr())
    return out


def permutation(n, seed, epoch, device="cuda"):
    out = torch.empty(n, dtype=torch.int32, device=device)
    call("rlhip_permutation", ptr(out), n, seed, epoch, stream_ptr())
    return out


def mlp2_nparams(n_in, h, n_out):
    return int(_lib.lib.rlhip_mlp2_nparams(n_in, h, n_out))


def mlp2_init(n_in, h, n_out, seed, net_id, device="cuda"):
    p = torch.empty(mlp2_nparams(n_in, h, n_out), dtype=torch.float32, device=device)
    call("rlhip_mlp2_init_f32", ptr(p), n_in, h, n_out, seed, net_id, stream_ptr())
    return p


def mlp2_forward(params, n_in, h, n_out, act, x):
    """x: SoA (n_in, batch) -> (n_out, batch)."""
    batch = x.shape[1]
    out = torch.empty((n_out, batch), dtype=torch.float32, device=x.device)
    call("rlhip_mlp2_forward_f32", ptr(params), n_in, h, n_out, act, ptr(x), batch, ptr(out), stream_ptr())
    return out


