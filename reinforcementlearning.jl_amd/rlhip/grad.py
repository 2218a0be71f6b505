"""torch.autograd.Function classes over the forward entry points of csrc/cov_heads.hip and their pullbacks (csrc/cov_heads_grad.hip).

The reference writes mvnormlogpdf, vec_to_tril and the Gaussian KL divergences to be differentiated (Zygote pulls back through them:
RLCore/src/utils/distributions.jl, networks.jl:359-381); here `ops.mvnormlogpdf`, `ops.vec_to_tril`, the three KLs and
`CovGaussianNetwork`'s log-probabilities route through these classes whenever autograd is recording and an input requires a gradient
(`ops._wants_grad`).  The forward of every class IS the plain call -- a Function's forward runs with grad mode off, so the wrapper it
calls takes its ordinary path -- which makes the values bit-identical either way.  Each backward is one launch; outputs nobody
asked for (`ctx.needs_input_grad`) are passed as NULL and skipped by the kernel.  Tensors are the column-major storages `ops` documents.
Sampled actions carry no gradient (the reference draws them under `ignore_derivatives`): the sampling log-probability is pulled
back as (model)(state, action) at the sampled action.

The diagonal heads (csrc/heads.hip, pullbacks in csrc/heads_grad.hip) and `ops.normlogpdf` / `ops.diagnormlogpdf` follow the same pattern.
`GaussianHeadSample` keeps only mu and raw_sigma: its backward launch regenerates the draws from (seed, env_id_base, step).  A
GaussianNetwork's actions carry no gradient; a SoftGaussianNetwork's actions do (the reparameterisation trick), and a cotangent that
autograd does not supply reaches the kernel as NULL."""
import torch

from . import ops


def _c(g):
    """an incoming cotangent as contiguous Float32 (autograd hands over expanded views, e.g. from sum())"""
    return g.contiguous()


class VecToTril(torch.autograd.Function):
    @staticmethod
    def forward(ctx, chol_vec, da):
        ctx.save_for_backward(chol_vec)
        ctx.da = da
        return ops.vec_to_tril(chol_vec, da)

    @staticmethod
    def backward(ctx, dL):
        (chol_vec,) = ctx.saved_tensors
        return ops.vec_to_tril_backward(chol_vec, _c(dL), ctx.da), None


class MvNormLogPdf(torch.autograd.Function):
    @staticmethod
    def forward(ctx, mu, L, x):
        ctx.save_for_backward(mu, L, x)
        return ops.mvnormlogpdf(mu, L, x)

    @staticmethod
    def backward(ctx, dlogp):
        return ops.mvnormlogpdf_backward(*ctx.saved_tensors, _c(dlogp), need=ctx.needs_input_grad)


class CovHeadLogp(torch.autograd.Function):
    """(model::CovGaussianNetwork)(state, action) on the heads' outputs: mu (n, da), chol_vec (n, nv), action (n, K, da) -> (n, K)"""

    @staticmethod
    def forward(ctx, mu, chol_vec, action):
        from . import heads

        ctx.save_for_backward(mu, chol_vec, action)
        return heads.cov_logp(mu, chol_vec, action)

    @staticmethod
    def backward(ctx, dlogp):
        dmu, dvec = ops.cov_gaussian_head_logp_backward(*ctx.saved_tensors, _c(dlogp), need=ctx.needs_input_grad[:2])
        return dmu, dvec, None


class CovHeadSample(torch.autograd.Function):
    """the sampling calls: -> actions (n, K, da) [no gradient], logp (n, K) [pulled back at the sampled actions]"""

    @staticmethod
    def forward(ctx, mu, chol_vec, K, seed, env_id_base, step):
        from . import heads

        act, lp, _ = heads.cov_sample(mu, chol_vec, K, seed, env_id_base, step, True, False)
        ctx.save_for_backward(mu, chol_vec, act)
        ctx.mark_non_differentiable(act)
        return act, lp

    @staticmethod
    def backward(ctx, _dact, dlogp):
        dmu, dvec = ops.cov_gaussian_head_logp_backward(*ctx.saved_tensors, _c(dlogp), need=ctx.needs_input_grad[:2])
        return dmu, dvec, None, None, None, None


class NormLogPdf(torch.autograd.Function):
    @staticmethod
    def forward(ctx, mu, sigma, x):
        ctx.save_for_backward(mu, sigma, x)
        return ops.normlogpdf(mu, sigma, x)

    @staticmethod
    def backward(ctx, dout):
        return ops.normlogpdf_backward(*ctx.saved_tensors, _c(dout), need=ctx.needs_input_grad)


class DiagNormLogPdf(torch.autograd.Function):
    @staticmethod
    def forward(ctx, mu, sigma, x):
        ctx.save_for_backward(mu, sigma, x)
        return ops.diagnormlogpdf(mu, sigma, x)

    @staticmethod
    def backward(ctx, dout):
        return ops.diagnormlogpdf_backward(*ctx.saved_tensors, _c(dout), need=ctx.needs_input_grad)


class GaussianHeadLogp(torch.autograd.Function):
    """(model::GaussianNetwork / SoftGaussianNetwork)(state, action) on the heads' outputs: mu, raw_sigma (n, d), action (n, K, d) [data]
    -> (n, K)"""

    @staticmethod
    def forward(ctx, mu, raw_sigma, action, min_sigma, max_sigma, squash, soft):
        from . import heads

        ctx.save_for_backward(mu, raw_sigma, action)
        ctx.head = (min_sigma, max_sigma, squash, soft)
        return heads.gaussian_logp(mu, raw_sigma, action, min_sigma, max_sigma, squash, soft)

    @staticmethod
    def backward(ctx, dlogp):
        dmu, draw = ops.gaussian_head_logp_backward(*ctx.saved_tensors, _c(dlogp), *ctx.head, need=ctx.needs_input_grad[:2])
        return dmu, draw, None, None, None, None, None


class GaussianHeadSample(torch.autograd.Function):
    """the sampling calls: -> actions (n, K, d), logp (n, K) or None.  Only mu and raw_sigma are saved: the backward launch regenerates the
    draws from (seed, env_id_base, step).  soft = 0: the actions carry no gradient; soft = 1: both outputs do, and a cotangent nobody
    supplied is handed over as NULL (its terms are skipped), not as zeros."""

    @staticmethod
    def forward(ctx, mu, raw_sigma, K, min_sigma, max_sigma, squash, soft, seed, env_id_base, step, want_logp):
        from . import heads

        ctx.save_for_backward(mu, raw_sigma)
        ctx.head = (K, min_sigma, max_sigma, squash, soft, seed, env_id_base, step)
        ctx.set_materialize_grads(False)
        act, lp = heads.gaussian_sample(mu, raw_sigma, K, min_sigma, max_sigma, squash, soft, seed, env_id_base, step, want_logp)
        if not soft:
            ctx.mark_non_differentiable(act)
        return act, lp

    @staticmethod
    def backward(ctx, dact, dlogp):
        soft = ctx.head[4]
        if not soft:
            dact = None
        if dlogp is None and dact is None:
            return (None,) * 11
        dmu, draw = ops.gaussian_head_sample_backward(*ctx.saved_tensors, *ctx.head, dact=None if dact is None else _c(dact),
                                                      dlogp=None if dlogp is None else _c(dlogp), need=ctx.needs_input_grad[:2])
        return (dmu, draw) + (None,) * 9


class MvNormKL(torch.autograd.Function):
    @staticmethod
    def forward(ctx, mu1, L1, mu2, L2):
        ctx.save_for_backward(mu1, L1, mu2, L2)
        return ops.mvnormkldivergence(mu1, L1, mu2, L2)

    @staticmethod
    def backward(ctx, dout):
        return ops.mvnormkldivergence_backward(*ctx.saved_tensors, _c(dout), need=ctx.needs_input_grad)


class DiagNormKL(torch.autograd.Function):
    @staticmethod
    def forward(ctx, mu1, sigma1, mu2, sigma2):
        ctx.save_for_backward(mu1, sigma1, mu2, sigma2)
        return ops.diagnormkldivergence(mu1, sigma1, mu2, sigma2)

    @staticmethod
    def backward(ctx, dout):
        return ops.diagnormkldivergence_backward(*ctx.saved_tensors, _c(dout), need=ctx.needs_input_grad)


class NormKL(torch.autograd.Function):
    @staticmethod
    def forward(ctx, mu1, sigma1, mu2, sigma2):
        ctx.save_for_backward(mu1, sigma1, mu2, sigma2)
        return ops.normkldivergence(mu1, sigma1, mu2, sigma2)

    @staticmethod
    def backward(ctx, dout):
        return ops.normkldivergence_backward(*ctx.saved_tensors, _c(dout), need=ctx.needs_input_grad)
