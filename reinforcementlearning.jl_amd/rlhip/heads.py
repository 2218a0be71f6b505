"""Stochastic Gaussian policy heads (host-side mirror).

Reference: RLCore/src/utils/networks.jl -- `GaussianNetwork(pre, μ, σ; min_σ, max_σ, squash)` :44-116 and
`SoftGaussianNetwork(pre, μ, σ; min_σ, max_σ)` :130-199.  `pre`, `μ`, `σ` are callables on device tensors
(`HipApproximator.forward`, `ops.mlp2_forward`, ...) that return (features, batch) matrices in the reference's
column-major sense, i.e. torch tensors of shape (batch, features) whose memory is (d x n) column-major; the head itself
-- clamp, sampling, squash, log-probability with the tanh correction -- is one launch (csrc/heads.hip).  `rng` is the
shared Philox NORMAL stream: (seed, env_id_base + column, step) with `step` advancing by one per sampling call.

With torch modules as `mu` / `sigma` both heads are trainable: while autograd is recording and a head output requires a gradient, the
log-probabilities of `net(state, action)` and of the sampling calls are pulled back in one launch (rlhip/grad.py, csrc/heads_grad.hip),
with values bit-identical to the plain path.  A GaussianNetwork's sampled actions carry no gradient (`ignore_derivatives` :69, :94); a
SoftGaussianNetwork's actions do (the reparameterisation trick :153-185): the backward launch regenerates the draws from
(seed, env_id_base, step), so no noise tensor is kept.  Given actions are data: one that requires a gradient is refused."""
import torch

from . import ops
from ._lib import call
from .ops import _wants_grad, ptr, stream_ptr


def _cm(x):
    """(d, n) Julia-shaped view -> contiguous (n, d) storage (= d x n column-major)"""
    return x.t().contiguous() if x.dim() == 2 else x.contiguous()


class GaussianNetwork:
    soft = 0

    def __init__(self, pre=None, mu=None, sigma=None, min_sigma=0.0, max_sigma=float("inf"), squash="identity", seed=0,
                 env_id_base=0):
        if squash not in ("identity", "tanh"):
            raise ValueError("squash must be identity or tanh")  # "Other squashing functions are not supported" :36
        self.pre = pre if pre is not None else (lambda x: x)
        self.mu, self.sigma = mu, sigma
        self.min_sigma, self.max_sigma = float(min_sigma), float(max_sigma)
        self.squash = 1 if squash == "tanh" else 0
        self.seed, self.env_id_base, self.step = int(seed), int(env_id_base), 0

    # -- (model)(state): mu, sigma (d, n)
    def heads(self, state):
        x = self.pre(state)
        mu, raw = self.mu(x), self.sigma(x)
        return mu, raw

    def __call__(self, state, action=None, is_sampling=False, is_return_log_prob=False):
        if action is not None:
            return self.logp(state, action)
        mu, raw = self.heads(state)
        if not is_sampling:
            return mu, raw.clamp(self.min_sigma, self.max_sigma)  # :65-67,79
        a, lp = self._sample(mu, raw, 1, is_return_log_prob)
        a = a[:, 0, :].t()  # (d, n)
        return (a, lp.reshape(1, -1)) if is_return_log_prob else a

    def sample(self, state, action_samples):
        """(model)(state::(ns, 1, n), action_samples::Int) -> actions (d, K, n), logp (1, K, n)  :90-100"""
        if state.dim() == 3:
            state = state[:, 0, :]
        mu, raw = self.heads(state)
        a, lp = self._sample(mu, raw, int(action_samples), True)
        return a.permute(2, 1, 0), lp.t().unsqueeze(0)

    def logp(self, state, action):
        """(model)(state, action) -> logp (1, n) or (1, K, n)  :110-116"""
        three = action.dim() == 3
        if state.dim() == 3:
            state = state[:, 0, :]
        mu, raw = self.heads(state)
        d, n = mu.shape
        act = action.permute(2, 1, 0).contiguous() if three else action.t().contiguous().reshape(n, 1, d)
        if _wants_grad(act):
            raise NotImplementedError("the actions given to (model)(state, action) are data here: they get no gradient (detach them)")
        mu_s, raw_s = _cm(mu), _cm(raw)  # keep the transposed copies alive across the (asynchronous) call
        if _wants_grad(mu_s, raw_s):
            from . import grad

            out = grad.GaussianHeadLogp.apply(mu_s, raw_s, act, self.min_sigma, self.max_sigma, self.squash, self.soft)
        else:
            out = gaussian_logp(mu_s, raw_s, act, self.min_sigma, self.max_sigma, self.squash, self.soft)
        return out.t().unsqueeze(0) if three else out.reshape(1, n)

    def _sample(self, mu, raw, K, want_logp):
        """-> actions (n, K, d), logp (n, K) or None: the storages of the reference's arrays"""
        mu_s, raw_s = _cm(mu), _cm(raw)  # keep the transposed copies alive across the (asynchronous) call
        args = (K, self.min_sigma, self.max_sigma, self.squash, self.soft, self.seed, self.env_id_base, self.step, want_logp)
        if (want_logp or self.soft) and _wants_grad(mu_s, raw_s):  # a GaussianNetwork's actions alone carry no gradient
            from . import grad

            act, lp = grad.GaussianHeadSample.apply(mu_s, raw_s, *args)
        else:
            act, lp = gaussian_sample(mu_s, raw_s, *args)
        self.step += 1
        return act, lp


class SoftGaussianNetwork(GaussianNetwork):
    """SoftGaussianNetwork: tanh-squashed actions, logp = sum(normlogpdf - 2 (log 2 - z - softplus(-2 z)))  :147-198"""
    soft = 1

    def __init__(self, pre=None, mu=None, sigma=None, min_sigma=0.0, max_sigma=float("inf"), seed=0, env_id_base=0):
        super().__init__(pre, mu, sigma, min_sigma, max_sigma, "tanh", seed, env_id_base)


class CovGaussianNetwork:
    """CovGaussianNetwork(pre, μ, Σ)  RLCore/src/utils/networks.jl:221-381: a Gaussian policy with a full covariance matrix.

    `mu` maps the features to the means (da, n) and `Sigma` to the Cholesky vectors (da (da + 1) / 2, n); `vec_to_tril`, the draw
    `z = μ + L ε` and `mvnormlogpdf(μ, L, z)` are one launch (csrc/cov_heads.hip).  Call forms, in the reference's shapes:
      net(state)                  state (ns, n) -> μ (da, n), L (da, da, n);  state (ns, 1, n) -> μ (da, 1, n), L (da, da, n)   :247-289
      net(state, is_sampling=True[, is_return_log_prob=True])   actions (da, n) [(da, 1, n)] and logp (1, n) [(1, 1, n)]
      net.sample(state, K)        actions (da, K, n), logp (1, K, n)                                                           :300-312
      net(state, action)          action (da, n) -> (1, n);  action (da, K, n) -> (1, K, n)                                    :327-343
    `step` advances by one per sampling call.

    With torch modules as `mu` / `Sigma` the head is trainable: while autograd is recording and a head output requires a gradient, the
    log-probabilities of `net(state, action)` and of the sampling calls are pulled back in one launch (rlhip/grad.py,
    csrc/cov_heads_grad.hip), `net(state)`'s L through `vec_to_tril`'s pullback; the values are bit-identical to the plain path and
    the sampled actions carry no gradient, as in the reference (`ignore_derivatives`)."""

    def __init__(self, pre=None, mu=None, Sigma=None, seed=0, env_id_base=0):
        self.pre = pre if pre is not None else (lambda x: x)
        self.mu, self.Sigma = mu, Sigma
        self.seed, self.env_id_base, self.step = int(seed), int(env_id_base), 0

    def heads(self, state):
        """-> μ (da, n), cholesky_vec (nv, n); a 3-D state (ns, 1, n) is the 2-D one with a unit middle axis (:280)"""
        if state.dim() == 3:
            state = state[:, 0, :]
        x = self.pre(state)
        mu, vec = self.mu(x), self.Sigma(x)
        da = mu.shape[0]
        if mu.dim() != 2 or vec.dim() != 2 or vec.shape[0] != da * (da + 1) // 2 or vec.shape[1] != mu.shape[1]:
            raise ValueError(f"CovGaussianNetwork: μ {tuple(mu.shape)} needs a Σ head of shape ({da * (da + 1) // 2}, {mu.shape[1]}), "
                             f"got {tuple(vec.shape)}")
        return mu, vec

    def __call__(self, state, action=None, is_sampling=False, is_return_log_prob=False):
        if action is not None:
            return self.logp(state, action)
        three = state.dim() == 3
        mu, vec = self.heads(state)
        if not is_sampling:
            da, n = mu.shape
            L = ops.vec_to_tril(_cm(vec), da)
            return (mu.unsqueeze(1) if three else mu), L.permute(2, 1, 0)  # :270, :285
        a, lp = self._sample(mu, vec, 1, is_return_log_prob)
        a = a.permute(2, 1, 0) if three else a[:, 0, :].t()
        if not is_return_log_prob:
            return a
        return a, (lp.t().unsqueeze(0) if three else lp.reshape(1, -1))

    def sample(self, state, action_samples):
        """(model)(state::(ns, 1, n), action_samples::Int) -> actions (da, K, n), logp (1, K, n)  :300-312"""
        mu, vec = self.heads(state)
        a, lp = self._sample(mu, vec, int(action_samples), True)
        return a.permute(2, 1, 0), lp.t().unsqueeze(0)

    def logp(self, state, action):
        """(model)(state, action) -> logp (1, n) or (1, K, n)  :327-343"""
        three = action.dim() == 3
        mu, vec = self.heads(state)
        da, n = mu.shape
        if action.shape[0] != da or action.shape[-1] != n:
            raise ValueError(f"CovGaussianNetwork: actions {tuple(action.shape)} for μ {tuple(mu.shape)}")
        act = action.permute(2, 1, 0).contiguous() if three else action.t().contiguous().reshape(n, 1, da)
        mu_s, vec_s = _cm(mu), _cm(vec)  # keep the transposed copies alive across the (asynchronous) call
        if _wants_grad(act):  # a gradient for the actions too: the composition, byte for byte the fused call
            out = ops.mvnormlogpdf(mu_s, ops.vec_to_tril(vec_s, da), act)
        elif _wants_grad(mu_s, vec_s):
            from . import grad

            out = grad.CovHeadLogp.apply(mu_s, vec_s, act)
        else:
            out = cov_logp(mu_s, vec_s, act)
        return out.t().unsqueeze(0) if three else out.reshape(1, n)

    def _sample(self, mu, vec, K, want_logp, want_L=False):
        """-> actions (n, K, da), logp (n, K) or None[, L (n, da, da)]: the storages of the reference's arrays"""
        mu_s, vec_s = _cm(mu), _cm(vec)  # keep the transposed copies alive across the (asynchronous) call
        if want_logp and not want_L and _wants_grad(mu_s, vec_s):
            from . import grad

            act, lp = grad.CovHeadSample.apply(mu_s, vec_s, K, self.seed, self.env_id_base, self.step)
            L = None
        else:
            act, lp, L = cov_sample(mu_s, vec_s, K, self.seed, self.env_id_base, self.step, want_logp, want_L)
        self.step += 1
        return (act, lp, L) if want_L else (act, lp)


def gaussian_logp(mu_s, raw_s, act, min_sigma, max_sigma, squash, soft):
    """the (state, action) launch on storages: mu_s, raw_s (n, d), act (n, K, d) -> logp (n, K); no autograd"""
    n, d = mu_s.shape
    K = act.shape[1]
    out = torch.empty((n, K), dtype=torch.float32, device=mu_s.device)
    call("rlhip_gaussian_head_logp_f32", ptr(mu_s), ptr(raw_s), ptr(act), d, n, K, min_sigma, max_sigma, squash, soft, ptr(out),
         stream_ptr())
    return out


def gaussian_sample(mu_s, raw_s, K, min_sigma, max_sigma, squash, soft, seed, env_id_base, step, want_logp):
    """the sampling launch on storages -> actions (n, K, d), logp (n, K) or None; no autograd"""
    n, d = mu_s.shape
    act = torch.empty((n, K, d), dtype=torch.float32, device=mu_s.device)
    lp = torch.empty((n, K), dtype=torch.float32, device=mu_s.device) if want_logp else None
    call("rlhip_gaussian_head_sample_f32", ptr(mu_s), ptr(raw_s), d, n, K, min_sigma, max_sigma, squash, soft, seed, env_id_base, step,
         ptr(act), ptr(lp), stream_ptr())
    return act, lp


def cov_logp(mu_s, vec_s, act):
    """the (state, action) launch on storages: mu_s (n, da), vec_s (n, nv), act (n, K, da) -> logp (n, K); no autograd"""
    n, da = mu_s.shape
    K = act.shape[1]
    out = torch.empty((n, K), dtype=torch.float32, device=mu_s.device)
    call("rlhip_cov_gaussian_head_logp_f32", ptr(mu_s), ptr(vec_s), ptr(act), da, n, K, ptr(out), None, stream_ptr())
    return out


def cov_sample(mu_s, vec_s, K, seed, env_id_base, step, want_logp, want_L):
    """the sampling launch on storages -> actions (n, K, da), logp (n, K) or None, L (n, da, da) or None; no autograd"""
    n, da = mu_s.shape
    act = torch.empty((n, K, da), dtype=torch.float32, device=mu_s.device)
    lp = torch.empty((n, K), dtype=torch.float32, device=mu_s.device) if want_logp else None
    L = torch.empty((n, da, da), dtype=torch.float32, device=mu_s.device) if want_L else None
    call("rlhip_cov_gaussian_head_sample_f32", ptr(mu_s), ptr(vec_s), da, n, K, seed, env_id_base, step, ptr(act), ptr(lp), ptr(L),
         stream_ptr())
    return act, lp, L


class CategoricalNetwork:
    """CategoricalNetwork(model) RLCore/src/utils/networks.jl:405-432 (+ masked methods :459-472).

    `model` maps a state batch to logits shaped (na, n).  `(net)(state; is_sampling, is_return_log_prob)` returns the
    logits, or a one-hot `z` (na, n) drawn with the Gumbel-max trick (`sample_categorical` :425-432, one launch:
    rlhip_categorical_sample_f32 on the GUMBEL Philox stream), or `(z, logits)`; with a Bool `mask` (na, n) the masked
    logits are `logits + ifelse(mask, 0, typemin)` (:461) and masked actions are never drawn.  `actions` holds the
    0-based indices of the last draw (what the env kernels take)."""

    def __init__(self, model, seed=0, env_id_base=0):
        self.model, self.seed, self.env_id_base, self.step = model, int(seed), int(env_id_base), 0
        self.actions = None

    def __call__(self, state, mask=None, is_sampling=False, is_return_log_prob=False):
        from ._lib import call
        from .ops import _u8, ptr, stream_ptr

        lg = self.model(state).contiguous()
        na, n = lg.shape
        m8 = _u8(mask)
        logits = torch.empty_like(lg) if mask is not None else lg
        z = torch.empty_like(lg) if is_sampling else None
        if is_sampling:
            self.actions = torch.empty(n, dtype=torch.int32, device=lg.device)
        if mask is not None or is_sampling:  # masked logits, Gumbel-max draw and one-hot in ONE launch behind the ABI
            call("rlhip_categorical_network_f32", ptr(lg), na, n, ptr(m8), self.seed, self.env_id_base, self.step,
                 ptr(logits) if mask is not None else None, ptr(self.actions) if is_sampling else None, ptr(z),
                 stream_ptr())
        if not is_sampling:
            return logits
        self.step += 1
        return (z, logits) if is_return_log_prob else z
