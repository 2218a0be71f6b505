"""FQFLearner -- the fully parameterised quantile function (FQF) distributional DQN learner under the unchanged QBasedPolicy.

The member of the distributional family that stops choosing quantile levels by hand (QR-DQN) or at random (IQN): a small
fraction-proposal network on the state embedding, q = softmax(Wf psi(s) + bf), places them -- tau the cumulative sum of q, tau_hat the
midpoints -- and the quantile network is IQN's ImplicitQuantileNet evaluated at tau_hat (Yang et al. 2019).  Q is the d-weighted sum of
the quantiles, d[i] = tau[i + 1] - tau[i].  The quantile network trains on the quantile-Huber loss at the placed levels, the fraction
network on the paper's gradient 2 F^-1(tau_i) - F^-1(tau_hat_i) - F^-1(tau_hat_{i-1}) (minus ent_coef times the entropy's).
include/rlhip.h states the update (csrc/fqf.hip implements it, tests/fqf_ref.py states the mathematics in Float64).

Out of scope, refused by name: NoisyDense, dueling heads, three-layer and bf16 networks, sharded runs (world > 1), a fused vec-step,
UInt8 frames, kappa = 0.
"""
import math

import torch

from . import _lib
from ._lib import call
from .c51 import DistributionalLearner, _opt
from .dqn import refuse_noisy
from .iqn import IQNApproximator
from .ops import clip_adam_, ptr, stream_ptr

ENVELOPE = "obs_dim 2..16, hidden a multiple of 32 and <= 256, 1..4 actions, n_cos even and 2..64, 2..32 fractions"


# ----------------------------------------------------------------------------- functional layer
def fqf_frac_nparams(h, N):
    return int(_lib.lib.rlhip_fqf_frac_nparams(h, N))


def fqf_workspace(ns, h, na, n_cos, N, batch, device="cuda"):
    nbytes = int(_lib.lib.rlhip_fqf_workspace_bytes(ns, h, na, n_cos, N, batch))
    if nbytes < 0:
        raise ValueError(f"the FQF kernels take {ENVELOPE}, batch >= 1; got obs_dim = {ns}, hidden = {h}, actions = {na}, n_cos = {n_cos}, "
                         f"N = {N}, batch = {batch}")
    return torch.empty(nbytes, dtype=torch.uint8, device=device)


def fqf_forward(params, frac_params, ns, h, na, n_cos, N, act, obs, q_out=None, quantiles=None, tau=None, tau_hat=None):
    """obs (ns, n) -> Q (na, n), the d-weighted sum of the quantiles at the placed levels; `quantiles` ((N * na), n), `tau` (N + 1, n) and
    `tau_hat` (N, n) are written where given"""
    n = obs.shape[1]
    q_out = q_out if q_out is not None else torch.empty((na, n), dtype=torch.float32, device=obs.device)
    call("rlhip_fqf_forward_f32", ptr(params), ptr(frac_params), ns, h, na, n_cos, N, act, ptr(obs), n, ptr(q_out), _opt(quantiles), _opt(tau),
         _opt(tau_hat), stream_ptr())
    return q_out


def fqf_plan(params, frac_params, ns, h, na, n_cos, N, act, obs, eps, seed, env_id_base, step, actions=None, q_out=None):
    """plan! in one launch: byte for byte `fqf_forward` then `eps_greedy_select` -> (0-based actions, q (na, n))"""
    n = obs.shape[1]
    actions = actions if actions is not None else torch.empty(n, dtype=torch.int32, device=obs.device)
    q_out = q_out if q_out is not None else torch.empty((na, n), dtype=torch.float32, device=obs.device)
    call("rlhip_fqf_plan_f32", ptr(params), ptr(frac_params), ns, h, na, n_cos, N, act, ptr(obs), n, float(eps), seed, env_id_base, step,
         ptr(actions), ptr(q_out), stream_ptr())
    return actions, q_out


def fqf_grad_batch(ns, h, na, n_cos, N, act, kappa, ent_coef, params, target_params, frac_params, s, a, r, term, s_next, gamma, n_used=None,
                   weights=None, double_dqn=False, workspace=None, grad=None, frac_grad=None, loss=None, ql=None, target=None, sel=None,
                   tau=None, tau_hat=None, ent=None):
    """loss and gradients on a gathered batch (s / s_next (ns, batch)) at the levels the online fraction net places on s
    -> (grad, frac_grad, loss).  ql (batch,): the unweighted per-sample quantile-Huber loss; target (N, batch): T_j; sel (batch,) int32:
    a*; tau (N + 1, batch) / tau_hat (N, batch): the placed levels; ent (batch,): the entropy of the fractions."""
    dev, b = params.device, a.numel()
    workspace = workspace if workspace is not None else fqf_workspace(ns, h, na, n_cos, N, b, dev)
    grad = grad if grad is not None else torch.empty_like(params)
    frac_grad = frac_grad if frac_grad is not None else torch.empty_like(frac_params)
    loss = loss if loss is not None else torch.empty(1, dtype=torch.float32, device=dev)
    if term.dtype == torch.bool:
        term = term.view(torch.uint8)
    call("rlhip_fqf_grad_batch_f32", ns, h, na, n_cos, N, act, kappa, ent_coef, ptr(params), ptr(target_params), ptr(frac_params), ptr(s),
         ptr(a), ptr(r), ptr(term), ptr(s_next), b, gamma, _opt(n_used), _opt(weights), int(bool(double_dqn)), ptr(workspace), ptr(grad),
         ptr(frac_grad), ptr(loss), _opt(ql), _opt(target), _opt(sel), _opt(tau), _opt(tau_hat), _opt(ent), stream_ptr())
    return grad, frac_grad, loss


# ---------------------------------------------------------------------------------- approximator
class FQFApproximator(IQNApproximator):
    """An IQNApproximator (the quantile network: `.params` + Adam state, the vector TargetNetwork copies) plus the fraction-proposal
    network Dense(h, n_fractions): `.frac_params` = [Wf | bf] with an Adam state and learning rate of its own (the paper trains it with
    a much smaller one).  `optimise_(grad)` steps the quantile vector on `grad` and the fraction vector on `.frac_grad`, which the
    learner's gradient launch has written; each vector is clipped by its own global norm."""

    def __init__(self, n_in, hidden, n_actions, n_fractions=32, n_cos=64, act="relu", lr=1e-3, frac_lr=2.5e-6, beta1=0.9, beta2=0.999,
                 eps=1e-8, seed=0, net_id=0, device="cuda", params=None, frac_params=None):
        super().__init__(n_in, hidden, n_actions, n_cos, act, lr, beta1, beta2, eps, seed, net_id, device, params)
        nf = fqf_frac_nparams(hidden, int(n_fractions))
        if nf < 0:
            raise ValueError(f"FQFApproximator: the FQF kernels take {ENVELOPE}")
        if frac_params is None:
            frac_params = torch.empty(nf, dtype=torch.float32, device=device)
            call("rlhip_fqf_frac_init_f32", ptr(frac_params), hidden, int(n_fractions), seed, net_id, stream_ptr())
        else:
            frac_params = torch.as_tensor(frac_params, dtype=torch.float32, device=device).clone()
            if frac_params.numel() != nf:
                raise ValueError(f"FQFApproximator: frac_params has {frac_params.numel()} elements, the fraction network {nf}")
        self.n_fractions, self.frac_lr = int(n_fractions), frac_lr
        self.frac_params = frac_params
        self.frac_grad = torch.zeros_like(frac_params)
        self.frac_m, self.frac_v = torch.zeros_like(frac_params), torch.zeros_like(frac_params)
        self.frac_beta_pow = torch.tensor([beta1, beta2], dtype=torch.float32, device=device)
        self.frac_gn = torch.zeros(1, dtype=torch.float32, device=device)

    def optimise_(self, grad, clip_norm=0.0, grad_scale=1.0):
        super().optimise_(grad, clip_norm, grad_scale)
        clip_adam_(self.frac_params, self.frac_grad, self.frac_m, self.frac_v, self.frac_beta_pow, grad_scale, clip_norm, self.frac_lr,
                   self.beta1, self.beta2, self.eps, self.frac_gn)


# --------------------------------------------------------------------------------------- learner
class FQFLearner(DistributionalLearner):
    """FQFLearner(approximator = TargetNetwork(FQFApproximator(ns, h, n_actions, n_fractions, n_cos)), n_actions, n_fractions = 32,
    n_cos = 64, kappa = 1.0, ent_coef = 0.0, ...).  The gate, the counters and the tail of an update are DQNLearner's; every update is the
    batch form

        draw -> gather -> rlhip_fqf_grad_batch_f32 -> [priority write-back] -> clip + Adam on both vectors -> target sync

    on record rings (ns 2..4) and frame rings (ns 5..16), uniform or prioritized, 1-step or n-step, plain or Double DQN.  The levels of a
    sample are those the online fraction net places on s, used for s and s'; nothing is drawn.  The target network is the quantile
    vector's.  The written-back priority is (ql + per_eps)^per_alpha of the UNWEIGHTED per-sample loss."""

    def __init__(self, approximator, n_actions, n_fractions=32, n_cos=64, kappa=1.0, ent_coef=0.0, batchsize=32, gamma=0.99,
                 min_replay_history=100, update_freq=1, max_grad_norm=0.0, seed=0, process_group=None, per_eps=1e-6, per_alpha=0.6,
                 per_beta=0.0, n_step=1, double_dqn=False):
        n_actions, N = int(n_actions), int(n_fractions)
        net = getattr(approximator, "network", None)
        refuse_noisy(net, "FQFLearner")
        if getattr(net, "frac_params", None) is None or getattr(net, "n_cos", None) is None:
            raise TypeError("FQFLearner: the approximator is a TargetNetwork(FQFApproximator(ns, h, n_actions, n_fractions, n_cos)); "
                            "NoisyDense, dueling, three-layer and bf16 networks are out of scope")
        net = self._check_approximator_(approximator, process_group, n_actions, 1, "1", "n_actions")
        if (net.n_fractions, net.n_cos) != (N, int(n_cos)):
            raise ValueError(f"FQFLearner: the network has n_fractions = {net.n_fractions}, n_cos = {net.n_cos}; the learner "
                             f"n_fractions = {N}, n_cos = {n_cos}")
        if not (math.isfinite(float(kappa)) and float(kappa) > 0.0):
            raise ValueError(f"FQFLearner: kappa must be finite and > 0 (kappa = 0, the pure quantile loss, is out of scope), got {kappa}")
        if not (math.isfinite(float(ent_coef)) and float(ent_coef) >= 0.0):
            raise ValueError(f"FQFLearner: ent_coef must be finite and >= 0, got {ent_coef}")
        if int(update_freq) < 1 or int(batchsize) < 1:
            raise ValueError("update_freq and batchsize must be >= 1")
        # (raises for a shape outside the kernels' envelope, before any C call that launches)
        self.workspace = fqf_workspace(net.n_in, net.hidden, n_actions, net.n_cos, N, int(batchsize), net.params.device)
        self.n_actions, self.N, self.kappa, self.ent_coef = n_actions, N, float(kappa), float(ent_coef)
        self._init_update_state_(approximator, batchsize, gamma, min_replay_history, update_freq, max_grad_norm, seed, process_group,
                                 per_eps, per_alpha, per_beta, n_step, double_dqn)
        # the per-sample quantile-Huber loss, then its priority
        self.ql = torch.zeros(self.batchsize, dtype=torch.float32, device=net.params.device)

    # ------------------------------------------------------------------------------------ plan!
    def _net_args(self):
        net = self.approximator.network
        return net.params, net.frac_params, net.n_in, net.hidden, self.n_actions, net.n_cos, self.N, net.act

    def forward(self, x):
        """forward(learner, s) -> Q (na, n)"""
        return fqf_forward(*self._net_args(), x)

    def quantiles(self, x):
        """-> (Q (na, n), the quantiles th (N, na, n) at tau_hat, tau (N + 1, n), tau_hat (N, n))"""
        n = x.shape[1]
        th = torch.empty((self.n_actions * self.N, n), dtype=torch.float32, device=x.device)
        tau = torch.empty((self.N + 1, n), dtype=torch.float32, device=x.device)
        that = torch.empty((self.N, n), dtype=torch.float32, device=x.device)
        q = fqf_forward(*self._net_args(), x, quantiles=th, tau=tau, tau_hat=that)
        return q, th.view(self.n_actions, self.N, -1).permute(1, 0, 2), tau, that

    def plan_distributional_(self, obs, eps, seed, env_id_base, step, actions=None, q_out=None):
        """QBasedPolicy's plan! for this learner: fractions, quantiles, their weighted sum and the eps-greedy choice in one launch"""
        if q_out is not None and q_out.shape[0] != self.n_actions:
            q_out = None
        return fqf_plan(*self._net_args(), obs, eps, seed, env_id_base, step, actions, q_out)

    # -------------------------------------------------------------------------------- optimise!
    def _grad_launch_(self, batch, gamma, weights):
        s, a, r, t, sn, n_used = batch
        tn = self.approximator
        net = tn.network
        ws = self.workspace if a.numel() == self.batchsize else None
        fqf_grad_batch(net.n_in, net.hidden, self.n_actions, net.n_cos, self.N, net.act, self.kappa, self.ent_coef, net.params, tn.target,
                       net.frac_params, s, a, r, t, sn, gamma, n_used, weights, self.double_dqn, ws, self.grad, net.frac_grad, self.loss,
                       self.ql)
        return self.ql
