"""IQNLearner -- the implicit-quantile (IQN) distributional DQN learner under the unchanged QBasedPolicy.

The second distributional member of the QBasedPolicy family the reference's design blog names (C51 and IQN).  The quantile level is an
INPUT of the network: ImplicitQuantileNet(psi = Dense(ns, h, act), phi = Dense(n_cos, h, relu), header = Dense(h, na)) maps a state and
a drawn level tau to one quantile per action, th = header(psi(s) .* phi(cos.(pi (1:n_cos) tau))); the loss is the quantile-Huber loss
between N online and N' target levels (Dabney et al. 2018).  The Zoo's IQNLearner is not in the reference snapshot, so include/rlhip.h
states the update (csrc/iqn.hip implements it, tests/iqn_ref.py states the mathematics in Float64).

FQF (levels placed by a fraction-proposal network) is FQFLearner, rlhip/fqf.py.
Out of scope, refused by name: kappa = 0, NoisyDense, a fused vec-step, three-layer and bf16 networks, dueling distributional
heads, sharded runs (world > 1), UInt8 frames.
"""
import math

import torch

from . import _lib
from ._lib import call
from .c51 import DistributionalLearner, _opt
from .dqn import HipApproximator, refuse_noisy
from .ops import ptr, stream_ptr

ENVELOPE = "obs_dim 2..16, hidden a multiple of 32 and <= 256, 1..4 actions, n_cos even and 2..64, 1..64 levels"


# ----------------------------------------------------------------------------- functional layer
def iqn_nparams(ns, h, na, n_cos):
    return int(_lib.lib.rlhip_iqn_nparams(ns, h, na, n_cos))


def iqn_workspace(ns, h, na, n_cos, N, N_target, batch, device="cuda"):
    nbytes = int(_lib.lib.rlhip_iqn_workspace_bytes(ns, h, na, n_cos, N, N_target, batch))
    if nbytes < 0:
        raise ValueError(f"the IQN kernels take {ENVELOPE}, batch >= 1; got obs_dim = {ns}, hidden = {h}, actions = {na}, n_cos = {n_cos}, "
                         f"N = {N}, N_target = {N_target}, batch = {batch}")
    return torch.empty(nbytes, dtype=torch.uint8, device=device)


def iqn_forward(params, ns, h, na, n_cos, K, act, obs, seed, env_id_base, step, q_out=None, quantiles=None, tau=None):
    """obs (ns, n) at K levels drawn under (seed, env_id_base + env, step) -> Q (na, n), the mean over the levels; `quantiles`
    ((K * na), n) and `tau` (K, n) are written where given"""
    n = obs.shape[1]
    q_out = q_out if q_out is not None else torch.empty((na, n), dtype=torch.float32, device=obs.device)
    call("rlhip_iqn_forward_f32", ptr(params), ns, h, na, n_cos, K, act, ptr(obs), n, seed, env_id_base, step, ptr(q_out), _opt(quantiles),
         _opt(tau), stream_ptr())
    return q_out


def iqn_plan(params, ns, h, na, n_cos, K, act, obs, eps, seed, env_id_base, step, actions=None, q_out=None, tau=None):
    """plan! in one launch: byte for byte `iqn_forward` then `eps_greedy_select` -> (0-based actions, q (na, n))"""
    n = obs.shape[1]
    actions = actions if actions is not None else torch.empty(n, dtype=torch.int32, device=obs.device)
    q_out = q_out if q_out is not None else torch.empty((na, n), dtype=torch.float32, device=obs.device)
    call("rlhip_iqn_plan_f32", ptr(params), ns, h, na, n_cos, K, act, ptr(obs), n, float(eps), seed, env_id_base, step, ptr(actions),
         ptr(q_out), _opt(tau), stream_ptr())
    return actions, q_out


def iqn_grad_batch(ns, h, na, n_cos, N, N_target, act, kappa, params, target_params, s, a, r, term, s_next, gamma, seed, draw_ctr,
                   n_used=None, weights=None, double_dqn=False, workspace=None, grad=None, loss=None, ql=None, target=None, sel=None,
                   tau=None, tau_target=None):
    """loss and gradient of the quantile-Huber loss between N online and N_target target levels, drawn under (seed, batch position,
    draw_ctr), on a gathered batch (s / s_next (ns, batch)) -> (grad, loss).  ql (batch,): the unweighted per-sample loss; target
    (N_target, batch): T_j; sel (batch,) int32: a*; tau (N, batch) / tau_target (N_target, batch): the drawn levels."""
    dev, b = params.device, a.numel()
    workspace = workspace if workspace is not None else iqn_workspace(ns, h, na, n_cos, N, N_target, b, dev)
    grad = grad if grad is not None else torch.empty_like(params)
    loss = loss if loss is not None else torch.empty(1, dtype=torch.float32, device=dev)
    if term.dtype == torch.bool:
        term = term.view(torch.uint8)
    call("rlhip_iqn_grad_batch_f32", ns, h, na, n_cos, N, N_target, act, kappa, ptr(params), ptr(target_params), ptr(s), ptr(a), ptr(r),
         ptr(term), ptr(s_next), b, gamma, _opt(n_used), _opt(weights), int(bool(double_dqn)), seed, draw_ctr, ptr(workspace), ptr(grad),
         ptr(loss), _opt(ql), _opt(target), _opt(sel), _opt(tau), _opt(tau_target), stream_ptr())
    return grad, loss


# ---------------------------------------------------------------------------------- approximator
class IQNApproximator(HipApproximator):
    """FluxApproximator(model = ImplicitQuantileNet(psi = Dense(ns, h, act), phi = Dense(n_cos, h, relu), header = Dense(h, n_actions)),
    optimiser = Adam(lr)): flat parameters [W1 | b1 | Wphi | bphi | W2 | b2] + Adam state.  TargetNetwork, clip + Adam, Polyak and the
    checkpoint walk treat it as any HipApproximator; only IQNLearner evaluates it."""

    def __init__(self, n_in, hidden, n_actions, n_cos=64, act="relu", lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, seed=0, net_id=0,
                 device="cuda", params=None):
        np_ = iqn_nparams(n_in, hidden, n_actions, n_cos)
        if np_ < 0:
            raise ValueError(f"IQNApproximator: the IQN kernels take {ENVELOPE}")
        if params is None:
            params = torch.empty(np_, dtype=torch.float32, device=device)
            call("rlhip_iqn_init_f32", ptr(params), n_in, hidden, n_actions, n_cos, seed, net_id, stream_ptr())
        elif torch.as_tensor(params).numel() != np_:
            raise ValueError(f"IQNApproximator: params has {torch.as_tensor(params).numel()} elements, the network {np_}")
        super().__init__(n_in, hidden, n_actions, act, lr, beta1, beta2, eps, seed, net_id, device, params, layers=2)
        self.n_cos = int(n_cos)

    def forward(self, x):
        raise NotImplementedError("IQNApproximator: the network takes a state AND drawn quantile levels; use IQNLearner.forward / quantiles")


# --------------------------------------------------------------------------------------- learner
class IQNLearner(DistributionalLearner):
    """IQNLearner(approximator = TargetNetwork(IQNApproximator(ns, h, n_actions, n_cos)), n_actions, N = 32, N_target = 32, K = 32,
    kappa = 1.0, ...): N online and N_target target levels per sample and update, K levels per plan!.  The gate, the counters and the
    tail of an update are DQNLearner's; every update is the batch form

        draw -> gather -> rlhip_iqn_grad_batch_f32 -> [priority write-back] -> clip + Adam -> target sync

    on record rings (ns 2..4) and frame rings (ns 5..16), uniform or prioritized, 1-step or n-step, plain or Double DQN.  The levels of an
    update are drawn under (seed, batch position, draw_ctr), those of plan! under the explorer's (seed, env id, step), each with a Philox
    tag of its own.  The written-back priority is (ql + per_eps)^per_alpha of the UNWEIGHTED per-sample loss."""

    def __init__(self, approximator, n_actions, N=32, N_target=32, K=32, kappa=1.0, batchsize=32, gamma=0.99, min_replay_history=100,
                 update_freq=1, max_grad_norm=0.0, seed=0, process_group=None, per_eps=1e-6, per_alpha=0.6, per_beta=0.0, n_step=1,
                 double_dqn=False):
        n_actions, N, N_target, K = int(n_actions), int(N), int(N_target), int(K)
        refuse_noisy(getattr(approximator, "network", None), "IQNLearner")
        if getattr(getattr(approximator, "network", None), "n_cos", None) is None:
            raise TypeError("IQNLearner: the approximator is a TargetNetwork(IQNApproximator(ns, h, n_actions, n_cos)); NoisyDense, "
                            "three-layer and bf16 networks are out of scope")
        net = self._check_approximator_(approximator, process_group, n_actions, 1, "1", "n_actions")
        if not (math.isfinite(float(kappa)) and float(kappa) > 0.0):
            raise ValueError(f"IQNLearner: kappa must be finite and > 0 (kappa = 0, the pure quantile loss, is out of scope), got {kappa}")
        if int(update_freq) < 1 or int(batchsize) < 1:
            raise ValueError("update_freq and batchsize must be >= 1")
        # (raise for a shape outside the kernels' envelope, before any C call that launches)
        iqn_workspace(net.n_in, net.hidden, n_actions, net.n_cos, K, K, 1, net.params.device)
        self.workspace = iqn_workspace(net.n_in, net.hidden, n_actions, net.n_cos, N, N_target, int(batchsize), net.params.device)
        self.n_actions, self.N, self.N_target, self.K, self.kappa = n_actions, N, N_target, K, float(kappa)
        self._init_update_state_(approximator, batchsize, gamma, min_replay_history, update_freq, max_grad_norm, seed, process_group,
                                 per_eps, per_alpha, per_beta, n_step, double_dqn)
        self.plan_seed, self.forward_ctr = seed, 0  # the level draws of forward / quantiles outside plan!
        # the per-sample quantile-Huber loss, then its priority
        self.ql = torch.zeros(self.batchsize, dtype=torch.float32, device=net.params.device)

    # ------------------------------------------------------------------------------------ plan!
    def _net_args(self):
        net = self.approximator.network
        return net.params, net.n_in, net.hidden, self.n_actions, net.n_cos, self.K, net.act

    def forward(self, x, seed=None, env_id_base=0, step=None):
        """forward(learner, s) -> Q (na, n), the mean over K drawn levels; without (seed, step) every call draws new levels"""
        return self.quantiles(x, seed, env_id_base, step)[0]

    def quantiles(self, x, seed=None, env_id_base=0, step=None):
        """-> (Q (na, n), the quantiles th (K, na, n), their levels tau (K, n))"""
        if step is None:
            step, self.forward_ctr = self.forward_ctr, self.forward_ctr + 1
        n = x.shape[1]
        th = torch.empty((self.n_actions * self.K, n), dtype=torch.float32, device=x.device)
        tau = torch.empty((self.K, n), dtype=torch.float32, device=x.device)
        q = iqn_forward(*self._net_args(), x, self.plan_seed if seed is None else seed, env_id_base, step, quantiles=th, tau=tau)
        return q, th.view(self.n_actions, self.K, -1).permute(1, 0, 2), tau

    def plan_distributional_(self, obs, eps, seed, env_id_base, step, actions=None, q_out=None):
        """QBasedPolicy's plan! for this learner: K levels, the mean of the quantiles and the eps-greedy choice in one launch"""
        if q_out is not None and q_out.shape[0] != self.n_actions:
            q_out = None
        return iqn_plan(*self._net_args(), obs, eps, seed, env_id_base, step, actions, q_out)

    # -------------------------------------------------------------------------------- optimise!
    def _grad_launch_(self, batch, gamma, weights):
        s, a, r, t, sn, n_used = batch
        tn = self.approximator
        net = tn.network
        ws = self.workspace if a.numel() == self.batchsize else None
        iqn_grad_batch(net.n_in, net.hidden, self.n_actions, net.n_cos, self.N, self.N_target, net.act, self.kappa, net.params, tn.target, s,
                       a, r, t, sn, gamma, self.seed, self.draw_ctr, n_used, weights, self.double_dqn, ws, self.grad, self.loss, self.ql)
        return self.ql
