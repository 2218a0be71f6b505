"""QRDQNLearner -- the quantile-regression (QR-DQN) distributional DQN learner under the unchanged QBasedPolicy.

The sibling of RainbowLearner that needs no hand-chosen support [v_min, v_max]: the value of every action is N quantiles at the fixed
levels tau_k = (2 k + 1) / (2 N), fitted by the quantile-Huber loss (Dabney et al. 2018).  The Zoo's QRDQNLearner is not in the
reference snapshot, so include/rlhip.h states the update (csrc/qrdqn.hip implements it, tests/qrdqn_ref.py replays it).  The network is
the shipped two-layer layout with n_actions * n_quantiles output rows, row k + n_quantiles * o = quantile k of action o.

Out of scope, refused by name: IQN and FQF, kappa = 0, NoisyDense, a fused vec-step, three-layer and bf16 networks, dueling
distributional heads, sharded runs (world > 1), UInt8 frames.
"""
import math

import torch

from . import _lib
from ._lib import call
from .c51 import DistributionalLearner, _opt
from .ops import ptr, stream_ptr

ENVELOPE = "obs_dim 2..16, hidden a multiple of 4 and <= 256, 1..4 actions, n_quantiles 1..64"


# ----------------------------------------------------------------------------- functional layer
def qrdqn_workspace(ns, h, na, n_quantiles, batch, device="cuda"):
    nbytes = int(_lib.lib.rlhip_qrdqn_workspace_bytes(ns, h, na, n_quantiles, batch))
    if nbytes < 0:
        raise ValueError(f"the QR-DQN kernels take {ENVELOPE}, batch >= 1; got obs_dim = {ns}, hidden = {h}, actions = {na}, "
                         f"n_quantiles = {n_quantiles}, batch = {batch}")
    return torch.empty(nbytes, dtype=torch.uint8, device=device)


def qrdqn_forward(params, ns, h, na, n_quantiles, act, obs, q_out=None, quantiles=None):
    """forward(learner, s): obs (ns, n) -> Q (na, n) = mean_k th[k, o]; `quantiles` ((n_quantiles * na), n) is written where given"""
    n = obs.shape[1]
    q_out = q_out if q_out is not None else torch.empty((na, n), dtype=torch.float32, device=obs.device)
    call("rlhip_qrdqn_forward_f32", ptr(params), ns, h, na, n_quantiles, act, ptr(obs), n, ptr(q_out), _opt(quantiles), stream_ptr())
    return q_out


def qrdqn_plan(params, ns, h, na, n_quantiles, act, obs, eps, seed, env_id_base, step, actions=None, q_out=None):
    """plan! in one launch: byte for byte `qrdqn_forward` then `eps_greedy_select` -> (0-based actions, q (na, n))"""
    n = obs.shape[1]
    actions = actions if actions is not None else torch.empty(n, dtype=torch.int32, device=obs.device)
    q_out = q_out if q_out is not None else torch.empty((na, n), dtype=torch.float32, device=obs.device)
    call("rlhip_qrdqn_plan_f32", ptr(params), ns, h, na, n_quantiles, act, ptr(obs), n, float(eps), seed, env_id_base, step, ptr(actions),
         ptr(q_out), stream_ptr())
    return actions, q_out


def qrdqn_grad_batch(ns, h, na, n_quantiles, act, kappa, params, target_params, s, a, r, term, s_next, gamma, n_used=None, weights=None,
                     double_dqn=False, workspace=None, grad=None, loss=None, ql=None, target=None, sel=None):
    """loss and gradient of the quantile-Huber loss on a gathered batch (s / s_next (ns, batch)) -> (grad, loss).  n_used: the
    transitions each n-step window used; weights: importance-sampling weights; ql (batch,): the unweighted per-sample loss; target
    (n_quantiles, batch): the Bellman target quantiles T_j; sel (batch,) int32: the bootstrap action a*."""
    dev, b = params.device, a.numel()
    workspace = workspace if workspace is not None else qrdqn_workspace(ns, h, na, n_quantiles, b, dev)
    grad = grad if grad is not None else torch.empty_like(params)
    loss = loss if loss is not None else torch.empty(1, dtype=torch.float32, device=dev)
    if term.dtype == torch.bool:
        term = term.view(torch.uint8)
    call("rlhip_qrdqn_grad_batch_f32", ns, h, na, n_quantiles, act, kappa, ptr(params), ptr(target_params), ptr(s), ptr(a), ptr(r),
         ptr(term), ptr(s_next), b, gamma, _opt(n_used), _opt(weights), int(bool(double_dqn)), ptr(workspace), ptr(grad), ptr(loss),
         _opt(ql), _opt(target), _opt(sel), stream_ptr())
    return grad, loss


# --------------------------------------------------------------------------------------- learner
class QRDQNLearner(DistributionalLearner):
    """QRDQNLearner(approximator = TargetNetwork(HipApproximator(ns, h, n_actions * n_quantiles)), n_actions, n_quantiles = 51,
    kappa = 1.0, ...): the value of every action is n_quantiles quantiles of its return; the loss is the quantile-Huber loss of every
    (target quantile, quantile) pair.  The gate, the counters and the tail of an update are DQNLearner's; every update is the batch form

        draw -> gather -> rlhip_qrdqn_grad_batch_f32 -> [priority write-back] -> clip + Adam -> target sync

    on record rings (ns 2..4: uniform or prioritized, 1-step or n-step through the sampler's fold) and on frame rings (ns 5..16).
    The written-back priority is (ql + per_eps)^per_alpha of the UNWEIGHTED per-sample loss."""

    def __init__(self, approximator, n_actions, n_quantiles=51, kappa=1.0, batchsize=32, gamma=0.99, min_replay_history=100, update_freq=1,
                 max_grad_norm=0.0, seed=0, process_group=None, per_eps=1e-6, per_alpha=0.6, per_beta=0.0, n_step=1, double_dqn=False):
        n_actions, n_quantiles = int(n_actions), int(n_quantiles)
        net = self._check_approximator_(approximator, process_group, n_actions, n_quantiles, "n_quantiles", "n_actions * n_quantiles")
        if not (math.isfinite(float(kappa)) and float(kappa) > 0.0):
            raise ValueError(f"QRDQNLearner: kappa must be finite and > 0 (kappa = 0, the pure quantile loss, is out of scope), got {kappa}")
        if int(update_freq) < 1 or int(batchsize) < 1:
            raise ValueError("update_freq and batchsize must be >= 1")
        # (raises for a shape outside the kernels' envelope, before any C call that launches)
        self.workspace = qrdqn_workspace(net.n_in, net.hidden, n_actions, n_quantiles, int(batchsize), net.params.device)
        self.n_actions, self.n_quantiles, self.kappa = n_actions, n_quantiles, float(kappa)
        self._init_update_state_(approximator, batchsize, gamma, min_replay_history, update_freq, max_grad_norm, seed, process_group,
                                 per_eps, per_alpha, per_beta, n_step, double_dqn)
        # the per-sample quantile-Huber loss, then its priority
        self.ql = torch.zeros(self.batchsize, dtype=torch.float32, device=net.params.device)

    # ------------------------------------------------------------------------------------ plan!
    def _net_args(self):
        net = self.approximator.network
        return net.params, net.n_in, net.hidden, self.n_actions, self.n_quantiles, net.act

    def forward(self, x):
        """forward(learner, s) -> Q (na, n), the mean of every action's quantiles"""
        return qrdqn_forward(*self._net_args(), x)

    def quantiles(self, x):
        """-> the quantiles (n_quantiles, na, n)"""
        th = torch.empty((self.n_actions * self.n_quantiles, x.shape[1]), dtype=torch.float32, device=x.device)
        qrdqn_forward(*self._net_args(), x, quantiles=th)
        return th.view(self.n_actions, self.n_quantiles, -1).permute(1, 0, 2)

    def plan_distributional_(self, obs, eps, seed, env_id_base, step, actions=None, q_out=None):
        """QBasedPolicy's plan! for this learner: the mean of the quantiles and the eps-greedy choice in one launch"""
        if q_out is not None and q_out.shape[0] != self.n_actions:
            q_out = None
        return qrdqn_plan(*self._net_args(), obs, eps, seed, env_id_base, step, actions, q_out)

    # -------------------------------------------------------------------------------- optimise!
    def _grad_launch_(self, batch, gamma, weights):
        s, a, r, t, sn, n_used = batch
        tn = self.approximator
        net = tn.network
        ws = self.workspace if a.numel() == self.batchsize else None
        qrdqn_grad_batch(net.n_in, net.hidden, self.n_actions, self.n_quantiles, net.act, self.kappa, net.params, tn.target, s, a, r, t, sn,
                         gamma, n_used, weights, self.double_dqn, ws, self.grad, self.loss, self.ql)
        return self.ql
