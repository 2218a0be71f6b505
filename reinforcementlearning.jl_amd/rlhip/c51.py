"""RainbowLearner -- the categorical (C51) distributional DQN learner under the unchanged QBasedPolicy.

The reference's design blog names C51 and IQN as the distributional members of the QBasedPolicy family: "the estimation is not the
Q-values directly. But we can still fit them into the QBasedPolicy. The main change is to override ... plan! ... to use the Q value
distribution".  The Zoo's RainbowLearner left the tree with the rest of the Zoo, so include/rlhip.h states the update (csrc/c51.hip
implements it, tests/c51_ref.py replays it).  The network is the shipped two-layer layout with n_actions * n_atoms output rows,
row k + n_atoms * o = atom k of action o.

Out of scope, refused by name: IQN, NoisyDense, a fused vec-step, three-layer and bf16 networks, dueling distributional
heads, sharded runs (world > 1), UInt8 frames.
"""
import torch

from . import _lib
from ._lib import call
from .dqn import DQNLearner, _Scratch
from .ops import ptr, stream_ptr

ENVELOPE = "obs_dim 2..16, hidden a multiple of 4 and <= 256, 1..4 actions, n_atoms 2..64"


# ----------------------------------------------------------------------------- functional layer
def _opt(t):
    return None if t is None else ptr(t)


def c51_workspace(ns, h, na, n_atoms, batch, device="cuda"):
    nbytes = int(_lib.lib.rlhip_c51_workspace_bytes(ns, h, na, n_atoms, batch))
    if nbytes < 0:
        raise ValueError(f"the C51 kernels take {ENVELOPE}, batch >= 1; got obs_dim = {ns}, hidden = {h}, actions = {na}, "
                         f"n_atoms = {n_atoms}, batch = {batch}")
    return torch.empty(nbytes, dtype=torch.uint8, device=device)


def c51_forward(params, ns, h, na, n_atoms, act, v_min, v_max, obs, q_out=None, probs=None, logits=None):
    """forward(learner, s): obs (ns, n) -> Q (na, n) = sum_k z_k p[k, o]; `probs` / `logits` ((n_atoms * na), n) are written where given"""
    n = obs.shape[1]
    q_out = q_out if q_out is not None else torch.empty((na, n), dtype=torch.float32, device=obs.device)
    call("rlhip_c51_forward_f32", ptr(params), ns, h, na, n_atoms, act, v_min, v_max, ptr(obs), n, ptr(q_out), _opt(probs), _opt(logits),
         stream_ptr())
    return q_out


def c51_plan(params, ns, h, na, n_atoms, act, v_min, v_max, obs, eps, seed, env_id_base, step, actions=None, q_out=None):
    """plan! in one launch: byte for byte `c51_forward` then `eps_greedy_select` -> (0-based actions, q (na, n))"""
    n = obs.shape[1]
    actions = actions if actions is not None else torch.empty(n, dtype=torch.int32, device=obs.device)
    q_out = q_out if q_out is not None else torch.empty((na, n), dtype=torch.float32, device=obs.device)
    call("rlhip_c51_plan_f32", ptr(params), ns, h, na, n_atoms, act, v_min, v_max, ptr(obs), n, float(eps), seed, env_id_base, step,
         ptr(actions), ptr(q_out), stream_ptr())
    return actions, q_out


def c51_grad_batch(ns, h, na, n_atoms, act, v_min, v_max, params, target_params, s, a, r, term, s_next, gamma, n_used=None, weights=None,
                   double_dqn=False, workspace=None, grad=None, loss=None, ce=None, proj=None, sel=None):
    """loss and gradient of the categorical cross-entropy on a gathered batch (s / s_next (ns, batch)) -> (grad, loss).  n_used: the
    transitions each n-step window used; weights: importance-sampling weights; ce (batch,): the unweighted per-sample loss; proj
    (n_atoms, batch): the projected target distribution; sel (batch,) int32: the bootstrap action a*."""
    dev, b = params.device, a.numel()
    workspace = workspace if workspace is not None else c51_workspace(ns, h, na, n_atoms, b, dev)
    grad = grad if grad is not None else torch.empty_like(params)
    loss = loss if loss is not None else torch.empty(1, dtype=torch.float32, device=dev)
    if term.dtype == torch.bool:
        term = term.view(torch.uint8)
    call("rlhip_c51_grad_batch_f32", ns, h, na, n_atoms, act, v_min, v_max, ptr(params), ptr(target_params), ptr(s), ptr(a), ptr(r),
         ptr(term), ptr(s_next), b, gamma, _opt(n_used), _opt(weights), int(bool(double_dqn)), ptr(workspace), ptr(grad), ptr(loss),
         _opt(ce), _opt(proj), _opt(sel), stream_ptr())
    return grad, loss


# --------------------------------------------------------------------------------------- learner
class DistributionalLearner(DQNLearner):
    """What the distributional learners (RainbowLearner, QRDQNLearner) share: the admission checks of the approximator, the state of an
    update and the batch form

        draw -> gather -> the learner's gradient entry (`_grad_launch_`) -> [priority write-back] -> clip + Adam -> target sync

    on record rings (ns 2..4) and frame rings (ns 5..16).  The gate, the counters and the tail are DQNLearner's (`should_update_`,
    `_draw_`, `_is_weights_`, `_exchange_and_apply_`).  Messages name the learner's own type."""

    def _check_approximator_(self, approximator, process_group, n_actions, n_rows, rows, net_doc):
        name = type(self).__name__
        net = getattr(approximator, "network", None)
        if net is None or not hasattr(approximator, "target"):
            raise TypeError(f"{name}: the approximator is a TargetNetwork(HipApproximator(ns, h, {net_doc}))")
        if getattr(net, "dueling_params", None) is not None:
            raise NotImplementedError(f"{name}: a DuelingApproximator (dueling distributional heads) is out of scope; use a "
                                      "HipApproximator")
        if getattr(net, "layers", 2) == 3:
            raise NotImplementedError(f"{name}: three-layer (layers = 3, bf16 MFMA) networks are out of scope; use a two-layer "
                                      "HipApproximator (layers = 2)")
        if process_group is not None:
            import torch.distributed as dist

            if dist.get_world_size(process_group) > 1:
                raise NotImplementedError(f"{name}: sharded runs (process_group with world > 1) are out of scope")
        if net.n_out != n_actions * n_rows:
            raise ValueError(f"{name}: the network has n_out = {net.n_out} output rows, n_actions * {rows} = "
                             f"{n_actions} * {n_rows} = {n_actions * n_rows}")
        return net

    def _init_update_state_(self, approximator, batchsize, gamma, min_replay_history, update_freq, max_grad_norm, seed, process_group,
                            per_eps, per_alpha, per_beta, n_step, double_dqn):
        net = approximator.network
        dev = net.params.device
        self.double_dqn = bool(double_dqn)
        self.n_step = int(n_step)
        self._nstep = None
        if self.n_step > 1:
            from .trajectory import NStepBatchSampler

            self._nstep = NStepBatchSampler(self.n_step, gamma, batchsize, seed=seed)
        self.per_eps, self.per_alpha, self.per_beta = float(per_eps), float(per_alpha), per_beta
        self.approximator = approximator
        self.batchsize, self.gamma = int(batchsize), gamma
        self.min_replay_history, self.update_freq, self.max_grad_norm = min_replay_history, update_freq, max_grad_norm
        self.seed, self.draw_ctr, self.n_updates = seed, 0, 0
        self.vec_steps = 0
        self.process_group = process_group
        self.grad = torch.zeros_like(net.params)
        self.loss = torch.zeros(1, dtype=torch.float32, device=dev)
        self.is_weights = torch.ones(self.batchsize, dtype=torch.float32, device=dev)
        self._batch = None  # the gathered batch of the last update (scratch)
        self._idx = self._key = self._prio = None

    def _grad_launch_(self, batch, gamma, weights):
        """the learner's gradient entry on the gathered batch -> the (batchsize,) tensor of UNWEIGHTED per-sample losses"""
        raise NotImplementedError

    def _gradient_batch_(self, batch, gamma, prioritized, traces):
        per_sample = self._grad_launch_(batch, gamma, self._is_weights_() if prioritized else None)
        if prioritized:  # trajectory[:priority, keys] = (loss_i + eps)^alpha under the drawn keys, in this call: before any further push
            call("rlhip_per_priority_f32", ptr(per_sample), self.batchsize, self.per_eps, self.per_alpha, ptr(per_sample), stream_ptr())
            traces.set_priority_(self._key, per_sample)
        return self._exchange_and_apply_()

    def _update_batch_(self, traces, prioritized):
        """a frame ring (ns 5..16): the three draws of DQNLearner's batch form, gathered by the sampler"""
        return self._gradient_batch_(self._draw_batch_(traces, prioritized), self.gamma, prioritized, traces)

    def _update_(self, traces, prioritized):
        """a record ring (ns 2..4): DQNLearner's draw, then the gather of the drawn (or folded) transitions"""
        net = self.approximator.network
        if traces.obs_dim != net.n_in:
            raise ValueError(f"{type(self).__name__}: the traces hold observations of {traces.obs_dim} components, the network takes "
                             f"{net.n_in}")
        ring, idx, gamma, _ = self._draw_(traces, prioritized)
        if idx is None:  # (the plain DQN learner draws inside its gradient launch: the same Philox draw, made here)
            idx = traces.sample_indices(self.batchsize, self.seed, self.draw_ctr)
        batch = ring.gather(idx) + (None,)
        self._batch = _Scratch(batch)
        return self._gradient_batch_(batch, gamma, prioritized, traces)


class RainbowLearner(DistributionalLearner):
    """RainbowLearner(approximator = TargetNetwork(HipApproximator(ns, h, n_actions * n_atoms)), n_actions, n_atoms = 51, v_min, v_max,
    ...): the value of every action is a categorical distribution over the atoms z_k = v_min + k (v_max - v_min) / (n_atoms - 1); the
    loss is the cross-entropy against the projected Bellman target.  The gate, the counters and the tail of an update are DQNLearner's
    (`should_update_`, `_draw_`, `_is_weights_`, `_exchange_and_apply_`); every update is the batch form

        draw -> gather -> rlhip_c51_grad_batch_f32 -> [priority write-back] -> clip + Adam -> target sync

    on record rings (ns 2..4: uniform or prioritized, 1-step or n-step through the sampler's fold) and on frame rings (ns 5..16).
    The written-back priority is (ce + per_eps)^per_alpha of the UNWEIGHTED per-sample cross-entropy."""

    def __init__(self, approximator, n_actions, n_atoms=51, v_min=-10.0, v_max=10.0, batchsize=32, gamma=0.99, min_replay_history=100,
                 update_freq=1, max_grad_norm=0.0, seed=0, process_group=None, per_eps=1e-6, per_alpha=0.6, per_beta=0.0, n_step=1,
                 double_dqn=False):
        n_actions, n_atoms = int(n_actions), int(n_atoms)
        net = self._check_approximator_(approximator, process_group, n_actions, n_atoms, "n_atoms", "n_actions * n_atoms")
        if not float(v_min) < float(v_max) or not all(map(lambda v: abs(float(v)) < float("inf"), (v_min, v_max))):
            raise ValueError(f"RainbowLearner: the support needs finite v_min < v_max, got [{v_min}, {v_max}]")
        if int(update_freq) < 1 or int(batchsize) < 1:
            raise ValueError("update_freq and batchsize must be >= 1")
        # (raises for a shape outside the kernels' envelope, before any C call that launches)
        self.workspace = c51_workspace(net.n_in, net.hidden, n_actions, n_atoms, int(batchsize), net.params.device)
        self.n_actions, self.n_atoms, self.v_min, self.v_max = n_actions, n_atoms, float(v_min), float(v_max)
        self._init_update_state_(approximator, batchsize, gamma, min_replay_history, update_freq, max_grad_norm, seed, process_group,
                                 per_eps, per_alpha, per_beta, n_step, double_dqn)
        # the per-sample cross-entropy, then its priority
        self.ce = torch.zeros(self.batchsize, dtype=torch.float32, device=net.params.device)

    # ------------------------------------------------------------------------------------ plan!
    def _net_args(self):
        net = self.approximator.network
        return net.params, net.n_in, net.hidden, self.n_actions, self.n_atoms, net.act, self.v_min, self.v_max

    def forward(self, x):
        """forward(learner, s) -> Q (na, n), the expectation of every action's distribution"""
        return c51_forward(*self._net_args(), x)

    def distribution(self, x):
        """-> (Q (na, n), probabilities (n_atoms, na, n))"""
        probs = torch.empty((self.n_actions * self.n_atoms, x.shape[1]), dtype=torch.float32, device=x.device)
        q = c51_forward(*self._net_args(), x, probs=probs)
        return q, probs.view(self.n_actions, self.n_atoms, -1).permute(1, 0, 2)

    def plan_distributional_(self, obs, eps, seed, env_id_base, step, actions=None, q_out=None):
        """QBasedPolicy's plan! for this learner: the expectation of the distribution and the eps-greedy choice in one launch"""
        if q_out is not None and q_out.shape[0] != self.n_actions:
            q_out = None
        return c51_plan(*self._net_args(), obs, eps, seed, env_id_base, step, actions, q_out)

    # -------------------------------------------------------------------------------- optimise!
    def _grad_launch_(self, batch, gamma, weights):
        s, a, r, t, sn, n_used = batch
        tn = self.approximator
        net = tn.network
        ws = self.workspace if a.numel() == self.batchsize else None
        c51_grad_batch(net.n_in, net.hidden, self.n_actions, self.n_atoms, net.act, self.v_min, self.v_max, net.params, tn.target, s, a, r,
                       t, sn, gamma, n_used, weights, self.double_dqn, ws, self.grad, self.loss, self.ce)
        return self.ce
