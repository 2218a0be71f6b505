"""SACPolicy -- Soft Actor-Critic on the continuous vector envs (PendulumEnv, ContinuousMountainCarEnv, CartPoleEnv(continuous = True)).

The reference's SoftGaussianNetwork is "mainly used for SAC" (RLCore/src/utils/networks.jl:127-128) and its docs name SACPolicy on
Pendulum as the continuous off-policy baseline; the type itself left the tree with the Zoo, so include/rlhip.h states the update
(csrc/sac.hip implements it, tests/sac_ref.py replays it).  The policy fits the unchanged `run(Agent(policy, trajectory), env)`:
`Agent` pushes the env's Float32 action tensor through the ring push, so its bits land in the record's action word.

Out of scope, refused by name: more than one action component, frame rings and obs_dim > 4, prioritized or n-step replay,
importance-sampling weights, three-layer or bf16 networks, a fused vec-step, sharded runs (world > 1), Float64 envs.
"""
import ctypes as C
import math

import torch

from . import _lib
from ._lib import call
from .ops import ptr, stream_ptr


# ----------------------------------------------------------------------------- functional layer
def sac_workspace(ns, h, batch, device="cuda"):
    nbytes = int(_lib.lib.rlhip_sac_workspace_bytes(ns, h, batch))
    if nbytes < 0:
        raise ValueError(f"the SAC kernels take obs_dim 2..4, hidden a multiple of 4 and <= 256, batch >= 1; got obs_dim = {ns}, "
                         f"hidden = {h}, batch = {batch}")
    return torch.empty(nbytes, dtype=torch.uint8, device=device)


def _opt(t):
    return None if t is None else ptr(t)


def sac_plan(actor, ns, h, act, obs, min_sigma, max_sigma, action_scale, seed, env_id_base, step, deterministic=False, action=None,
             logp=None, mu=None, rho=None, raw_sigma=None):
    """plan! for the (ns, n) observations `obs` in one launch -> action (n,); the other outputs are written where given"""
    n = obs.shape[1]
    action = action if action is not None else torch.empty(n, dtype=torch.float32, device=obs.device)
    call("rlhip_sac_plan_f32", ptr(actor), ns, h, act, ptr(obs), n, min_sigma, max_sigma, action_scale, int(bool(deterministic)), seed,
         env_id_base, step, ptr(action), _opt(logp), _opt(mu), _opt(rho), _opt(raw_sigma), stream_ptr())
    return action


def sac_critic_grad(traces, h, act, actor, critics, targets, idx, alpha, gamma, min_sigma, max_sigma, action_scale, seed, step,
                    workspace=None, grad=None, loss=None, y=None):
    """loss (2,) and gradient of [Q1 | Q2] against the soft TD target on the transitions `idx` of a record ring -> (grad, loss)"""
    b, dev = idx.numel(), critics.device
    workspace = workspace if workspace is not None else sac_workspace(traces.obs_dim, h, b, dev)
    grad = grad if grad is not None else torch.empty_like(critics)
    loss = loss if loss is not None else torch.empty(2, dtype=torch.float32, device=dev)
    call("rlhip_sac_critic_grad_f32", C.byref(traces.rb), h, act, ptr(actor), ptr(critics), ptr(targets), b, ptr(idx), ptr(alpha), gamma,
         min_sigma, max_sigma, action_scale, seed, step, ptr(workspace), ptr(grad), ptr(loss), _opt(y), stream_ptr())
    return grad, loss


def sac_actor_grad(traces, h, act, actor, critics, idx, alpha, min_sigma, max_sigma, action_scale, seed, step, alpha_lr=0.0,
                   target_entropy=0.0, alpha_out=None, workspace=None, grad=None, stats=None, sel=None, logp=None):
    """gradient of the actor loss mean(alpha logp - min(Q1, Q2)) and its statistics (loss, mean q, mean logp) -> (grad, stats); with
    alpha_lr > 0 and `alpha_out` (which may be `alpha`) also the entropy coefficient's step"""
    b, dev = idx.numel(), actor.device
    workspace = workspace if workspace is not None else sac_workspace(traces.obs_dim, h, b, dev)
    grad = grad if grad is not None else torch.empty_like(actor)
    stats = stats if stats is not None else torch.empty(3, dtype=torch.float32, device=dev)
    call("rlhip_sac_actor_grad_f32", C.byref(traces.rb), h, act, ptr(actor), ptr(critics), b, ptr(idx), ptr(alpha), min_sigma, max_sigma,
         action_scale, seed, step, alpha_lr, target_entropy, _opt(alpha_out), ptr(workspace), ptr(grad), ptr(stats), _opt(sel),
         _opt(logp), stream_ptr())
    return grad, stats


# ---------------------------------------------------------------------------------------- policy
class _Adam:
    """Adam(lr) state of one flat vector (Flux defaults)"""

    def __init__(self, params, lr):
        self.lr, self.beta1, self.beta2, self.eps = float(lr), 0.9, 0.999, 1e-8
        self.m, self.v = torch.zeros_like(params), torch.zeros_like(params)
        self.beta_pow = torch.tensor([self.beta1, self.beta2], dtype=torch.float32, device=params.device)
        self.gn = torch.zeros(1, dtype=torch.float32, device=params.device)

    def step_(self, params, grad, clip_norm):
        from .ops import adam_, clip_adam_

        if clip_norm > 0.0:
            clip_adam_(params, grad, self.m, self.v, self.beta_pow, 1.0, clip_norm, self.lr, self.beta1, self.beta2, self.eps, self.gn)
        else:
            adam_(params, grad, self.m, self.v, self.beta_pow, self.lr, self.beta1, self.beta2, self.eps)


class SACPolicy:
    """SACPolicy(; policy = SoftGaussianNetwork(pre = Dense(ns, h, act), mu = Dense(h, 1), sigma = Dense(h, 1, softplus)),
    qnetwork1/2 = Chain(Dense(ns + 1, h, act), Dense(h, 1)), their targets, gamma, tau, alpha, batchsize, start_steps, update_after,
    update_freq, automatic_entropy_tuning, lr_alpha, target_entropy, ...) on a HipVecEnv with one Float32 action component.

    `actor` is mlp2(ns, h, 2) (row 0 mu, row 1 the pre-softplus sigma), `critics` = [Q1 | Q2], each mlp2(ns + 1, h, 1) on
    vcat(s, u), `targets` their Polyak copy.  One update: draw -> critic gradient -> Adam over [Q1 | Q2] -> actor gradient (against the
    stepped critics) with the alpha step -> Adam over the actor -> Polyak with rho = 1 - tau.  plan! draws under `seed` at the vec-step
    counter, updates under `seed + 1` at the update counter (include/rlhip.h: stream separation)."""

    def __init__(self, env, hidden=64, act="relu", gamma=0.99, tau=0.005, alpha=0.2, batchsize=64, start_steps=0, update_after=1000,
                 update_freq=1, automatic_entropy_tuning=True, lr_alpha=3e-3, target_entropy=-1.0, lr=3e-3, min_sigma=0.0,
                 max_sigma=math.inf, action_scale=None, max_grad_norm=0.0, seed=0, process_group=None):
        from .ops import mlp2_init

        if not getattr(env, "continuous", False):
            raise ValueError("SACPolicy: a continuous-action env (PendulumEnv, ContinuousMountainCarEnv, CartPoleEnv(continuous = True))")
        if getattr(env, "is_f64", 0):
            raise NotImplementedError("SACPolicy: Float64 envs are out of scope (the kernels and the record ring are Float32)")
        sp = env.action_space()
        if len(sp.lo) != 1:
            raise NotImplementedError("SACPolicy: one action component (da = 1); da > 1 is out of scope")
        ns = int(env.state().shape[0])
        if not 2 <= ns <= 4:
            raise NotImplementedError(f"SACPolicy: observations of 2..4 components (record rings); obs_dim = {ns} (frame rings and "
                                      "obs_dim > 4) is out of scope")
        if isinstance(act, str) and act not in ("relu", "tanh"):
            raise ValueError("act must be 'relu' or 'tanh'")
        if hidden % 4 != 0 or not 4 <= hidden <= 256:
            raise NotImplementedError("SACPolicy: two-layer Float32 networks with hidden a multiple of 4 and <= 256 (three-layer and "
                                      "bf16 networks are out of scope)")
        if process_group is not None:
            import torch.distributed as dist

            if dist.get_world_size(process_group) > 1:
                raise NotImplementedError("SACPolicy: sharded runs (world > 1) are out of scope")
        if int(update_freq) < 1 or int(batchsize) < 1:
            raise ValueError("update_freq and batchsize must be >= 1")
        dev = env.device
        self.n_in, self.hidden = ns, int(hidden)
        self.act = {"relu": 0, "tanh": 1}[act] if isinstance(act, str) else int(act)
        self.gamma, self.tau, self.batchsize = float(gamma), float(tau), int(batchsize)
        self.start_steps, self.update_after, self.update_freq = int(start_steps), int(update_after), int(update_freq)
        self.automatic_entropy_tuning, self.lr_alpha, self.target_entropy = bool(automatic_entropy_tuning), float(lr_alpha), float(target_entropy)
        self.min_sigma, self.max_sigma = float(min_sigma), float(max_sigma)
        self.action_lo, self.action_hi = float(sp.lo[0]), float(sp.hi[0])
        self.action_scale = float(sp.hi[0]) if action_scale is None else float(action_scale)
        self.max_grad_norm, self.seed = float(max_grad_norm), int(seed)
        self.actor = mlp2_init(ns, self.hidden, 2, self.seed, 0, dev)
        self.critics = torch.cat([mlp2_init(ns + 1, self.hidden, 1, self.seed, 1, dev), mlp2_init(ns + 1, self.hidden, 1, self.seed, 2, dev)])
        self.targets = self.critics.clone()
        self.alpha = torch.tensor([float(alpha)], dtype=torch.float32, device=dev)
        self.actor_opt, self.critic_opt = _Adam(self.actor, lr), _Adam(self.critics, lr)
        self.vec_steps = 0   # optimise! calls so far (one per vec-step): the update_freq gate
        self.plan_steps = 0  # plan! calls so far: the step of the exploration draws
        self.n_updates = 0   # the step of the update draws and of the index draw
        self.actor_grad, self.critic_grad = torch.zeros_like(self.actor), torch.zeros_like(self.critics)
        self.critic_loss = torch.zeros(2, dtype=torch.float32, device=dev)
        self.actor_stats = torch.zeros(3, dtype=torch.float32, device=dev)
        self.workspace = _Scratch(sac_workspace(ns, self.hidden, self.batchsize, dev))
        self.last_idx = _Scratch(None)  # the indices of the last update

    # ------------------------------------------------------------------------------------ plan!
    def plan_(self, env, deterministic=False):
        """plan!(policy, env) -> Float32 actions (n,).  The first `start_steps` vec-steps are uniform in the action box (the draw of
        RandomPolicy); `deterministic = True` (evaluation) is action_scale * tanh(mu) and advances no counter."""
        if deterministic:
            return sac_plan(self.actor, self.n_in, self.hidden, self.act, env.state(), self.min_sigma, self.max_sigma, self.action_scale,
                            self.seed, env.env_id_base, 0, deterministic=True)
        self.plan_steps += 1
        step = self.plan_steps
        if step <= self.start_steps:
            from .ops import fill_uniform

            u = fill_uniform(env.n, self.seed, step, 7, env.device)
            return u * (self.action_hi - self.action_lo) + self.action_lo
        return sac_plan(self.actor, self.n_in, self.hidden, self.act, env.state(), self.min_sigma, self.max_sigma, self.action_scale,
                        self.seed, env.env_id_base, step)

    # -------------------------------------------------------------------------------- optimise!
    def check_traces(self, traces):
        """what the update reads: a record ring with Float32 actions and this policy's observation width, uniform 1-step replay"""
        if hasattr(traces, "sample_prioritized"):
            raise NotImplementedError("SACPolicy: prioritized replay (and importance-sampling weights) is out of scope; use "
                                      "CircularArraySARTSTraces(..., action_dtype = torch.float32)")
        if not getattr(traces, "records_layout", False):
            raise NotImplementedError("SACPolicy: frame-layout traces (UInt8 frames, obs_dim > 4) are out of scope; the update reads a "
                                      "record ring (Float32 observations of 2..4 components)")
        if getattr(traces, "action_dtype", torch.int32) != torch.float32:
            raise TypeError("SACPolicy: the traces must store Float32 actions: CircularArraySARTSTraces(..., action_dtype = torch.float32)")
        if traces.obs_dim != self.n_in:
            raise ValueError(f"SACPolicy: the traces hold observations of {traces.obs_dim} components, the networks take {self.n_in}")

    def optimise_(self, trajectory):
        """optimise!(policy, PostActStage, trajectory): at most one update per vec-step, behind update_after / update_freq and the
        trajectory's InsertSampleRatioController"""
        traces = trajectory.container
        self.check_traces(traces)
        if getattr(trajectory.sampler, "n", 1) != 1:
            raise NotImplementedError("SACPolicy: n-step replay (NStepBatchSampler) is out of scope")
        self.vec_steps += 1
        if traces.n_transitions() < self.update_after or self.vec_steps % self.update_freq != 0:
            return False
        if not trajectory.controller.on_sample_():
            return False
        self.update_(traces)
        return True

    def update_(self, traces, idx=None):
        """one update on `idx` (flat logical indices; None: rlhip_ring_sample_indices under (seed + 1, the update counter))"""
        useed, step, h = self.seed + 1, self.n_updates, self.hidden
        idx = self.last_idx.t = traces.sample_indices(self.batchsize, useed, step) if idx is None else idx
        ws = self.workspace.t
        if idx.numel() != self.batchsize:
            ws = sac_workspace(self.n_in, h, idx.numel(), self.actor.device)
        sac_critic_grad(traces, h, self.act, self.actor, self.critics, self.targets, idx, self.alpha, self.gamma, self.min_sigma,
                        self.max_sigma, self.action_scale, useed, step, ws, self.critic_grad, self.critic_loss)
        self.critic_opt.step_(self.critics, self.critic_grad, self.max_grad_norm)
        tune = self.automatic_entropy_tuning and self.lr_alpha > 0.0
        sac_actor_grad(traces, h, self.act, self.actor, self.critics, idx, self.alpha, self.min_sigma, self.max_sigma,
                       self.action_scale, useed, step, self.lr_alpha if tune else 0.0, self.target_entropy, self.alpha if tune else None,
                       ws, self.actor_grad, self.actor_stats)
        self.actor_opt.step_(self.actor, self.actor_grad, self.max_grad_norm)
        from .ops import polyak_

        polyak_(self.targets, self.critics, 1.0 - self.tau)
        self.n_updates += 1


class _Scratch:
    """a buffer rewritten in full before every use: not state of the policy (rlhip/checkpoint.py leaves it out)"""
    checkpoint_scratch = True

    def __init__(self, t):
        self.t = t
