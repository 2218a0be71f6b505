"""TD3Policy and DDPGPolicy -- the deterministic-actor off-policy learners on the continuous vector envs (PendulumEnv,
ContinuousMountainCarEnv, CartPoleEnv(continuous = True)).

The reference's homepage lists DDPG and its docs build MADDPG on DDPGPolicy; the types themselves left the tree with the Zoo, so
include/rlhip.h states the update (csrc/td3.hip implements it on unit-sliced kernels, tests/td3_ref.py is its Float64 model).  The
policies fit the unchanged `run(Agent(policy, trajectory), env)`, as SACPolicy does.

`layers = 3` (two hidden layers: 256-256 in the TD3 paper's code, 400-300 in the DDPG paper) routes the same update to
csrc/td3_mlp3.hip (the hidden x hidden layer on the f32 MFMA; tests/td3_mlp3_ref.py); `layers = 2`, the default, is the path above.

Out of scope, refused by name: more than one action component, frame rings and obs_dim > 4, prioritized or n-step replay,
bf16 networks, a fused vec-step, sharded runs (world > 1), Float64 envs.
"""
import ctypes as C

import torch

from . import _lib
from ._lib import call
from .ops import ptr, stream_ptr
from .sac import _Adam, _opt, _Scratch


# ----------------------------------------------------------------------------- functional layer
_ENTRY = {2: "rlhip_td3_", 3: "rlhip_td3_mlp3_"}  # layers -> the prefix of its four entry points
_HIDDEN = {2: 16, 3: 32}                          # layers -> hidden is a multiple of this, up to 256


def td3_workspace(ns, h, n_critics, batch, device="cuda", layers=2):
    nbytes = int(getattr(_lib.lib, _ENTRY[layers] + "workspace_bytes")(ns, h, n_critics, batch))
    if nbytes < 0:
        m = _HIDDEN[layers]
        raise ValueError(f"the TD3 kernels take obs_dim 2..4, hidden a multiple of {m} in {m}..256, 1 or 2 critics, batch >= 1; got "
                         f"obs_dim = {ns}, hidden = {h}, n_critics = {n_critics}, batch = {batch}")
    return torch.empty(nbytes, dtype=torch.uint8, device=device)


def td3_plan(actor, ns, h, act, obs, action_scale, act_noise, action_lo, action_hi, seed, env_id_base, step, deterministic=False,
             action=None, mu=None, layers=2):
    """plan! for the (ns, n) observations `obs` in one launch -> action (n,) = clamp(action_scale tanh(mu) + act_noise N(0, 1))"""
    n = obs.shape[1]
    action = action if action is not None else torch.empty(n, dtype=torch.float32, device=obs.device)
    call(_ENTRY[layers] + "plan_f32", ptr(actor), ns, h, act, ptr(obs), n, action_scale, act_noise, action_lo, action_hi,
         int(bool(deterministic)), seed, env_id_base, step, ptr(action), _opt(mu), stream_ptr())
    return action


def td3_critic_grad(traces, h, act, n_critics, actor_target, critics, critic_targets, idx, gamma, action_scale, target_noise, noise_clip,
                    action_lo, action_hi, seed, step, workspace=None, grad=None, loss=None, y=None, noise=None, layers=2):
    """loss (n_critics,) and gradient of the critics against the smoothed, clipped double-Q target on the transitions `idx` of a record
    ring -> (grad, loss)"""
    b, dev = idx.numel(), critics.device
    workspace = workspace if workspace is not None else td3_workspace(traces.obs_dim, h, n_critics, b, dev, layers)
    grad = grad if grad is not None else torch.empty_like(critics)
    loss = loss if loss is not None else torch.empty(n_critics, dtype=torch.float32, device=dev)
    call(_ENTRY[layers] + "critic_grad_f32", C.byref(traces.rb), h, act, n_critics, ptr(actor_target), ptr(critics), ptr(critic_targets), b,
         ptr(idx), gamma, action_scale, target_noise, noise_clip, action_lo, action_hi, seed, step, ptr(workspace), ptr(grad), ptr(loss),
         _opt(y), _opt(noise), stream_ptr())
    return grad, loss


def td3_actor_grad(traces, h, act, actor, critics, idx, action_scale, workspace=None, grad=None, stats=None, layers=2):
    """gradient of the actor loss mean(-Q1(s, action_scale tanh(mu(s)))) and its statistics (loss, mean Q1) -> (grad, stats);
    `critics` starts with Q1"""
    b, dev = idx.numel(), actor.device
    workspace = workspace if workspace is not None else td3_workspace(traces.obs_dim, h, 1, b, dev, layers)
    grad = grad if grad is not None else torch.empty_like(actor)
    stats = stats if stats is not None else torch.empty(2, dtype=torch.float32, device=dev)
    call(_ENTRY[layers] + "actor_grad_f32", C.byref(traces.rb), h, act, ptr(actor), ptr(critics), b, ptr(idx), action_scale, ptr(workspace),
         ptr(grad), ptr(stats), stream_ptr())
    return grad, stats


# ---------------------------------------------------------------------------------------- policy
class TD3Policy:
    """TD3Policy(; behavior_actor = Chain(Dense(ns, h, act), Dense(h, 1, tanh)), behavior_critic(s) = Chain(Dense(ns + 1, h, act),
    Dense(h, 1)), their targets, gamma, rho = 1 - tau, batchsize, start_steps, update_after, update_freq, policy_freq, target_act_limit
    = noise_clip, target_act_noise = target_noise, act_limit, act_noise) on a HipVecEnv with one Float32 action component.

    `actor` is mlp2(ns, h, 1), `critics` = [Q1 | Q2] ([Q1] with n_critics = 1), each mlp2(ns + 1, h, 1) on vcat(s, u);
    `actor_target` and `critic_targets` their Polyak copies.  One update: draw -> critic gradient -> Adam over the critics; on every
    policy_freq-th update -> actor gradient (against the stepped critics) -> Adam over the actor -> Polyak over both target vectors
    with rho = 1 - tau.  plan! draws under `seed` at the vec-step counter, the critic launch under `seed + 1` at the update counter
    (include/rlhip.h: stream separation).  `act_noise`, `target_noise` and `noise_clip` are in action units."""

    def __init__(self, env, hidden=64, act="relu", gamma=0.99, tau=0.005, batchsize=64, start_steps=0, update_after=1000, update_freq=1,
                 policy_freq=2, n_critics=2, act_noise=0.1, target_noise=0.2, noise_clip=0.5, lr=3e-3, action_scale=None,
                 max_grad_norm=0.0, seed=0, process_group=None, layers=2):
        from .dqn import mlp3_init
        from .ops import mlp2_init

        name = type(self).__name__
        if not getattr(env, "continuous", False):
            raise ValueError(f"{name}: a continuous-action env (PendulumEnv, ContinuousMountainCarEnv, CartPoleEnv(continuous = True))")
        if getattr(env, "is_f64", 0):
            raise NotImplementedError(f"{name}: Float64 envs are out of scope (the kernels and the record ring are Float32)")
        sp = env.action_space()
        if len(sp.lo) != 1:
            raise NotImplementedError(f"{name}: one action component (da = 1); da > 1 is out of scope")
        ns = int(env.state().shape[0])
        if not 2 <= ns <= 4:
            raise NotImplementedError(f"{name}: observations of 2..4 components (record rings); obs_dim = {ns} (frame rings and "
                                      "obs_dim > 4) is out of scope")
        if isinstance(act, str) and act not in ("relu", "tanh"):
            raise ValueError("act must be 'relu' or 'tanh'")
        if layers not in (2, 3):
            raise ValueError("layers must be 2 (one hidden layer) or 3 (two hidden layers)")
        if layers == 2 and (hidden % 16 != 0 or not 16 <= hidden <= 256):
            raise NotImplementedError(f"{name}: two-layer Float32 networks with hidden a multiple of 16 in 16..256 (three-layer networks: "
                                      "layers = 3; bf16 networks are out of scope)")
        if layers == 3 and (hidden % 32 != 0 or not 32 <= hidden <= 256):
            raise NotImplementedError(f"{name}: three-layer Float32 networks with hidden a multiple of 32 in 32..256 (bf16 networks are "
                                      "out of scope)")
        if int(n_critics) not in (1, 2):
            raise ValueError("n_critics must be 1 (DDPG) or 2 (TD3)")
        if process_group is not None:
            import torch.distributed as dist

            if dist.get_world_size(process_group) > 1:
                raise NotImplementedError(f"{name}: sharded runs (world > 1) are out of scope")
        if int(update_freq) < 1 or int(batchsize) < 1 or int(policy_freq) < 1:
            raise ValueError("update_freq, policy_freq and batchsize must be >= 1")
        dev = env.device
        self.n_in, self.hidden, self.n_critics, self.layers = ns, int(hidden), int(n_critics), int(layers)
        init = mlp2_init if layers == 2 else mlp3_init
        self.act = {"relu": 0, "tanh": 1}[act] if isinstance(act, str) else int(act)
        self.gamma, self.tau, self.batchsize = float(gamma), float(tau), int(batchsize)
        self.start_steps, self.update_after, self.update_freq = int(start_steps), int(update_after), int(update_freq)
        self.policy_freq = int(policy_freq)
        self.act_noise, self.target_noise, self.noise_clip = float(act_noise), float(target_noise), float(noise_clip)
        self.action_lo, self.action_hi = float(sp.lo[0]), float(sp.hi[0])
        self.action_scale = float(sp.hi[0]) if action_scale is None else float(action_scale)
        self.max_grad_norm, self.seed = float(max_grad_norm), int(seed)
        self.actor = init(ns, self.hidden, 1, self.seed, 0, dev)
        self.critics = torch.cat([init(ns + 1, self.hidden, 1, self.seed, 1 + c, dev) for c in range(self.n_critics)])
        self.actor_target, self.critic_targets = self.actor.clone(), self.critics.clone()
        self.actor_opt, self.critic_opt = _Adam(self.actor, lr), _Adam(self.critics, lr)
        self.vec_steps = 0   # optimise! calls so far (one per vec-step): the update_freq gate
        self.plan_steps = 0  # plan! calls so far: the step of the exploration draws
        self.n_updates = 0   # the step of the target-noise draws and of the index draw; the policy_freq gate
        self.actor_grad, self.critic_grad = torch.zeros_like(self.actor), torch.zeros_like(self.critics)
        self.critic_loss = torch.zeros(self.n_critics, dtype=torch.float32, device=dev)
        self.actor_stats = torch.zeros(2, dtype=torch.float32, device=dev)
        self.workspace = _Scratch(td3_workspace(ns, self.hidden, self.n_critics, self.batchsize, dev, self.layers))
        self.last_idx = _Scratch(None)    # the indices of the last update
        self.last_noise = _Scratch(torch.zeros(self.batchsize, dtype=torch.float32, device=dev))  # its clipped target noise

    # ------------------------------------------------------------------------------------ plan!
    def plan_(self, env, deterministic=False):
        """plan!(policy, env) -> Float32 actions (n,).  The first `start_steps` vec-steps are uniform in the action box (the draw of
        RandomPolicy); `deterministic = True` (evaluation) adds no noise and advances no counter."""
        args = (self.actor, self.n_in, self.hidden, self.act, env.state(), self.action_scale, self.act_noise, self.action_lo,
                self.action_hi, self.seed, env.env_id_base)
        if deterministic:
            return td3_plan(*args, 0, deterministic=True, layers=self.layers)
        self.plan_steps += 1
        step = self.plan_steps
        if step <= self.start_steps:
            from .ops import fill_uniform

            u = fill_uniform(env.n, self.seed, step, 7, env.device)
            return u * (self.action_hi - self.action_lo) + self.action_lo
        return td3_plan(*args, step, layers=self.layers)

    # -------------------------------------------------------------------------------- optimise!
    def check_traces(self, traces):
        """what the update reads: a record ring with Float32 actions and this policy's observation width, uniform 1-step replay"""
        name = type(self).__name__
        if hasattr(traces, "sample_prioritized"):
            raise NotImplementedError(f"{name}: prioritized replay (and importance-sampling weights) is out of scope; use "
                                      "CircularArraySARTSTraces(..., action_dtype = torch.float32)")
        if not getattr(traces, "records_layout", False):
            raise NotImplementedError(f"{name}: frame-layout traces (UInt8 frames, obs_dim > 4) are out of scope; the update reads a "
                                      "record ring (Float32 observations of 2..4 components)")
        if getattr(traces, "action_dtype", torch.int32) != torch.float32:
            raise TypeError(f"{name}: the traces must store Float32 actions: CircularArraySARTSTraces(..., action_dtype = torch.float32)")
        if traces.obs_dim != self.n_in:
            raise ValueError(f"{name}: the traces hold observations of {traces.obs_dim} components, the networks take {self.n_in}")

    def optimise_(self, trajectory):
        """optimise!(policy, PostActStage, trajectory): at most one update per vec-step, behind update_after / update_freq and the
        trajectory's InsertSampleRatioController"""
        traces = trajectory.container
        self.check_traces(traces)
        if getattr(trajectory.sampler, "n", 1) != 1:
            raise NotImplementedError(f"{type(self).__name__}: n-step replay (NStepBatchSampler) is out of scope")
        self.vec_steps += 1
        if traces.n_transitions() < self.update_after or self.vec_steps % self.update_freq != 0:
            return False
        if not trajectory.controller.on_sample_():
            return False
        self.update_(traces)
        return True

    def update_(self, traces, idx=None):
        """one update on `idx` (flat logical indices; None: rlhip_ring_sample_indices under (seed + 1, the update counter))"""
        from .ops import polyak_

        useed, step, h = self.seed + 1, self.n_updates, self.hidden
        idx = self.last_idx.t = traces.sample_indices(self.batchsize, useed, step) if idx is None else idx
        ws, noise = self.workspace.t, self.last_noise.t
        if idx.numel() != self.batchsize:
            ws = td3_workspace(self.n_in, h, self.n_critics, idx.numel(), self.actor.device, self.layers)
            noise = self.last_noise.t = torch.zeros(idx.numel(), dtype=torch.float32, device=self.actor.device)
        td3_critic_grad(traces, h, self.act, self.n_critics, self.actor_target, self.critics, self.critic_targets, idx, self.gamma,
                        self.action_scale, self.target_noise, self.noise_clip, self.action_lo, self.action_hi, useed, step, ws,
                        self.critic_grad, self.critic_loss, None, noise, layers=self.layers)
        self.critic_opt.step_(self.critics, self.critic_grad, self.max_grad_norm)
        self.n_updates += 1
        if self.n_updates % self.policy_freq == 0:
            td3_actor_grad(traces, h, self.act, self.actor, self.critics, idx, self.action_scale, ws, self.actor_grad, self.actor_stats,
                           layers=self.layers)
            self.actor_opt.step_(self.actor, self.actor_grad, self.max_grad_norm)
            polyak_(self.actor_target, self.actor, 1.0 - self.tau)
            polyak_(self.critic_targets, self.critics, 1.0 - self.tau)


class DDPGPolicy(TD3Policy):
    """DDPGPolicy(; behavior_actor, behavior_critic, their targets, gamma, rho, batchsize, start_steps, update_after, update_freq,
    act_limit, act_noise): TD3 with one critic, no target smoothing and an actor step on every update."""

    def __init__(self, env, **kw):
        for fixed in ("n_critics", "target_noise", "policy_freq"):
            if fixed in kw:
                raise TypeError(f"DDPGPolicy fixes {fixed} (n_critics = 1, target_noise = 0, policy_freq = 1); use TD3Policy to set it")
        super().__init__(env, n_critics=1, target_noise=0.0, policy_freq=1, **kw)
