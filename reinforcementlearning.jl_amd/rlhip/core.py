"""run(policy, env, stop_condition, hook) for the vectorised env -- host mirror of the reference's
experiment loop, stages, stop conditions, hooks, Agent and RandomPolicy.

Reference files mirrored (src/ReinforcementLearningCore/src/...):
    core/run.jl:22-78            run / _run (scalar loop with 6 stages)
    core/stages.jl:10-37         stage types, default no-op push!/optimise!
    core/stop_conditions.jl      StopAfterNSteps (:48-76), StopAfterNEpisodes (:87-119), StopIfAny/All (:18-38)
    core/hooks.jl                EmptyHook, ComposedHook (:37-62), StepsPerEpisode, TotalRewardPerEpisode (:146-196),
                                 BatchStepsPerEpisode (:202-231), TimePerStep (:243-262), DoEveryNSteps
    policies/agent/agent_base.jl Agent: PreEpisode push (state,), PostAct push (state, action, reward, terminal)
    policies/random_policy.jl    RandomPolicy
and the vector-env specialisation of `_run` that the historical MultiThreadEnv used
(docs/homepage/blog/an_introduction_to_reinforcement_learning_jl_design_implementations_thoughts/index.md:351-374):
no episode stages; per vec-step  plan! -> PreAct push -> act! -> PostAct push -> stop check.

Host-side only: counters and callbacks.  Everything touching env state, trajectories or parameters is
a HIP kernel launched through the C ABI by the objects this loop drives.
"""
import functools
import time

import torch

# ------------------------------------------------------------------------------------- stages
PRE_EXPERIMENT_STAGE = "PreExperimentStage"
POST_EXPERIMENT_STAGE = "PostExperimentStage"
PRE_EPISODE_STAGE = "PreEpisodeStage"
POST_EPISODE_STAGE = "PostEpisodeStage"
PRE_ACT_STAGE = "PreActStage"
POST_ACT_STAGE = "PostActStage"


# ---------------------------------------------------------------------------- stop conditions
class StopAfterNSteps:
    """StopAfterNSteps(step; cur = 1): `check!` returns cur >= step, THEN increments (stop_conditions.jl:65-69),
    so exactly `step` steps are executed (test core/stop_conditions.jl:8: 11 trues in 20 calls for n = 10).
    On the vector env one check = one vec-step (the reference's MultiThreadEnv loop counted the same way)."""

    def __init__(self, step, cur=1):
        self.step, self.cur = int(step), int(cur)

    def check_(self, policy=None, env=None):
        res = self.cur >= self.step
        self.cur += 1
        return res


class StopAfterNEpisodes:
    """StopAfterNEpisodes(episode; cur = 0)  stop_conditions.jl:87-119.  On the vector env every terminated
    instance counts as one episode (one device->host read of the terminal flags per check)."""

    def __init__(self, episode, cur=0):
        self.episode, self.cur = int(episode), int(cur)

    def check_(self, policy, env):
        self.cur += int(env.is_terminated().sum())
        return self.cur >= self.episode


class StopIfAny:
    def __init__(self, *conds):
        self.conds = conds

    def check_(self, policy, env):
        return any([c.check_(policy, env) for c in self.conds])  # all are evaluated, like check!.(...)


class StopIfAll:
    def __init__(self, *conds):
        self.conds = conds

    def check_(self, policy, env):
        return all([c.check_(policy, env) for c in self.conds])


class StopAfterNSeconds:
    def __init__(self, seconds):
        self.deadline = time.time() + seconds

    def check_(self, policy, env):
        return time.time() > self.deadline


# -------------------------------------------------------------------------------------- hooks
class EmptyHook:
    def push_(self, stage, policy, env):
        return None

    def __add__(self, other):
        return ComposedHook(self, other)


class ComposedHook(EmptyHook):
    """ComposedHook(hooks...)  hooks.jl:37-62"""

    def __init__(self, *hooks):
        self.hooks = list(hooks)

    def push_(self, stage, policy, env):
        for h in self.hooks:
            h.push_(stage, policy, env)


class BatchStepsPerEpisode(EmptyHook):
    """BatchStepsPerEpisode(batchsize)  hooks.jl:202-231 -- vector-env aware; the per-env step counters are
    device tensors, finished episode lengths are pulled to the host only when episodes finish."""

    def __init__(self, batchsize, device="cuda"):
        self.steps = [[] for _ in range(batchsize)]
        self.step = torch.zeros(batchsize, dtype=torch.int64, device=device)

    def push_(self, stage, policy, env):
        if stage != POST_ACT_STAGE:
            return
        self.step += 1
        t = env.is_terminated()
        if bool(t.any()):
            idx = torch.nonzero(t).flatten().tolist()
            vals = self.step[t].tolist()
            for i, v in zip(idx, vals):
                self.steps[i].append(v)
            self.step[t] = 0


class TotalBatchRewardPerEpisode(EmptyHook):
    """TotalRewardPerEpisode (hooks.jl:146-196) for the vector env: running return per instance on the
    device, finished returns appended to `rewards[i]`."""

    def __init__(self, batchsize, device="cuda"):
        self.rewards = [[] for _ in range(batchsize)]
        self.reward = torch.zeros(batchsize, dtype=torch.float64, device=device)

    def push_(self, stage, policy, env):
        if stage != POST_ACT_STAGE:
            return
        self.reward += env.reward().to(torch.float64)
        t = env.is_terminated()
        if bool(t.any()):
            idx = torch.nonzero(t).flatten().tolist()
            vals = self.reward[t].tolist()
            for i, v in zip(idx, vals):
                self.rewards[i].append(v)
            self.reward[t] = 0


class DeviceEpisodeStats(EmptyHook):
    """TotalRewardPerEpisode + BatchStepsPerEpisode (hooks.jl:146-231) with the accumulators and the finished-episode
    log on the device (hooks.hip): `push_` is one kernel launch and never synchronises; `.steps[i]` / `.rewards[i]`
    (lists per env instance, as the reference hooks expose them) are materialised from the device log on access."""

    def __init__(self, batchsize, log_capacity=1 << 20, device="cuda"):
        import numpy as np

        self.n, self.cap, self.vec_step = int(batchsize), int(log_capacity), 0
        self._steps_acc = torch.zeros(self.n, dtype=torch.int32, device=device)
        self._ret_acc = torch.zeros(self.n, dtype=torch.float64, device=device)
        self._log = torch.zeros((self.cap, 3), dtype=torch.int64, device=device)  # 24-byte records
        self._count = torch.zeros(1, dtype=torch.int32, device=device)
        self._np = np

    def push_(self, stage, policy, env):
        if stage != POST_ACT_STAGE:
            return
        from ._lib import call
        from .ops import ptr, stream_ptr

        r = env.reward()
        if r.dtype != torch.float32:
            r = r.to(torch.float32)
        call("rlhip_hook_episode_stats", ptr(r), ptr(env._done), self.n, self.vec_step, ptr(self._steps_acc),
             ptr(self._ret_acc), ptr(self._log), self.cap, ptr(self._count), stream_ptr())
        self.vec_step += 1

    def records(self):
        """finished episodes as a structured numpy array sorted by (vec_step, env)"""
        np = self._np
        count = int(self._count.item())
        if count > self.cap:
            raise OverflowError(f"episode log overflow: {count} episodes finished, capacity {self.cap}")
        dt = np.dtype([("vec_step", np.uint32), ("env", np.uint32), ("steps", np.int32), ("pad", np.int32),
                       ("total_reward", np.float64)])
        rec = self._log[:count].cpu().numpy().view(dt).reshape(-1)
        return np.sort(rec, order=["vec_step", "env"])

    @property
    def steps(self):
        out = [[] for _ in range(self.n)]
        for e, s in zip(self.records()["env"].tolist(), self.records()["steps"].tolist()):
            out[e].append(s)
        return out

    @property
    def rewards(self):
        rec = self.records()
        out = [[] for _ in range(self.n)]
        for e, v in zip(rec["env"].tolist(), rec["total_reward"].tolist()):
            out[e].append(v)
        return out


class StepsPerEpisode(EmptyHook):
    """StepsPerEpisode  hooks.jl:64-101, for a single-instance env (n_envs = 1)."""

    def __init__(self):
        self.steps, self.count = [], 0

    def push_(self, stage, policy, env):
        if stage == POST_ACT_STAGE:
            self.count += 1
            if bool(env.is_terminated()[0]):
                self.steps.append(self.count)
                self.count = 0
        elif stage == POST_EXPERIMENT_STAGE and self.count > 0:
            self.steps.append(self.count)
            self.count = 0


class TimePerStep(EmptyHook):
    """TimePerStep(; max_steps = 100)  hooks.jl:243-262"""

    def __init__(self, max_steps=100):
        self.times, self.max_steps, self.t = [], max_steps, time.time()

    def push_(self, stage, policy, env):
        if stage == POST_ACT_STAGE:
            now = time.time()
            self.times.append(now - self.t)
            self.times = self.times[-self.max_steps:]
            self.t = now


class DoEveryNSteps(EmptyHook):
    """DoEveryNSteps(f; n = 1, t = 0)  hooks.jl:265-290"""

    def __init__(self, f, n=1, t=0):
        self.f, self.n, self.t = f, n, t

    def push_(self, stage, policy, env):
        if stage == POST_ACT_STAGE:
            self.t += 1
            if self.t % self.n == 0:
                self.f(self.t, policy, env)


# ------------------------------------------------------------------------------------ policies
class RandomPolicy:
    """RandomPolicy(action_space; rng)  random_policy.jl:18-32: plan! = rand(rng, action_space).  The draws
    come from the EXPLORE Philox stream (one block per env per call), selection by the eps-greedy kernel
    with eps = 1 (pure random branch)."""

    def __init__(self, action_space=None, seed=0):
        self.action_space, self.seed, self.step = action_space, int(seed), 1
        self._dummy = None

    def plan_(self, env):
        from .ops import eps_greedy_select

        sp = self.action_space or env.action_space()
        step = self.step
        self.step += 1
        if sp.n is None:  # continuous: uniform in the box from the SYNTH stream
            from .ops import fill_uniform

            u = fill_uniform(env.n, self.seed, step, 7, env.device)
            lo, hi = sp.lo[0], sp.hi[0]
            return (u * (hi - lo) + lo).to(env.T)
        if self._dummy is None or self._dummy.shape != (sp.n, env.n):
            self._dummy = torch.zeros((sp.n, env.n), dtype=torch.float32, device=env.device)
        return eps_greedy_select(self._dummy, 1.0, self.seed, step, env.env_id_base) + 1

    def push_(self, stage, env, action=None):
        return None

    def optimise_(self, stage):
        return None


class Agent:
    """Agent(policy, trajectory)  agent_base.jl:18-66 on the vector env: the PreEpisode push of (state,)
    happens once (there are no episode stages; instances auto-reset), PostAct pushes
    (state = s', action, reward, terminal) as ONE batched device push."""

    def __init__(self, policy, trajectory):
        self.policy, self.trajectory = policy, trajectory
        self._started = False

    def plan_(self, env):
        return self.policy.plan_(env)

    def push_(self, stage, env, action=None):
        if stage == PRE_EXPERIMENT_STAGE or (stage == PRE_ACT_STAGE and not self._started):
            if not self._started:
                self.trajectory.push_state_(env.state().to(torch.float32))
                self._started = True
        elif stage == POST_ACT_STAGE:
            a0 = (action - 1).to(torch.int32) if not env.continuous else action
            self.trajectory.push_transition_(env.state().to(torch.float32), a0.contiguous(),
                                             env.reward().to(torch.float32), env._done)

    def optimise_(self, stage):
        if stage == POST_ACT_STAGE and hasattr(self.policy, "optimise_"):
            return self.policy.optimise_(self.trajectory)
        return None


class PPOAgent:
    """Agent(policy = PPOPolicy, trajectory = PPOTrajectory) with the per-step drop-in protocol:
    PreAct push (state, action, action_log_prob), PostAct push (reward, terminal), update every
    `update_freq` vec-steps (blog index.html:15238-15287)."""

    def __init__(self, policy):
        self.policy = policy

    def plan_(self, env):
        return self.policy.plan_(env)

    def push_(self, stage, env, action=None):
        if stage == PRE_ACT_STAGE:
            self.policy.push_preact_(env)
        elif stage == POST_ACT_STAGE:
            self.policy.push_postact_(env)

    def optimise_(self, stage):
        if stage == POST_ACT_STAGE and self.policy.n_pushed == self.policy.T:
            self.policy.finish_rollout_()
            self.policy.update_()


# ----------------------------------------------------------------------------------------- run
def run(policy, env, stop_condition=None, hook=None):
    """run(policy, env, stop_condition, hook) -> hook   (core/run.jl:22-31) for a HipVecEnv.

    `_run(policy, env::HipVecEnv, ...)`: the MultiThreadEnv specialisation -- no episode stages:
        push!(hook/policy, PreExperimentStage)
        loop:  action = plan!(policy, env); push!(policy, PreActStage, env, action); push!(hook, PreActStage)
               act!(env, action)
               push!(policy, PostActStage, env, action); optimise!(policy, PostActStage); push!(hook, PostActStage)
               check!(stop_condition) -> break
        push!(policy/hook, PostExperimentStage)
    """
    stop_condition = stop_condition or StopAfterNSteps(1)
    hook = hook or EmptyHook()
    from .timing import timer as tm  # `@timeit_debug timer "<label>"` of run.jl:46-72, no-ops unless enabled

    hook.push_(PRE_EXPERIMENT_STAGE, policy, env)
    policy.push_(PRE_EXPERIMENT_STAGE, env)
    while True:
        with tm("plan!"):
            action = policy.plan_(env)
        with tm("push!(policy) PreActStage"):
            policy.push_(PRE_ACT_STAGE, env, action)
        with tm("push!(hook) PreActStage"):
            hook.push_(PRE_ACT_STAGE, policy, env)
        with tm("act!"):
            env.act_(action)
        with tm("push!(policy) PostActStage"):
            policy.push_(POST_ACT_STAGE, env, action)
        with tm("optimise! PostActStage"):
            policy.optimise_(POST_ACT_STAGE)
        with tm("push!(hook) PostActStage"):
            hook.push_(POST_ACT_STAGE, policy, env)
        if stop_condition.check_(policy, env):
            break
    policy.push_(POST_EXPERIMENT_STAGE, env)
    hook.push_(POST_EXPERIMENT_STAGE, policy, env)
    return hook


def _refuse_sac(policy, loop):
    """the fused vec-steps are DQN's: a SACPolicy runs on the per-stage loop"""
    if type(policy).__name__ == "SACPolicy":
        raise NotImplementedError(f"{loop}: a fused vec-step for SACPolicy is out of scope; use the per-stage loop, rlhip.run")
    if hasattr(getattr(policy, "learner", None), "plan_distributional_"):
        # (the vec-step kernels plan on scalar Q-values and train on Huber(TD))
        if type(policy.learner).__name__ == "QRDQNLearner":
            raise NotImplementedError(f"{loop}: a fused vec-step for QRDQNLearner (quantiles of the value distribution per action) is "
                                      "out of scope; use the per-stage loop, rlhip.run")
        raise NotImplementedError(f"{loop}: a fused vec-step for RainbowLearner (a categorical value distribution per action) is out "
                                  "of scope; use the per-stage loop, rlhip.run")


def run_fused_dqn(agent, env, stop_condition=None, hook=None):
    """`run(agent, env, stop, hook)` for Agent{QBasedPolicy{DQNLearner}} on a HipVecEnv with the whole loop body
    (plan! -> act! -> push! -> optimise!) as ONE C-ABI call per vec-step (rlhip_dqn_vec_step_f32).  Same kernels,
    same order, same counters as `run`: parameters, trajectory and explorer state end bit-identical
    (tests/test_gpu_run.py).  Hooks see the PostAct stage of every step."""
    from . import _lib

    policy, traj = agent.policy, agent.trajectory
    _refuse_sac(policy, "run_fused_dqn")
    learner, ex = policy.learner, policy.explorer
    tn = learner.approximator
    net = tn.network
    traces = traj.container
    if ex.is_break_tie or env.continuous or env.is_f64 or hasattr(traces, "sample_prioritized") \
            or learner.process_group is not None or getattr(learner, "n_step", 1) != 1 or getattr(learner, "double_dqn", False):
        raise NotImplementedError("fused DQN step: plain eps-greedy, Float32 discrete env, uniform 1-step replay, 1 GPU, "
                                  "plain DQN targets (double_dqn=True runs on the per-stage loop)")
    if getattr(net, "dueling_params", None) is not None:
        # the fused vec-step steps Adam on the vector its kernels read; a dueling net trains another vector than the one they read
        raise NotImplementedError("fused DQN step: plain Q-networks only; a DuelingApproximator (dueling_params) runs on the "
                                  "per-stage loop, rlhip.run")
    _refuse_wide_obs(net, "fused DQN step")
    a = _lib.DqnStepArgs()
    stop_condition, hook = _fused_dqn_begin(agent, env, stop_condition, hook, a)
    # the gate is should_update_ itself, on the transitions the step's push leaves
    return _fused_dqn_steps(agent, env, stop_condition, hook, "rlhip_dqn_vec_step_f32", a, a, learner.should_update_, traces.n_env)


def _refuse_wide_obs(net, loop):
    """the fused vec-steps read record rings (observations of 2..4 components); wider observations train on the per-stage loop"""
    if getattr(net, "n_in", 0) > 4:
        raise NotImplementedError(f"{loop}: observations of 2..4 components; a Q-network on {net.n_in} components (n_in > 4, e.g. "
                                  "AcrobotRK4Env) runs on the per-stage loop, rlhip.run")


def _fused_dqn_begin(agent, env, stop_condition, hook, a):
    """what both fused DQN loops do once their admission checks have passed: the PreExperiment pushes, the policy's action / Q buffers
    and the rlhip_dqn_step_args fields that stay fixed over the run -> (stop_condition, hook) with their defaults"""
    import ctypes as C

    from .ops import ptr

    policy, traces = agent.policy, agent.trajectory.container
    learner, ex = policy.learner, policy.explorer
    tn = learner.approximator
    net = tn.network
    stop_condition = stop_condition or StopAfterNSteps(1)
    hook = hook or EmptyHook()
    hook.push_(PRE_EXPERIMENT_STAGE, agent, env)
    agent.push_(PRE_EXPERIMENT_STAGE, env)
    if policy._actions is None:
        policy._actions = torch.empty(env.n, dtype=torch.int32, device=env.device)
        policy._q = torch.empty((net.n_out, env.n), dtype=torch.float32, device=env.device)
    a.kind, a.env_cfg, a.st, a.n = env.kind, C.addressof(env.cfg), C.addressof(env._st), env.n
    a.env_seed, a.env_id_base = env.seed, env.env_id_base
    a.obs, a.last_obs = ptr(env.state()), ptr(env._last_obs)
    a.ring = C.addressof(traces.rb)
    a.layers, a.h, a.na, a.act = net.layers, net.hidden, net.n_out, net.act
    a.params, a.target = ptr(net.params), ptr(tn.target)
    a.packed = ptr(net.packed) if net.layers == 3 else None
    a.target_packed = ptr(tn.target_packed) if net.layers == 3 else None
    a.m, a.v, a.beta_pow = ptr(net.m), ptr(net.v), ptr(net.beta_pow)
    a.lr, a.beta1, a.beta2, a.adam_eps = net.lr, net.beta1, net.beta2, net.eps
    a.max_grad_norm, a.grad_scale = learner.max_grad_norm, 1.0
    a.explorer_seed, a.batch, a.gamma, a.huber_delta = ex.seed, learner.batchsize, learner.gamma, learner.delta
    a.sampler_seed, a.rho = learner.seed, tn.rho
    a.workspace, a.grad, a.loss, a.gn = ptr(learner.workspace), ptr(learner.grad), ptr(learner.loss), ptr(net.gn)
    a.actions, a.q = ptr(policy._actions), ptr(policy._q)
    return stop_condition, hook


def _fused_dqn_steps(agent, env, stop_condition, hook, name, args, a, gate, per_step, before_call=None):
    """the loop of every fused DQN form and its epilogue: one call of `name` per vec-step on `args` (passed by reference), whose
    rlhip_dqn_step_args part `a` receives the per-step fields.  `gate(trajectory, count)` is `do_update`, asked with `per_step` times
    the number of vec-steps the trajectory holds once the step's push has happened (per_step = n_env: the gate counts transitions);
    it advances the learner's vec-step counter.  `before_call()`, when given, sets a form's own per-step fields once those of `a`
    are in place."""
    import ctypes as C

    from ._lib import call
    from .ops import stream_ptr

    traj = agent.trajectory
    learner, ex = agent.policy.learner, agent.policy.explorer
    tn = learner.approximator
    traces, ctrl = traj.container, traj.controller
    s = stream_ptr()
    while True:
        a.eps, a.explorer_step = ex.get_eps(), ex.step
        ex.step += 1
        # the transition pushed by this call counts towards min_replay_history / the sample-ratio controller / the n-step guard
        ctrl.on_insert_(1)
        a.do_update = int(gate(traj, min(len(traces) + 1, traces.capacity) * per_step))  # warm-up, update_freq, sample / insert controller
        a.draw_ctr = learner.draw_ctr
        a.do_sync = int(a.do_update and (tn.n_optimise + 1) % tn.sync_freq == 0)
        if before_call is not None:
            before_call()
        call(name, C.byref(args), s)
        if a.do_update:
            learner.draw_ctr += 1
            learner.n_updates += 1
            tn.n_optimise = 0 if a.do_sync else tn.n_optimise + 1
        hook.push_(POST_ACT_STAGE, agent, env)
        if stop_condition.check_(agent, env):
            break
    env._obs_valid = True
    agent.push_(POST_EXPERIMENT_STAGE, env)
    hook.push_(POST_EXPERIMENT_STAGE, agent, env)
    return hook


def _folded_update_gate(learner, trajectory, len_after):
    """`do_update` of one fused vec-step for a learner with folded batches: DQNLearner.optimise_'s gate on the trajectory as the
    step's push leaves it (`len_after` stored vec-steps).  While fewer than n_step steps are stored the vec-step counts, the
    controller is not asked and no draw counter moves -- the per-stage learner's n-step guard."""
    if getattr(learner, "_nstep", None) is not None and len_after < learner.n_step:
        learner.vec_steps += 1
        return False
    return bool(learner.should_update_(trajectory, len_after * trajectory.container.n_env))


def _folded_scratch(learner, traces, net):
    """(folded ring, idx, iota, fold workspace or None): the scratch DQNLearner makes with its first folded update -- owned by the
    same NStepBatchSampler / DoubleTargetFold objects, so a later rlhip.run on the agent finds what it would have made itself"""
    from .trajectory import folded_scratch

    b, dev = learner.batchsize, traces.state.device
    double = learner._double_fold() if learner.double_dqn else None
    folded, iota = folded_scratch(learner._nstep if learner._nstep is not None else double, traces, b)
    idx = torch.empty(b, dtype=torch.int64, device=dev)
    if double is None:
        return folded, idx, iota, None
    # the per-stage Double DQN update leaves the indices its fold took in `_idx`: the draw, or the n-step iota
    learner._idx = idx if learner._nstep is None else iota
    if learner._nstep is not None:
        double.own_iota(b, dev)  # the in-place fold's index vector of the per-stage loop
    return folded, idx, iota, double.workspace(net, b, dev)


def run_fused_dqn_folded(agent, env, stop_condition=None, hook=None):
    """`run_fused_dqn` for learners whose batches are folded: DQNLearner(n_step > 1), DQNLearner(double_dqn = True), a
    DuelingApproximator, any combination -- and the plain learner.  The whole loop body is ONE C-ABI call per vec-step
    (rlhip_dqn_vec_step_fold_f32): the kernels, their order and the counters are those of `run`, so parameters, optimiser state,
    trajectory and explorer end bit-identical to the per-stage loop (tests/test_gpu_fused_folds.py) and either loop may continue
    the other.  Prioritized traces run on run_fused_dqn_prioritized; tie-breaking explorers, continuous / Float64 envs and a process
    group stay on `run`."""
    import ctypes as C

    from . import _lib
    from .ops import ptr

    policy, traj = agent.policy, agent.trajectory
    _refuse_sac(policy, "run_fused_dqn_folded")
    learner, ex = policy.learner, policy.explorer
    tn = learner.approximator
    net = tn.network
    traces = traj.container
    if hasattr(traces, "sample_prioritized"):
        raise NotImplementedError("fused folded DQN step: uniform replay only; prioritized traces (CircularPrioritizedTraces) run "
                                  "on rlhip.run_fused_dqn_prioritized or the per-stage loop, rlhip.run")
    if ex.is_break_tie:
        raise NotImplementedError("fused folded DQN step: plain eps-greedy only; a tie-breaking explorer (is_break_tie) runs on the "
                                  "per-stage loop, rlhip.run")
    if env.continuous or env.is_f64:
        raise NotImplementedError("fused folded DQN step: Float32 discrete envs only; a continuous or Float64 env runs on the "
                                  "per-stage loop, rlhip.run")
    if learner.process_group is not None:
        raise NotImplementedError("fused folded DQN step: 1 GPU; a learner with a process group (process_group) runs on the "
                                  "per-stage loop, rlhip.run")
    _refuse_wide_obs(net, "fused folded DQN step")
    n_step, double = int(getattr(learner, "n_step", 1)), bool(getattr(learner, "double_dqn", False))
    dueling = getattr(net, "dueling_params", None) is not None
    f = _lib.DqnFoldStepArgs()
    stop_condition, hook = _fused_dqn_begin(agent, env, stop_condition, hook, f.base)
    f.n_step, f.double_dqn, f.td = n_step, int(double), ptr(learner.td)
    if n_step > 1 or double:
        folded, idx, iota, ws = _folded_scratch(learner, traces, net)
        f.folded, f.idx, f.iota = C.addressof(folded.rb), ptr(idx), ptr(iota)
        f.fold_workspace = ptr(ws) if ws is not None else None
    if dueling:
        f.dueling_params, f.target_dueling, f.grad_dueling = ptr(net.dueling_params), ptr(tn.target_dueling), ptr(net._grad.t)
    return _fused_dqn_steps(agent, env, stop_condition, hook, "rlhip_dqn_vec_step_fold_f32", f, f.base,
                            functools.partial(_folded_update_gate, learner), 1)


class _PerStepScratch:
    """the fused prioritized step's own buffers on a learner, rewritten in full by every update (rlhip/checkpoint.py leaves them out)"""
    checkpoint_scratch = True

    def __init__(self, batch, device):
        self.batch = batch
        self.td_raw = torch.zeros(batch, dtype=torch.float32, device=device)  # |Q(s,a) - y|: the write-back's input
        self.idx = torch.empty(batch, dtype=torch.int64, device=device)
        self.key = torch.empty(batch, dtype=torch.int64, device=device)
        self.prio = torch.empty(batch, dtype=torch.float32, device=device)


def run_fused_dqn_prioritized(agent, env, stop_condition=None, hook=None):
    """`run_fused_dqn_folded` for learners over prioritized replay: DQNLearner on CircularPrioritizedTraces, 1-step or n-step, plain or
    Double DQN targets, plain or dueling nets, with or without importance-sampling weights (`per_beta`, a number or a callable
    n_updates -> beta).  The whole loop body is ONE C-ABI call per vec-step (rlhip_dqn_vec_step_per_f32), with the priority power and
    the sum-tree write-back as one launch (rlhip_per_writeback_f32): the kernels, their order and the counters are those of `run`, so
    parameters, optimiser state, trajectory, sum-tree and explorer end bit-identical to the per-stage loop
    (tests/test_gpu_fused_per.py) and either loop may continue the other.  `learner.td` holds the written-back priorities, as the
    per-stage learner leaves them.  Uniform traces run on run_fused_dqn_folded; tie-breaking explorers, continuous / Float64 envs
    and a process group stay on `run`."""
    import ctypes as C

    from . import _lib
    from .ops import ptr

    policy, traj = agent.policy, agent.trajectory
    _refuse_sac(policy, "run_fused_dqn_prioritized")
    learner, ex = policy.learner, policy.explorer
    tn = learner.approximator
    net = tn.network
    traces = traj.container
    if not hasattr(traces, "sample_prioritized"):
        raise NotImplementedError("fused prioritized DQN step: prioritized traces (CircularPrioritizedTraces) only; uniform replay runs "
                                  "on rlhip.run_fused_dqn_folded")
    if ex.is_break_tie:
        raise NotImplementedError("fused prioritized DQN step: plain eps-greedy only; a tie-breaking explorer (is_break_tie) runs on "
                                  "the per-stage loop, rlhip.run")
    if env.continuous or env.is_f64:
        raise NotImplementedError("fused prioritized DQN step: Float32 discrete envs only; a continuous or Float64 env runs on the "
                                  "per-stage loop, rlhip.run")
    if learner.process_group is not None:
        raise NotImplementedError("fused prioritized DQN step: 1 GPU; a learner with a process group (process_group) runs on the "
                                  "per-stage loop, rlhip.run")
    n_step, double = int(getattr(learner, "n_step", 1)), bool(getattr(learner, "double_dqn", False))
    if getattr(traces, "n_step", 1) != n_step:
        raise ValueError(f"DQNLearner(n_step = {n_step}) needs CircularPrioritizedTraces(..., n_step = {n_step}): "
                         f"these traces mask windows of {getattr(traces, 'n_step', 1)}")
    _refuse_wide_obs(net, "fused prioritized DQN step")
    dueling = getattr(net, "dueling_params", None) is not None
    p = _lib.DqnPerStepArgs()
    f = p.fold
    stop_condition, hook = _fused_dqn_begin(agent, env, stop_condition, hook, f.base)
    b, dev = learner.batchsize, traces.state.device
    sc = getattr(learner, "_per_step", None)
    if sc is None or sc.batch != b or sc.td_raw.device != dev:
        sc = learner._per_step = _PerStepScratch(b, dev)
    idx, key, prio = sc.idx, sc.key, sc.prio
    if n_step > 1 or double:
        folded, fidx, iota, ws = _folded_scratch(learner, traces, net)
        f.folded, f.iota = C.addressof(folded.rb), ptr(iota)
        f.fold_workspace = ptr(ws) if ws is not None else None
    if n_step > 1:  # the draw buffers of NStepBatchSampler.sample_fold_prioritized: the per-stage learner leaves all three on itself
        smp = learner._nstep
        if smp._draw is None or smp._draw[0].numel() != b or smp._draw[0].device != dev:
            smp._draw = (idx, key, prio)
        idx, key, prio = smp._draw
        smp.key, smp.priority = key, prio
        learner._idx = idx
    elif double:  # the indices the Double DQN fold took
        learner._idx = idx = fidx
    learner._key, learner._prio = key, prio
    f.n_step, f.double_dqn, f.td, f.idx = n_step, int(double), ptr(sc.td_raw), ptr(idx)
    if dueling:
        f.dueling_params, f.target_dueling, f.grad_dueling = ptr(net.dueling_params), ptr(tn.target_dueling), ptr(net._grad.t)
    p.tree, p.default_priority = ptr(traces.priorities), traces.default_priority
    p.per_eps, p.per_alpha = learner.per_eps, learner.per_alpha
    p.key, p.prio, p.is_weights, p.priority_out = ptr(key), ptr(prio), ptr(learner.is_weights), ptr(learner.td)

    def per_step_fields():  # _is_weights_'s beta for the update this step makes: a schedule is asked once per update, as there
        if f.base.do_update:
            beta = float(learner.per_beta(learner.n_updates)) if callable(learner.per_beta) else float(learner.per_beta)
            p.per_beta = beta if beta > 0.0 else 0.0

    return _fused_dqn_steps(agent, env, stop_condition, hook, "rlhip_dqn_vec_step_per_f32", p, f.base,
                            functools.partial(_folded_update_gate, learner), 1, per_step_fields)


def run_fused_ppo(policy, env, n_updates, hook=None):
    """The same loop with the T-step rollout fused into one launch per update period (hooks see one
    PostActStage per period with the LAST step's reward / terminal flags)."""
    hook = hook or EmptyHook()
    hook.push_(PRE_EXPERIMENT_STAGE, policy, env)
    for _ in range(n_updates):
        policy.rollout_(env)
        policy.update_()
        hook.push_(POST_ACT_STAGE, policy, env)
    hook.push_(POST_EXPERIMENT_STAGE, policy, env)
    return hook
