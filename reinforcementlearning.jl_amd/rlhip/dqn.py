"""QBasedPolicy / DQN learner / explorers / approximators on the vectorised env (host mirror).

Reference surface mirrored here:
    QBasedPolicy            src/ReinforcementLearningCore/src/policies/q_based_policy.jl:13-49
    EpsilonGreedyExplorer   .../policies/explorers/epsilon_greedy_explorer.jl:38-131 (GreedyExplorer :200-214)
    FluxApproximator        .../policies/learners/flux_approximator.jl:11-46
    TargetNetwork           .../policies/learners/target_network.jl:27-88
    BasicDQN/DQN learner    removed Zoo; spec docs/src/rlcore.md:28 and the blog config
                            docs/homepage/blog/a_practical_introduction_to_RL.jl/index.html:15121-15147
All numerics are HIP kernels behind the C ABI (dqn.hip, select.hip, optim.hip).
"""
import ctypes as C

import torch

from . import _lib
from ._lib import call
from .ops import ptr, stream_ptr


# ----------------------------------------------------------------------------- functional layer
def dqn_workspace(ns, h, na, batch, device="cuda"):
    nbytes = int(_lib.lib.rlhip_dqn_workspace_bytes(ns, h, na, batch))
    return torch.zeros(nbytes, dtype=torch.uint8, device=device)  # zeroed: the tail holds rlhip_dqn_update_f32's counters


def dqn_update(traces, h, na, act, params, target_params, batch, gamma, delta, seed, draw_ctr, workspace, grad, loss, m, v,
               beta_pow, grad_scale, max_grad_norm, lr, beta1, beta2, eps, gn=None):
    """optimise!(learner, batch) in place: ONE launch up to 2048 samples (gradient; the workgroup that departs last reduces, clips, steps), two beyond."""
    call("rlhip_dqn_update_f32", C.byref(traces.rb), h, na, act, ptr(params), ptr(target_params), batch, gamma, delta,
         seed, draw_ctr, ptr(workspace), ptr(grad), ptr(loss), ptr(m), ptr(v), ptr(beta_pow), grad_scale, max_grad_norm,
         lr, beta1, beta2, eps, ptr(gn) if gn is not None else None, stream_ptr())
    return grad, loss


def dqn_grad(traces, h, na, act, params, target_params, batch, gamma, delta, seed, draw_ctr, workspace=None,
             grad=None, loss=None):
    """One DQN learner step up to the gradient: sample `batch` transitions, TD target, Huber, backward."""
    dev = params.device
    workspace = workspace if workspace is not None else dqn_workspace(traces.obs_dim, h, na, batch, dev)
    grad = grad if grad is not None else torch.empty_like(params)
    loss = loss if loss is not None else torch.empty(1, dtype=torch.float32, device=dev)
    call("rlhip_dqn_grad_f32", C.byref(traces.rb), h, na, act, ptr(params), ptr(target_params), batch, gamma,
         delta, seed, draw_ctr, ptr(workspace), ptr(grad), ptr(loss), stream_ptr())
    return grad, loss


def dqn_plan(params, ns, h, na, act, obs, eps, seed, env_id_base, step, actions=None, q_out=None):
    """plan!(QBasedPolicy, env): Q forward + eps-greedy for n envs; returns (0-based actions, q (na, n))."""
    n = obs.shape[1]
    actions = actions if actions is not None else torch.empty(n, dtype=torch.int32, device=obs.device)
    q_out = q_out if q_out is not None else torch.empty((na, n), dtype=torch.float32, device=obs.device)
    call("rlhip_dqn_plan_f32", ptr(params), ns, h, na, act, ptr(obs), n, float(eps), seed, env_id_base, step,
         ptr(actions), ptr(q_out), stream_ptr())
    return actions, q_out


MAX_WIDE_OBS = 16  # the widest observation the two-layer DQN kernels take (csrc/dqn_batch.hip); 2..4 components: csrc/dqn.hip


def check_wide_net(net, who):
    """the refusals for a Q-network on more than four observation components, raised before any C call"""
    if net.n_in > MAX_WIDE_OBS:
        raise ValueError(f"{who}: the DQN kernels take observations of up to {MAX_WIDE_OBS} Float32 components, this network has "
                         f"n_in = {net.n_in}; images and stacked frames need a convolutional network, which this library does not have")
    if getattr(net, "layers", 2) == 3:
        raise NotImplementedError(f"{who}: three-layer (bf16 MFMA) networks take observations of 2..4 components; with n_in = {net.n_in} "
                                  "use a two-layer HipApproximator / DuelingApproximator (layers = 2)")


def dqn_plan_obsn(params, ns, h, na, act, obs, eps, seed, env_id_base, step, actions=None, q_out=None):
    """`dqn_plan` for observations of 5..16 components (rlhip_dqn_plan_obsn_f32): byte for byte `mlp2_forward` then `eps_greedy_select`"""
    n = obs.shape[1]
    actions = actions if actions is not None else torch.empty(n, dtype=torch.int32, device=obs.device)
    q_out = q_out if q_out is not None else torch.empty((na, n), dtype=torch.float32, device=obs.device)
    call("rlhip_dqn_plan_obsn_f32", ptr(params), ns, h, na, act, ptr(obs), n, float(eps), seed, env_id_base, step,
         ptr(actions), ptr(q_out), stream_ptr())
    return actions, q_out


def dqn_batch_workspace(ns, h, na, batch, device="cuda"):
    nbytes = int(_lib.lib.rlhip_dqn_batch_workspace_bytes(ns, h, na, batch))
    if nbytes < 0:
        raise ValueError(f"rlhip_dqn_grad_batch_f32 takes ns 5..16, hidden a multiple of 4 and <= 256, 1..4 actions, batch >= 1; "
                         f"got ns = {ns}, hidden = {h}, actions = {na}, batch = {batch}")
    return torch.empty(nbytes, dtype=torch.uint8, device=device)


def dqn_grad_batch(ns, h, na, act, params, target_params, s, a, r, term, s_next, gamma, delta=1.0, n_used=None, weights=None,
                   double_dqn=False, workspace=None, grad=None, loss=None, td=None):
    """loss and gradient of the two-layer Q-network on a gathered batch (s / s_next (ns, batch), as `traces.gather` returns them
    from a frame ring) -> (grad, loss).  n_used: the transitions each n-step window used (discount gamma ** n_used[b]); weights:
    importance-sampling weights; td (batch,): |Q(s, a) - y| per sample."""
    dev, b = params.device, a.numel()
    workspace = workspace if workspace is not None else dqn_batch_workspace(ns, h, na, b, dev)
    grad = grad if grad is not None else torch.empty_like(params)
    loss = loss if loss is not None else torch.empty(1, dtype=torch.float32, device=dev)
    if term.dtype == torch.bool:
        term = term.view(torch.uint8)
    call("rlhip_dqn_grad_batch_f32", ns, h, na, act, ptr(params), ptr(target_params), ptr(s), ptr(a), ptr(r), ptr(term), ptr(s_next), b,
         gamma, None if n_used is None else ptr(n_used), None if weights is None else ptr(weights), int(bool(double_dqn)), delta,
         ptr(workspace), ptr(grad), ptr(loss), None if td is None else ptr(td), stream_ptr())
    return grad, loss


def mlp3_init(ns, h, na, seed, net_id=0, device="cuda"):
    p = torch.empty(int(_lib.lib.rlhip_mlp3_nparams(ns, h, na)), dtype=torch.float32, device=device)
    call("rlhip_mlp3_init_f32", ptr(p), ns, h, na, seed, net_id, stream_ptr())
    return p


def mlp3_pack(params, ns, h, na, packed=None):
    """bf16 copies of W2 in both MFMA operand orders (refresh after every parameter update)."""
    if packed is None:
        packed = torch.empty(int(_lib.lib.rlhip_mlp3_packed_elems(h)), dtype=torch.int16, device=params.device)
    call("rlhip_mlp3_pack_bf16", ptr(params), ns, h, na, ptr(packed), stream_ptr())
    return packed


def dqn3_plan(params, packed, ns, h, na, act, obs, eps=0.0, seed=0, env_id_base=0, step=0, actions=None, q_out=None,
              want_actions=True):
    n = obs.shape[1]
    if want_actions and actions is None:
        actions = torch.empty(n, dtype=torch.int32, device=obs.device)
    q_out = q_out if q_out is not None else torch.empty((na, n), dtype=torch.float32, device=obs.device)
    call("rlhip_dqn3_plan_f32", ptr(params), ptr(packed), ns, h, na, act, ptr(obs), n, float(eps), seed, env_id_base,
         step, ptr(actions) if want_actions else None, ptr(q_out), stream_ptr())
    return actions, q_out


def dqn3_workspace(ns, h, na, batch, device="cuda"):
    # zeroed: the tail holds rlhip_dqn3_update_f32's counters
    return torch.zeros(int(_lib.lib.rlhip_dqn3_workspace_bytes(ns, h, na, batch)), dtype=torch.uint8, device=device)


def dqn3_update(traces, h, na, act, params, packed, target_params, target_packed, batch, gamma, delta, seed, draw_ctr,
                workspace, grad, loss, m, v, beta_pow, grad_scale, max_grad_norm, lr, beta1, beta2, eps, gn=None):
    """optimise!(learner, batch) of the 3-layer learner in two launches (params, moments, packed updated in place)."""
    call("rlhip_dqn3_update_f32", C.byref(traces.rb), h, na, act, ptr(params), ptr(packed), ptr(target_params),
         ptr(target_packed), batch, gamma, delta, seed, draw_ctr, ptr(workspace), ptr(grad), ptr(loss), ptr(m), ptr(v),
         ptr(beta_pow), grad_scale, max_grad_norm, lr, beta1, beta2, eps, ptr(gn) if gn is not None else None,
         stream_ptr())
    return grad, loss


def dqn3_grad(traces, h, na, act, params, packed, target_params, target_packed, batch, gamma, delta, seed, draw_ctr,
              idx=None, workspace=None, grad=None, loss=None, td=None):
    dev = params.device
    workspace = workspace if workspace is not None else dqn3_workspace(traces.obs_dim, h, na, batch, dev)
    grad = grad if grad is not None else torch.empty_like(params)
    loss = loss if loss is not None else torch.empty(1, dtype=torch.float32, device=dev)
    call("rlhip_dqn3_grad_f32", C.byref(traces.rb), h, na, act, ptr(params), ptr(packed), ptr(target_params),
         ptr(target_packed), batch, None if idx is None else ptr(idx), gamma, delta, seed, draw_ctr, ptr(workspace),
         ptr(grad), ptr(loss), None if td is None else ptr(td), stream_ptr())
    return grad, loss


# ----------------------------------------------------------------------------------- explorers
class EpsilonGreedyExplorer:
    """EpsilonGreedyExplorer(; ϵ_stable, kind = :linear, ϵ_init = 1.0, warmup_steps = 0, decay_steps = 0,
    step = 1, is_break_tie = false, rng) -- epsilon_greedy_explorer.jl:38-67.  One `step` per call, shared
    by all N lanes of a vector env (the historical `policy(env)` was a single call per vec-step)."""

    def __init__(self, eps_stable, kind="linear", eps_init=1.0, warmup_steps=0, decay_steps=0, step=1,
                 is_break_tie=False, seed=0):
        if kind not in ("linear", "exp"):
            raise ValueError("kind must be 'linear' or 'exp'")
        self.eps_stable, self.kind, self.eps_init = float(eps_stable), kind, float(eps_init)
        self.warmup_steps, self.decay_steps, self.step = int(warmup_steps), int(decay_steps), int(step)
        self.is_break_tie, self.seed = bool(is_break_tie), int(seed)

    def get_eps(self, step=None):
        """get_ϵ(s[, step])  :69-90"""
        step = self.step if step is None else step
        return _lib.lib.rlhip_get_eps(0 if self.kind == "linear" else 1, self.eps_stable, self.eps_init,
                                      self.warmup_steps, self.decay_steps, step)

    def plan_(self, values, mask=None, env_id_base=0):
        """plan!(s, values[, mask]) for a (na, N) device tensor of values -> 1-based actions."""
        from .ops import eps_greedy_select

        eps = self.get_eps()
        step = self.step
        self.step += 1  # :104,:110 -- incremented on every call, before the draw
        a0 = eps_greedy_select(values, eps, self.seed, step, env_id_base, mask, self.is_break_tie)
        return a0 + 1


    def prob(self, values, mask=None):
        """prob(s, values[, mask])  :141-194 -- the Float64 probability of every action of every env, (na, N) like `values`
        (the reference returns `Categorical(probs)` per env; the step counter does not advance)."""
        from .ops import eps_greedy_prob

        return eps_greedy_prob(values, self.get_eps(), mask, self.is_break_tie)


class GreedyExplorer(EpsilonGreedyExplorer):
    """GreedyExplorer()  :200-214 -- findmax first-index rule, no randomness."""

    def __init__(self):
        super().__init__(0.0)

    def get_eps(self, step=None):
        return 0.0


# -------------------------------------------------------------------------------- approximators
class HipApproximator:
    """FluxApproximator(model = Chain(Dense(ns, h, act), Dense(h, n_out)), optimiser = Adam(lr)).
    Flat parameters in Flux.destructure order + Adam state, all in HBM."""

    def __init__(self, n_in, hidden, n_out, act="relu", lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, seed=0,
                 net_id=0, device="cuda", params=None, layers=2):
        """layers = 3: Chain(Dense(n_in, h, act), Dense(h, h, act), Dense(h, n_out)) -- the blog's DQN model; the
        hidden x hidden layer runs in bf16 on the MFMA (dqn3.hip at hidden = 128, the streaming kernels of ppo3w.hip at 256)."""
        if layers not in (2, 3):
            raise ValueError("layers must be 2 or 3")
        self.n_in, self.hidden, self.n_out, self.layers = n_in, hidden, n_out, layers
        self.act = {"relu": 0, "tanh": 1}[act] if isinstance(act, str) else int(act)
        self.lr, self.beta1, self.beta2, self.eps = lr, beta1, beta2, eps
        from .ops import mlp2_init

        init = mlp2_init if layers == 2 else mlp3_init
        self.params = init(n_in, hidden, n_out, seed, net_id, device) if params is None else \
            torch.as_tensor(params, dtype=torch.float32, device=device).clone()
        self.packed = mlp3_pack(self.params, n_in, hidden, n_out) if layers == 3 else None
        self.m = torch.zeros_like(self.params)
        self.v = torch.zeros_like(self.params)
        self.beta_pow = torch.tensor([beta1, beta2], dtype=torch.float32, device=device)
        self.gn = torch.zeros(1, dtype=torch.float32, device=device)

    def forward(self, x):
        """forward(A, x) = A.model(x)  (flux_approximator.jl:43): x (n_in, batch) -> (n_out, batch)."""
        from .ops import mlp2_forward

        if self.layers == 3:
            return dqn3_plan(self.params, self.packed, self.n_in, self.hidden, self.n_out, self.act, x,
                             want_actions=False)[1]
        return mlp2_forward(self.params, self.n_in, self.hidden, self.n_out, self.act, x)

    def optimise_(self, grad, clip_norm=0.0, grad_scale=1.0):
        """optimise!(A, grad) = Flux.Optimise.update!(A.optimiser_state, A.model, grad)  (:46)."""
        from .ops import clip_adam_

        clip_adam_(self.params, grad, self.m, self.v, self.beta_pow, grad_scale, clip_norm, self.lr, self.beta1,
                   self.beta2, self.eps, self.gn)
        if self.layers == 3:
            mlp3_pack(self.params, self.n_in, self.hidden, self.n_out, self.packed)


def dueling_nparams(n_in, h, n_out, layers=2):
    return int(_lib.lib.rlhip_dueling_nparams(n_in, h, n_out, layers))


def fold_dueling(duel, eff, n_in, h, n_out, layers, duel2=None, eff2=None):
    """dueling vector(s) -> effective plain vector(s), one launch (csrc/dueling.hip); the second pair is the target net"""
    call("rlhip_dueling_fold_f32", ptr(duel), ptr(eff), ptr(duel2), ptr(eff2), n_in, h, n_out, layers, stream_ptr())
    return eff


def unfold_dueling_grad(grad_eff, grad_duel, n_in, h, n_out, layers):
    """gradient of the effective plain vector -> gradient of the dueling vector (chain rule of the fold), one launch"""
    call("rlhip_dueling_unfold_grad_f32", ptr(grad_eff), ptr(grad_duel), n_in, h, n_out, layers, stream_ptr())
    return grad_duel


class _Scratch:
    """a buffer rewritten in full before every use: not state of the path (rlhip/checkpoint.py leaves it out)"""
    checkpoint_scratch = True

    def __init__(self, t):
        self.t = t


class DuelingApproximator(HipApproximator):
    """FluxApproximator(model = DuelingNetwork(base, val, adv), optimiser = Adam(lr))  RLCore/src/utils/networks.jl:510-522, with
    `val = Dense(h, 1)` and `adv = Dense(h, n_out)`:  Q = val .+ adv .- mean(adv, dims = 1).

    `.dueling_params` is the trained vector, [plain layout with (Wadv, badv) as its last Dense | Wval (h) | bval (1)]; `.m` / `.v`
    have its length.  `.params` is the EFFECTIVE plain vector (rlhip_dueling_fold_f32) -- the one every kernel reads: plan, act,
    gradient and the Double DQN fold run unchanged, and DQNLearner / QBasedPolicy / DoubleTargetFold need no edit.  optimise_ maps
    the plain gradient back (rlhip_dueling_unfold_grad_f32), steps clip + Adam on the dueling vector (the global norm is the dueling
    gradient's, as Flux would take it) and folds again.

    A fresh val head is Glorot-uniform for Dense(h, 1), bias 0: Wval[j] = (2 u_j - 1) sqrt(6 / (h + 1)) with u from
    rlhip_fill_uniform_f32(seed, t = net_id * 4 + 3, tag = 6 (INIT)) -- tensor id 3 of the net, beside the ids 0..2 that
    rlhip_mlp2_init_f32 / rlhip_mlp3_init_f32 use.  `params` (a plain vector) seeds base and adv; `dueling_params` is the whole vector."""

    def __init__(self, n_in, hidden, n_out, act="relu", lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, seed=0,
                 net_id=0, device="cuda", params=None, layers=2, dueling_params=None):
        if layers not in (2, 3):
            raise ValueError("layers must be 2 or 3")
        if not 1 <= n_out <= 4:
            raise ValueError("the dueling fold takes 1..4 actions")
        nd = dueling_nparams(n_in, hidden, n_out, layers)
        if dueling_params is not None:
            if params is not None:
                raise ValueError("give params (a plain vector: base and adv) or dueling_params (the whole vector), not both")
            duel = torch.as_tensor(dueling_params, dtype=torch.float32, device=device).clone()
            if duel.numel() != nd:
                raise ValueError(f"dueling_params has {duel.numel()} elements, the network {nd}")
            params = duel[:nd - hidden - 1]  # the constructor below copies it; overwritten by the fold
        super().__init__(n_in, hidden, n_out, act, lr, beta1, beta2, eps, seed, net_id, device, params, layers)
        if dueling_params is None:
            from .ops import fill_uniform

            wval = (2.0 * fill_uniform(hidden, seed, net_id * 4 + 3, 6, device) - 1.0) * float((6.0 / (hidden + 1)) ** 0.5)
            duel = torch.cat([self.params, wval, torch.zeros(1, dtype=torch.float32, device=device)])
        self.dueling_params = duel.contiguous()
        self.m = torch.zeros_like(self.dueling_params)
        self.v = torch.zeros_like(self.dueling_params)
        self._grad = _Scratch(torch.zeros_like(self.dueling_params))
        self.refold_()

    def refold_(self):
        """.params (and .packed) from .dueling_params"""
        fold_dueling(self.dueling_params, self.params, self.n_in, self.hidden, self.n_out, self.layers)
        if self.layers == 3:
            mlp3_pack(self.params, self.n_in, self.hidden, self.n_out, self.packed)

    def optimise_(self, grad, clip_norm=0.0, grad_scale=1.0):
        """`grad` is the gradient of `.params` as the plain kernels wrote it"""
        from .ops import clip_adam_

        g = unfold_dueling_grad(grad, self._grad.t, self.n_in, self.hidden, self.n_out, self.layers)
        clip_adam_(self.dueling_params, g, self.m, self.v, self.beta_pow, grad_scale, clip_norm, self.lr, self.beta1,
                   self.beta2, self.eps, self.gn)
        self.refold_()


class TargetNetwork:
    """TargetNetwork(network; sync_freq = 1, ρ = 0f0)  target_network.jl:27-60.  With a DuelingApproximator the target is kept as a
    dueling vector too (`target_dueling`): Polyak runs on the dueling vectors and `target`, the effective vector, is folded again."""

    def __init__(self, network, sync_freq=1, rho=0.0):
        if not 0 <= rho <= 1:
            raise AssertionError("ρ must in [0,1]")  # :50
        self.network, self.sync_freq, self.rho, self.n_optimise = network, int(sync_freq), float(rho), 0
        self.target = network.params.clone()
        self.target_packed = network.packed.clone() if getattr(network, "layers", 2) == 3 else None
        if getattr(network, "dueling_params", None) is not None:
            self.target_dueling = network.dueling_params.clone()

    def forward(self, x):
        return self.network.forward(x)

    def optimise_(self, grad, **kw):
        """optimise!(tn, grad)  :70-88: update the network, then every sync_freq calls
        dest = ρ·dest + (1-ρ)·src and reset the counter."""
        from .ops import polyak_

        self.network.optimise_(grad, **kw)
        self.n_optimise += 1
        if self.n_optimise % self.sync_freq == 0:
            net = self.network
            if getattr(net, "dueling_params", None) is not None:
                polyak_(self.target_dueling, net.dueling_params, self.rho)
                fold_dueling(self.target_dueling, self.target, net.n_in, net.hidden, net.n_out, getattr(net, "layers", 2))
            else:
                polyak_(self.target, self.network.params, self.rho)
            self.n_optimise = 0
            if getattr(net, "layers", 2) == 3:
                mlp3_pack(self.target, net.n_in, net.hidden, net.n_out, self.target_packed)


# -------------------------------------------------------------------------------------- learner
class DQNLearner:
    """BasicDQN / DQN learner on a device trajectory: every `update_freq` vec-steps (once
    `min_replay_history` transitions are stored, and while the trajectory's InsertSampleRatioController
    allows another batch) sample a batch, TD target with the target network, Huber loss, gradient,
    [all-reduce], Adam, target sync.  At most ONE batch per optimise! call (the reference's
    `for batch in trajectory` may yield several to catch up after a warm-up; a vec-step already inserts
    n_env transitions at once).

    Prioritized replay (CircularPrioritizedTraces): batches are drawn in proportion to the stored priorities,
    (|td| + per_eps)^per_alpha is written back, and -- round 4 -- the loss carries the importance-sampling weights
    of PrioritizedDQN when `per_beta > 0`: w = 1 ./ ((priority .+ 1f-10) .^ beta), w ./= maximum(w),
    loss = mean(w .* huber(td)) (`per_beta` may be a callable n_updates -> beta for the usual annealing towards 1;
    per_beta = 0, the default, is the proportional-sampling variant without weights).

    Every form -- 1-step or n-step, uniform or prioritized, plain or Double DQN targets -- is the same pipeline behind optimise_'s
    gate (`_update_`), each stage defined once: `_draw_` (the batch as a (ring, idx) pair with its discount), `_is_weights_`
    (prioritized traces, beta > 0), the DoubleTargetFold (`double_dqn`), `_gradient_` (the one choice of the gradient entry, by
    layers and weights), the priority write-back under the drawn keys, `_exchange_and_apply_`.  A stage a form does not need is
    skipped, and the plain learner keeps its shortest form: no draw of its own, the gradient launch samples."""

    def __init__(self, approximator, batchsize=32, gamma=0.99, huber_delta=1.0, min_replay_history=100,
                 update_freq=1, max_grad_norm=0.0, seed=0, process_group=None, per_eps=1e-6, per_alpha=0.6, per_beta=0.0, n_step=1,
                 double_dqn=False):
        """n_step > 1: batches come from NStepBatchSampler(n_step, gamma, batchsize) -- the window folded on the device into one
        transition -- and the TD target is R + gamma^n (1 - t) max Qt(s_{i+n}); per-stage loop.  Uniform replay, or
        prioritized replay over CircularPrioritizedTraces(..., n_step = n_step): window starts drawn from the masked sum-tree and
        folded in the same launch (rlhip_per_sample_fold_nstep_f32), priorities written back under the drawn keys.
        double_dqn = True (`is_enable_double_DQN` of the removed DQNLearner): the bootstrap value is Qt(s')[findmax(Q(s'))] instead of
        max Qt(s').  Every per-stage update form folds its sampled batch first (DoubleTargetFold: the finished target y in the
        reward field, terminal = 1) and runs the same gradient kernels on the folded ring; the fused vec-step stays plain DQN."""
        self.double_dqn = bool(double_dqn)
        self._double = None  # the DoubleTargetFold: see _double_fold
        self.n_step = int(n_step)
        self._nstep = None
        if self.n_step > 1:
            from .trajectory import NStepBatchSampler

            self._nstep = NStepBatchSampler(self.n_step, gamma, batchsize, seed=seed)
        self.per_eps, self.per_alpha, self.per_beta = float(per_eps), float(per_alpha), per_beta
        self.approximator = approximator  # a TargetNetwork
        net = approximator.network
        self.batchsize, self.gamma, self.delta = batchsize, gamma, huber_delta
        self.min_replay_history, self.update_freq, self.max_grad_norm = min_replay_history, update_freq, max_grad_norm
        if int(update_freq) < 1:
            raise ValueError("update_freq must be >= 1")
        self.seed, self.draw_ctr, self.n_updates = seed, 0, 0
        self.vec_steps = 0  # optimise! calls so far (one per vec-step): the update_freq gate
        self.process_group = process_group
        self.grad = torch.zeros_like(net.params)
        self.loss = torch.zeros(1, dtype=torch.float32, device=net.params.device)
        # observations of more than four components live in a frame ring: the update runs the same stages on a gathered batch
        # (`_update_batch_`, csrc/dqn_batch.hip)
        if self._wide:
            check_wide_net(net, "DQNLearner")
            ws = dqn_batch_workspace
        else:
            ws = dqn_workspace if net.layers == 2 else dqn3_workspace
        self.workspace = ws(net.n_in, net.hidden, net.n_out, batchsize, net.params.device)
        self._batch = None  # the gathered batch of the last update on a frame ring (scratch)
        dev = net.params.device
        self.td = torch.zeros(batchsize, dtype=torch.float32, device=dev)
        self.is_weights = torch.ones(batchsize, dtype=torch.float32, device=dev)
        self._idx = self._key = self._prio = None

    def forward(self, x):
        return self.approximator.forward(x)

    @property
    def _wide(self):
        """observations of more than four components (a property: a checkpoint holds the network, not this)"""
        return getattr(getattr(self.approximator, "network", None), "n_in", 0) > 4

    def should_update_(self, trajectory, n_transitions=None):
        """the gate of optimise!: warm-up, every `update_freq`-th vec-step, the trajectory's sample / insert controller.
        Advances the vec-step counter (call once per vec-step; run_fused_dqn uses it for its `do_update` flag)."""
        self.vec_steps += 1
        n = trajectory.container.n_transitions() if n_transitions is None else n_transitions
        if n < self.min_replay_history or self.vec_steps % self.update_freq != 0:
            return False
        return bool(trajectory.controller.on_sample_())

    def optimise_(self, trajectory):
        traces = trajectory.container
        prioritized = hasattr(traces, "sample_prioritized")
        batch_form = self._wide or not getattr(traces, "records_layout", True)
        if batch_form:
            self._check_batch_form(traces, prioritized)
        if self._nstep is not None and len(traces) < self.n_step:
            # not one full window yet: the vec-step counts, the controller is not asked (no sample is drawn; over prioritized
            # traces the masked tree has no mass yet)
            self.vec_steps += 1
            return False
        if self._nstep is not None and prioritized and getattr(traces, "n_step", 1) != self.n_step:
            raise ValueError(f"DQNLearner(n_step = {self.n_step}) needs CircularPrioritizedTraces(..., n_step = {self.n_step}): "
                             f"these traces mask windows of {getattr(traces, 'n_step', 1)}")
        if not self.should_update_(trajectory):
            return False
        if batch_form:
            return self._update_batch_(traces, prioritized)
        return self._update_(traces, prioritized)

    def _check_batch_form(self, traces, prioritized):
        """what the update on a gathered batch takes: a frame ring of Float32 observations with the network's 5..16 components,
        uniform, or prioritized through CircularPrioritizedFrameTraces masked for this learner's n_step.  Raised before any C call."""
        net = self.approximator.network
        if traces.dtype != torch.float32:
            raise NotImplementedError("DQNLearner: UInt8 frames (and stacks of them, n_stack) need a convolutional Q-network, which this "
                                      "library does not have; NStepBatchSampler / BatchSampler serve such rings to a learner of your own")
        if traces.obs_dim > MAX_WIDE_OBS:
            raise ValueError(f"DQNLearner: observations of up to {MAX_WIDE_OBS} Float32 components, these traces have obs_dim = "
                             f"{traces.obs_dim}")
        if traces.obs_dim != net.n_in:
            raise ValueError(f"DQNLearner: the traces hold observations of {traces.obs_dim} components, the network takes {net.n_in}")
        if prioritized:
            from .trajectory import CircularPrioritizedFrameTraces

            if not isinstance(traces, CircularPrioritizedFrameTraces):
                raise NotImplementedError("DQNLearner: prioritized replay of observations wider than four components takes "
                                          "CircularPrioritizedFrameTraces(..., n_step = n_step)")
            if traces.n_step != self.n_step:
                raise ValueError(f"DQNLearner(n_step = {self.n_step}) needs CircularPrioritizedFrameTraces(..., n_step = {self.n_step}): "
                                 f"these traces mask windows of {traces.n_step}")

    def _update_batch_(self, traces, prioritized):
        """`_update_` on a frame ring: the same stages, each on the batch form -- draw + gather by sampler, importance-sampling
        weights, gradient (rlhip_dqn_grad_batch_f32: Double DQN and the per-sample discount gamma ** n_used are part of its target
        line), priority write-back under the drawn keys, exchange and apply"""
        b = self.batchsize
        s, a, r, t, sn, n_used = self._draw_batch_(traces, prioritized)
        weights = self._is_weights_() if prioritized else None
        tn = self.approximator
        net = tn.network
        dqn_grad_batch(net.n_in, net.hidden, net.n_out, net.act, net.params, tn.target, s, a, r, t, sn, self.gamma, self.delta, n_used,
                       weights, self.double_dqn, self.workspace, self.grad, self.loss, self.td)
        if prioritized:
            call("rlhip_per_priority_f32", ptr(self.td), b, self.per_eps, self.per_alpha, ptr(self.td), stream_ptr())
            traces.set_priority_(self._key, self.td)
        return self._exchange_and_apply_()

    def _draw_batch_(self, traces, prioritized):
        """the draw of the batch form on a frame ring -> (s, a, r, t, s', n_used or None), gathered; `_idx` (and `_key` / `_prio` of a
        prioritized draw) are left on the learner, the batch in `_batch` (scratch)"""
        b, n = self.batchsize, self.n_step
        if prioritized:  # draw + (n-step) gather in one launch; n = 1 is the plain transition with n_used = 1
            (self._idx, self._key, self._prio), batch = traces.sample_gather_nstep_prioritized(b, n, self.gamma, self.seed, self.draw_ctr)
        elif self._nstep is not None:
            self._idx = self._nstep.sample_indices(traces, self.draw_ctr)
            batch = traces.gather_nstep(self._idx, n, self.gamma)
        else:  # the Philox draw the record-ring gradient launch evaluates inline
            self._idx = traces.sample_indices(b, self.seed, self.draw_ctr)
            batch = traces.gather(self._idx) + (None,)
        self._batch = _Scratch(batch)
        return batch

    def _update_(self, traces, prioritized):
        """one update behind the gate, the same stages for every form: draw, importance-sampling weights, Double DQN fold, gradient,
        priority write-back, exchange and apply"""
        ring, idx, gamma, in_place = self._draw_(traces, prioritized)
        weights = self._is_weights_() if prioritized else None
        if self.double_dqn:  # the finished target y into the reward field; an n-step ring is rewritten in place, gamma^n as the discount
            tn = self.approximator
            ring, idx = self._double_fold().fold(ring, None if in_place else idx, tn.network, tn.target, tn.target_packed, gamma, in_place)
        self._gradient_(ring, idx, gamma, weights)
        if prioritized:  # trajectory[:priority, keys] = (|td| + eps)^alpha under the ORIGINAL keys, in this call: before any further push
            call("rlhip_per_priority_f32", ptr(self.td), self.batchsize, self.per_eps, self.per_alpha, ptr(self.td), stream_ptr())
            traces.set_priority_(self._key, self.td)
        return self._exchange_and_apply_()

    def _draw_(self, traces, prioritized):
        """-> (ring, idx, discount, whether `ring` is a folded batch of this learner's that a Double DQN fold may rewrite in place).
        Prioritized draws leave their keys and priorities in `_key` / `_prio`; `_idx` is set by every Double DQN form (the indices its
        fold takes) and by the prioritized n-step form (the drawn window starts)."""
        smp = self._nstep
        if smp is not None and prioritized:  # window starts from the masked tree, draw + window fold in one launch
            ring, idx, self._idx, self._key, self._prio = smp.sample_fold_prioritized(traces, self.draw_ctr)
            return ring, idx, smp.gamma_n, True
        ring, gamma, in_place = traces, self.gamma, False
        if smp is not None:
            ring, idx = smp.fold(traces, smp.sample_indices(traces, self.draw_ctr))
            gamma, in_place = smp.gamma_n, True
        elif prioritized:  # prioritized BatchSampler: keys + priorities from the device sum-tree
            idx, self._key, self._prio = traces.sample_prioritized(self.batchsize, self.seed, self.draw_ctr)
        elif self.double_dqn:  # the draw the plain gradient launch evaluates inline: the flag does not change which transitions are sampled
            idx = traces.sample_indices(self.batchsize, self.seed, self.draw_ctr)
        else:
            idx = None  # the plain learner: the draw happens inside the gradient launch
        if self.double_dqn:
            self._idx = idx
        return ring, idx, gamma, in_place

    def _is_weights_(self):
        """importance-sampling weights of the drawn priorities -> `is_weights`, or None while beta = 0"""
        beta = float(self.per_beta(self.n_updates)) if callable(self.per_beta) else float(self.per_beta)
        if not beta > 0.0:
            return None
        call("rlhip_per_is_weights_f32", ptr(self._prio), self.batchsize, beta, ptr(self.is_weights), stream_ptr())
        return self.is_weights

    def _double_fold(self):
        """the learner's DoubleTargetFold, made on first use (a checkpoint carries the flag, not the scratch: a learner built without
        the flag that loaded a double_dqn = True checkpoint makes it here too)"""
        if self._double is None:
            from .trajectory import DoubleTargetFold

            self._double = DoubleTargetFold()
        return self._double

    def _gradient_(self, ring, idx, gamma, weights):
        """the gradient entry for (layers, weights or not) on `ring` at `idx` -> grad, loss, td.  idx = None is the plain learner, which
        draws inside the launch: two layers take the entry without indices (and without td), three a NULL index pointer."""
        tn = self.approximator
        net = tn.network
        if net.layers == 3:
            if weights is not None:
                call("rlhip_dqn3_grad_w_f32", C.byref(ring.rb), net.hidden, net.n_out, net.act, ptr(net.params), ptr(net.packed),
                     ptr(tn.target), ptr(tn.target_packed), self.batchsize, ptr(idx), ptr(weights), gamma, self.delta,
                     ptr(self.workspace), ptr(self.grad), ptr(self.loss), ptr(self.td), stream_ptr())
            else:
                dqn3_grad(ring, net.hidden, net.n_out, net.act, net.params, net.packed, tn.target, tn.target_packed, self.batchsize,
                          gamma, self.delta, self.seed, self.draw_ctr, idx, self.workspace, self.grad, self.loss, self.td)
        elif weights is not None:
            call("rlhip_dqn_grad_idx_w_f32", C.byref(ring.rb), net.hidden, net.n_out, net.act, ptr(net.params), ptr(tn.target),
                 self.batchsize, ptr(idx), ptr(weights), gamma, self.delta, ptr(self.workspace), ptr(self.grad), ptr(self.loss),
                 ptr(self.td), stream_ptr())
        elif idx is not None:
            call("rlhip_dqn_grad_idx_f32", C.byref(ring.rb), net.hidden, net.n_out, net.act, ptr(net.params), ptr(tn.target),
                 self.batchsize, ptr(idx), gamma, self.delta, ptr(self.workspace), ptr(self.grad), ptr(self.loss), ptr(self.td),
                 stream_ptr())
        else:
            dqn_grad(ring, net.hidden, net.n_out, net.act, net.params, tn.target, self.batchsize, gamma, self.delta, self.seed,
                     self.draw_ctr, self.workspace, self.grad, self.loss)

    def _exchange_and_apply_(self):
        """the tail of every update form (1-step, n-step, prioritized): draw counter, gradient all-reduce over the process group,
        clip (1 / world scale) + Adam"""
        self.draw_ctr += 1
        scale = 1.0
        if self.process_group is not None:
            import torch.distributed as dist

            world = dist.get_world_size(self.process_group)
            if world > 1:
                if not hasattr(self, "_hipcomm"):  # rlhip_comm_* (csrc/comm.hip): p2p kernel or RCCL behind one call
                    from .dist import HipComm

                    self._hipcomm = HipComm.create(self.process_group, self.grad.numel(), self.grad.device)
                if self._hipcomm.ok:
                    self._hipcomm.all_reduce_(self.grad)
                    self._hipcomm.check()
                else:
                    dist.all_reduce(self.grad, op=dist.ReduceOp.SUM, group=self.process_group)
                scale = 1.0 / world
        self.approximator.optimise_(self.grad, clip_norm=self.max_grad_norm, grad_scale=scale)
        self.n_updates += 1
        return True


class QBasedPolicy:
    """QBasedPolicy(; learner, explorer)  q_based_policy.jl:13-49.  plan! on the vector env is one fused
    launch (Q forward + eps-greedy)."""

    def __init__(self, learner, explorer):
        self.learner, self.explorer = learner, explorer
        self._actions = None
        self._q = None

    def plan_(self, env):
        net = self.learner.approximator.network
        ex = self.explorer
        wide = net.n_in > 4  # observations of 5..16 components: the plan launch of csrc/dqn_batch.hip
        if wide:
            check_wide_net(net, "QBasedPolicy")
        dist = getattr(self.learner, "plan_distributional_", None)  # a learner whose network estimates a value DISTRIBUTION per action
        if ex.is_break_tie:  # tie-break variant: unfused path (forward, then the selection kernel)
            values = self.learner.forward(env.state()) if dist is not None else net.forward(env.state())
            return ex.plan_(values, env_id_base=env.env_id_base)
        eps = ex.get_eps()
        step = ex.step
        ex.step += 1
        if dist is not None:  # plan! on the expectation of the distribution, one launch (csrc/c51.hip)
            self._actions, self._q = dist(env.state(), eps, ex.seed, env.env_id_base, step, self._actions, self._q)
        elif net.layers == 3:
            self._actions, self._q = dqn3_plan(net.params, net.packed, net.n_in, net.hidden, net.n_out, net.act,
                                               env.state(), eps, ex.seed, env.env_id_base, step, self._actions,
                                               self._q)
        elif wide:
            self._actions, self._q = dqn_plan_obsn(net.params, net.n_in, net.hidden, net.n_out, net.act, env.state(), eps,
                                                   ex.seed, env.env_id_base, step, self._actions, self._q)
        else:
            self._actions, self._q = dqn_plan(net.params, net.n_in, net.hidden, net.n_out, net.act, env.state(), eps,
                                              ex.seed, env.env_id_base, step, self._actions, self._q)
        return self._actions + 1

    def optimise_(self, trajectory):
        """optimise!(policy, stage, trajectory) -> optimise!(learner, stage, trajectory)  (:49)."""
        return self.learner.optimise_(trajectory)
