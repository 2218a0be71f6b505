"""NoisyApproximator -- NoisyDense networks (Fortunato et al. 2018, factorised Gaussian noise) for RainbowLearner: the sixth Rainbow
ingredient.  include/rlhip.h (the NoisyDense section) states every formula; csrc/noisy.hip implements it, tests/noisy_ref.py restates it
in Float64.

Acting draws an independent noise sample per env inside the plan launch (rlhip_noisy_c51_plan_f32 reads the noisy vector).  Learning is the
dueling idiom: one sample per update and net is folded into a plain vector (rlhip_noisy_fold_f32), the unchanged C51 gradient runs on it,
and the gradient is mapped back with the regenerated draws (rlhip_noisy_unfold_grad_f32).

Out of scope, refused by name: independent noise, per-sample noise inside a batch, noisy QR-DQN / IQN / scalar DQN, noisy
three-layer nets, sharded runs, a fused vec-step, bf16 nets.  A noisy dueling head is a class of its own, NoisyDuelingApproximator
(rlhip/dist_dueling.py): this one keeps its plain head.
"""
import torch

from . import _lib
from ._lib import call
from .dqn import HipApproximator, _Scratch
from .ops import noisy_fold, noisy_unfold_grad, ptr, stream_ptr

ENVELOPE = "obs_dim 2..16, hidden a multiple of 4 and <= 256, 2..256 output rows"


def _opt(t):
    return None if t is None else ptr(t)


def noisy_nparams(n_in, h, n_out):
    return int(_lib.lib.rlhip_noisy_nparams(n_in, h, n_out))


def noisy_plan_tile():
    """envs per workgroup of the noisy plan launch"""
    return int(_lib.lib.rlhip_noisy_plan_tile())


def noisy_init(n_in, h, n_out, seed, net_id=0, sigma0=0.5, device="cuda"):
    nn = noisy_nparams(n_in, h, n_out)
    if nn < 0:
        raise ValueError(f"NoisyApproximator: the noisy kernels take {ENVELOPE}; got n_in = {n_in}, hidden = {h}, n_out = {n_out}")
    p = torch.empty(nn, dtype=torch.float32, device=device)
    call("rlhip_noisy_init_f32", ptr(p), n_in, h, n_out, seed, net_id, sigma0, stream_ptr())
    return p


def noisy_c51_forward(noisy, ns, h, na, n_atoms, act, v_min, v_max, obs, seed, env_id_base, step, q_out=None, probs=None, logits=None):
    """`c51_forward` with an independent noise sample per env, drawn under (seed, env_id_base + env, step)"""
    n = obs.shape[1]
    q_out = q_out if q_out is not None else torch.empty((na, n), dtype=torch.float32, device=obs.device)
    call("rlhip_noisy_c51_forward_f32", ptr(noisy), ns, h, na, n_atoms, act, v_min, v_max, ptr(obs), n, seed, env_id_base, step, ptr(q_out),
         _opt(probs), _opt(logits), stream_ptr())
    return q_out


def noisy_c51_plan(noisy, ns, h, na, n_atoms, act, v_min, v_max, obs, eps, seed, env_id_base, step, actions=None, q_out=None):
    """plan! in one launch: byte for byte `noisy_c51_forward` then `eps_greedy_select` -> (0-based actions, q (na, n))"""
    n = obs.shape[1]
    actions = actions if actions is not None else torch.empty(n, dtype=torch.int32, device=obs.device)
    q_out = q_out if q_out is not None else torch.empty((na, n), dtype=torch.float32, device=obs.device)
    call("rlhip_noisy_c51_plan_f32", ptr(noisy), ns, h, na, n_atoms, act, v_min, v_max, ptr(obs), n, float(eps), seed, env_id_base, step,
         ptr(actions), ptr(q_out), stream_ptr())
    return actions, q_out


class NoisyApproximator(HipApproximator):
    """FluxApproximator(model = Chain(NoisyDense(ns, h, act), NoisyDense(h, n_out)), optimiser = Adam(lr)).

    `.noisy_params` is the trained vector [mu | sigma] (each half in the plain layout); `.m` / `.v` / `._grad` have its length.
    `.params` is the EFFECTIVE plain vector of the latest fold, mu + sigma .* xi -- the one the gradient kernel reads.  `resample_`
    folds a fresh sample (and the target net's, in the same launch); `optimise_` maps the plain gradient back with the draws of the
    latest fold, then steps clip + Adam on the noisy vector (the global norm is the noisy gradient's)."""

    def __init__(self, n_in, hidden, n_out, act="relu", lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, seed=0, net_id=0, device="cuda",
                 sigma0=0.5, noisy_params=None, layers=2, dueling=False):
        if layers != 2 or dueling:
            raise NotImplementedError("NoisyApproximator: two-layer plain heads only; noisy three-layer (layers = 3) networks are out of "
                                      "scope, a noisy dueling head is rlhip.NoisyDuelingApproximator")
        nn = noisy_nparams(n_in, hidden, n_out)
        if nn < 0:
            raise ValueError(f"NoisyApproximator: the noisy kernels take {ENVELOPE}; got n_in = {n_in}, hidden = {hidden}, n_out = {n_out}")
        if noisy_params is None:
            noisy = noisy_init(n_in, hidden, n_out, seed, net_id, sigma0, device)
        else:
            noisy = torch.as_tensor(noisy_params, dtype=torch.float32, device=device).clone().contiguous()
            if noisy.numel() != nn:
                raise ValueError(f"NoisyApproximator: noisy_params has {noisy.numel()} elements, the network {nn}")
        super().__init__(n_in, hidden, n_out, act, lr, beta1, beta2, eps, seed, net_id, device, noisy[:nn // 2], layers=2)
        self.noisy_params = noisy
        self.noise_seed, self.counter = int(seed), 0
        self.m = torch.zeros_like(noisy)
        self.v = torch.zeros_like(noisy)
        self._grad = _Scratch(torch.zeros_like(noisy))
        self.resample_(0)

    def resample_(self, counter, target=None):
        """.params <- the fold of .noisy_params under (noise_seed, counter); target: a TargetNetwork whose `target` is folded from its
        `target_noisy` in the same launch, under the target net's tag"""
        self.counter = int(counter)
        noisy_fold(self.noisy_params, self.params, self.n_in, self.hidden, self.n_out, self.noise_seed, self.counter,
                   None if target is None else target.target_noisy, None if target is None else target.target)

    def forward(self, x):
        raise NotImplementedError("NoisyApproximator: the network is evaluated with drawn noise; use RainbowLearner.forward / distribution")

    def optimise_(self, grad, clip_norm=0.0, grad_scale=1.0):
        """`grad` is the gradient of `.params` as the plain kernels wrote it"""
        from .ops import clip_adam_

        g = noisy_unfold_grad(grad, self._grad.t, self.n_in, self.hidden, self.n_out, self.noise_seed, self.counter)
        clip_adam_(self.noisy_params, g, self.m, self.v, self.beta_pow, grad_scale, clip_norm, self.lr, self.beta1, self.beta2, self.eps,
                   self.gn)

