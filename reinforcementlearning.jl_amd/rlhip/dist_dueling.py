"""DistDuelingApproximator / NoisyDuelingApproximator -- DuelingNetwork heads (RLCore/src/utils/networks.jl:510-522) for the
distributional learners: per atom (quantile) k,  l[k, o] = v[k] + a[k, o] - mean_o' a[k, o'].  include/rlhip.h (the dueling
distributional section) states every formula; csrc/dist_dueling.hip and csrc/noisy.hip implement it, tests/dist_dueling_ref.py replays it.

The trained vector is a plain mlp2(ns, h, (1 + na) K) vector: na K advantage rows in C51's row order, then K value rows.  Learning is
the dueling idiom of DuelingApproximator: the vector is folded into the effective plain mlp2(ns, h, na K) vector, the unchanged C51 /
QR-DQN kernels run on it, and the gradient is mapped back.  A noisy dueling net folds noise and combine in one launch and acts with one
noise sample per env, combining in the output domain (rlhip_noisy_c51_dueling_plan_f32).

Out of scope, refused by name: dueling IQN, noisy dueling QR-DQN, three-layer and bf16 nets, sharded runs, a fused vec-step.
"""
import torch

from . import _lib
from ._lib import call
from .dqn import HipApproximator, _Scratch
from .noisy import _opt, noisy_init
from .ops import (dist_dueling_fold, dist_dueling_unfold_grad, mlp2_init, mlp2_nparams, noisy_dueling_fold, noisy_dueling_unfold_grad, ptr,
                  stream_ptr)

ENVELOPE = "obs_dim 2..16, hidden a multiple of 4 and <= 256, 1..4 actions, 1..64 atoms / quantiles, (1 + n_actions) * n_atoms <= 256"


def dist_dueling_nparams(n_in, h, na, K):
    """the length of a dueling distributional vector, mlp2(n_in, h, (1 + na) K); -1 outside the envelope"""
    return int(_lib.lib.rlhip_dist_dueling_nparams(n_in, h, na, K))


def _check(who, n_in, h, na, K, k_min=1):
    nd = dist_dueling_nparams(n_in, h, na, K)
    if nd < 0 or K < k_min:
        raise ValueError(f"{who}: the dueling distributional kernels take {ENVELOPE}; got n_in = {n_in}, hidden = {h}, n_actions = {na}, "
                         f"n_atoms = {K}")
    return nd


def noisy_c51_dueling_forward(noisy, ns, h, na, n_atoms, act, v_min, v_max, obs, seed, env_id_base, step, q_out=None, probs=None,
                              logits=None):
    """`noisy_c51_forward` on a noisy dueling vector; probs / logits ((n_atoms * na), n) are the COMBINED rows"""
    n = obs.shape[1]
    q_out = q_out if q_out is not None else torch.empty((na, n), dtype=torch.float32, device=obs.device)
    call("rlhip_noisy_c51_dueling_forward_f32", ptr(noisy), ns, h, na, n_atoms, act, v_min, v_max, ptr(obs), n, seed, env_id_base, step,
         ptr(q_out), _opt(probs), _opt(logits), stream_ptr())
    return q_out


def noisy_c51_dueling_plan(noisy, ns, h, na, n_atoms, act, v_min, v_max, obs, eps, seed, env_id_base, step, actions=None, q_out=None):
    """plan! in one launch: byte for byte `noisy_c51_dueling_forward` then `eps_greedy_select` -> (0-based actions, q (na, n))"""
    n = obs.shape[1]
    actions = actions if actions is not None else torch.empty(n, dtype=torch.int32, device=obs.device)
    q_out = q_out if q_out is not None else torch.empty((na, n), dtype=torch.float32, device=obs.device)
    call("rlhip_noisy_c51_dueling_plan_f32", ptr(noisy), ns, h, na, n_atoms, act, v_min, v_max, ptr(obs), n, float(eps), seed, env_id_base,
         step, ptr(actions), ptr(q_out), stream_ptr())
    return actions, q_out


class DistDuelingApproximator(HipApproximator):
    """FluxApproximator(model = DuelingNetwork(base, val = Dense(h, n_atoms), adv = Dense(h, n_actions * n_atoms)), optimiser = Adam(lr))
    for RainbowLearner (n_atoms atoms) and QRDQNLearner (n_atoms = its n_quantiles).

    `.dueling_params` is the trained vector, mlp2(n_in, hidden, (1 + n_actions) * n_atoms); `.m` / `.v` have its length.  `.params` is
    the EFFECTIVE plain vector (rlhip_dist_dueling_fold_f32), n_out = n_actions * n_atoms rows -- the one every kernel reads.
    `optimise_` maps the plain gradient back (rlhip_dist_dueling_unfold_grad_f32), steps clip + Adam on the dueling vector (the global
    norm is the dueling gradient's) and folds again."""
    dist_dueling = True

    def __init__(self, n_in, hidden, n_actions, n_atoms, act="relu", lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, seed=0, net_id=0,
                 device="cuda", dueling_params=None):
        nd = _check("DistDuelingApproximator", n_in, hidden, n_actions, n_atoms)
        n_out = n_actions * n_atoms
        if dueling_params is None:
            duel = mlp2_init(n_in, hidden, n_out + n_atoms, seed, net_id, device)
        else:
            duel = torch.as_tensor(dueling_params, dtype=torch.float32, device=device).clone().contiguous()
            if duel.numel() != nd:
                raise ValueError(f"DistDuelingApproximator: dueling_params has {duel.numel()} elements, the network {nd}")
        # (`params` is overwritten by the fold)
        super().__init__(n_in, hidden, n_out, act, lr, beta1, beta2, eps, seed, net_id, device, duel[:mlp2_nparams(n_in, hidden, n_out)])
        self.n_actions, self.n_atoms = int(n_actions), int(n_atoms)
        self.dueling_params = duel
        self.m = torch.zeros_like(duel)
        self.v = torch.zeros_like(duel)
        self._grad = _Scratch(torch.zeros_like(duel))
        self.refold_()

    def fold_(self, duel, eff, duel2=None, eff2=None):
        """effective vector(s) from dueling vector(s) of this shape (TargetNetwork folds its target with it)"""
        return dist_dueling_fold(duel, eff, self.n_in, self.hidden, self.n_actions, self.n_atoms, duel2, eff2)

    def refold_(self):
        """.params from .dueling_params"""
        self.fold_(self.dueling_params, self.params)

    def optimise_(self, grad, clip_norm=0.0, grad_scale=1.0):
        """`grad` is the gradient of `.params` as the plain kernels wrote it"""
        from .ops import clip_adam_

        g = dist_dueling_unfold_grad(grad, self._grad.t, self.n_in, self.hidden, self.n_actions, self.n_atoms)
        clip_adam_(self.dueling_params, g, self.m, self.v, self.beta_pow, grad_scale, clip_norm, self.lr, self.beta1, self.beta2, self.eps,
                   self.gn)
        self.refold_()


class NoisyDuelingApproximator(HipApproximator):
    """FluxApproximator(model = DuelingNetwork of NoisyDense layers, optimiser = Adam(lr)) for RainbowLearner: NoisyApproximator with a
    dueling head.

    `.noisy_params` is the trained vector [mu | sigma], each half mlp2(n_in, hidden, (1 + n_actions) * n_atoms); `.m` / `.v` / `._grad`
    have its length.  `.params` is the EFFECTIVE plain vector of the latest fold, n_actions * n_atoms rows: noise and dueling combine in
    one launch (rlhip_noisy_dueling_fold_f32; `fused = False`: the two-launch composition, byte for byte the same).  Acting reads the
    noisy vector (rlhip_noisy_c51_dueling_plan_f32)."""
    dist_dueling = True

    def __init__(self, n_in, hidden, n_actions, n_atoms, act="relu", lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, seed=0, net_id=0,
                 device="cuda", sigma0=0.5, noisy_params=None, fused=True):
        nd = _check("NoisyDuelingApproximator", n_in, hidden, n_actions, n_atoms, k_min=2)
        n_out = n_actions * n_atoms
        if noisy_params is None:
            noisy = noisy_init(n_in, hidden, n_out + n_atoms, seed, net_id, sigma0, device)
        else:
            noisy = torch.as_tensor(noisy_params, dtype=torch.float32, device=device).clone().contiguous()
            if noisy.numel() != 2 * nd:
                raise ValueError(f"NoisyDuelingApproximator: noisy_params has {noisy.numel()} elements, the network {2 * nd}")
        super().__init__(n_in, hidden, n_out, act, lr, beta1, beta2, eps, seed, net_id, device, noisy[:mlp2_nparams(n_in, hidden, n_out)])
        self.n_actions, self.n_atoms, self.fused = int(n_actions), int(n_atoms), bool(fused)
        self.noisy_params = noisy
        self.noise_seed, self.counter = int(seed), 0
        self.m = torch.zeros_like(noisy)
        self.v = torch.zeros_like(noisy)
        self._grad = _Scratch(torch.zeros_like(noisy))
        # the M'-row vectors of the two-launch composition (scratch; made on first use)
        self._mid = None
        self.resample_(0)

    def _shape(self):
        return self.n_in, self.hidden, self.n_actions, self.n_atoms

    def _mid_(self):
        if self._mid is None:
            self._mid = _Scratch(torch.zeros((3, self.noisy_params.numel() // 2), dtype=torch.float32, device=self.noisy_params.device))
        return self._mid.t

    def resample_(self, counter, target=None):
        """.params <- the fold of .noisy_params under (noise_seed, counter); target: a TargetNetwork whose `target` is folded from its
        `target_noisy` in the same launch, under the target net's tag"""
        from .ops import noisy_fold

        self.counter = int(counter)
        n2, e2 = (None, None) if target is None else (target.target_noisy, target.target)
        if self.fused:
            noisy_dueling_fold(self.noisy_params, self.params, *self._shape(), self.noise_seed, self.counter, n2, e2)
            return
        mid = self._mid_()
        rows = (1 + self.n_actions) * self.n_atoms
        noisy_fold(self.noisy_params, mid[0], self.n_in, self.hidden, rows, self.noise_seed, self.counter, n2, None if n2 is None else mid[1])
        dist_dueling_fold(mid[0], self.params, *self._shape(), None if n2 is None else mid[1], e2)

    def forward(self, x):
        raise NotImplementedError("NoisyDuelingApproximator: the network is evaluated with drawn noise; use RainbowLearner.forward / "
                                  "distribution")

    def optimise_(self, grad, clip_norm=0.0, grad_scale=1.0):
        """`grad` is the gradient of `.params` as the plain kernels wrote it"""
        from .ops import clip_adam_, noisy_unfold_grad

        if self.fused:
            g = noisy_dueling_unfold_grad(grad, self._grad.t, *self._shape(), self.noise_seed, self.counter)
        else:
            mid = dist_dueling_unfold_grad(grad, self._mid_()[2], *self._shape())
            g = noisy_unfold_grad(mid, self._grad.t, self.n_in, self.hidden, (1 + self.n_actions) * self.n_atoms, self.noise_seed,
                                  self.counter)
        clip_adam_(self.noisy_params, g, self.m, self.v, self.beta_pow, grad_scale, clip_norm, self.lr, self.beta1, self.beta2, self.eps,
                   self.gn)
