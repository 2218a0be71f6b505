"""The judges of the dueling distributional kernels judged on the CPU, and what of the new surface needs no device:

  * the Float32 replay of the update path (fold -> C51 replay -> unfold) against float64 autograd of the dueling C51 loss on every
    gradient case of tests/test_gpu_dist_dueling.py: a* equal, the top-two target-Q gap above 1e-3 and every ReLU pre-activation
    1e-6 off zero at every sample, the distance inside the bar the C51 replay is held to;
  * the parameter-domain fold against the output-domain combine in float64 (they are the same function);
  * RLHIP_EINVAL before any launch for every shape outside the envelope, at every new entry point; symbols and signatures;
  * the Python refusals and admissions, on CPU tensors."""
import numpy as np
import pytest
import torch

import c51_ref as C
import dist_dueling_ref as D
from test_c51_reference import FAKE, GRAD_BAR, _lib

GRAD_CASES = [(b, dbl, ex) for b in (8, 24) for dbl in (False, True) for ex in (False, True)]


@pytest.mark.parametrize("shape", D.SHAPES)
def test_replay_against_float64_autograd_of_the_dueling_loss(shape):
    for k in GRAD_CASES:
        c = D.case(*shape, *k)
        m, (g, rp) = D.torch_model(c), D.replay_grad(c)
        assert m["gap"] > 1e-3 and m["zmin"] > 1e-6 and np.array_equal(rp["sel"], m["sel"]), k
        print(f"{shape} {k}: replay {C.rel(g, m['grad']):.3e} of max|g|, gap {m['gap']:.2e}")
        assert C.rel(g, m["grad"]) <= GRAD_BAR and abs(rp["loss"] - m["loss"]) <= 1e-6 * max(1.0, abs(m["loss"]))


@pytest.mark.parametrize("shape", D.SHAPES)
def test_the_fold_is_the_output_domain_combine(shape):
    ns, h, na, K = shape
    rng = np.random.default_rng(sum(shape))
    duel, hid = rng.normal(0, 0.5, C.nparams(ns, h, (1 + na) * K)), rng.normal(0, 1, (h, 5))
    rows = lambda v, r: D._head(v, ns, h, r)[:h].T @ hid + D._head(v, ns, h, r)[h][:, None]  # noqa: E731
    eff = D.fold(duel, *shape, dtype=np.float64)
    assert np.abs(rows(eff, na * K) - D.combine(rows(duel, (1 + na) * K), na, K)).max() <= 1e-12
    g = rng.normal(0, 1, eff.size)  # the unfold is the transpose of the fold
    assert abs(g @ eff - D.unfold(g, *shape, dtype=np.float64) @ duel) <= 1e-9 * np.abs(g).sum()
    assert D.fold(duel.astype(np.float32), *shape).dtype == np.float32 and C.rel(D.fold(duel.astype(np.float32), *shape), eff) <= 1e-6


BAD = [(D.REFUSED, "at most 256 rows"), ((1, 8, 2, 5), "obs dim"), ((4, 6, 2, 5), "multiple of 4"), ((4, 8, 5, 5), "na must be"),
       ((4, 8, 2, 65), "at most 64"), ((4, 8, 2, 0), "at most 64")]
ENTRIES = {"rlhip_dist_dueling_fold_f32": lambda s: (FAKE, FAKE, None, None, *s, None),
           "rlhip_dist_dueling_unfold_grad_f32": lambda s: (FAKE, FAKE, *s, None),
           "rlhip_noisy_dueling_fold_f32": lambda s: (FAKE, FAKE, None, None, *s, 1, 0, None),
           "rlhip_noisy_dueling_unfold_grad_f32": lambda s: (FAKE, FAKE, *s, 1, 0, None),
           "rlhip_noisy_c51_dueling_forward_f32": lambda s: (FAKE, *s, 0, -1.0, 1.0, FAKE, 8, 1, 0, 0, FAKE, None, None, None),
           "rlhip_noisy_c51_dueling_plan_f32": lambda s: (FAKE, *s, 0, -1.0, 1.0, FAKE, 8, 0.1, 1, 0, 0, FAKE, None, None)}


@pytest.mark.parametrize("entry", list(ENTRIES))
@pytest.mark.parametrize("shape,message", BAD)
def test_every_shape_outside_the_envelope_is_einval_before_any_launch(entry, shape, message):
    lib = _lib()
    assert hasattr(lib.lib, entry) and entry in lib.declared_symbols() and lib.lib.rlhip_abi_version() == 2
    with pytest.raises(lib.RLHipArgumentError, match=message):
        lib.call(entry, *ENTRIES[entry](shape))
    assert lib.lib.rlhip_dist_dueling_nparams(*shape) == -1
    assert lib.lib.rlhip_dist_dueling_nparams(4, 256, 4, 51) == C.nparams(4, 256, 255)


def test_the_learners_admit_the_new_approximators_and_keep_their_refusals(monkeypatch):
    import rlhip as rl
    from rlhip import dist_dueling as dd

    for name in ("dist_dueling_fold", "noisy_dueling_fold"):
        monkeypatch.setattr(dd, name, lambda *a, **k: None)
    duel = rl.DistDuelingApproximator(4, 8, 2, 51, device="cpu", dueling_params=np.zeros(C.nparams(4, 8, 153), np.float32))
    noisy = rl.NoisyDuelingApproximator(4, 8, 2, 51, device="cpu", noisy_params=np.zeros(2 * C.nparams(4, 8, 153), np.float32))
    assert duel.params.numel() == C.nparams(4, 8, 102) and duel.m.numel() == duel.dueling_params.numel() == C.nparams(4, 8, 153)
    assert noisy.params.numel() == C.nparams(4, 8, 102) and noisy.m.numel() == noisy.noisy_params.numel()
    tn, tnn = rl.TargetNetwork(duel), rl.TargetNetwork(noisy)
    assert tn.target_dueling.numel() == duel.dueling_params.numel() and tnn.target_noisy.numel() == noisy.noisy_params.numel()
    lr = rl.RainbowLearner(tn, 2, n_atoms=51, batchsize=4)
    assert lr.grad.numel() == duel.params.numel() and rl.QRDQNLearner(tn, 2, n_quantiles=51, batchsize=4).n_quantiles == 51
    assert rl.RainbowLearner(tnn, 2, n_atoms=51, batchsize=4)._noisy_entries == (rl.noisy_c51_dueling_forward, rl.noisy_c51_dueling_plan)
    with pytest.raises(NotImplementedError, match="QRDQNLearner: a NoisyApproximator"):
        rl.QRDQNLearner(tnn, 2, n_quantiles=51)
    with pytest.raises(TypeError, match="IQNLearner: the approximator is a TargetNetwork.IQNApproximator"):
        rl.IQNLearner(tn, 2)
    with pytest.raises(ValueError, match="n_actions = 2, n_atoms = 51"):
        rl.RainbowLearner(tn, 3, n_atoms=34)
    with pytest.raises(NotImplementedError, match="NoisyDuelingApproximator"):
        rl.NoisyApproximator(4, 8, 8, dueling=True)
    for cls in (rl.DistDuelingApproximator, rl.NoisyDuelingApproximator):
        with pytest.raises(ValueError, match=r"\(1 \+ n_actions\) \* n_atoms <= 256"):
            cls(*D.REFUSED, device="cpu")
    scalar = rl.TargetNetwork(rl.HipApproximator(4, 8, 102, device="cpu", params=np.zeros(C.nparams(4, 8, 102), np.float32)))
    scalar.network.dueling_params = torch.zeros(1)
    with pytest.raises(NotImplementedError, match="DuelingApproximator folds ONE mean"):
        rl.RainbowLearner(scalar, 2)
