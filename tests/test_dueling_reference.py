"""DuelingNetwork Q-networks as a parameter fold (csrc/dueling.hip, rlhip.DuelingApproximator) -- the CPU half:

  * the identity the device path rests on: fold -> the oracle's plain DQN loss / gradient -> unfold (tests/dueling_ref.py) IS the
    Float64 autograd gradient of the literal `val + adv - mean(adv)` network, at the project's f32 bar (1e-6 of max|g|);
  * the folded forward against the literal Float32 network (1e-6 of max|Q|);
  * unfold against a Float64 evaluation of the chain rule, and as the adjoint of the fold; na = 1; layout and nparams;
  * argument validation of the three entry points (before any HIP call: the library loads without a GPU), signatures in header /
    ctypes / Julia glue;
  * host logic without a device: TargetNetwork's counter and sync with a dueling network, the fused vec-step's refusal, the
    checkpoint's key set."""
import ctypes as C
import os
import re
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

import oracle
import dueling_ref as dr
from double_dqn_ref import trained_nets
from test_julia_glue_signatures import GLUE, glue_ccalls, header_prototypes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (ns, h, na, act, batch): the six shapes the identity was measured at (gradient error <= 1.9e-7 of max|g|, forward <= 4.3e-7 of max|Q|)
SHAPES = [(4, 128, 2, 0, 64), (4, 128, 2, 1, 64), (2, 64, 3, 0, 96), (4, 256, 4, 1, 200), (3, 128, 3, 0, 2048), (4, 64, 4, 0, 4096)]
_CASES = {}


def _case(ns, h, na, act, b, seed):
    """dueling nets whose Q-values have separated (adv = the trained head, val Glorot) and a synthetic batch; computed once"""
    key = (ns, h, na, act, b, seed)
    if key not in _CASES:
        rng = np.random.default_rng(seed)
        p, pt = trained_nets(2, ns, h, na, act, seed, steps=150)
        d, dt = dr.make(ns, h, na, 2, p, rng), dr.make(ns, h, na, 2, pt, rng)
        s = rng.standard_normal((ns, b)).astype(np.float32)
        sn = (s + 0.1 * rng.standard_normal((ns, b))).astype(np.float32)
        a = rng.integers(0, na, b).astype(np.int32)
        r = rng.standard_normal(b).astype(np.float32)
        t = (rng.random(b) < 0.1).astype(np.uint8)
        _CASES[key] = (d, dt, s, a, r, t, sn)
    return _CASES[key]


@pytest.mark.parametrize("seed", [1, 2])
@pytest.mark.parametrize("ns,h,na,act,b", SHAPES)
def test_composed_gradient_is_the_autograd_gradient_of_the_literal_network(ns, h, na, act, b, seed):
    d, dt, s, a, r, t, sn = _case(ns, h, na, act, b, seed)
    loss, g, pe, pte = dr.composed(2, ns, h, na, act, d, dt, s, a, r, t, sn, 0.99)
    ref_loss, ref, _ = dr.torch_f64_grad(d, dt, ns, h, na, act, s, a, r, t, sn, 0.99)
    err = np.abs(g.astype(np.float64) - ref).max() / np.abs(ref).max()
    print(f"ns={ns} h={h} na={na} act={act} batch={b} seed={seed}: gradient error / max|g| = {err:.2e}, loss {loss:.6f} vs {ref_loss:.6f}")
    assert g.size == dr.nparams(ns, h, na, 2) and np.abs(ref).max() > 0
    assert err <= 1e-6, err
    assert loss == pytest.approx(ref_loss, rel=1e-5)


@pytest.mark.parametrize("seed", [1, 2])
@pytest.mark.parametrize("ns,h,na,act,b", SHAPES)
def test_folded_forward_is_the_literal_network(ns, h, na, act, b, seed):
    d, _, s, *_ = _case(ns, h, na, act, b, seed)
    q = oracle.mlp2_forward(dr.fold(d, ns, h, na, 2), ns, h, na, act, s)
    lit = dr.literal_q(d, ns, h, na, act, s)
    err = np.abs(q - lit).max() / np.abs(lit).max()
    print(f"ns={ns} h={h} na={na} act={act} seed={seed}: max|Q_eff - Q_literal| / max|Q| = {err:.2e}")
    assert err <= 1e-6, err
    # ... and the literal network is not the plain one: the val head and the mean matter
    plain = oracle.mlp2_forward(np.ascontiguousarray(d[:oracle.mlp2_nparams(ns, h, na)]), ns, h, na, act, s)
    assert np.abs(plain - lit).max() > 1e-3 * np.abs(lit).max()


@pytest.mark.parametrize("layers,ns,h,na", [(2, 4, 1, 1), (2, 2, 5, 3), (2, 4, 64, 4), (2, 4, 128, 2), (3, 3, 256, 3), (3, 4, 128, 2)])
def test_unfold_is_the_chain_rule_of_the_fold(layers, ns, h, na):
    rng = np.random.default_rng(h + na)
    n, nd = dr.plain_nparams(ns, h, na, layers), dr.nparams(ns, h, na, layers)
    g = rng.standard_normal(n).astype(np.float32)
    u, u64 = dr.unfold(g, ns, h, na, layers), dr.unfold_f64(g, ns, h, na, layers)
    nb = n - na * h - na
    assert u.dtype == np.float32 and u.size == nd and np.array_equal(u[:nb], g[:nb])
    # Float32 against Float64: the sum takes na - 1 roundings of partial sums <= na M (M = max|g| of the head), the mean one more of a
    # value <= M, the difference one of a value <= 2 M: dWval within na (na - 1) 2^-24 M, dWadv within (na - 1 + 1 + 2) 2^-24 M
    M = np.abs(g[nb:]).max()
    tol = max(na * (na - 1), na + 2) * 2.0 ** -24 * M
    assert np.abs(u - u64).max() <= tol, (np.abs(u - u64).max(), tol)
    # the adjoint identity <fold(d), g> = <d, unfold(g)> of the linear map, in Float64
    d = rng.standard_normal(nd)
    adv = d[nb:nb + na * h + na].reshape(h + 1, na)
    fold64 = np.concatenate([d[:nb], (d[nb + na * h + na:][:, None] + adv - adv.mean(1, keepdims=True)).reshape(-1)])
    assert np.dot(fold64, g.astype(np.float64)) == pytest.approx(np.dot(d, u64), rel=1e-12, abs=1e-12)
    # the Float32 fold against that Float64 map: one rounding of (val + adv) <= 2 M', the sum and the mean as above, the difference
    d32 = d.astype(np.float32)
    d64 = d32.astype(np.float64)
    adv = d64[nb:nb + na * h + na].reshape(h + 1, na)
    f64 = np.concatenate([d64[:nb], (d64[nb + na * h + na:][:, None] + adv - adv.mean(1, keepdims=True)).reshape(-1)])
    Mp = np.abs(d32[nb:]).max()
    assert np.abs(dr.fold(d32, ns, h, na, layers) - f64).max() <= (na + 5) * 2.0 ** -24 * Mp


def test_one_action_gives_an_exactly_zero_advantage_gradient():
    ns, h, na = 4, 33, 1
    rng = np.random.default_rng(0)
    g = rng.standard_normal(dr.plain_nparams(ns, h, na, 2)).astype(np.float32)
    u = dr.unfold(g, ns, h, na, 2)
    off = dr.offsets(ns, h, na, 2)
    for k in ("Wadv", "badv"):  # x - x / 1 = 0
        o, n = off[k]
        assert not u[o:o + n].any()
    o, n = off["Wval"]
    assert np.array_equal(u[o:o + n], g[h * ns + h:h * ns + 2 * h]) and u[-1] == g[-1]


@pytest.mark.parametrize("layers", [2, 3])
def test_nparams_and_layout_offsets(layers):
    from rlhip import _lib

    f = _lib.lib.rlhip_dueling_nparams
    for ns, h, na in ((4, 128, 2), (2, 5, 3), (3, 256, 3), (4, 1, 1), (4, 64, 4)):
        plain = int((_lib.lib.rlhip_mlp2_nparams if layers == 2 else _lib.lib.rlhip_mlp3_nparams)(ns, h, na))
        assert plain == dr.plain_nparams(ns, h, na, layers)
        assert f(ns, h, na, layers) == plain + h + 1 == dr.nparams(ns, h, na, layers)
        off = dr.offsets(ns, h, na, layers)
        assert off["Wadv"] == (plain - na * h - na, na * h) and off["badv"] == (plain - na, na)
        assert off["Wval"] == (plain, h) and off["bval"] == (plain + h, 1)
        if layers == 3:
            assert off["W2"] == (h * ns + h, h * h)
    assert f(4, 128, 2, 4) == -1 and f(0, 128, 2, layers) == -1 and f(4, 0, 2, layers) == -1 and f(4, 128, 0, layers) == -1


def test_argument_errors_come_before_any_device_call():
    from rlhip import _lib

    a, b, c, d = (C.c_void_p(4096 * k) for k in (1, 2, 3, 4))  # never dereferenced: every call below is refused first
    fold = lambda *x: _lib.call("rlhip_dueling_fold_f32", *x)  # noqa: E731
    unf = lambda *x: _lib.call("rlhip_dueling_unfold_grad_f32", *x)  # noqa: E731
    bad = [(a, b, None, None, 4, 128, 5, 2, None), (a, b, None, None, 4, 128, 0, 2, None), (a, b, None, None, 4, 0, 2, 2, None),
           (a, b, None, None, 4, 128, 2, 1, None), (a, b, None, None, 4, 128, 2, 4, None), (None, b, None, None, 4, 128, 2, 2, None),
           (a, None, None, None, 4, 128, 2, 2, None), (a, a, None, None, 4, 128, 2, 2, None), (a, b, c, None, 4, 128, 2, 2, None),
           (a, b, None, d, 4, 128, 2, 2, None), (a, b, c, c, 4, 128, 2, 3, None), (a, b, c, b, 4, 128, 2, 3, None)]
    for args in bad:
        with pytest.raises(_lib.RLHipArgumentError, match="invalid argument"):
            fold(*args)
    for args in [(a, b, 4, 128, 5, 2, None), (a, b, 4, 128, 0, 3, None), (a, b, 4, 0, 2, 2, None), (a, b, 4, 128, 2, 0, None),
                 (None, b, 4, 128, 2, 2, None), (a, None, 4, 128, 2, 2, None), (a, a, 4, 128, 2, 2, None)]:
        with pytest.raises(_lib.RLHipArgumentError, match="invalid argument"):
            unf(*args)
    assert _lib.lib.rlhip_abi_version() == 2


def test_signatures_of_the_new_calls_agree():
    from rlhip import _lib

    protos = header_prototypes()
    ctype = {_lib.i32: "Int32", _lib.i64: "Int64", _lib.f32: "Float32"}
    calls = {c[0]: c for c in glue_ccalls()}
    for name in ("rlhip_dueling_nparams", "rlhip_dueling_fold_f32", "rlhip_dueling_unfold_grad_f32"):
        assert name in protos and name in _lib._PROTOS and hasattr(_lib.lib, name), name
        rt, plist = protos[name]
        res, args = _lib._PROTOS[name]
        assert ctype[res] == rt and [ctype.get(x, "ptr") for x in args] == plist, name
        assert name in calls and calls[name][1] == rt and calls[name][2] == plist, name
    src = open(GLUE).read()
    for needle in ("function fold_dueling!(", "function unfold_dueling_grad!(", "function HipDuelingApproximator(model::DuelingNetwork",
                   "function dueling_from_flux(", "function dueling_to_flux("):
        assert needle in src, needle
    assert re.search(r"export[^#]*\bHipDuelingApproximator\b", src, flags=re.S)
    # the permutation of the glue, restated: Flux.destructure order (base, val, adv) <-> flat (base, adv, val)
    h, na, nb = 5, 3, 7
    theta = np.arange(nb + (h + 1) + (na * h + na))
    flat = np.concatenate([theta[:nb], theta[nb + h + 1:], theta[nb:nb + h + 1]])
    back = np.concatenate([flat[:nb], flat[nb + na * h + na:], flat[nb:nb + na * h + na]])
    assert np.array_equal(back, theta) and flat[nb] == nb + h + 1 and flat[-1] == nb + h


# ------------------------------------------------------------------------------------------------ host logic without a device
class _Net:
    """what TargetNetwork reads of an approximator, on host tensors"""

    def __init__(self, dueling):
        self.n_in, self.hidden, self.n_out, self.layers, self.packed = 4, 8, 2, 2, None
        self.params = torch.arange(10, dtype=torch.float32)
        if dueling:
            self.dueling_params = torch.arange(19, dtype=torch.float32)
        self.calls = []

    def optimise_(self, grad, **kw):
        self.calls.append(kw)
        self.params += 1
        if hasattr(self, "dueling_params"):
            self.dueling_params += 2


@pytest.mark.parametrize("rho", [0.0, 0.5])
def test_target_network_counter_and_sync_with_a_dueling_network(monkeypatch, rho):
    import rlhip as rl
    from rlhip import dqn, ops

    log = []

    def polyak_(dst, src, r):
        log.append(("polyak", dst, src, r))
        dst.mul_(r).add_(src, alpha=1 - r)

    def fold_dueling(duel, eff, n_in, h, n_out, layers, duel2=None, eff2=None):
        log.append(("fold", duel, eff, (n_in, h, n_out, layers)))
        eff.copy_(duel[:eff.numel()] + 100)  # a stand-in: only "the effective target was rewritten from the dueling target" matters

    monkeypatch.setattr(ops, "polyak_", polyak_)
    monkeypatch.setattr(dqn, "fold_dueling", fold_dueling)
    net = _Net(dueling=True)
    tn = rl.TargetNetwork(net, sync_freq=3, rho=rho)
    assert torch.equal(tn.target, net.params) and torch.equal(tn.target_dueling, net.dueling_params)
    assert tn.target_dueling.data_ptr() != net.dueling_params.data_ptr()
    t0 = tn.target_dueling.clone()
    for k in range(1, 8):
        tn.optimise_(None, clip_norm=0.5)
        assert tn.n_optimise == k % 3 and len(net.calls) == k and net.calls[-1] == {"clip_norm": 0.5}
        assert len(log) == 2 * (k // 3)
    kinds = [e[0] for e in log]
    assert kinds == ["polyak", "fold"] * 2
    assert log[0][1] is tn.target_dueling and log[0][2] is net.dueling_params and log[0][3] == rho
    assert log[1][1] is tn.target_dueling and log[1][2] is tn.target and log[1][3] == (4, 8, 2, 2)
    # after the first sync (three updates of +2): rho = 0 is a hard copy
    first = rho * t0 + (1 - rho) * (t0 + 6)
    second = rho * first + (1 - rho) * (t0 + 12)
    assert torch.equal(tn.target_dueling, second) and torch.equal(tn.target, second[:10] + 100)
    # a plain network: the path as it was -- Polyak on (target, params), no fold, no dueling target
    log.clear()
    plain = _Net(dueling=False)
    tp = rl.TargetNetwork(plain, sync_freq=2, rho=rho)
    assert getattr(tp, "target_dueling", None) is None
    tp.optimise_(None)
    tp.optimise_(None)
    assert [e[0] for e in log] == ["polyak"] and log[0][1] is tp.target and log[0][2] is plain.params and tp.n_optimise == 0


class _Reached(Exception):
    pass


def test_fused_vec_step_refuses_a_dueling_network():
    from rlhip import core

    class Hook:
        def push_(self, *a):
            raise _Reached

    def stub(net):
        learner = NS(approximator=NS(network=net), explorer=None, process_group=None, n_step=1)
        agent = NS(policy=NS(learner=learner, explorer=NS(is_break_tie=False)), trajectory=NS(container=NS()))
        return agent, NS(continuous=False, is_f64=False)

    for net in (NS(), NS(dueling_params=None)):  # a plain network is admitted
        with pytest.raises(_Reached):
            core.run_fused_dqn(*stub(net), None, Hook())
    with pytest.raises(NotImplementedError, match="per-stage loop"):
        core.run_fused_dqn(*stub(NS(dueling_params=torch.zeros(3))), None, Hook())


def test_checkpoint_carries_the_dueling_vectors_online_and_target():
    import rlhip as rl
    from rlhip import checkpoint, dqn

    net = object.__new__(rl.DuelingApproximator)  # the fields of a 4 -> 8 -> 2 dueling net on host tensors: no device needed
    net.n_in, net.hidden, net.n_out, net.layers, net.act, net.packed = 4, 8, 2, 2, 0, None
    net.lr, net.beta1, net.beta2, net.eps = 1e-3, 0.9, 0.999, 1e-8
    nd, n = dr.nparams(4, 8, 2, 2), dr.plain_nparams(4, 8, 2, 2)
    net.params, net.dueling_params = torch.randn(n), torch.randn(nd)
    net.m, net.v, net._grad = torch.randn(nd), torch.rand(nd), dqn._Scratch(torch.randn(nd))
    net.beta_pow, net.gn = torch.tensor([0.9, 0.999]), torch.zeros(1)
    tn = rl.TargetNetwork(net, sync_freq=4, rho=0.5)
    tn.n_optimise = 3
    d = checkpoint.state_dict(tn)
    assert set(d) == {"n_optimise", "rho", "sync_freq", "target", "target_dueling", "network/act", "network/beta1", "network/beta2",
                      "network/beta_pow", "network/dueling_params", "network/eps", "network/gn", "network/hidden", "network/layers",
                      "network/lr", "network/m", "network/n_in", "network/n_out", "network/params", "network/v"}
    assert d["network/dueling_params"].shape == (nd,) == d["network/m"].shape == d["target_dueling"].shape and d["target"].shape == (n,)
    # ... and goes back in place, bit for bit
    net2 = object.__new__(rl.DuelingApproximator)
    net2.__dict__.update({k: (v.clone().zero_() if isinstance(v, torch.Tensor) else v) for k, v in net.__dict__.items() if k != "_grad"})
    tn2 = rl.TargetNetwork(net2, sync_freq=4, rho=0.5)
    checkpoint.load_state_dict(tn2, d)
    for k in ("params", "dueling_params", "m", "v", "beta_pow"):
        assert torch.equal(getattr(net2, k), getattr(net, k)), k
    assert torch.equal(tn2.target_dueling, tn.target_dueling) and torch.equal(tn2.target, tn.target) and tn2.n_optimise == 3
