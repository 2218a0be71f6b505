"""Double DQN (`DQNLearner(double_dqn=True)`, rlhip_dqn_fold_double_f32 / rlhip_dqn3_fold_double_f32) -- the CPU half:

  * the target composed from the oracle's existing functions (tests/double_dqn_ref.py) against an independent torch restatement,
    `gather(Qt(s'), argmax(Q(s')))`;
  * the identity the device fold rests on: the oracle's DQN loss / gradient on the record (reward = y, terminal = 1) IS the
    autograd gradient of the Double DQN Huber loss (two- and three-layer nets);
  * header / ctypes / Julia signatures of the new calls agree; the keyword exists and the fused vec-step refuses it."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

import oracle
from double_dqn_ref import compose, loss_grad, top_two_gap, trained_nets
from test_julia_glue_signatures import GLUE, SCALARS, glue_ccalls, header_prototypes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GAMMA = 0.97


def _bf16(x):  # round to bf16 in the forward pass, identity in the backward pass
    return x + (x.bfloat16().float() - x).detach()


def _torch_q(layers, p, ns, h, na, act, x):
    f = torch.relu if act == 0 else torch.tanh
    if layers == 2:
        W1, b1 = p[:h * ns].reshape(ns, h).T, p[h * ns:h * ns + h]
        o = h * ns + h
        W2, b2 = p[o:o + na * h].reshape(h, na).T, p[o + na * h:]
        return W2 @ f(W1 @ x + b1[:, None]) + b2[:, None]
    o = 0
    W1 = p[o:o + h * ns].reshape(ns, h).T; o += h * ns
    b1 = p[o:o + h]; o += h
    W2 = p[o:o + h * h].reshape(h, h).T; o += h * h
    b2 = p[o:o + h]; o += h
    W3 = p[o:o + na * h].reshape(h, na).T; o += na * h
    b3 = p[o:]
    h1 = f(W1 @ x + b1[:, None])
    h2 = f(_bf16(W2) @ _bf16(h1) + b2[:, None])  # the bf16 hidden x hidden layer of oracle/rlo_mlp3.c
    return W3 @ h2 + b3[:, None]


def _batch(ns, na, b, seed):
    rng = np.random.default_rng(seed)
    s = rng.standard_normal((ns, b)).astype(np.float32)
    sn = (s + 0.1 * rng.standard_normal((ns, b))).astype(np.float32)
    a = rng.integers(0, na, b).astype(np.int32)
    r = rng.standard_normal(b).astype(np.float32)
    t = (rng.random(b) < 0.2).astype(np.uint8)
    return s, a, r, t, sn


@pytest.mark.parametrize("layers,ns,h,na,act", [(2, 4, 64, 2, 0), (2, 3, 100, 3, 1), (2, 2, 256, 4, 0), (3, 4, 128, 2, 0),
                                                (3, 3, 128, 3, 1)])
def test_composed_oracle_target_and_folded_gradient_vs_torch(layers, ns, h, na, act):
    b = 257
    p, pt = trained_nets(layers, ns, h, na, act, seed=ns + h, steps=60, batch=64)
    s, a, r, t, sn = _batch(ns, na, b, seed=h)
    assert t.any() and not t.all()
    y, astar, q, qt = compose(layers, ns, h, na, act, p, pt, r, t, sn, GAMMA)
    P, PT = torch.tensor(p, requires_grad=True), torch.tensor(pt)
    with torch.no_grad():
        tq, tqt = _torch_q(layers, P, ns, h, na, act, torch.tensor(sn)), _torch_q(layers, PT, ns, h, na, act, torch.tensor(sn))
        ta = tq.argmax(0)
        ty = torch.tensor(r) + GAMMA * (1 - torch.tensor(t, dtype=torch.float32)) * tqt.gather(0, ta[None])[0]
    # torch sums in another order (and, three-layer, rounds through its own bf16 cast): a few Float32 ulps of the Q scale
    qtol = (1e-5 if layers == 2 else 1e-4) * (1 + np.abs(q).max())
    np.testing.assert_allclose(tq.numpy(), q, rtol=0, atol=qtol)
    decisive = top_two_gap(q) > 4 * qtol
    assert decisive.mean() > 0.9
    assert np.array_equal(ta.numpy()[decisive], astar[decisive])
    np.testing.assert_allclose(ty.numpy()[decisive], y[decisive], rtol=0, atol=qtol)
    assert np.array_equal(y[t != 0], r[t != 0])  # a terminal sample: y = r exactly
    # the identity: the oracle's loss / gradient with (reward = y, terminal = 1) = autograd of huber(Q(s, a), y_double)
    ol, og = loss_grad(layers, ns, h, na, act, p, pt, s, a, y, sn, GAMMA)
    qa = _torch_q(layers, P, ns, h, na, act, torch.tensor(s))[torch.tensor(a, dtype=torch.long), torch.arange(b)]
    ref = torch.nn.HuberLoss(delta=1.0)(qa, torch.tensor(y))
    ref.backward()
    assert ol == pytest.approx(float(ref.detach()), rel=1e-4)
    # three-layer: the oracle rounds dz2 to bf16 for its two GEMMs (one bf16 ulp = 2^-8 relative), autograd does not
    gtol = 1e-5 if layers == 2 else 2.0 ** -7
    g = P.grad.numpy()
    assert np.abs(g - og).max() <= gtol * np.abs(og).max(), np.abs(g - og).max() / np.abs(og).max()
    # ... and the gamma handed to the gradient call cannot matter on such a record
    ol2, og2 = loss_grad(layers, ns, h, na, act, p, pt, s, a, y, sn, 0.5)
    assert ol2 == ol and np.array_equal(og2, og)


def test_signatures_of_the_new_calls_agree():
    from rlhip import _lib

    protos = header_prototypes()
    ctype = {_lib.i32: "Int32", _lib.i64: "Int64", _lib.f32: "Float32"}
    calls = {c[0]: c for c in glue_ccalls()}
    for name in ("rlhip_dqn_double_workspace_bytes", "rlhip_dqn_fold_double_f32", "rlhip_dqn3_fold_double_f32"):
        assert name in protos and name in _lib._PROTOS and hasattr(_lib.lib, name), name
        rt, plist = protos[name]
        res, args = _lib._PROTOS[name]
        assert ctype[res] == rt and [ctype.get(a, "ptr") for a in args] == plist, name
        assert name in calls and calls[name][1] == rt and calls[name][2] == plist, name
    assert protos["rlhip_dqn_fold_double_f32"][1].count("ptr") == 8 and len(protos["rlhip_dqn3_fold_double_f32"][1]) == 15
    assert _lib.lib.rlhip_abi_version() == 2
    # the Julia glue (no Julia runtime in the test image: structure only, whitespace-tolerant).  The keyword exists, and in the body
    # of optimise!(::HipDQNLearner, ...) a branch on L.double_dqn into optimise_double! stands in front of the first plain update call
    src = open(GLUE).read()
    assert re.search(r"function\s+HipDQNLearner\(tn::HipTargetNetwork;[^)]*\bdouble_dqn\s*=\s*false\b", src, flags=re.S)
    body = src[src.index("function optimise!(L::HipDQNLearner"):]
    body = body[:body.index("\nend\n")]
    branch = re.search(r"L\.double_dqn\s*(&&|\?)\s*(return\s+)?optimise_double!\(L,\s*t\)|if\s+L\.double_dqn\b", body)
    assert branch and branch.start() < body.index(":rlhip_dqn_update_f32") and branch.start() < body.index(":rlhip_dqn3_update_f32")
    dbl = src[src.index("function optimise_double!(L::HipDQNLearner"):]
    dbl = dbl[:dbl.index("\nend\n")]
    order = [dbl.index(k) for k in (":rlhip_ring_sample_indices", "fold_double!(", ":rlhip_dqn_grad_idx_f32", ":rlhip_dqn3_grad_f32")]
    assert order == sorted(order) and "L.folded.rb" in dbl and "L.iota.ptr" in dbl


def test_workspace_bytes_and_argument_errors_without_a_device():
    from rlhip import _lib

    wb = _lib.lib.rlhip_dqn_double_workspace_bytes
    assert wb(4, 128, 2, 512, 2) == 0
    assert wb(4, 128, 2, 512, 3) == 4 * 512 * 4 + 2 * (2 * 512 * 4)
    assert wb(3, 256, 3, 333, 3) >= (3 + 3 + 3) * 333 * 4 and wb(3, 256, 3, 333, 3) % 256 == 0
    assert wb(4, 128, 2, 512, 4) == -1 and wb(4, 128, 2, 0, 2) == -1
    with pytest.raises(_lib.RLHipArgumentError):  # validation happens before any HIP call
        _lib.call("rlhip_dqn_fold_double_f32", None, 128, 2, 0, None, None, None, 8, 0.99, None, None, None, None)


class _Reached(Exception):
    pass


def _fused_stub(**learner_kw):
    """the objects run_fused_dqn's admission condition reads, every field on its admitting value; a hook that says so when the
    condition lets the call through (its first action behind the condition is hook.push_)"""
    from types import SimpleNamespace as NS

    learner = NS(approximator=NS(network=NS()), explorer=None, process_group=None, n_step=1, **learner_kw)
    agent = NS(policy=NS(learner=learner, explorer=NS(is_break_tie=False)), trajectory=NS(container=NS()))
    env = NS(continuous=False, is_f64=False)

    class Hook:
        def push_(self, *a):
            raise _Reached

    return agent, env, Hook()


def test_learner_keyword_and_fused_step_refusal():
    import rlhip as rl
    from rlhip import core, dqn

    sig = inspect.signature(dqn.DQNLearner.__init__)
    assert sig.parameters["double_dqn"].default is False
    assert list(sig.parameters)[-1] == "double_dqn"  # appended: no positional call of the parent's signature changes meaning
    # the fused vec-step admits the plain learner (with and without the attribute) and refuses double_dqn = True, saying why
    for kw in ({}, {"double_dqn": False}):
        agent, env, hook = _fused_stub(**kw)
        with pytest.raises(_Reached):
            core.run_fused_dqn(agent, env, None, hook)
    agent, env, hook = _fused_stub(double_dqn=True)
    with pytest.raises(NotImplementedError, match="double_dqn"):
        core.run_fused_dqn(agent, env, None, hook)
    assert getattr(rl.DoubleTargetFold, "checkpoint_scratch", False)


def test_in_place_fold_takes_no_indices_and_the_helper_is_made_on_demand():
    import rlhip as rl
    from types import SimpleNamespace as NS

    with pytest.raises(ValueError, match="idx = None"):  # refused before anything touches a device
        rl.DoubleTargetFold().fold(NS(n_env=4), torch.arange(4), None, None, None, 0.9, in_place=True)
    # the learner holds the flag; the fold helper (scratch) appears with the first folded update, so a checkpoint's flag is enough
    src_init = inspect.signature(rl.DQNLearner.__init__)
    assert "double_dqn" in src_init.parameters
    from rlhip import checkpoint

    class Owner:
        pass

    o = Owner()
    o.double_dqn, o._double, o.scratch = True, None, rl.DoubleTargetFold()
    Owner.__module__ = "rlhip.fake"
    assert checkpoint.state_dict(o) == {"double_dqn": True}
