"""The entries of csrc/dqn_batch.hip at the C boundary, and the Python refusals in front of them.  No GPU: every argument rule returns
RLHIP_EINVAL with its message before any launch (the pointers handed over are never dereferenced), and every refusal of
rlhip/dqn.py / rlhip/core.py is raised before any C call (the objects live on CPU tensors or are plain namespaces)."""
import ctypes as C
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

FAKE = 0x1000  # a non-NULL address no check may follow


def _lib():
    from rlhip import _lib

    return _lib


def test_library_exports_the_three_entries():
    _lib_ = _lib()
    for name in ("rlhip_dqn_plan_obsn_f32", "rlhip_dqn_grad_batch_f32", "rlhip_dqn_batch_workspace_bytes"):
        assert hasattr(_lib_.lib, name), name
        assert name in _lib_.declared_symbols()
    assert _lib_.lib.rlhip_abi_version() == 2


def _grad(ns=6, h=128, na=3, act=0, batch=32, null=None):
    p = {k: FAKE for k in ("params", "target", "s", "a", "r", "term", "sn", "ws", "grad", "loss")}
    if null:
        p[null] = None
    _lib().call("rlhip_dqn_grad_batch_f32", ns, h, na, act, p["params"], p["target"], p["s"], p["a"], p["r"], p["term"], p["sn"], batch,
                0.99, None, None, 0, 1.0, p["ws"], p["grad"], p["loss"], None, None)


@pytest.mark.parametrize("kw,message", [(dict(ns=4), "obs dim must be 5..16"), (dict(ns=17), "obs dim must be 5..16"),
                                        (dict(h=6), "multiple of 4"), (dict(h=260), "multiple of 4"), (dict(h=0), "multiple of 4"),
                                        (dict(na=0), "na must be 1..4"), (dict(na=5), "na must be 1..4"), (dict(act=2), "act must be"),
                                        (dict(batch=0), "empty batch")] +
                         [(dict(null=k), "NULL argument") for k in ("params", "target", "s", "a", "r", "term", "sn", "ws", "grad", "loss")])
def test_grad_batch_refuses_before_any_launch(kw, message):
    with pytest.raises(_lib().RLHipArgumentError, match=message):
        _grad(**kw)


def test_grad_batch_refusal_names_the_record_ring_entry():
    with pytest.raises(_lib().RLHipArgumentError, match="rlhip_dqn_grad_idx_f32"):
        _grad(ns=4)


def test_batch_workspace_bytes():
    f = _lib().lib.rlhip_dqn_batch_workspace_bytes
    np_ = 6 * 128 + 128 + 3 * 128 + 3
    assert f(6, 128, 3, 1) == (np_ + 1) * 4 and f(6, 128, 3, 64) == (np_ + 1) * 4 and f(6, 128, 3, 65) == 2 * (np_ + 1) * 4
    assert f(6, 128, 3, 64 * 256) == f(6, 128, 3, 1 << 20) == 256 * (np_ + 1) * 4  # a larger batch gives the workgroups further tiles
    for bad in ((4, 128, 3, 32), (17, 128, 3, 32), (6, 6, 3, 32), (6, 260, 3, 32), (6, 128, 0, 32), (6, 128, 5, 32), (6, 128, 3, 0)):
        assert f(*bad) == -1, bad


def _plan(ns=6, h=128, na=3, act=0, n=8, params=FAKE, obs=FAKE, actions=FAKE):
    _lib().call("rlhip_dqn_plan_obsn_f32", params, ns, h, na, act, obs, n, 0.1, 1, 0, 1, actions, None, None)


@pytest.mark.parametrize("kw,message", [(dict(ns=4), "rlhip_dqn_plan_f32"), (dict(ns=2), "rlhip_dqn_plan_f32"), (dict(ns=17), "rlhip_dqn_plan_f32"),
                                        (dict(na=0), "na must be 1..4"), (dict(na=5), "na must be 1..4"), (dict(h=0), "hidden"),
                                        (dict(act=3), "act must be"), (dict(params=None), "NULL argument"), (dict(obs=None), "NULL argument"),
                                        (dict(actions=None), "NULL argument")])
def test_plan_obsn_refuses_before_any_launch(kw, message):
    with pytest.raises(_lib().RLHipArgumentError, match=message):
        _plan(**kw)


def test_plan_obsn_takes_an_empty_env_set():
    _plan(n=0)  # a no-op: nothing is launched, no pointer is followed


# ------------------------------------------------------------------------------------------ Python: refusals before any C call
def _cpu_net(n_in, h=8, n_out=3):
    import rlhip as rl

    return rl.HipApproximator(n_in, h, n_out, params=np.zeros(n_in * h + h + n_out * h + n_out, np.float32), device="cpu")


def test_learner_constructs_on_wide_observations_and_refuses_the_rest():
    import rlhip as rl

    learner = rl.DQNLearner(rl.TargetNetwork(_cpu_net(6)), batchsize=16)
    assert learner._wide and learner.workspace.numel() == int(_lib().lib.rlhip_dqn_batch_workspace_bytes(6, 8, 3, 16))
    assert not rl.DQNLearner(rl.TargetNetwork(_cpu_net(4)), batchsize=16)._wide
    with pytest.raises(ValueError, match="up to 16"):
        rl.DQNLearner(rl.TargetNetwork(_cpu_net(17)), batchsize=16)
    net3 = NS(n_in=6, hidden=128, n_out=3, layers=3, act=0, params=torch.zeros(8), packed=torch.zeros(8))
    with pytest.raises(NotImplementedError, match="layers = 2"):
        rl.DQNLearner(rl.TargetNetwork(net3), batchsize=16)
    for net in (net3, NS(n_in=20, layers=2)):
        policy = rl.QBasedPolicy(NS(approximator=NS(network=net)), NS(is_break_tie=False))
        with pytest.raises((NotImplementedError, ValueError), match="QBasedPolicy"):
            policy.plan_(None)


def _traces(**kw):
    d = dict(records_layout=False, dtype=torch.float32, obs_dim=6, n_env=4, capacity=8)
    d.update(kw)
    return NS(**d)


def test_learner_refuses_rings_it_cannot_train_on():
    import rlhip as rl

    learner = rl.DQNLearner(rl.TargetNetwork(_cpu_net(6)), batchsize=16)
    traj = lambda tr: NS(container=tr)  # noqa: E731
    with pytest.raises(NotImplementedError, match="convolutional"):  # UInt8 frames / n_stack
        learner.optimise_(traj(_traces(dtype=torch.uint8)))
    with pytest.raises(ValueError, match="up to 16"):
        learner.optimise_(traj(_traces(obs_dim=24)))
    with pytest.raises(ValueError, match="components, the network takes 6"):
        learner.optimise_(traj(_traces(obs_dim=8)))
    with pytest.raises(NotImplementedError, match="CircularPrioritizedFrameTraces"):  # a prioritized ring of another class
        learner.optimise_(traj(_traces(sample_prioritized=None)))
    narrow = rl.DQNLearner(rl.TargetNetwork(_cpu_net(4)), batchsize=16)
    with pytest.raises(NotImplementedError, match="convolutional"):  # a frame ring under a narrow network: UInt8 frames
        narrow.optimise_(traj(_traces(dtype=torch.uint8, obs_dim=4)))
    assert learner.vec_steps == 0 and narrow.vec_steps == 0  # nothing moved


@pytest.mark.parametrize("loop,container", [("run_fused_dqn", NS()), ("run_fused_dqn_folded", NS()),
                                            ("run_fused_dqn_prioritized", NS(sample_prioritized=None, n_step=1))])
def test_fused_loops_send_wide_observations_to_the_per_stage_loop(loop, container):
    import rlhip as rl

    class Hook:
        def push_(self, *a):
            raise AssertionError("the refusal comes before anything is pushed")

    learner = NS(approximator=NS(network=NS(n_in=6, layers=2)), process_group=None, n_step=1, double_dqn=False)
    agent = NS(policy=NS(learner=learner, explorer=NS(is_break_tie=False)), trajectory=NS(container=container))
    with pytest.raises(NotImplementedError, match=r"n_in > 4.*rlhip\.run"):
        getattr(rl, loop)(agent, NS(continuous=False, is_f64=False), None, Hook())
