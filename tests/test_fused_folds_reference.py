"""The fused vec-step for folded learners (n-step, Double DQN, DuelingNetwork), host side: the two new entry points
(rlhip_dqn_sample_fold_f32, rlhip_dqn_vec_step_fold_f32), the ctypes mirror of rlhip_dqn_fold_step_args, the argument checks that
need no device, the admission condition of run_fused_dqn_folded and its n-step warm-up guard against DQNLearner.optimise_'s own.
The device side is tests/test_gpu_fused_folds.py."""
import ctypes as C
import os
import subprocess
import tempfile
from types import SimpleNamespace as NS

import pytest

torch = pytest.importorskip("torch")

from rlhip import _lib  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbols_are_exported_and_declared():
    for name in ("rlhip_dqn_sample_fold_f32", "rlhip_dqn_vec_step_fold_f32"):
        assert hasattr(_lib.lib, name) and name in _lib._PROTOS and name in _lib.declared_symbols()
    assert _lib.lib.rlhip_abi_version() == 2  # entry points were added, nothing changed


def test_fold_step_args_mirror_has_the_c_layout():
    fields = [n for n, _ in _lib.DqnFoldStepArgs._fields_]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "rlhip.h"\nint main(void) {\n' \
          '    printf("%zu %zu", sizeof(rlhip_dqn_fold_step_args), sizeof(rlhip_dqn_step_args));\n' + \
          "".join(f'    printf(" %zu", offsetof(rlhip_dqn_fold_step_args, {n}));\n' for n in fields) + "    return 0;\n}\n"
    with tempfile.TemporaryDirectory() as d:
        with open(os.path.join(d, "t.c"), "w") as f:
            f.write(src)
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "t.c"), "-o", os.path.join(d, "t")], check=True)
        out = [int(x) for x in subprocess.run([os.path.join(d, "t")], capture_output=True, text=True, check=True).stdout.split()]
    assert out[0] == C.sizeof(_lib.DqnFoldStepArgs) and out[1] == C.sizeof(_lib.DqnStepArgs)
    assert out[2:] == [getattr(_lib.DqnFoldStepArgs, n).offset for n in fields]
    assert fields == ["base", "n_step", "double_dqn", "folded", "idx", "iota", "td", "fold_workspace", "dueling_params",
                      "target_dueling", "grad_dueling"]


FAKE = 0x10000  # a 64-byte aligned address that nothing dereferences: every call below is refused before a launch


def _ring(capacity, n_env, obs_dim, stored, where=FAKE):
    rb = _lib.Ring()
    if obs_dim <= 4:
        _lib.call("rlhip_ring_init", C.byref(rb), capacity, n_env, obs_dim, 4, where, None, None, None)
    else:
        _lib.call("rlhip_ring_init", C.byref(rb), capacity, n_env, obs_dim, 4, where, where, where, where)
    rb.len_rt, rb.len_sa = stored, stored + 1
    return rb


GOOD = dict(src=(8, 6, 4, 5), batch=16, n_step=3, double=1, h=64, na=2, act=0, params=FAKE, target=FAKE, folded=(1, 16, 4, 0))
BAD = [("a frame ring", dict(src=(8, 6, 5, 5)), "record rings"),
       ("obs_dim 1", dict(src=(8, 6, 1, 5), folded=(1, 16, 1, 0)), "obs_dim 2..4"),
       ("h not a multiple of 4", dict(h=66), "multiple of 4"),
       ("h > 256", dict(h=260), "multiple of 4"),
       ("h 0", dict(h=0), "multiple of 4"),
       ("na 5", dict(na=5), "na must be"),
       ("na 0", dict(na=0), "na must be"),
       ("act 2", dict(act=2), "act must be"),
       ("n_step 0", dict(n_step=0), "n_step"),
       ("n_step 33", dict(n_step=33, src=(64, 6, 4, 40)), "n_step"),
       ("batch 0", dict(batch=0), "bad arguments"),
       ("folded of another batch", dict(folded=(1, 17, 4, 0)), "n_env = batch"),
       ("folded of another obs_dim", dict(folded=(1, 16, 3, 0)), "n_env = batch"),
       ("fewer than n_step stored steps", dict(src=(8, 6, 4, 2)), "fewer than n_step"),
       ("an empty trajectory", dict(src=(8, 6, 4, 0), n_step=1), "empty"),
       ("double_dqn without the online net", dict(params=None), "double_dqn needs"),
       ("double_dqn without the target net", dict(target=None), "double_dqn needs")]


@pytest.mark.parametrize("what,change,message", BAD, ids=[b[0] for b in BAD])
def test_sample_fold_refuses_bad_arguments_without_a_device(what, change, message):
    kw = dict(GOOD, **change)
    src, folded = _ring(*kw["src"]), _ring(*kw["folded"], where=2 * FAKE)
    before = [(getattr(r, f)) for r in (src, folded) for f in ("head_sa", "len_sa", "head_rt", "len_rt")]
    with pytest.raises(_lib.RLHipArgumentError, match=message):
        _lib.call("rlhip_dqn_sample_fold_f32", C.byref(src), kw["batch"], kw["n_step"], kw["double"], 0.99, 1, 0, kw["h"], kw["na"],
                  kw["act"], kw["params"], kw["target"], C.byref(folded), None, None, None)
    assert before == [(getattr(r, f)) for r in (src, folded) for f in ("head_sa", "len_sa", "head_rt", "len_rt")]


def test_sample_fold_refuses_null_and_aliased_rings():
    src = _ring(8, 16, 4, 5)
    for a, b, message in ((None, C.byref(_ring(1, 16, 4, 0, 2 * FAKE)), "bad arguments"), (C.byref(src), None, "bad arguments"),
                          (C.byref(src), C.byref(src), "alias")):
        with pytest.raises(_lib.RLHipArgumentError, match=message):
            _lib.call("rlhip_dqn_sample_fold_f32", a, 16, 1, 0, 0.99, 1, 0, 64, 2, 0, None, None, b, None, None, None)


def test_vec_step_fold_refuses_before_anything_moves():
    """argument checks come before the first launch: NULL struct, NULL pointers, dueling pointers given in part"""
    with pytest.raises(_lib.RLHipArgumentError, match="args is NULL"):
        _lib.call("rlhip_dqn_vec_step_fold_f32", None, None)
    f = _lib.DqnFoldStepArgs()
    with pytest.raises(_lib.RLHipArgumentError, match="NULL argument"):
        _lib.call("rlhip_dqn_vec_step_fold_f32", C.byref(f), None)
    ring, folded = _ring(8, 6, 4, 5), _ring(1, 17, 4, 0, 2 * FAKE)
    a = f.base
    a.kind, a.n, a.layers, a.h, a.na, a.batch = 0, 6, 2, 64, 2, 16
    a.env_cfg = a.st = a.obs = a.params = a.actions = FAKE
    a.ring = C.addressof(ring)
    f.n_step, f.double_dqn = 3, 1
    f.dueling_params = FAKE
    with pytest.raises(_lib.RLHipArgumentError, match="all given or all NULL"):
        _lib.call("rlhip_dqn_vec_step_fold_f32", C.byref(f), None)
    f.dueling_params = None
    with pytest.raises(_lib.RLHipArgumentError, match="folded / idx / iota"):
        _lib.call("rlhip_dqn_vec_step_fold_f32", C.byref(f), None)
    f.folded, f.idx, f.iota = C.addressof(folded), FAKE, FAKE
    with pytest.raises(_lib.RLHipArgumentError, match="n_env = batch"):
        _lib.call("rlhip_dqn_vec_step_fold_f32", C.byref(f), None)
    f.n_step = 40
    with pytest.raises(_lib.RLHipArgumentError, match="n_step"):
        _lib.call("rlhip_dqn_vec_step_fold_f32", C.byref(f), None)
    assert (ring.head_sa, ring.len_sa, ring.head_rt, ring.len_rt) == (0, 6, 0, 5)


# ------------------------------------------------------------------------------------ run_fused_dqn_folded: admission
class _Reached(Exception):
    pass


def _fused_stub(net=None, container=None, break_tie=False, **learner_kw):
    """the objects the admission condition reads; a hook that says so when the condition lets the call through (the first action
    behind the condition is hook.push_)"""
    kw = dict(process_group=None, n_step=1, double_dqn=False)
    kw.update(learner_kw)
    learner = NS(approximator=NS(network=net or NS()), **kw)
    agent = NS(policy=NS(learner=learner, explorer=NS(is_break_tie=break_tie)), trajectory=NS(container=container or NS()))
    env = NS(continuous=False, is_f64=False)

    class Hook:
        def push_(self, *a):
            raise _Reached

    return agent, env, Hook()


@pytest.mark.parametrize("kw", [{}, {"n_step": 3}, {"double_dqn": True}, {"n_step": 5, "double_dqn": True},
                                {"net": NS(dueling_params=object())}, {"net": NS(dueling_params=object()), "n_step": 3, "double_dqn": True}],
                         ids=["plain", "nstep", "double", "nstep+double", "dueling", "dueling+nstep+double"])
def test_run_fused_dqn_folded_admits_the_folded_learners(kw):
    import rlhip as rl

    agent, env, hook = _fused_stub(**kw)
    with pytest.raises(_Reached):
        rl.run_fused_dqn_folded(agent, env, None, hook)
    # ... while run_fused_dqn keeps refusing every one of them but the plain learner, in the words its tests pin
    agent, env, hook = _fused_stub(**kw)
    if kw:
        with pytest.raises(NotImplementedError, match="fused DQN step"):
            rl.core.run_fused_dqn(agent, env, None, hook)
    else:
        with pytest.raises(_Reached):
            rl.core.run_fused_dqn(agent, env, None, hook)


def test_run_fused_dqn_folded_refuses_by_name():
    import rlhip as rl

    for kw, cause in (({"container": NS(sample_prioritized=None)}, "prioritized"), ({"break_tie": True}, "is_break_tie"),
                      ({"process_group": object()}, "process_group")):
        agent, env, hook = _fused_stub(n_step=3, double_dqn=True, **kw)
        with pytest.raises(NotImplementedError, match=cause):
            rl.run_fused_dqn_folded(agent, env, None, hook)
    for field, cause in (("continuous", "continuous"), ("is_f64", "Float64")):
        agent, env, hook = _fused_stub(double_dqn=True)
        setattr(env, field, True)
        with pytest.raises(NotImplementedError, match=cause):
            rl.run_fused_dqn_folded(agent, env, None, hook)


# ------------------------------------------------------------------------------------ the n-step warm-up guard
class _Traces:
    """a trajectory container of `n_env` envs that holds min(pushes, capacity) vec-steps"""

    def __init__(self, capacity, n_env):
        self.capacity, self.n_env, self.pushes = capacity, n_env, 0

    def __len__(self):
        return min(self.pushes, self.capacity)

    def n_transitions(self):
        return len(self) * self.n_env


class _Controller:
    def __init__(self, allow_every=1):
        self.calls, self.inserted, self.allow_every = 0, 0, allow_every

    def on_insert_(self, n=1):
        self.inserted += n

    def on_sample_(self):
        self.calls += 1
        return self.calls % self.allow_every == 0


def _gate_learner(n_step, update_freq, min_replay_history):
    from rlhip import dqn

    class Learner(dqn.DQNLearner):  # optimise_ as shipped up to the update itself, which only counts
        def __init__(self):
            self.n_step, self._nstep = n_step, (object() if n_step > 1 else None)
            self.double_dqn, self.vec_steps, self.draw_ctr, self.n_updates = True, 0, 0, 0
            self.update_freq, self.min_replay_history = update_freq, min_replay_history
            self.approximator = NS(network=None)

        def _update_(self, traces, prioritized):
            assert len(traces) >= self.n_step, "an update without one full window"
            self.draw_ctr += 1
            self.n_updates += 1
            return True

    return Learner()


@pytest.mark.parametrize("n_step,update_freq,min_replay_history,allow_every", [(3, 1, 0, 1), (3, 2, 0, 1), (4, 1, 12, 1), (2, 1, 0, 2),
                                                                               (1, 1, 0, 1), (5, 3, 7, 1)])
def test_nstep_warm_up_guard_moves_the_counters_as_the_learner_does(n_step, update_freq, min_replay_history, allow_every):
    """per-stage: push, then DQNLearner.optimise_; fused: the gate of run_fused_dqn_folded on the length the push WILL leave.  The same
    trajectory lengths 0 .. n_step + 2 and beyond the wrap: vec_steps, draw_ctr and the controller's calls agree after every step"""
    from rlhip import core

    cap, n_env = n_step + 1, 3
    a = (_gate_learner(n_step, update_freq, min_replay_history), NS(container=_Traces(cap, n_env), controller=_Controller(allow_every)))
    b = (_gate_learner(n_step, update_freq, min_replay_history), NS(container=_Traces(cap, n_env), controller=_Controller(allow_every)))
    asked_during_warm_up = 0
    for length in range(0, n_step + 4):  # the stored length BEFORE the step: 0 .. n_step + 2, then past the capacity
        la, ta = a
        assert len(ta.container) == min(length, cap)
        ta.container.pushes += 1  # rlhip.run: push!, then optimise!
        ta.controller.on_insert_(1)
        ua = la.optimise_(ta)
        lb, tb = b
        tb.controller.on_insert_(1)  # run_fused_dqn_folded: the gate first, the push inside the call
        ub = core._folded_update_gate(lb, tb, min(len(tb.container) + 1, tb.container.capacity))
        tb.container.pushes += 1
        if ub:
            lb.draw_ctr += 1
            lb.n_updates += 1
        assert bool(ua) == bool(ub), f"stored {length}: per-stage updates {ua}, fused {ub}"
        assert (la.vec_steps, la.draw_ctr, la.n_updates) == (lb.vec_steps, lb.draw_ctr, lb.n_updates) and la.vec_steps == length + 1
        assert (ta.controller.calls, ta.controller.inserted) == (tb.controller.calls, tb.controller.inserted)
        if length + 1 < n_step:
            assert not ub and lb.draw_ctr == 0
            asked_during_warm_up = tb.controller.calls
    assert asked_during_warm_up == 0, "the controller was asked before one full window was stored"
    assert a[0].n_updates > 0
