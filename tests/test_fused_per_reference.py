"""The fused vec-step of prioritized-replay DQN learners, host side: the two new entry points (rlhip_per_writeback_f32,
rlhip_dqn_vec_step_per_f32), the ctypes mirror of rlhip_dqn_per_step_args, the argument checks that need no device, the admission
condition of run_fused_dqn_prioritized and the per-step fields it hands to the call against what the per-stage learner would use.
The device side is tests/test_gpu_per_writeback.py and tests/test_gpu_fused_per.py."""
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
    for name in ("rlhip_per_writeback_f32", "rlhip_dqn_vec_step_per_f32"):
        assert hasattr(_lib.lib, name) and name in _lib._PROTOS and name in _lib.declared_symbols()
    assert _lib.lib.rlhip_abi_version() == 2  # entry points were added, nothing changed


def test_per_step_args_mirror_has_the_c_layout():
    fields = [n for n, _ in _lib.DqnPerStepArgs._fields_]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "rlhip.h"\nint main(void) {\n' \
          '    printf("%zu %zu", sizeof(rlhip_dqn_per_step_args), sizeof(rlhip_dqn_fold_step_args));\n' + \
          "".join(f'    printf(" %zu", offsetof(rlhip_dqn_per_step_args, {n}));\n' for n in fields) + "    return 0;\n}\n"
    with tempfile.TemporaryDirectory() as d:
        with open(os.path.join(d, "t.c"), "w") as f:
            f.write(src)
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "t.c"), "-o", os.path.join(d, "t")], check=True)
        out = [int(x) for x in subprocess.run([os.path.join(d, "t")], capture_output=True, text=True, check=True).stdout.split()]
    assert out[0] == C.sizeof(_lib.DqnPerStepArgs) and out[1] == C.sizeof(_lib.DqnFoldStepArgs)
    assert out[2:] == [getattr(_lib.DqnPerStepArgs, n).offset for n in fields]
    assert fields == ["fold", "tree", "default_priority", "per_eps", "per_alpha", "per_beta", "key", "prio", "is_weights", "priority_out"]


FAKE = 0x10000  # a 64-byte aligned address that nothing dereferences: every call below is refused before a launch


def _ring(capacity, n_env, obs_dim, stored, where=FAKE):
    rb = _lib.Ring()
    _lib.call("rlhip_ring_init", C.byref(rb), capacity, n_env, obs_dim, 4, where, None, None, None)
    rb.len_rt, rb.len_sa = stored, stored + 1
    return rb


def test_writeback_refuses_bad_arguments_without_a_device():
    wb = lambda *a: _lib.call("rlhip_per_writeback_f32", *a, None)  # noqa: E731
    for args, message in (((FAKE, 0, FAKE, FAKE, 4, 1e-6, 0.6, 2 * FAKE), "bad sizes"), ((FAKE, 8, FAKE, FAKE, -1, 1e-6, 0.6, 2 * FAKE), "bad sizes"),
                          ((FAKE, 8, FAKE, FAKE, 4, -1.0, 0.6, 2 * FAKE), "bad arguments"), ((FAKE, 8, FAKE, FAKE, 4, 1e-6, -0.5, 2 * FAKE), "bad arguments"),
                          ((None, 8, FAKE, FAKE, 4, 1e-6, 0.6, 2 * FAKE), "NULL"), ((FAKE, 8, None, FAKE, 4, 1e-6, 0.6, 2 * FAKE), "NULL"),
                          ((FAKE, 8, FAKE, None, 4, 1e-6, 0.6, 2 * FAKE), "NULL"), ((FAKE, 8, FAKE, FAKE, 4, 1e-6, 0.6, None), "NULL"),
                          ((FAKE, 8, FAKE, FAKE, 4, 1e-6, 0.6, FAKE), "overlap"), ((FAKE, 8, FAKE, FAKE, 4, 1e-6, 0.6, FAKE + 12), "overlap"),
                          ((FAKE, 8, FAKE, FAKE + 12, 4, 1e-6, 0.6, FAKE), "overlap"), ((FAKE, 8, FAKE, FAKE, 1 << 31, 1e-6, 0.6, 1 << 40), "too many")):
        with pytest.raises(_lib.RLHipArgumentError, match=message):
            wb(*args)
    wb(None, 8, None, None, 0, 1e-6, 0.6, None)  # n == 0: OK without a launch, as the two shipped entry points


def _good_step(ring, folded):
    """a call that would pass every check (n_step 3, Double DQN, beta > 0, an update): the cases below break one thing each"""
    p = _lib.DqnPerStepArgs()
    f, a = p.fold, p.fold.base
    a.kind, a.n, a.layers, a.h, a.na, a.batch, a.do_update = 0, 6, 2, 64, 2, 16, 1
    a.env_cfg = a.st = a.obs = a.params = a.actions = FAKE
    a.target = a.m = a.v = a.beta_pow = a.workspace = a.grad = a.loss = FAKE
    a.ring = C.addressof(ring)
    f.n_step, f.double_dqn = 3, 1
    f.folded, f.idx, f.iota, f.td = C.addressof(folded), FAKE, FAKE, FAKE
    p.tree, p.default_priority, p.per_eps, p.per_alpha, p.per_beta = FAKE, 100.0, 1e-6, 0.6, 0.4
    p.key, p.prio, p.is_weights, p.priority_out = FAKE, FAKE, FAKE, 2 * FAKE
    return p


def _set(p, path, value):
    obj = p
    *head, last = path.split(".")
    for h in head:
        obj = getattr(obj, h)
    setattr(obj, last, value)


BAD_STEP = [("NULL tree", {"tree": None}, "NULL tree"),
            ("default_priority 0", {"default_priority": 0.0}, "default_priority"),
            ("default_priority < 0", {"default_priority": -1.0}, "default_priority"),
            ("per_eps < 0", {"per_eps": -1e-3}, "per_eps"),
            ("per_alpha < 0", {"per_alpha": -0.5}, "per_eps"),
            ("per_beta < 0", {"per_beta": -0.1}, "per_eps"),
            ("is_weights missing with beta > 0", {"is_weights": None}, "is_weights"),
            ("key missing", {"key": None}, "missing"),
            ("prio missing", {"prio": None}, "missing"),
            ("td missing", {"fold.td": None}, "missing"),
            ("priority_out missing", {"priority_out": None}, "missing"),
            ("priority_out is td", {"priority_out": FAKE}, "overlap"),
            ("priority_out overlaps td", {"priority_out": FAKE + 60}, "overlap"),
            ("n_step 0", {"fold.n_step": 0}, "n_step"),
            ("n_step 33", {"fold.n_step": 33}, "n_step"),
            ("n_step above the capacity", {"fold.n_step": 9}, "n_step"),
            ("fewer than n_step stored steps", {"fold.n_step": 8}, "fewer than n_step"),
            ("h not a multiple of 4", {"fold.base.h": 66}, "multiple of 4"),
            ("dueling pointers given in part", {"fold.dueling_params": FAKE}, "all given or all NULL"),
            ("no folded ring where a fold runs", {"fold.folded": None}, "folded / idx / iota")]


@pytest.mark.parametrize("what,change,message", BAD_STEP, ids=[b[0] for b in BAD_STEP])
def test_vec_step_per_refuses_before_anything_moves(what, change, message):
    ring, folded = _ring(8, 6, 4, 5), _ring(1, 16, 4, 0, 2 * FAKE)
    p = _good_step(ring, folded)
    for path, value in change.items():
        _set(p, path, value)
    with pytest.raises(_lib.RLHipArgumentError, match=message):
        _lib.call("rlhip_dqn_vec_step_per_f32", C.byref(p), None)
    assert (ring.head_sa, ring.len_sa, ring.head_rt, ring.len_rt) == (0, 6, 0, 5)
    assert (folded.head_sa, folded.len_sa, folded.head_rt, folded.len_rt) == (0, 1, 0, 0)


def test_vec_step_per_further_refusals():
    with pytest.raises(_lib.RLHipArgumentError, match="args is NULL"):
        _lib.call("rlhip_dqn_vec_step_per_f32", None, None)
    with pytest.raises(_lib.RLHipArgumentError, match="NULL argument"):
        _lib.call("rlhip_dqn_vec_step_per_f32", C.byref(_lib.DqnPerStepArgs()), None)
    # a frame ring: refused although n_step == 1 without Double DQN folds nothing (every gradient entry point reads a record ring)
    frames = _lib.Ring()
    _lib.call("rlhip_ring_init", C.byref(frames), 8, 6, 5, 4, FAKE, FAKE, FAKE, FAKE)
    frames.len_rt, frames.len_sa = 5, 6
    p = _good_step(frames, _ring(1, 16, 4, 0, 2 * FAKE))
    p.fold.base.kind, p.fold.n_step, p.fold.double_dqn = 0, 1, 0
    with pytest.raises(_lib.RLHipArgumentError):
        _lib.call("rlhip_dqn_vec_step_per_f32", C.byref(p), None)
    assert (frames.len_sa, frames.len_rt) == (6, 5)
    # the n_step == 1 learner without weights needs neither a folded ring nor is_weights; the network shapes are checked although
    # nothing is folded
    ring = _ring(8, 6, 4, 5)
    p = _good_step(ring, _ring(1, 16, 4, 0, 2 * FAKE))
    p.fold.n_step, p.fold.double_dqn, p.fold.folded, p.fold.iota, p.per_beta, p.is_weights = 1, 0, None, None, 0.0, None
    p.fold.base.h = 66
    with pytest.raises(_lib.RLHipArgumentError, match="multiple of 4"):
        _lib.call("rlhip_dqn_vec_step_per_f32", C.byref(p), None)
    assert (ring.head_sa, ring.len_sa, ring.head_rt, ring.len_rt) == (0, 6, 0, 5)


# ------------------------------------------------------------------------------------ run_fused_dqn_prioritized: admission
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


def _prioritized(n_step=1):
    return NS(sample_prioritized=None, n_step=n_step)


@pytest.mark.parametrize("kw", [{}, {"n_step": 3}, {"double_dqn": True}, {"n_step": 5, "double_dqn": True},
                                {"net": NS(dueling_params=object())}, {"net": NS(dueling_params=object()), "n_step": 3, "double_dqn": True}],
                         ids=["plain", "nstep", "double", "nstep+double", "dueling", "dueling+nstep+double"])
def test_run_fused_dqn_prioritized_admits_every_prioritized_form(kw):
    import rlhip as rl

    agent, env, hook = _fused_stub(container=_prioritized(kw.get("n_step", 1)), **kw)
    with pytest.raises(_Reached):
        rl.run_fused_dqn_prioritized(agent, env, None, hook)
    # ... while the two shipped fused loops keep refusing prioritized traces
    for loop, words in ((rl.run_fused_dqn_folded, "prioritized"), (rl.run_fused_dqn, "fused DQN step")):
        agent, env, hook = _fused_stub(container=_prioritized(kw.get("n_step", 1)), **kw)
        with pytest.raises(NotImplementedError, match=words):
            loop(agent, env, None, hook)


def test_run_fused_dqn_prioritized_refuses_by_name():
    import rlhip as rl

    agent, env, hook = _fused_stub(n_step=3)
    with pytest.raises(NotImplementedError, match="run_fused_dqn_folded"):  # uniform traces: the other loop, by name
        rl.run_fused_dqn_prioritized(agent, env, None, hook)
    for kw, cause in (({"break_tie": True}, "is_break_tie"), ({"process_group": object()}, "process_group")):
        agent, env, hook = _fused_stub(container=_prioritized(3), n_step=3, double_dqn=True, **kw)
        with pytest.raises(NotImplementedError, match=cause):
            rl.run_fused_dqn_prioritized(agent, env, None, hook)
    for field, cause in (("continuous", "continuous"), ("is_f64", "Float64")):
        agent, env, hook = _fused_stub(container=_prioritized())
        setattr(env, field, True)
        with pytest.raises(NotImplementedError, match=cause):
            rl.run_fused_dqn_prioritized(agent, env, None, hook)
    # traces that mask windows of another width: DQNLearner.optimise_'s ValueError
    for learner_n, traces_n in ((3, 1), (1, 3), (3, 5)):
        agent, env, hook = _fused_stub(container=_prioritized(traces_n), n_step=learner_n)
        with pytest.raises(ValueError, match=rf"n_step = {learner_n}\) needs CircularPrioritizedTraces"):
            rl.run_fused_dqn_prioritized(agent, env, None, hook)
    # the refusal of the folded loop names this one
    agent, env, hook = _fused_stub(container=_prioritized())
    with pytest.raises(NotImplementedError, match="run_fused_dqn_prioritized"):
        rl.run_fused_dqn_folded(agent, env, None, hook)


# ------------------------------------------------------------------------------------ the per-step fields
def _schedule(n_updates):
    return min(1.0, 0.4 + 0.125 * n_updates)


class _Traces:
    """CircularPrioritizedTraces as far as the hosts read it, on CPU tensors; `pushes` counts the stored vec-steps"""
    n_step = 1
    default_priority = 100.0

    def __init__(self, capacity, n_env):
        self.capacity, self.n_env, self.pushes = capacity, n_env, 0
        self.rb = _lib.Ring()
        self.state = torch.zeros(4)
        self.priorities = torch.zeros(2 * capacity * n_env)

    def sample_prioritized(self, *a):
        raise AssertionError("the recorded per-stage update draws nothing")

    def __len__(self):
        return min(self.pushes, self.capacity)

    def n_transitions(self):
        return len(self) * self.n_env


class _Controller:
    def __init__(self, answers):
        self.answers, self.inserted = list(answers), 0

    def on_insert_(self, n=1):
        self.inserted += n

    def on_sample_(self):
        return self.answers.pop(0)


def _host_agent(record):
    """a prioritized DQN agent whose device work is replaced by `record`: real DQNLearner gate and tail, real TargetNetwork counter,
    real EpsilonGreedyExplorer schedule"""
    from rlhip import dqn

    net = NS(layers=2, hidden=64, n_out=2, n_in=4, act=0, params=torch.zeros(8), m=torch.zeros(8), v=torch.zeros(8),
             beta_pow=torch.zeros(2), gn=torch.zeros(1), lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, optimise_=lambda g, **kw: None)
    tn = object.__new__(dqn.TargetNetwork)
    tn.network, tn.sync_freq, tn.rho, tn.n_optimise, tn.target, tn.target_packed = net, 2, 0.0, 1, torch.zeros(8), None

    class Learner(dqn.DQNLearner):
        def __init__(self):
            self.n_step, self._nstep, self.double_dqn, self._double = 1, None, False, None
            self.per_eps, self.per_alpha, self.per_beta = 1e-6, 0.6, _schedule
            self.approximator, self.batchsize, self.gamma, self.delta = tn, 4, 0.99, 1.0
            self.min_replay_history, self.update_freq, self.max_grad_norm = 0, 1, 1.0
            self.seed, self.draw_ctr, self.n_updates, self.vec_steps, self.process_group = 3, 7, 2, 0, None
            self.grad, self.loss, self.workspace = torch.zeros(8), torch.zeros(1), torch.zeros(8, dtype=torch.uint8)
            self.td, self.is_weights = torch.zeros(4), torch.ones(4)
            self._idx = self._key = None
            self._prio = torch.ones(4)

        def _update_(self, traces, prioritized):  # the stages that move host state, as shipped; the device stages only leave their arguments
            assert prioritized
            self._is_weights_()
            record("update", self.draw_ctr)
            return self._exchange_and_apply_()

    learner = Learner()
    ex = dqn.EpsilonGreedyExplorer(0.05, kind="exp", decay_steps=20, seed=4, step=5)
    policy = NS(learner=learner, explorer=ex, _actions=torch.zeros(3, dtype=torch.int32), _q=torch.zeros(2, 3))
    traces = _Traces(8, 3)
    traj = NS(container=traces, controller=_Controller([True, False, True]))
    agent = NS(policy=policy, trajectory=traj, push_=lambda *a: None)
    return agent, learner, ex, tn, traces


def test_per_step_fields_are_those_the_per_stage_learner_would_use(monkeypatch):
    """three vec-steps (update, the controller says no, update) with the launch helper recorded: eps, explorer_step, draw_ctr,
    do_update, do_sync and the scheduled beta of rlhip_dqn_vec_step_per_f32 against the per-stage learner's own host code"""
    import rlhip as rl
    from rlhip import core, dqn, ops

    # ---- per-stage: QBasedPolicy.plan_'s explorer lines, the push, DQNLearner.optimise_ with its device calls recorded
    stage = []
    agent, learner, ex, tn, traces = _host_agent(lambda *a: stage.append(a))
    host_ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731  (the stand-ins live in host memory)
    for mod in (dqn, ops):
        monkeypatch.setattr(mod, "ptr", host_ptr)
        monkeypatch.setattr(mod, "stream_ptr", lambda: None)
    monkeypatch.setattr(dqn, "call", lambda name, *a: stage.append((name, a[2])))  # rlhip_per_is_weights_f32(prio, n, beta, ...)
    monkeypatch.setattr(ops, "polyak_", lambda *a: stage.append(("sync",)))
    want = []
    for _ in range(3):
        eps, step = ex.get_eps(), ex.step
        ex.step += 1
        traces.pushes += 1
        agent.trajectory.controller.on_insert_(1)
        del stage[:]
        updated = bool(learner.optimise_(agent.trajectory))
        row = dict(eps=eps, explorer_step=step, do_update=int(updated), do_sync=int(("sync",) in stage))
        if updated:
            row["per_beta"] = pytest.approx([a[1] for a in stage if a[0] == "rlhip_per_is_weights_f32"][0], rel=1e-7)  # (a C float)
            row["draw_ctr"] = [a[1] for a in stage if a[0] == "update"][0]
        want.append(row)
    assert [w["do_update"] for w in want] == [1, 0, 1] and [w["do_sync"] for w in want] == [1, 0, 0]
    final = (learner.draw_ctr, learner.n_updates, learner.vec_steps, ex.step, tn.n_optimise, agent.trajectory.controller.inserted)
    # ---- fused: the same objects, built again; the call itself replaced
    agent, learner, ex, tn, traces = _host_agent(lambda *a: None)
    env = NS(continuous=False, is_f64=False, kind=0, cfg=C.c_int(0), _st=C.c_int(0), n=3, seed=1, env_id_base=0, device="cpu",
             state=lambda: torch.zeros(4, 3), _last_obs=torch.zeros(4, 3))
    got = []

    def fake_call(name, args, stream):
        assert name == "rlhip_dqn_vec_step_per_f32"
        p = args._obj
        a = p.fold.base
        got.append(dict(eps=a.eps, explorer_step=a.explorer_step, do_update=a.do_update, do_sync=a.do_sync, per_beta=p.per_beta,
                        draw_ctr=a.draw_ctr))
        assert p.fold.n_step == 1 and p.fold.double_dqn == 0 and p.default_priority == 100.0
        assert p.priority_out == learner.td.data_ptr() and p.fold.td not in (None, p.priority_out)
        assert p.is_weights == learner.is_weights.data_ptr() and p.key == learner._key.data_ptr() and p.prio == learner._prio.data_ptr()
        traces.pushes += 1

    monkeypatch.setattr(_lib, "call", fake_call)
    rl.run_fused_dqn_prioritized(agent, env, core.StopAfterNSteps(3))
    assert len(got) == 3
    for g, w in zip(got, want):
        for k, v in w.items():
            assert g[k] == v, f"{k}: fused {g[k]}, per-stage {v}"
    assert final == (learner.draw_ctr, learner.n_updates, learner.vec_steps, ex.step, tn.n_optimise, agent.trajectory.controller.inserted)
    assert learner._idx is None, "the per-stage 1-step learner without Double DQN sets no _idx"
