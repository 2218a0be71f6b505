#!/usr/bin/env python3
"""The ABI call trace of the DQN host layer, recorded on the CPU -> tests/golden/dqn_host_trace.json.

What DQNLearner.optimise_, NStepBatchSampler, DoubleTargetFold, run_fused_dqn and run_fused_dqn_folded hand to the C ABI -- which
entry points, with which arguments, in which order -- is everything the host layer decides: the numerics live behind the ABI.  This
script drives the real classes on CPU tensors with the launch helpers replaced by recorders and writes the ordered list of

    ABI name + normalised arguments             (`call` of rlhip.dqn / rlhip.trajectory / rlhip.core / rlhip.ops / rlhip._lib)
    traces.sample_prioritized / sample_indices / set_priority_        (methods of the stub traces)
    controller.on_insert_ / on_sample_                                (stub controller)
    approximator.optimise_(grad, clip_norm, grad_scale)               (stub target network)

and, after every optimise_ call / fused vec-step, the learner's counters, which of `_idx` / `_key` / `_prio` are set (and to which
buffer), the key list of checkpoint.state_dict(learner) and the arguments a callable `per_beta` was evaluated with during the call
(how often and with what; where between two launches the host evaluates it is not pinned).  tests/test_dqn_host_call_trace.py compares a fresh recording with the
stored one.  Regenerate (python tests/golden/make_dqn_host_trace.py) only when the calls are MEANT to change.

A pointer is recorded as a name, never as an address: `ptr` hands out a made-up aligned address per tensor and the recorder maps it
back to the tensor's attribute path from the objects of the run (`learner.grad`, `tn.target`, `traces.rb`, `nstep._folded.rb`, ...;
the learner's `_idx` / `_key` / `_prio` are not used as names, so they show which buffer they alias); a tensor nothing holds is
`scratch#k:dtype[shape]`, numbered by first appearance.  Ring structs and the struct of a fused vec-step are read through the
`byref` object / the address the host code passes.  Host-only library functions run for real (rlhip_gamma_pow, rlhip_get_eps, the
*_workspace_bytes / *_nparams functions, rlhip_ring_init, rlhip_ring_length); of a recorded launch only the host-visible effect the
loops depend on is imitated: a push moves the ring's length counters.
"""
import contextlib
import ctypes as C
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for _p in (ROOT, os.path.join(ROOT, "reinforcementlearning.jl_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import torch  # noqa: E402

import rlhip as rl  # noqa: E402
from rlhip import _lib, checkpoint, core, dqn, ops, trajectory  # noqa: E402

OUT = os.path.join(HERE, "dqn_host_trace.json")
REAL_CALL = _lib.call
STREAM = 0x40  # what the recorded stream_ptr returns
SLOTS = ("_idx", "_key", "_prio")
BYREF = type(C.byref(C.c_int()))
N_IN, HIDDEN, N_OUT, BATCH, N_ENV, CAPACITY = 4, 64, 2, 8, 4, 8


def _walkable(v):
    return hasattr(v, "__dict__") and not isinstance(v, type) and \
        (getattr(type(v), "trace_walk", False) or type(v).__module__.split(".")[0] == "rlhip")


class Recorder:
    def __init__(self):
        self.events, self.roots = [], []  # roots: (name, getter), in naming priority
        self._fake, self._addr, self._scratch, self._keep = {}, {}, {}, []
        self._last_keys = None
        self.beta_calls = None  # a list once per_beta is a callable: the arguments of its evaluations since the last state record

    # ------------------------------------------------------------------ the replaced launch helpers
    def ptr(self, t):
        if t is None:
            return None
        if not t.is_contiguous():
            raise _lib.RLHipArgumentError("tensor must be contiguous")
        a = self._fake.get(id(t))
        if a is None:
            a = 0x100000 * (len(self._fake) + 1)
            self._fake[id(t)], self._addr[a] = a, t  # _addr keeps the tensor alive: an id is never reused
        return C.c_void_p(a)

    def stream_ptr(self):
        return C.c_void_p(STREAM)

    def call(self, name, *args):
        rc = 0
        if name == "rlhip_ring_init":  # host only: fills the struct the real length / layout queries read
            rc = REAL_CALL(name, *args)
        self.events.append([name] + [self.norm(a) for a in args])
        if name == "rlhip_ring_push_state":
            ring = args[0]._obj
            ring.len_sa = max(ring.len_sa, 1)
        elif name in ("rlhip_dqn_vec_step_f32", "rlhip_dqn_vec_step_fold_f32"):
            st = args[0]._obj
            ring = _lib.Ring.from_address((st.base if hasattr(st, "base") else st).ring)
            ring.len_rt = min(ring.len_rt + 1, ring.capacity)
            ring.len_sa = ring.len_rt + 1
        return rc

    def event(self, name, *args):
        self.events.append([name] + [self.norm(a) for a in args])

    @contextlib.contextmanager
    def patched(self):
        saved = []

        def put(mod, name, new):
            if hasattr(mod, name):
                saved.append((mod, name, getattr(mod, name)))
                setattr(mod, name, new)

        put(_lib, "call", self.call)
        for mod in (dqn, trajectory, core, ops):
            put(mod, "call", self.call)
            put(mod, "ptr", self.ptr)
            put(mod, "stream_ptr", self.stream_ptr)
        try:
            yield self
        finally:
            for mod, name, old in reversed(saved):
                setattr(mod, name, old)

    # ------------------------------------------------------------------ names
    def _names(self):
        """(id -> path of every tensor, address -> path of every C struct) reachable from the roots; the first path wins"""
        tensors, structs, seen = {}, {}, set()

        def walk(obj, path, depth):
            if id(obj) in seen or depth > 5:
                return
            seen.add(id(obj))
            if isinstance(obj, (list, tuple)):
                items = [(f"{path}[{i}]", v) for i, v in enumerate(obj)]
            else:
                items = [(f"{path}.{k}", v) for k, v in sorted(vars(obj).items()) if not (path == "learner" and k in SLOTS)]
            for p, v in items:
                if isinstance(v, torch.Tensor):
                    tensors.setdefault(id(v), p)
                elif isinstance(v, C.Structure):
                    structs.setdefault(C.addressof(v), p)
                elif isinstance(v, (list, tuple)) or _walkable(v):
                    walk(v, p, depth + 1)

        for name, get in self.roots:
            obj = get()
            if obj is not None:
                walk(obj, name, 0)
        return tensors, structs

    def tensor_name(self, t, tensors=None):
        tensors = self._names()[0] if tensors is None else tensors
        if id(t) in tensors:
            return tensors[id(t)]
        if id(t) not in self._scratch:
            self._keep.append(t)
            self._scratch[id(t)] = f"scratch#{len(self._scratch)}:{str(t.dtype).replace('torch.', '')}{list(t.shape)}"
        return self._scratch[id(t)]

    def address_name(self, a, names=None):
        if a is None or a == 0:
            return None
        if a == STREAM:
            return "stream"
        tensors, structs = self._names() if names is None else names
        if a in self._addr:
            return self.tensor_name(self._addr[a], tensors)
        return structs.get(a, "unknown address")

    def ring_name(self, ring, names=None):
        structs = (self._names() if names is None else names)[1]
        return f"{structs.get(C.addressof(ring), 'ring?')}<{ring.capacity}x{ring.n_env}x{ring.obs_dim}>"

    def struct_fields(self, st, names):
        out = {}
        for name, ftype in st._fields_:
            v = getattr(st, name)
            if ftype is C.c_void_p:
                a = self.address_name(v, names)
                if a is not None and a.endswith(".rb"):
                    a = self.ring_name(_lib.Ring.from_address(v), names)
                out[name] = a
            elif isinstance(v, C.Structure):
                out[name] = self.struct_fields(v, names)
            else:
                out[name] = v
        return out

    def norm(self, a):
        if a is None or isinstance(a, (str, float)):
            return a
        if isinstance(a, (bool, int)):
            return int(a)
        if isinstance(a, torch.Tensor):
            return self.tensor_name(a)
        if isinstance(a, C.c_void_p):
            return self.address_name(a.value)
        if isinstance(a, BYREF):
            obj = a._obj
            if isinstance(obj, _lib.Ring):
                return self.ring_name(obj)
            if isinstance(obj, (_lib.DqnStepArgs, _lib.DqnFoldStepArgs)):
                return {type(obj).__name__: self.struct_fields(obj, self._names())}
            return type(obj).__name__
        raise TypeError(f"an argument the recorder does not know: {a!r}")

    # ------------------------------------------------------------------ the learner after an optimise_ call / a vec-step
    def state(self, learner, **extra):
        tensors = self._names()[0]
        keys = sorted(checkpoint.state_dict(learner))
        rec = dict(extra, vec_steps=learner.vec_steps, draw_ctr=learner.draw_ctr, n_updates=learner.n_updates)
        for s in SLOTS:
            t = getattr(learner, s)
            rec[s] = None if t is None else self.tensor_name(t, tensors)
        if self.beta_calls is not None:
            rec["per_beta_calls"], self.beta_calls = self.beta_calls, []
        rec["state_dict"] = "as before" if keys == self._last_keys else keys
        self._last_keys = keys
        self.events.append(["state", rec])


# ---------------------------------------------------------------------------------------------- stubs
class Net:
    """the fields of a HipApproximator / DuelingApproximator that the learner and the fused loops read"""
    trace_walk = True

    def __init__(self, layers, dueling=False):
        self.n_in, self.hidden, self.n_out, self.layers, self.act = N_IN, HIDDEN, N_OUT, layers, 0
        self.lr, self.beta1, self.beta2, self.eps = 1e-3, 0.9, 0.999, 1e-8
        nparams = _lib.lib.rlhip_mlp2_nparams if layers == 2 else _lib.lib.rlhip_mlp3_nparams
        self.params = torch.zeros(int(nparams(N_IN, HIDDEN, N_OUT)))
        self.packed = torch.zeros(int(_lib.lib.rlhip_mlp3_packed_elems(HIDDEN)), dtype=torch.int16) if layers == 3 else None
        trained = self.params
        if dueling:
            self.dueling_params = trained = torch.zeros(dqn.dueling_nparams(N_IN, HIDDEN, N_OUT, layers))
            self._grad = dqn._Scratch(torch.zeros_like(trained))
        self.m, self.v = torch.zeros_like(trained), torch.zeros_like(trained)
        self.beta_pow, self.gn = torch.tensor([0.9, 0.999]), torch.zeros(1)


class TargetNet:
    """TargetNetwork whose optimise_ is recorded"""
    trace_walk = True

    def __init__(self, rec, network, sync_freq=2, rho=0.25):
        self._rec, self.network, self.sync_freq, self.rho, self.n_optimise = rec, network, sync_freq, rho, 0
        self.target = network.params.clone()
        self.target_packed = network.packed.clone() if network.layers == 3 else None
        if hasattr(network, "dueling_params"):
            self.target_dueling = network.dueling_params.clone()

    def optimise_(self, grad, clip_norm=0.0, grad_scale=1.0):
        self._rec.event("approximator.optimise_", grad, float(clip_norm), float(grad_scale))


class Controller:
    trace_walk = True

    def __init__(self, rec):
        self._rec, self.n_inserted, self.n_sampled = rec, 0, 0

    def on_insert_(self, n=1):
        self.n_inserted += n
        self._rec.event("controller.on_insert_", n)

    def on_sample_(self):
        self.n_sampled += 1
        self._rec.event("controller.on_sample_")
        return True


def make_traces(rec, prioritized, n_step=1):
    """a real record ring on CPU storage whose draws and priority write-back are recorded instead of launched"""
    base = rl.CircularPrioritizedTraces if prioritized else rl.CircularArraySARTSTraces

    class Traces(base):
        trace_walk = True

        def sample_indices(self, batch, seed, draw_ctr):
            idx = torch.empty(batch, dtype=torch.int64)
            rec.event("traces.sample_indices", batch, seed, draw_ctr, "->", idx)
            return idx

    class PrioritizedTraces(Traces):
        def sample_prioritized(self, batch, seed, draw_ctr):
            out = (torch.empty(batch, dtype=torch.int64), torch.empty(batch, dtype=torch.int64), torch.empty(batch, dtype=torch.float32))
            rec.event("traces.sample_prioritized", batch, seed, draw_ctr, "->", *out)
            return out

        def set_priority_(self, keys, prio):
            rec.event("traces.set_priority_", keys, prio)

    if prioritized:
        return PrioritizedTraces(capacity=CAPACITY, n_env=N_ENV, obs_dim=N_IN, device="cpu", n_step=n_step)
    return Traces(capacity=CAPACITY, n_env=N_ENV, obs_dim=N_IN, device="cpu")


def set_length(traces, n):
    traces.rb.len_rt, traces.rb.len_sa = n, n + 1


class Env:
    """the fields of a HipVecEnv that the fused loops read"""
    trace_walk = True

    def __init__(self):
        self.kind, self.cfg, self._st, self.n, self.seed, self.env_id_base = 0, _lib.CartPoleCfg(), _lib.EnvState(), N_ENV, 11, 0
        self.continuous, self.is_f64, self.device, self._obs_valid = False, False, torch.device("cpu"), False
        self._obs, self._last_obs = torch.zeros((N_IN, N_ENV)), torch.zeros((N_IN, N_ENV))

    def state(self):
        return self._obs


def _roots(rec, learner, tn, traces, policy=None, env=None):
    rec.roots = [("net", lambda: tn.network), ("tn", lambda: tn), ("traces", lambda: traces), ("nstep", lambda: learner._nstep),
                 ("double", lambda: learner._double), ("env", lambda: env), ("policy", lambda: policy), ("learner", lambda: learner)]


# ---------------------------------------------------------------------------------------------- the traces
REPLAY = {"uniform": None, "per-beta0": 0.0, "per-beta0.4": 0.4, "per-beta-callable": "callable"}


def trace_per_stage(layers, replay, n_step, double):
    """DQNLearner.optimise_ through the n-step warm-up (stored lengths 0 .. n_step - 1), then two consecutive updates"""
    rec = Recorder()
    with rec.patched():
        tn = TargetNet(rec, Net(layers))
        beta = REPLAY[replay]
        if beta == "callable":
            rec.beta_calls = []

            def beta(n_updates):
                rec.beta_calls.append(n_updates)
                return 0.4 + 0.125 * n_updates
        learner = rl.DQNLearner(tn, batchsize=BATCH, gamma=0.99, huber_delta=1.5, min_replay_history=1, max_grad_norm=0.5, seed=3,
                                per_beta=0.0 if beta is None else beta, n_step=n_step, double_dqn=double)
        traces = make_traces(rec, replay != "uniform", n_step)
        traj = rl.Trajectory(traces, controller=Controller(rec))
        _roots(rec, learner, tn, traces)
        for length in range(n_step + 2):
            set_length(traces, length)
            rec.event("optimise_", "stored", length)
            rec.state(learner, updated=bool(learner.optimise_(traj)))
    return rec.events


FOLDED_FORMS = {"plain": {}, "nstep": dict(n_step=3), "double": dict(double_dqn=True), "nstep+double": dict(n_step=3, double_dqn=True),
                "dueling+double": dict(double_dqn=True)}


def trace_fused(loop, layers, form):
    """three vec-steps of run_fused_dqn / run_fused_dqn_folded from an empty trajectory; every field of the struct at every call"""
    rec = Recorder()
    with rec.patched():
        tn = TargetNet(rec, Net(layers, dueling=form.startswith("dueling")))
        learner = rl.DQNLearner(tn, batchsize=BATCH, gamma=0.99, huber_delta=1.5, min_replay_history=1, max_grad_norm=0.5, seed=3,
                                **FOLDED_FORMS[form])
        traces = make_traces(rec, False)
        traj = rl.Trajectory(traces, controller=Controller(rec))
        policy = rl.QBasedPolicy(learner, rl.EpsilonGreedyExplorer(0.1, eps_init=0.9, decay_steps=10, seed=5))
        agent, env = rl.Agent(policy, traj), Env()
        _roots(rec, learner, tn, traces, policy, env)

        class Hook(rl.EmptyHook):
            def push_(self, stage, agent, env):
                rec.event("hook", stage)
                if stage == core.POST_ACT_STAGE:
                    rec.state(learner, n_optimise=tn.n_optimise, explorer_step=policy.explorer.step)

        getattr(core, loop)(agent, env, rl.StopAfterNSteps(3), Hook())
        rec.event("end", "obs_valid", env._obs_valid)
    return rec.events


def build_traces():
    out = {}
    for layers in (2, 3):
        for replay in REPLAY:
            for n_step in (1, 3):
                for double in (False, True):
                    out[f"per-stage/layers{layers}/{replay}/n{n_step}/{'double' if double else 'plain'}"] = \
                        trace_per_stage(layers, replay, n_step, double)
    for layers in (2, 3):
        out[f"run_fused_dqn/layers{layers}/plain"] = trace_fused("run_fused_dqn", layers, "plain")
        for form in FOLDED_FORMS:
            out[f"run_fused_dqn_folded/layers{layers}/{form}"] = trace_fused("run_fused_dqn_folded", layers, form)
    return json.loads(json.dumps(out))  # tuples -> lists, as the stored file reads back


def render(traces):
    """one event per line"""
    lines = ["{"]
    names = list(traces)
    for i, name in enumerate(names):
        lines.append(f" {json.dumps(name)}: [")
        events = traces[name]
        lines += [f"  {json.dumps(e)}{',' if j + 1 < len(events) else ''}" for j, e in enumerate(events)]
        lines.append(" ]" + ("," if i + 1 < len(names) else ""))
    lines.append("}")
    return "\n".join(lines) + "\n"


if __name__ == "__main__":
    text = render(build_traces())
    with open(OUT, "w") as f:
        f.write(text)
    print(f"wrote {os.path.relpath(OUT, ROOT)}: {len(text)} bytes")
