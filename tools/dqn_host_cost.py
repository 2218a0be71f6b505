"""Host cost of DQNLearner.optimise_ alone (profiles/dqn_host_pipeline.md): every launch helper is a no-op, so what is timed is the
Python between the ABI calls of one update -- the part a host-side change can move.  Needs no GPU.

    python tools/dqn_host_cost.py [--tree DIR] [--blocks 9] [--reps 20000]

--tree DIR: time another checkout of this project (built there), e.g. the parent commit.  One process times one tree: to compare
two, alternate processes and read the minima (the machine's other work only ever adds).  The learner, traces and target network
are the stubs of tests/golden/make_dqn_host_trace.py.  One JSON line per form: [median, min] microseconds per call."""
import argparse
import ctypes as C
import importlib.util
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--tree", default=HERE)
ap.add_argument("--blocks", type=int, default=9)
ap.add_argument("--reps", type=int, default=20000)
args = ap.parse_args()
tree = os.path.abspath(args.tree)
sys.path.insert(0, tree)
sys.path.insert(0, os.path.join(tree, "reinforcementlearning.jl_amd"))

import rlhip as rl  # noqa: E402
from rlhip import _lib, core, dqn, ops, trajectory  # noqa: E402

assert os.path.abspath(rl.__file__).startswith(tree + os.sep), rl.__file__
spec = importlib.util.spec_from_file_location("make_dqn_host_trace", os.path.join(HERE, "tests", "golden", "make_dqn_host_trace.py"))
gen = importlib.util.module_from_spec(spec)
spec.loader.exec_module(gen)  # its `import rlhip` finds the package imported above
assert gen.rl is rl

POINTER = C.c_void_p(64)


def call(name, *a):
    return gen.REAL_CALL(name, *a) if name == "rlhip_ring_init" else 0


for mod in (_lib, dqn, trajectory, core, ops):
    for name, new in (("call", call), ("ptr", lambda t: None if t is None else POINTER), ("stream_ptr", lambda: POINTER)):
        if hasattr(mod, name):
            setattr(mod, name, new)


class Silent:
    beta_calls = None

    def event(self, *a):
        pass


def timed(layers, prioritized, n_step, double):
    rec = Silent()
    learner = rl.DQNLearner(gen.TargetNet(rec, gen.Net(layers)), batchsize=gen.BATCH, min_replay_history=1, seed=3,
                            per_beta=0.4 if prioritized else 0.0, n_step=n_step, double_dqn=double)
    traces = gen.make_traces(rec, prioritized, n_step)
    gen.set_length(traces, 6)
    traj = rl.Trajectory(traces, controller=gen.Controller(rec))
    for _ in range(2000):
        learner.optimise_(traj)
    us = []
    for _ in range(args.blocks):
        t0 = time.perf_counter()
        for _ in range(args.reps):
            learner.optimise_(traj)
        us.append((time.perf_counter() - t0) / args.reps * 1e6)
    return [round(statistics.median(us), 3), round(min(us), 3)]


print(json.dumps(dict(tree=tree, python=sys.version.split()[0], blocks=args.blocks, reps=args.reps, columns="[median, min] us")), flush=True)
for layers in (2, 3):
    for prioritized in (False, True):
        for n_step in (1, 3):
            for double in (False, True):
                print(json.dumps(dict(layers=layers, prioritized=prioritized, n_step=n_step, double_dqn=double,
                                      optimise_=timed(layers, prioritized, n_step, double))), flush=True)
