"""Which ABI calls the DQN host layer makes, with which arguments, in which order: a fresh recording on CPU tensors
(tests/golden/make_dqn_host_trace.py drives the real DQNLearner, NStepBatchSampler, DoubleTargetFold, run_fused_dqn and
run_fused_dqn_folded with the launch helpers replaced by recorders) against the stored one, tests/golden/dqn_host_trace.json.
The kernels are behind the ABI, so a host-side change that leaves this trace alone cannot move a number; the device side of
every form is tests/test_gpu_*.py."""
import importlib.util
import json
import os

import pytest

pytest.importorskip("torch")

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("make_dqn_host_trace", os.path.join(GOLDEN, "make_dqn_host_trace.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

with open(gen.OUT) as _f:
    STORED_TEXT = _f.read()
STORED = json.loads(STORED_TEXT)
_fresh = []


def fresh():
    if not _fresh:
        _fresh.append(gen.build_traces())
    return _fresh[0]


def test_the_matrix_is_complete():
    per_stage = [f"per-stage/layers{layers}/{replay}/n{n}/{form}" for layers in (2, 3)
                 for replay in ("uniform", "per-beta0", "per-beta0.4", "per-beta-callable") for n in (1, 3) for form in ("plain", "double")]
    fused = [f"{loop}/layers{layers}/{form}" for layers in (2, 3)
             for loop, forms in (("run_fused_dqn", ("plain",)),
                                 ("run_fused_dqn_folded", ("plain", "nstep", "double", "nstep+double", "dueling+double"))) for form in forms]
    assert sorted(STORED) == sorted(per_stage + fused) and len(STORED) == 32 + 12
    for name in per_stage:  # the warm-up (stored lengths 0 .. n_step - 1: no update), then two consecutive updates
        n = int(name.split("/")[3][1:])
        updated = [e[1]["updated"] for e in STORED[name] if e[0] == "state"]
        assert updated == [False] * n + [True, True], name
        assert [e[1]["n_updates"] for e in STORED[name] if e[0] == "state"][-1] == 2
    for name in fused:  # three vec-steps, every field of the struct at every call
        calls = [e for e in STORED[name] if e[0].startswith("rlhip_dqn_vec_step")]
        assert len(calls) == 3 and all(isinstance(c[1], dict) for c in calls), name
        (kind, fields), = calls[-1][1].items()
        base = fields["base"] if kind == "DqnFoldStepArgs" else fields
        assert base["do_update"] == 1 and base["ring"].startswith("traces.rb"), name


@pytest.mark.parametrize("name", sorted(STORED))
def test_the_host_layer_makes_the_stored_calls(name):
    got, want = fresh()[name], STORED[name]
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"{name}: event {i} differs\n  now    {json.dumps(g)}\n  stored {json.dumps(w)}"
    assert len(got) == len(want), f"{name}: {len(got)} events now, {len(want)} stored; the first extra one: " \
                                  f"{json.dumps(max(got, want, key=len)[min(len(got), len(want)):][:1])}"


def test_regenerating_gives_the_stored_file_byte_for_byte():
    assert sorted(fresh()) == sorted(STORED)
    assert gen.render(fresh()) == STORED_TEXT
