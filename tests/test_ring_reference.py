"""The oracle's replay ring (oracle/rlo_buffer.c: head / length counters, modulo slots) against the list model of
tests/ring_ref.py, which has no such arithmetic -- the CPU half of tests/test_gpu_ring_layouts.py, over the same
(n_env, obs_dim, capacity) list.  UInt8 content is pushed into the oracle as the Float32 values that hold it exactly."""
import numpy as np
import pytest

import oracle
from ring_ref import CASES, RingRef, case_id, frame_major, random_frame, random_traces


def _as_f32(batch):
    s, a, r, t, sn = batch
    return s.astype(np.float32), a, r, t, sn.astype(np.float32)


def _same(got, want, where):
    for name, g, w in zip(("state", "action", "reward", "terminal", "next_state"), got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, (where, name, g.dtype, w.dtype, g.shape, w.shape)
        assert np.array_equal(g, w), f"{where}: {name} differs"


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_oracle_ring_equals_the_list_model_after_every_push(case):
    dtype, od, n_env, cap, _ = case
    rng = np.random.default_rng([od, n_env, cap])
    ref = RingRef(cap, n_env, od, np.uint8 if dtype == "u8" else np.float32)
    ring = oracle.Ring(cap, n_env, od)
    f = random_frame(rng, dtype, od, n_env)
    ref.push_state(f)
    ring.push_state(f.astype(np.float32))
    assert len(ring) == len(ref) == 0
    for k in range(1, 2 * cap + 4):  # fill, exactly full, two wraps
        f, (a, r, t) = random_frame(rng, dtype, od, n_env), random_traces(rng, n_env)
        ref.push_transition(f, a, r, t)
        ring.push_transition(f.astype(np.float32), a, r, t)
        assert len(ring) == len(ref) == min(k, cap)
        total = len(ref) * n_env
        drawn = ring.sample_indices(300, 11, k)
        assert drawn.min() >= 0 and drawn.max() < total
        idx = np.concatenate([np.arange(total), drawn])
        _same(ring.gather(idx), _as_f32(ref.gather(idx)), f"push {k}")


def test_list_model_states_the_trace_semantics():
    """the model against transitions written out by hand: capacity 2, 2 envs, 4 pushes -> the newest two are kept"""
    ref = RingRef(2, 2, 3, np.uint8)
    frames = [np.arange(6, dtype=np.uint8).reshape(3, 2) + 10 * k for k in range(5)]
    ref.push_state(frames[0])
    with pytest.raises(AssertionError):
        ref.push_state(frames[0])
    for k in range(4):
        ref.push_transition(frames[k + 1], [k, k + 100], [k + 0.5, -k - 0.5], [k == 2, 0])
    assert len(ref) == 2 and ref.pushed_transitions == 4
    s, a, r, t, sn = ref.gather([0, 1, 2, 3])  # (li, e) = (0, 0), (0, 1), (1, 0), (1, 1): pushed transitions 2 and 3
    assert np.array_equal(s.T, [frames[2][:, 0], frames[2][:, 1], frames[3][:, 0], frames[3][:, 1]])
    assert np.array_equal(sn.T, [frames[3][:, 0], frames[3][:, 1], frames[4][:, 0], frames[4][:, 1]])
    assert a.tolist() == [2, 102, 3, 103] and r.tolist() == [2.5, -2.5, 3.5, -3.5] and t.tolist() == [1, 0, 0, 0]
    fs = frame_major((s, a, r, t, sn))[0]
    assert fs.shape == (4, 3) and fs.flags.c_contiguous and np.array_equal(fs[2], frames[3][:, 0])
    with pytest.raises(AssertionError):
        ref.gather([4])
    pooled = RingRef(1, 2, 3, np.uint8)
    pooled.push_state_maxpool(frames[1], frames[0][::-1])
    pooled.push_transition_maxpool(frames[0], frames[2][:, ::-1], [1, 2], [0.0, 1.0], [0, 1])
    s, a, r, t, sn = pooled.gather([1])
    assert np.array_equal(s[:, 0], np.maximum(frames[1], frames[0][::-1])[:, 1])
    assert np.array_equal(sn[:, 0], np.maximum(frames[0], frames[2][:, ::-1])[:, 1]) and (a[0], r[0], t[0]) == (2, 1.0, 1)
