"""n-step gathers of frame rings (rlhip_ring_gather_nstep, rlhip_ring_gather_stacked_nstep) -- the CPU half:

  * the list model of tests/ring_nstep_ref.py on hand-written windows (terminal at step 0, at the last step, a window cut by the ring's
    end, a reward of -0.0, gamma 0 and 1) and on hand-written stacks;
  * the model's (a, ret, term) against `oracle.ring_gather_nstep` on a record ring given the same (a, r, t) pushes;
  * header / ctypes / Julia signatures of the two new calls agree; every argument refusal is reached before a device call (the library
    loads without a GPU; fake pointers that nothing dereferences);
  * the census: the exhaustive batches of tests/test_gpu_ring_nstep.py, computed from the model alone, hold every kind of window that
    the kernels distinguish."""
import ctypes as C
import re

import numpy as np
import pytest

import oracle
import ring_nstep_ref as R
from ring_ref import case_id
from test_julia_glue_signatures import GLUE, glue_ccalls, header_prototypes


def _hand(rewards, terminals, cap=16):
    """a single-env ring of one-component Float32 frames: pushed frame k holds the value k, transition k the action k"""
    ref = R.RingNStepRef(cap, 1, 1, np.float32)
    ref.push_state(np.full((1, 1), 0.0, np.float32))
    for k, (r, t) in enumerate(zip(rewards, terminals)):
        ref.push_transition(np.full((1, 1), k + 1.0, np.float32), [k], [r], [t])
    return ref


def _bits(x):
    return np.float32(x).view(np.uint32)


def test_hand_written_windows():
    ref = _hand([1.0, 2.0, 4.0, 8.0, 16.0], [0, 0, 1, 0, 0])
    g = 0.5
    # a full window without a terminal: 1 + 0.5 * 2
    s, a, ret, t, sn, ns = ref.nstep_transition(0, 0, 2, g)
    assert (s[0], a, ret, t, sn[0], ns) == (0.0, 0, 2.0, 0, 2.0, 2)
    # a terminal at the last step: 1 + 0.5 * (2 + 0.5 * 4)
    s, a, ret, t, sn, ns = ref.nstep_transition(0, 0, 3, g)
    assert (s[0], a, ret, t, sn[0], ns) == (0.0, 0, 3.0, 1, 3.0, 3)
    # ... and the same window under a longer n: cut at, and including, the terminal step
    assert [x.tolist() for x in ref.nstep_transition(0, 0, 32, g)] == [x.tolist() for x in ref.nstep_transition(0, 0, 3, g)]
    # a terminal at step 0
    s, a, ret, t, sn, ns = ref.nstep_transition(2, 0, 5, g)
    assert (s[0], a, ret, t, sn[0], ns) == (2.0, 2, 4.0, 1, 3.0, 1)
    # a window cut by the ring's end: 8 + 0.5 * 16, not terminal, s' = the newest frame
    s, a, ret, t, sn, ns = ref.nstep_transition(3, 0, 4, g)
    assert (s[0], a, ret, t, sn[0], ns) == (3.0, 3, 16.0, 0, 5.0, 2)
    s, a, ret, t, sn, ns = ref.nstep_transition(4, 0, 4, g)
    assert (s[0], a, ret, t, sn[0], ns) == (4.0, 4, 16.0, 0, 5.0, 1)
    # gamma 0: the first reward; gamma 1: the plain sum
    assert ref.nstep_transition(0, 0, 3, 0.0)[2] == 1.0 and ref.nstep_transition(0, 0, 3, 1.0)[2] == 7.0
    # n = 1 is the stored transition
    for li in range(5):
        s, a, r, t, sn = ref.transition(li, 0)
        got = ref.nstep_transition(li, 0, 1, 0.99)
        assert (got[0][0], got[1], got[2], got[3], got[4][0], got[5]) == (s[0], a, r, t, sn[0], 1)


def test_a_reward_of_minus_zero_comes_back_as_plus_zero():
    ref = _hand([-0.0, -0.0, 3.0], [0, 0, 0])
    assert _bits(ref.transition(0, 0)[2]) == 0x80000000
    for n in (1, 2):
        for g in (0.99, 0.0, 1.0):
            assert _bits(ref.nstep_transition(0, 0, n, g)[2]) == 0  # -0 + g * (+0) = +0, -0 + g * (-0 + g * 0) = +0
    assert ref.nstep_transition(0, 0, 3, 1.0)[2] == 3.0


def test_the_fold_rounds_every_product_and_every_sum_to_float32():
    r = [np.float32(0.1), np.float32(0.7), np.float32(-1.3)]
    ref = _hand(r, [0, 0, 0])
    g = np.float32(0.99)
    want = np.float32(r[2] + np.float32(g * np.float32(0.0)))
    want = np.float32(r[1] + np.float32(g * want))
    want = np.float32(r[0] + np.float32(g * want))
    assert _bits(ref.nstep_transition(0, 0, 3, 0.99)[2]) == _bits(want)
    assert ref.nstep_transition(0, 0, 3, 0.99)[2].dtype == np.float32


def test_the_ring_keeps_the_newest_capacity_transitions():
    ref = _hand([float(k) for k in range(7)], [0, 0, 0, 1, 0, 0, 0], cap=4)  # transitions 3 .. 6 are kept; 3 is terminal
    assert len(ref) == 4
    s, a, ret, t, sn, ns = ref.nstep_transition(0, 0, 3, 1.0)
    assert (s[0], a, ret, t, sn[0], ns) == (3.0, 3, 3.0, 1, 4.0, 1)
    s, a, ret, t, sn, ns = ref.nstep_transition(1, 0, 32, 1.0)
    assert (s[0], a, ret, t, sn[0], ns) == (4.0, 4, 15.0, 0, 7.0, 3)


def test_hand_written_stacks():
    ref = _hand([0.0] * 6, [0, 0, 1, 0, 0, 0])  # frames 0 .. 6; transition 2 (frame 2 -> 3) ends an episode
    flat = lambda f, n: ref.stack(f, n)[:, 0].tolist()  # noqa: E731
    assert flat(0, 4) == [0.0, 0.0, 0.0, 0.0]              # frame 0 holds the value 0; the three before it do not exist
    assert ref.member_is_zero_filled(0, 4) == [True, True, True, False]
    assert flat(2, 4) == [0.0, 0.0, 1.0, 2.0] and ref.member_is_zero_filled(2, 4) == [True, False, False, False]
    assert flat(3, 4) == [0.0, 0.0, 0.0, 3.0]              # the episode boundary lies right behind the newest member
    assert flat(5, 4) == [0.0, 3.0, 4.0, 5.0] and ref.member_is_zero_filled(5, 4) == [True, False, False, False]
    assert flat(6, 2) == [5.0, 6.0] and flat(6, 1) == [6.0]
    # state stack at li, next stack at li + ns
    s, a, ret, t, sn, ns = ref.gather_stacked_nstep([1, 3], 3, 2, 0.9)
    assert ns.tolist() == [2, 2] and t.tolist() == [1, 0]
    assert s[:, :, 0].tolist() == [[0.0, 0.0, 1.0], [0.0, 0.0, 3.0]]
    assert sn[:, :, 0].tolist() == [[0.0, 0.0, 3.0], [3.0, 4.0, 5.0]]
    # n = 1: the anchors li and li + 1 of the 1-step stacked gather
    s, a, ret, t, sn, ns = ref.gather_stacked_nstep(np.arange(6), 4, 1, 0.9)
    for li in range(6):
        assert np.array_equal(s[li], ref.stack(li, 4)) and np.array_equal(sn[li], ref.stack(li + 1, 4))


@pytest.mark.parametrize("n_step", [1, 2, 3, 7, 32])
@pytest.mark.parametrize("gamma", R.GAMMAS)
def test_model_equals_the_oracle_fold_on_a_record_ring(n_step, gamma):
    cap, n_env = 7, 5
    for pushes in (2, cap, 2 * cap + 3):
        rng = np.random.default_rng([n_step, pushes])
        ref = R.fill(R.RingNStepRef(cap, n_env, 6, np.float32), rng, "f32", pushes, 0.25)
        ring = oracle.Ring(cap, n_env, 2)  # the same (a, r, t), states of its own
        ring.push_state(np.zeros((2, n_env), np.float32))
        for a, r, t in zip(ref.a, ref.r, ref.t):
            ring.push_transition(rng.standard_normal((2, n_env)).astype(np.float32), a, r, t)
        assert len(ring) == len(ref)
        idx = R.exhaustive_batch(ref, pushes)
        _, a, ret, t, _, ns = ref.gather_nstep(idx, n_step, gamma)
        _, oa, oret, ot, _ = oracle.ring_gather_nstep(ring, idx, n_step, gamma)
        assert np.array_equal(a, oa) and np.array_equal(t, ot)
        assert np.array_equal(ret.view(np.uint32), oret.view(np.uint32))
        assert ns.min() >= 1 and ns.max() <= min(n_step, len(ref))


SIGNATURES = {
    "rlhip_ring_gather_nstep": ("Int32", ["ptr", "ptr", "Int64", "Int32", "Float32", "ptr", "ptr", "ptr", "ptr", "ptr", "ptr", "ptr"]),
    "rlhip_ring_gather_stacked_nstep": ("Int32", ["ptr", "ptr", "Int64", "Int32", "Int32", "Float32", "ptr", "ptr", "ptr", "ptr", "ptr",
                                                  "ptr", "ptr"]),
}


def test_new_entry_points_are_declared_bound_and_called_with_their_types():
    from rlhip import _lib

    protos = header_prototypes()
    cls = {C.c_int32: "Int32", C.c_int64: "Int64", C.c_uint32: "UInt32", C.c_uint64: "UInt64", C.c_float: "Float32"}
    bound = {c[0]: c for c in glue_ccalls()}
    for name, sig in SIGNATURES.items():
        assert protos[name] == sig
        res, args = _lib._PROTOS[name]
        assert res is C.c_int32 and [cls.get(a, "ptr") for a in args] == sig[1]
        assert name in bound and bound[name][2] == sig[1], f"RLHip.jl has no matching ccall of {name}"
    assert _lib.lib.rlhip_abi_version() == 2  # entry points were added, nothing changed
    # the Julia host: a sampler type and its `sample` method on frame traces, which draws n-step starts and gathers them
    src = re.sub(r"#[^\n]*", "", open(GLUE).read())
    assert re.search(r"struct HipNStepBatchSampler\b", src)
    body = src[src.index("function sample(s::HipNStepBatchSampler, t::HipTrajectory)"):]
    body = body[:body.index("\nend")]
    assert ":rlhip_ring_sample_indices_nstep" in body and "gather_nstep!(" in body and "gather_stacked_nstep!(" in body
    assert "t.draw_ctr +=" in body and "n_steps = " in body
    assert re.search(r"export[^#]*\bHipNStepBatchSampler\b", open(GLUE).read(), flags=re.S)


FAKE = 0x10000  # a 64-byte aligned address that nothing dereferences: every call below is refused before a launch


def _ring(capacity, n_env, obs_dim, elem_bytes, stored, where=FAKE):
    from rlhip import _lib

    rb = _lib.Ring()
    if elem_bytes == 4 and obs_dim <= 4:
        _lib.call("rlhip_ring_init", C.byref(rb), capacity, n_env, obs_dim, 4, where, None, None, None)
    else:
        _lib.call("rlhip_ring_init", C.byref(rb), capacity, n_env, obs_dim, elem_bytes, where, where, where, where)
    rb.len_rt, rb.len_sa = stored, (stored + 1 if stored else 0)
    return rb


def test_arguments_are_refused_before_any_device_call():
    from rlhip._lib import RLHipArgumentError, call, lib

    small, frames, records = _ring(8, 3, 6, 4, 5), _ring(8, 1, 7056, 1, 5), _ring(8, 3, 4, 4, 5)
    assert lib.rlhip_ring_gather_is_frame_major(C.byref(frames)) == 1 and lib.rlhip_ring_gather_is_frame_major(C.byref(small)) == 0

    def plain(rb=small, idx=FAKE, batch=4, n_step=3, s=FAKE, a=FAKE, ret=FAKE, term=FAKE, sn=FAKE, n_used=None):
        call("rlhip_ring_gather_nstep", C.byref(rb), idx, batch, n_step, 0.9, s, a, ret, term, sn, n_used, None)

    def stacked(rb=frames, idx=FAKE, batch=4, n_stack=4, n_step=3, s=FAKE, a=FAKE, ret=FAKE, term=FAKE, sn=FAKE, n_used=None):
        call("rlhip_ring_gather_stacked_nstep", C.byref(rb), idx, batch, n_stack, n_step, 0.9, s, a, ret, term, sn, n_used, None)

    for f in (plain, stacked):
        for n_step in (0, 33, -1):
            with pytest.raises(RLHipArgumentError, match="n_step must be in 1..32"):
                f(n_step=n_step)
        with pytest.raises(RLHipArgumentError, match="rlhip_ring_fold_nstep"):
            f(rb=records)
        for nulled in ("idx", "s", "a", "ret", "term", "sn"):
            with pytest.raises(RLHipArgumentError, match="bad arguments"):
                f(**{nulled: None})
        with pytest.raises(RLHipArgumentError, match="bad arguments"):
            f(batch=-1)
    with pytest.raises(RLHipArgumentError, match="empty"):
        plain(rb=_ring(8, 3, 6, 4, 0))
    with pytest.raises(RLHipArgumentError, match="empty"):
        stacked(rb=_ring(8, 1, 7056, 1, 0))
    # the alignment conditions of the 1-step twins
    for kw in (dict(s=FAKE + 4), dict(sn=FAKE + 8), dict(rb=_ring(8, 1, 7056, 1, 5, FAKE + 1))):
        with pytest.raises(RLHipArgumentError, match="16-byte aligned"):
            plain(**dict(dict(rb=frames), **kw))
        with pytest.raises(RLHipArgumentError, match="16-byte aligned"):
            stacked(**kw)
    plain(rb=small, s=FAKE + 4, batch=0)  # (the small route has no alignment condition)
    # ... and the stacked gather's own preconditions
    for n_stack in (0, 9):
        with pytest.raises(RLHipArgumentError, match="n_stack must be in 1..8"):
            stacked(n_stack=n_stack)
    with pytest.raises(RLHipArgumentError, match="single-env"):
        stacked(rb=_ring(8, 3, 16, 1, 5))
    with pytest.raises(RLHipArgumentError, match="multiple of 16"):
        stacked(rb=_ring(8, 1, 1030, 1, 5))
    # an empty batch is not an error, and launches nothing (there is no device here)
    plain(batch=0)
    plain(rb=frames, batch=0)
    stacked(batch=0)
    # no call moved a counter of the ring
    assert (small.head_sa, small.len_sa, small.head_rt, small.len_rt) == (0, 6, 0, 5)


def test_sampler_on_cpu_only_objects_checks_its_arguments():
    import rlhip as rl

    with pytest.raises(ValueError, match="n_stack"):
        rl.NStepBatchSampler(3, 0.9, 16, n_stack=9)
    assert rl.NStepBatchSampler(3, 0.9, 16).n_stack is None and rl.NStepBatchSampler(3, 0.9, 16, n_stack=4).n_stack == 4
    tr = object.__new__(rl.CircularArraySARTSTraces)
    tr.__dict__.update(capacity=8, n_env=3, obs_dim=4, records_layout=True)
    with pytest.raises(ValueError, match="record ring"):
        rl.NStepBatchSampler(3, 0.9, 16, n_stack=4).sample(tr)
    for name in ("gather_nstep", "gather_stacked_nstep"):
        assert callable(getattr(rl.CircularArraySARTSTraces, name))


def _kinds(c, names):
    return {k for k in names if c[k] > 0}


WINDOWS = ("full", "terminal_cut", "terminal_at_n", "ring_end_cut")


@pytest.mark.parametrize("case", R.PLAIN_CASES, ids=case_id)
def test_census_of_the_plain_batches(case):
    """per case, over the n_step values of its WRAPPED fill: a full window without a terminal, a terminal cut with ns < n_step, a
    terminal exactly at step n_step, and a ring-end cut are all in the exhaustive batch; the short fill (two transitions) adds
    the windows of a ring that is not full"""
    cap = case[3]
    short, wrapped = R.plain_pushes(cap)
    ref = R.plain_model(case, wrapped)
    assert len(ref) == cap and ref.pushed_transitions == 2 * cap + 3
    idx = R.exhaustive_batch(ref, wrapped)
    assert set(idx.tolist()) == set(range(cap * ref.n_env)) and len(idx) > cap * ref.n_env
    seen = set()
    for n in R.PLAIN_NSTEPS(cap):
        c = R.census(ref, idx, n)
        assert sum(c[k] for k in WINDOWS) == len(idx)  # the four kinds partition the batch
        if n == 1:
            assert _kinds(c, WINDOWS) == {"full", "terminal_at_n"}
        seen |= _kinds(c, WINDOWS) if n > 1 else set()
    assert seen == set(WINDOWS), f"missing for n_step > 1: {set(WINDOWS) - seen}"
    ref = R.plain_model(case, short)
    assert len(ref) == 2
    idx = R.exhaustive_batch(ref, short)
    c = R.census(ref, idx, 32)
    assert c["full"] == 0 and c["ring_end_cut"] + c["terminal_cut"] == len(idx)


@pytest.mark.parametrize("case", R.STACKED_CASES, ids=lambda c: f"{c[0]}-{c[1]}-cap{c[2]}")
def test_census_of_the_stacked_batches(case):
    """per case and n_stack > 1, over the n_step values of the wrapped fill: the four kinds of window, a zero-filled member in each
    stack, ns < n_stack and ns >= n_stack"""
    everything = set(WINDOWS) | {"zero_s", "zero_sn", "ns_lt_stack", "ns_ge_stack"}
    for pushes in R.STACKED_PUSHES:
        ref = R.stacked_model(case, pushes)
        assert len(ref) == min(pushes, case[2])
        idx = R.exhaustive_batch(ref, pushes)
        for n_stack in R.STACKS:
            seen = set()
            for n in R.STACKED_NSTEPS:
                seen |= _kinds(R.census(ref, idx, n, n_stack), everything)
            if n_stack == 1:
                assert not seen & {"zero_s", "zero_sn", "ns_lt_stack"}  # a stack of one is never cut
            elif pushes == max(R.STACKED_PUSHES):
                assert seen == everything, f"n_stack {n_stack}: missing {everything - seen}"
            else:  # the short fill: the state stack of the oldest transition reaches before the oldest frame
                assert {"zero_s", "ns_lt_stack"} <= seen
