"""Prioritized n-step replay (CircularPrioritizedTraces(n_step), rlhip_ring_push_priority_nstep, rlhip_per_sample_fold_nstep_f32) -- the
CPU half:

  * the reference of tests/per_nstep_ref.py (the lagged push composed from `oracle.SumTree.fill_range`) against a brute-force numpy
    model of `mask * priority` after every push across fill, full and two wraps, with priority write-backs in between;
  * every start drawn from the masked tree has its n transitions ahead of it; n_step = 1 is `oracle.ring_push_priority`;
  * header / ctypes / Julia signatures of the two new calls agree; argument validation happens before any HIP call (the library
    loads without a GPU); a learner on CPU-only objects constructs and refuses traces masked for another n_step."""
import ctypes as C

import numpy as np
import pytest

import oracle
from per_nstep_ref import Mirror
from test_julia_glue_signatures import glue_ccalls, header_prototypes

DEFAULT = 2.5


def _push(m, rng, p_term=0.2):
    n_env, ns = m.ring.rb.n_env, m.ring.rb.obs_dim
    m.push_transition(rng.standard_normal((ns, n_env)).astype(np.float32), rng.integers(0, 2, n_env).astype(np.int32),
                      rng.standard_normal(n_env).astype(np.float32), (rng.random(n_env) < p_term).astype(np.uint8))


@pytest.mark.parametrize("n_step", [1, 2, 3, 8])
def test_masked_tree_equals_mask_times_priority_after_every_push(n_step):
    cap, n_env, ns = 8, 3, 2
    rng = np.random.default_rng(n_step)
    m = Mirror(cap, n_env, ns, n_step, DEFAULT)
    m.push_state(rng.standard_normal((ns, n_env)).astype(np.float32))
    plain = oracle.SumTree(cap * n_env)          # n_step = 1 only: the shipped push on the same ring
    prio_of = {}                                  # (transition number, env) -> priority written back
    for k in range(1, 2 * cap + 6):               # fill, exactly full (k = cap), two wraps
        _push(m, rng)
        want = np.zeros((cap, n_env), np.float32)
        for j in range(max(0, k - cap), k):       # transition j lives in physical frame j mod cap
            if j + n_step <= k:                   # n_step transitions at or after it
                for e in range(n_env):
                    want[j % cap, e] = prio_of.get((j, e), DEFAULT)
        assert np.array_equal(m.st.leaves().reshape(cap, n_env), want), f"push {k}"
        # internal nodes: left + right of the stored children (the rule of every tree in this project)
        t, P = m.st.tree, m.st.P
        for node in range(P - 1, 0, -1):
            assert t[node] == np.float32(t[2 * node] + t[2 * node + 1])
        if n_step == 1:
            oracle.ring_push_priority(m.ring, plain, DEFAULT)
            assert np.array_equal(plain.tree.view(np.uint32), m.st.tree.view(np.uint32))
        if len(m.ring) >= n_step:
            idx, key, prio = oracle.ring_sample_prioritized(m.ring, m.st, 64, 11, k)
            assert (idx // n_env).max() <= len(m.ring) - n_step, f"push {k}: a start without {n_step} transitions ahead"
            assert np.all(prio > 0)
            head = m.ring.rb.head_rt
            assert np.array_equal(key, ((idx // n_env + head) % cap) * n_env + idx % n_env)
            if n_step > 1 and k % 3 == 0:         # write-back under drawn keys (a masked leaf is never drawn), one of them zero
                newp = (rng.random(8) * 4).astype(np.float32)
                newp[0] = 0.0
                m.st.update(key[:8], newp)
                first = k - len(m.ring)
                for kk, pp in zip(key[:8], newp):  # sequential semantics: the last duplicate wins
                    li = (int(kk) // n_env - head) % cap
                    prio_of[(first + li, int(kk) % n_env)] = pp
    assert not np.array_equal(m.st.leaves(), np.zeros(cap * n_env, np.float32))


def test_reference_push_while_the_first_window_fills_leaves_no_mass():
    m = Mirror(8, 3, 2, 3, DEFAULT)
    rng = np.random.default_rng(0)
    m.push_state(np.zeros((2, 3), np.float32))
    for k in (1, 2):
        _push(m, rng)
        assert m.st.tree[1] == 0.0
    _push(m, rng)
    assert m.st.tree[1] == np.float32(3 * DEFAULT) and np.array_equal(m.st.leaves()[:3], np.full(3, DEFAULT, np.float32))


def test_new_entry_points_are_declared_bound_and_called_with_their_types():
    from rlhip import _lib

    protos = header_prototypes()
    want = {"rlhip_ring_push_priority_nstep": ("Int32", ["ptr", "ptr", "Float32", "Int32", "ptr"]),
            "rlhip_per_sample_fold_nstep_f32": ("Int32", ["ptr", "ptr", "Int64", "Int32", "Float32", "UInt64", "UInt32", "ptr", "ptr",
                                                          "ptr", "ptr", "ptr", "ptr"])}
    cls = {C.c_int32: "Int32", C.c_int64: "Int64", C.c_uint32: "UInt32", C.c_uint64: "UInt64", C.c_float: "Float32"}
    bound = {c[0] for c in glue_ccalls()}
    for name, sig in want.items():
        assert protos[name] == sig
        res, args = _lib._PROTOS[name]
        assert res is C.c_int32 and [cls.get(a, "ptr") for a in args] == sig[1]
        assert name in bound, f"RLHip.jl has no ccall of {name}"
    assert _lib.lib.rlhip_abi_version() == 2  # entry points were added, nothing changed


FAKE = 0x10000  # a 64-byte aligned address that nothing dereferences: every call below is refused before a launch


def _ring(capacity, n_env, obs_dim, stored, where=FAKE):
    from rlhip import _lib

    rb = _lib.Ring()
    if obs_dim <= 4:
        _lib.call("rlhip_ring_init", C.byref(rb), capacity, n_env, obs_dim, 4, where, None, None, None)
    else:
        _lib.call("rlhip_ring_init", C.byref(rb), capacity, n_env, obs_dim, 4, where, where, where, where)
    rb.len_rt, rb.len_sa = stored, stored + 1
    return rb


def _host_traces(rl, n_step, stored=0, cap=8, n_env=3, records_layout=True):
    """a CircularPrioritizedTraces without device storage: the host fields the learner and the sampler read before they launch"""
    tr = object.__new__(rl.CircularPrioritizedTraces)
    tr.__dict__.update(capacity=cap, n_env=n_env, obs_dim=4, records_layout=records_layout, rb=_ring(cap, n_env, 4, stored), n_step=n_step,
                       default_priority=DEFAULT, n_leaves=cap * n_env)
    return tr


def test_arguments_are_refused_before_any_device_call():
    from rlhip._lib import RLHipArgumentError, call

    src = _ring(8, 3, 4, 2)                       # two stored steps
    counters = lambda r: (r.head_sa, r.len_sa, r.head_rt, r.len_rt)  # noqa: E731
    for n_step, message in ((9, "capacity"), (0, "n_step"), (33, "n_step")):
        with pytest.raises(RLHipArgumentError, match=message):   # n_step > capacity: before anything moves
            call("rlhip_ring_push_priority_nstep", C.byref(src), FAKE, DEFAULT, n_step, None)
    with pytest.raises(RLHipArgumentError):
        call("rlhip_ring_push_priority_nstep", C.byref(src), None, DEFAULT, 2, None)
    with pytest.raises(RLHipArgumentError, match="record rings"):
        call("rlhip_ring_push_priority_nstep", C.byref(_ring(8, 3, 6, 2)), FAKE, DEFAULT, 2, None)
    with pytest.raises(RLHipArgumentError, match="no transition"):
        call("rlhip_ring_push_priority_nstep", C.byref(_ring(8, 3, 4, 0)), FAKE, DEFAULT, 2, None)
    folded = _ring(1, 4, 4, 0, 2 * FAKE)

    def fused(n_step, batch=4, dst=folded, s=src, tree=FAKE, idx=FAKE):
        call("rlhip_per_sample_fold_nstep_f32", C.byref(s), tree, batch, n_step, 0.9, 1, 0, idx, None, None, C.byref(dst), None, None)

    with pytest.raises(RLHipArgumentError, match="fewer than n_step"):
        fused(3)                                  # length 2 < n_step 3: the masked tree has no mass
    for kw, message in ((dict(n_step=33), "n_step"), (dict(n_step=2, batch=5), "n_env = batch"), (dict(n_step=2, batch=3, dst=src), "alias"),
                        (dict(n_step=2, s=_ring(4, 3, 6, 3)), "record rings"), (dict(n_step=2, tree=None), "bad arguments"),
                        (dict(n_step=2, idx=None), "bad arguments"), (dict(n_step=2, batch=0), "bad arguments"),
                        (dict(n_step=1, s=_ring(8, 3, 4, 0)), "empty")):
        with pytest.raises(RLHipArgumentError, match=message):
            fused(**kw)
    assert counters(src) == (0, 3, 0, 2) and counters(folded) == (0, 1, 0, 0)


def test_traces_constructor_checks_n_step_before_it_allocates():
    import rlhip as rl

    for kw in (dict(capacity=8, n_step=9), dict(capacity=64, n_step=33), dict(capacity=8, n_step=0)):
        with pytest.raises((ValueError, rl._lib.RLHipError)) as e:
            rl.CircularPrioritizedTraces(n_env=3, obs_dim=4, device="cpu", **kw)
        assert isinstance(e.value, ValueError) and "n_step" in str(e.value)


def test_learner_and_sampler_on_cpu_only_objects_construct_and_check_the_mask():
    import rlhip as rl

    ns, h, na = 4, 32, 2
    for double in (False, True):
        net = rl.HipApproximator(ns, h, na, params=oracle.mlp2_init(ns, h, na, 1, 0), device="cpu")
        learner = rl.DQNLearner(rl.TargetNetwork(net), batchsize=16, min_replay_history=1, n_step=3, double_dqn=double, per_beta=0.4)
        assert learner.n_step == 3 and learner._nstep.n == 3
        traj = rl.Trajectory(_host_traces(rl, 3, stored=2))
        assert learner.optimise_(traj) is False   # not one full window yet: no NotImplementedError, no draw, the vec-step counts
        assert learner.vec_steps == 1 and traj.controller.n_sampled == 0
        with pytest.raises(ValueError, match="n_step"):
            learner.optimise_(rl.Trajectory(_host_traces(rl, 2, stored=5)))
    smp = rl.NStepBatchSampler(3, 0.9, 16)
    with pytest.raises(ValueError, match="n_step"):
        smp.sample_indices(_host_traces(rl, 1, stored=5))
    with pytest.raises(rl._lib.RLHipArgumentError):   # the masked tree has no mass yet
        smp.sample_indices(_host_traces(rl, 3, stored=2))
    with pytest.raises(TypeError):
        smp.sample_fold_prioritized(object.__new__(rl.CircularArraySARTSTraces))


def test_checkpoint_carries_the_mask_width_and_the_traces_check_it_when_it_is_restored():
    import rlhip as rl

    a, b = _host_traces(rl, 3), _host_traces(rl, 1)
    d = rl.state_dict({"traces": a})
    assert d["traces/n_step"] == 3
    rl.load_state_dict({"traces": b}, d)
    assert b.n_step == 3 and type(b.n_step) is int
    for bad, message in ((9, "capacity"), (0, "1..32"), (33, "1..32")):   # what the constructor refuses, load refuses
        with pytest.raises(ValueError, match=message):
            rl.load_state_dict({"traces": b}, dict(d, **{"traces/n_step": np.asarray(bad)}))
        assert b.n_step == 3
    frames = _host_traces(rl, 1, records_layout=False)   # a frame ring serves n_step = 1 only
    with pytest.raises(ValueError, match="record ring"):
        rl.load_state_dict({"traces": frames}, d)
    del d["traces/n_step"]
    with pytest.raises(KeyError):                 # strict loading is what it was
        rl.load_state_dict({"traces": b}, d)
