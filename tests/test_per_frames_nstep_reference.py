"""Prioritized n-step replay on frame rings (CircularPrioritizedFrameTraces, rlhip_ring_push_priority_nstep_frames,
rlhip_ring_sample_gather_nstep_prioritized, rlhip_ring_sample_gather_stacked_nstep_prioritized) -- the CPU half:

  * every refusal of the three entry points happens before any device call (the library loads without a GPU; the pointers are fake);
  * the mask law on the model of tests/per_frames_nstep_ref.py after every push, and what the draws of the device test hold (census);
  * the new class: constructor checks before allocation, n_step through a checkpoint, layouts refused on either side;
  * header / ctypes / Julia prototypes agree;
  * kernel resources of per_frames_nstep.o (the recipe of tests/test_ring_nstep_kernel_resources.py): no scratch, no spilled VGPR,
    workgroup bound 256, LDS exactly the declared arrays:
      sample_gather_small_nstep_kernel<E>   l_ps, l_pn 2 x 256 x 8 = 4 096; the reward columns 32 x 256 x 4 = 32 768
      sample_gather_frames_nstep_kernel     l_rew 32 x 4 = 128; l_next 2 x 8 = 16; l_li 8
      sample_gather_stacked_nstep_kernel    l_rew 128; l_off 18 x 8 = 144; l_ks, l_kn 2 x 16 x 4 = 128"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import oracle
import per_frames_nstep_ref as P
import ring_nstep_ref as R
from ring_ref import case_id
from test_julia_glue_signatures import glue_ccalls, header_prototypes
from test_rollout_kernel_resources import LLVM, ROOT, _kernel_meta

FAKE = 0x10000  # a 64-byte aligned address that nothing dereferences: every call below is refused before a launch
PLAIN = "rlhip_ring_sample_gather_nstep_prioritized"
STACKED = "rlhip_ring_sample_gather_stacked_nstep_prioritized"
PUSH = "rlhip_ring_push_priority_nstep_frames"


def _ring(capacity, n_env, obs_dim, stored, elem_bytes=1, where=FAKE):
    from rlhip import _lib

    rb = _lib.Ring()
    if elem_bytes == 4 and obs_dim <= 4:
        _lib.call("rlhip_ring_init", C.byref(rb), capacity, n_env, obs_dim, 4, where, None, None, None)
    else:
        _lib.call("rlhip_ring_init", C.byref(rb), capacity, n_env, obs_dim, elem_bytes, where, where, where, where)
    rb.len_rt, rb.len_sa = stored, stored + 1
    return rb


def _counters(r):
    return r.head_sa, r.len_sa, r.head_rt, r.len_rt


def test_the_push_refuses_what_the_record_rings_push_refuses_in_the_same_order():
    from rlhip._lib import RLHipArgumentError, call

    src = _ring(8, 3, 6, 2, 4)                    # Float32 frames, two stored steps
    for n_step, message in ((9, "capacity"), (0, "n_step"), (33, "n_step")):
        with pytest.raises(RLHipArgumentError, match=message):
            call(PUSH, C.byref(src), FAKE, 2.5, n_step, None)
    with pytest.raises(RLHipArgumentError, match="bad arguments"):
        call(PUSH, C.byref(src), None, 2.5, 2, None)
    with pytest.raises(RLHipArgumentError, match="bad arguments"):
        call(PUSH, None, FAKE, 2.5, 2, None)
    records = _ring(8, 3, 4, 2, 4)
    with pytest.raises(RLHipArgumentError, match="frame rings"):
        call(PUSH, C.byref(records), FAKE, 2.5, 2, None)
    with pytest.raises(RLHipArgumentError, match="n_step"):        # the range of n_step comes before the layout ...
        call(PUSH, C.byref(records), FAKE, 2.5, 33, None)
    with pytest.raises(RLHipArgumentError, match="frame rings"):   # ... and the layout before the capacity
        call(PUSH, C.byref(records), FAKE, 2.5, 9, None)
    with pytest.raises(RLHipArgumentError, match="non-negative"):
        call(PUSH, C.byref(src), FAKE, -1.0, 2, None)
    with pytest.raises(RLHipArgumentError, match="capacity"):      # the capacity before the priority
        call(PUSH, C.byref(src), FAKE, -1.0, 9, None)
    with pytest.raises(RLHipArgumentError, match="no transition"):
        call(PUSH, C.byref(_ring(8, 3, 6, 0, 4)), FAKE, 2.5, 2, None)
    with pytest.raises(RLHipArgumentError, match="record rings"):  # the record rings' entry point keeps refusing frames
        call("rlhip_ring_push_priority_nstep", C.byref(src), FAKE, 2.5, 2, None)
    assert _counters(src) == (0, 3, 0, 2) and _counters(records) == (0, 3, 0, 2)


def test_the_fused_calls_refuse_their_arguments_before_any_device_call():
    from rlhip._lib import RLHipArgumentError, call

    ring = _ring(8, 1, 1024, 5)                   # frame-major UInt8, five stored steps
    small = _ring(8, 3, 6, 5, 4)                  # component-major Float32

    def plain(rb=ring, tree=FAKE, batch=4, n_step=3, idx=FAKE, key=None, prio=None, s=FAKE, a=FAKE, ret=FAKE, term=FAKE, sn=FAKE, nu=None):
        call(PLAIN, C.byref(rb), tree, batch, n_step, 0.99, 1, 0, idx, key, prio, s, a, ret, term, sn, nu, None)

    def stacked(rb=ring, tree=FAKE, batch=4, n_stack=4, n_step=3, idx=FAKE, s=FAKE, a=FAKE, ret=FAKE, term=FAKE, sn=FAKE):
        call(STACKED, C.byref(rb), tree, batch, n_stack, n_step, 0.99, 1, 0, idx, None, None, s, a, ret, term, sn, None, None)

    for f in (plain, stacked):
        for kw, message in ((dict(n_step=0), "n_step"), (dict(n_step=33), "n_step"), (dict(rb=_ring(8, 1, 4, 5, 4)), "frame rings"),
                            (dict(rb=_ring(8, 1, 1024, 0)), "empty"), (dict(tree=None), "bad arguments"), (dict(idx=None), "bad arguments"),
                            (dict(s=None), "bad arguments"), (dict(a=None), "bad arguments"), (dict(ret=None), "bad arguments"),
                            (dict(term=None), "bad arguments"), (dict(sn=None), "bad arguments"), (dict(batch=-1), "bad arguments"),
                            (dict(s=FAKE + 4), "16-byte aligned"), (dict(tree=FAKE + 4), "8-byte aligned")):
            with pytest.raises(RLHipArgumentError, match=message):
                f(**kw)
    for kw, message in ((dict(n_stack=0), "n_stack"), (dict(n_stack=9), "n_stack"), (dict(rb=_ring(8, 2, 1024, 5)), "single-env"),
                        (dict(rb=_ring(8, 1, 1030, 5)), "multiple of 16")):
        with pytest.raises(RLHipArgumentError, match=message):
            stacked(**kw)
    bad = _ring(8, 1, 1024, 5)
    bad.head_rt = 8                               # a key would be mapped through counters that are out of range
    with pytest.raises(RLHipArgumentError, match="counters"):
        plain(rb=bad)
    # what is NOT refused: windows wider than the ring holds (the call does not know the mask), NULL key / priority / n_used, batch 0
    plain(batch=0, n_step=32)
    plain(rb=small, batch=0)
    stacked(batch=0, n_step=32)
    assert _counters(ring) == (0, 6, 0, 5) and _counters(small) == (0, 6, 0, 5)


ALL = [("plain", c) for c in P.PLAIN_CASES] + [("stacked", c) for c in P.STACKED_CASES]


def _maker(kind, case, pushes):
    if kind == "plain":
        return (lambda n, sink=None: P.plain_ref(case, pushes, n, sink)), case[3], case[2]
    return (lambda n, sink=None: P.stacked_ref(case, pushes, n, sink)), case[2], 1


def _fill_states(kind, cap):
    return R.plain_pushes(cap) if kind == "plain" else R.STACKED_PUSHES


@pytest.mark.parametrize("kind,case", ALL, ids=[f"{k}-{case_id(c) if k == 'plain' else f'{c[0]}-{c[1]}-cap{c[2]}'}" for k, c in ALL])
def test_mask_law_on_the_model_after_every_push(kind, case):
    """the set of leaves with mass equals the set of stored starts with n transitions at or after them; n = 1 is the plain push"""
    dtype, od = case[0], case[1]
    cap, n_env = (case[3], case[2]) if kind == "plain" else (case[2], 1)
    od = min(od, 8)                               # (the law does not look at the frames)
    for n in P.masked_nsteps(cap):
        ref = P.PrioritizedFramesRef(cap, n_env, od, np.uint8 if dtype == "u8" else np.float32, n)
        ring, plain = oracle.Ring(cap, n_env, 1), oracle.SumTree(cap * n_env)   # n = 1 only: the oracle's push on its own ring
        rng = np.random.default_rng([cap, n_env, n])
        ref.push_state(np.zeros((od, n_env), ref.dtype))
        ring.push_state(np.zeros((1, n_env), np.float32))
        for k in range(2 * cap + 3):
            a, r, t = R.nstep_traces(rng, n_env, 0.25)
            ref.push_transition(np.zeros((od, n_env), ref.dtype), a, r, t)
            leaves = ref.st.leaves()
            assert set(np.flatnonzero(leaves).tolist()) == ref.complete_starts(), f"n {n}, push {k}"
            assert set(leaves.tolist()) <= {0.0, P.PRIORITY}
            assert len(ref.complete_starts()) == max(0, len(ref) - n + 1) * n_env
            tree = ref.st.tree
            for node in range(ref.st.P - 1, 0, -1):   # internal nodes: left + right of the stored children
                assert tree[node] == np.float32(tree[2 * node] + tree[2 * node + 1])
            if n == 1:
                ring.push_transition(np.zeros((1, n_env), np.float32), a, r, t)
                oracle.ring_push_priority(ring, plain, P.PRIORITY)
                assert np.array_equal(plain.tree.view(np.uint32), tree.view(np.uint32)), f"push {k}"
            if ref.has_mass():                    # every draw is a complete start, and its key maps back through the lists
                idx, key, prio = ref.draw(32, 3, k)
                assert set(key.tolist()) <= ref.complete_starts() and (prio == np.float32(P.PRIORITY)).all()
                assert (idx // n_env).max() <= len(ref) - n


@pytest.mark.parametrize("kind,case", ALL, ids=[f"{k}-{case_id(c) if k == 'plain' else f'{c[0]}-{c[1]}-cap{c[2]}'}" for k, c in ALL])
def test_the_draws_of_the_device_test_hold_every_kind_of_window(kind, case):
    """The census of tests/test_gpu_per_frames_nstep.py, from the model alone (seeds: P.SEED and the content salts), per fill state and
    per kind of tree -- nothing is summed over fill states or over kinds, except where said:
      every fill state    no window drawn from a masked or written tree is cut by the ring's end
      the wrapped ring    each of the masked, the written and the unmasked trees holds a terminal-cut window and a full multi-step
                          window, the unmasked tree also a ring-end cut; stacked cases with n_stack > 1: each kind of tree holds a
                          zero-filled member in s and in s' and a window with ns < n_stack; a window with ns >= n_stack needs n >= n_stack
                          steps, which only the capacity-wide and the 32-step windows have: it is asserted on the kinds of tree taken
                          together
      the ring not full   holds two (plain) or five (stacked) transitions: a single-env ring then has one or two starts per tree and
                          cannot hold a full and a terminal-cut window at once, so nothing more is asserted of it"""
    cap = case[3] if kind == "plain" else case[2]
    states = _fill_states(kind, cap)
    for n_stack in ((None,) if kind == "plain" else P.STACKS):
        for pushes in states:
            make, _, _ = _maker(kind, case, pushes)
            c = P.census(make, cap, n_stack)
            where = f"{pushes} pushes, n_stack {n_stack}"
            print(kind, case, where, c)
            assert set(c) == {"masked", "written", "unmasked"}, where
            assert c["masked"]["ring_end_cut"] == 0 and c["written"]["ring_end_cut"] == 0, where
            if pushes != states[-1]:
                continue
            for tree in ("masked", "written", "unmasked"):
                assert c[tree]["terminal_cut"] >= 1 and c[tree]["full_multi_step"] >= 1, (where, tree)
            assert c["unmasked"]["ring_end_cut"] >= 1, where
            if n_stack is not None and n_stack > 1:
                for tree in ("masked", "written", "unmasked"):
                    assert c[tree]["zero_s"] >= 1 and c[tree]["zero_sn"] >= 1 and c[tree]["ns_lt_stack"] >= 1, (where, tree)
                assert sum(c[tree]["ns_ge_stack"] for tree in c) >= 1, where


def _host_traces(rl, cls, n_step, stored=0, cap=8, n_env=1, obs_dim=1024, records_layout=False):
    """prioritized traces without device storage: the host fields the sampler and the checkpoint read before anything launches"""
    tr = object.__new__(cls)
    tr.__dict__.update(capacity=cap, n_env=n_env, obs_dim=obs_dim, records_layout=records_layout,
                       rb=_ring(cap, n_env, obs_dim, stored, 4 if records_layout else 1), default_priority=2.5, n_leaves=cap * n_env)
    tr.n_step = n_step  # (through the class's own check, as the constructor and a checkpoint assign it)
    return tr


def test_constructor_checks_come_before_any_allocation():
    import rlhip as rl

    huge = dict(capacity=2 ** 40, n_env=1, obs_dim=7056, dtype=torch.uint8, device="cpu")  # allocating this would fail another way
    for n_step, message in ((0, "1..32"), (33, "1..32"), (True, "1..32"), (2.5, "1..32")):
        with pytest.raises(ValueError, match=message):
            rl.CircularPrioritizedFrameTraces(n_step=n_step, **huge)
    with pytest.raises(ValueError, match="capacity"):
        rl.CircularPrioritizedFrameTraces(capacity=8, n_env=1, obs_dim=7056, dtype=torch.uint8, device="cpu", n_step=9)
    with pytest.raises(ValueError, match="frame layout"):
        rl.CircularPrioritizedFrameTraces(capacity=2 ** 40, n_env=3, obs_dim=4, device="cpu", n_step=2)
    with pytest.raises(ValueError, match="record ring"):           # the base class still refuses frames
        rl.CircularPrioritizedTraces(n_step=3, **huge)
    assert issubclass(rl.CircularPrioritizedFrameTraces, rl.CircularPrioritizedTraces)


def test_checkpoint_carries_n_step_and_each_class_refuses_the_other_layout():
    import rlhip as rl

    frames = rl.CircularPrioritizedFrameTraces
    a, b = _host_traces(rl, frames, 3), _host_traces(rl, frames, 1)
    d = rl.state_dict({"traces": a})
    assert d["traces/n_step"] == 3
    rl.load_state_dict({"traces": b}, d)
    assert b.n_step == 3 and type(b.n_step) is int
    for bad, message in ((9, "capacity"), (0, "1..32"), (33, "1..32")):
        with pytest.raises(ValueError, match=message):
            rl.load_state_dict({"traces": b}, dict(d, **{"traces/n_step": np.asarray(bad)}))
        assert b.n_step == 3
    with pytest.raises(ValueError, match="record ring"):           # the base class over a frame ring: n_step = 1 only, as before
        rl.load_state_dict({"traces": _host_traces(rl, rl.CircularPrioritizedTraces, 1)}, d)
    with pytest.raises(ValueError, match="frame layout"):          # the new class over a record layout: never
        _host_traces(rl, frames, 1, obs_dim=4, records_layout=True)


def test_sampler_refuses_before_any_launch():
    import rlhip as rl

    frames = rl.CircularPrioritizedFrameTraces
    for n_stack in (None, 4):
        smp = rl.NStepBatchSampler(3, 0.99, 16, n_stack=n_stack)
        with pytest.raises(rl._lib.RLHipArgumentError, match="no mass"):
            smp.sample(_host_traces(rl, frames, 3, stored=2))
        with pytest.raises(ValueError, match="n_step"):
            smp.sample(_host_traces(rl, frames, 2, stored=5))
        assert smp.draw_ctr == 0


def test_new_entry_points_are_declared_bound_and_called_with_their_types():
    from rlhip import _lib

    protos = header_prototypes()
    draw = ["ptr", "ptr", "Int64"]
    tail = ["Float32", "UInt64", "UInt32"] + ["ptr"] * 10
    want = {PUSH: ("Int32", ["ptr", "ptr", "Float32", "Int32", "ptr"]),
            PLAIN: ("Int32", draw + ["Int32"] + tail),
            STACKED: ("Int32", draw + ["Int32", "Int32"] + tail)}
    cls = {C.c_int32: "Int32", C.c_int64: "Int64", C.c_uint32: "UInt32", C.c_uint64: "UInt64", C.c_float: "Float32"}
    glue = {c[0]: c for c in glue_ccalls()}
    for name, sig in want.items():
        assert protos[name] == sig
        res, args = _lib._PROTOS[name]
        assert res is C.c_int32 and [cls.get(a, "ptr") for a in args] == sig[1]
        assert hasattr(_lib.lib, name)
        assert name in glue, f"RLHip.jl has no ccall of {name}"
        assert glue[name][1] == "Int32" and glue[name][2] == sig[1]
    assert protos[PUSH] == protos["rlhip_ring_push_priority_nstep"]
    assert _lib.lib.rlhip_abi_version() == 2      # entry points were added, nothing changed


OBJ = os.path.join(ROOT, "reinforcementlearning.jl_amd", "build", "per_frames_nstep.o")
# kernel -> (instantiations, LDS bytes)
KERNELS = {
    "sample_gather_small_nstep_kernel": (2, 2 * 256 * 8 + 32 * 256 * 4),
    "sample_gather_frames_nstep_kernel": (1, 32 * 4 + 2 * 8 + 8),
    "sample_gather_stacked_nstep_kernel": (1, 32 * 4 + 18 * 8 + 2 * 16 * 4),
}


@pytest.mark.skipif(not os.path.exists(f"{LLVM}/llvm-readelf"), reason="no llvm-readelf")
def test_fused_kernels_keep_their_registers_and_lds(tmp_path):
    import __graft_entry__ as g

    g.build()
    meta = _kernel_meta(OBJ, str(tmp_path))
    assert all(any(k in name for k in KERNELS) for name in meta), f"a kernel of per_frames_nstep.o this test does not know: {sorted(meta)}"
    bad = []
    for kernel, (count, lds) in KERNELS.items():
        mine = {k: v for k, v in meta.items() if kernel in k}
        assert len(mine) == count, f"expected {count} instantiations of {kernel}, found {sorted(mine)}"
        for name, m in mine.items():
            print(f"{name}: {m}")
            if m["scratch"] or m["vspill"]:
                bad.append(f"{name}: {m['scratch']} B of scratch, {m['vspill']} spilled VGPRs")
            if m["wg"] != 256:
                bad.append(f"{name}: workgroup bound {m['wg']}")
            if m["lds"] != lds:
                bad.append(f"{name}: {m['lds']} bytes of LDS, declared {lds}")
    assert not bad, "\n".join(bad)
