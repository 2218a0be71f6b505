"""rlhip_ring_gather_nstep / rlhip_ring_gather_stacked_nstep (csrc/ring_nstep.hip) on the device, byte for byte against the list model
of tests/ring_nstep_ref.py.  Every ring is filled through the push ABI, every output is poisoned with 0xA5 first, and the batch is
every valid flat index, shuffled, with duplicates added (what that batch holds is asserted on the CPU: the census of
tests/test_ring_nstep_reference.py).

Route per plain case (dtype, obs_dim x n_env, capacity):
  f32    6 x 5    cap 7   gather_small_nstep_kernel<float>
  f32    5 x 300  cap 3   a batch beyond one 256-sample tile
  u8     7 x 3    cap 5   gather_small_nstep_kernel<uint8_t>, odd frame size
  u8  1008 x 1    cap 4   small route with n_env = 1: below 1024 bytes
  u8  1030 x 1    cap 4   small route: no multiple of 16 bytes
  u8  1024 x 1    cap 6   gather_frames_nstep_kernel, the smallest frame-major frame (64 chunks: a quarter of the first trip)
  f32  256 x 1    cap 6   gather_frames_nstep_kernel on Float32 frames
  u8  7056 x 1    cap 6   gather_frames_nstep_kernel, 441 chunks: the second half-trip is partial
each after 2 pushes (ring not full) and after 2 * capacity + 3 (wrapped), n_step in {1, 2, 3, capacity, 32}, gamma in {0.99, 0, 1}.
Stacked cases (n_env = 1): u8 48, u8 7056, f32 8 at capacity 12, after 5 and 27 pushes, n_stack in {1, 2, 4, 8}, n_step in {1, 2, 5, 32}."""
import ctypes as C

import numpy as np
import pytest
import torch

import ring_nstep_ref as R
from ring_ref import case_id

pytestmark = pytest.mark.gpu

NAMES = ("state", "action", "return", "terminal", "next_state", "n_used")
GAMMA = 0.99


def _dev(x):
    return torch.as_tensor(np.ascontiguousarray(x), device="cuda")


def _traces(dtype, od, n_env, cap, cls=None, **kw):
    import rlhip

    cls = cls or rlhip.CircularArraySARTSTraces
    return cls(capacity=cap, n_env=n_env, obs_dim=od, dtype=torch.uint8 if dtype == "u8" else torch.float32, **kw)


def _sink(tr):
    def push(f, a, r, t):
        if a is None:
            tr.push_state_(_dev(f))
        else:
            tr.push_transition_(_dev(f), _dev(a), _dev(r), _dev(t))
    return push


def _same(got, want, where):
    for name, g, w in zip(NAMES, got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, (where, name, g.dtype, w.dtype, g.shape, w.shape)
        gb, wb = g.reshape(-1).view(np.uint8), w.reshape(-1).view(np.uint8)  # bytes: -0.0 is not +0.0 here
        if not np.array_equal(gb, wb):
            bad = np.argwhere(g.reshape(-1) != w.reshape(-1)).reshape(-1)
            first = int(bad[0]) if bad.size else int(np.argwhere(gb != wb)[0, 0]) // g.itemsize
            raise AssertionError(f"{where}: {name} differs in {max(len(bad), 1)} of {g.size} elements, first at flat {first}: "
                                 f"{g.reshape(-1)[first]!r} != {w.reshape(-1)[first]!r}")


def _poisoned(tr, b, shape):
    dev = tr.state.device
    raw = lambda n_el, dt: torch.full((n_el * torch.empty(0, dtype=dt).element_size(),), 0xA5, dtype=torch.uint8, device=dev).view(dt)  # noqa: E731
    n_state = int(np.prod(shape))
    return (raw(n_state, tr.dtype).view(shape), raw(b, torch.int32), raw(b, torch.float32), raw(b, torch.uint8),
            raw(n_state, tr.dtype).view(shape), raw(b, torch.int32))


def _gather_nstep(tr, idx, n_step, gamma, n_stack=None):
    """the C ABI on poisoned outputs (rlhip's wrappers allocate with torch.empty; here every byte must be written by the launch)"""
    from rlhip._lib import call
    from rlhip.ops import ptr, stream_ptr

    b = idx.numel()
    shape = (b, n_stack, tr.obs_dim) if n_stack else ((b, tr.obs_dim) if tr.frame_major else (tr.obs_dim, b))
    s, a, ret, t, sn, nu = out = _poisoned(tr, b, shape)
    if n_stack:
        call("rlhip_ring_gather_stacked_nstep", C.byref(tr.rb), ptr(idx), b, n_stack, n_step, gamma, ptr(s), ptr(a), ptr(ret), ptr(t),
             ptr(sn), ptr(nu), stream_ptr())
    else:
        call("rlhip_ring_gather_nstep", C.byref(tr.rb), ptr(idx), b, n_step, gamma, ptr(s), ptr(a), ptr(ret), ptr(t), ptr(sn), ptr(nu),
             stream_ptr())
    return tuple(x.cpu().numpy() for x in out)


PLAIN = [(c, p) for c in R.PLAIN_CASES for p in R.plain_pushes(c[3])]


@pytest.mark.parametrize("case,pushes", PLAIN, ids=[f"{case_id(c)}-{p}pushes" for c, p in PLAIN])
def test_gather_nstep_equals_the_list_model(case, pushes):
    dtype, od, n_env, cap, want_frame_major = case
    tr = _traces(dtype, od, n_env, cap)
    assert tr.frame_major == want_frame_major and not tr.records_layout  # the case still takes the kernel the table names
    ref = R.plain_model(case, pushes, _sink(tr))
    assert len(tr) == len(ref) == min(pushes, cap)
    idx = R.exhaustive_batch(ref, pushes)
    didx = _dev(idx)
    one = tuple(x.cpu().numpy() for x in tr.gather(didx))
    for n_step in R.PLAIN_NSTEPS(cap):
        for gamma in R.GAMMAS:
            got = _gather_nstep(tr, didx, n_step, gamma)
            want = ref.gather_nstep(idx, n_step, gamma)
            _same(got, R.frame_major6(want) if want_frame_major else want, f"n_step {n_step}, gamma {gamma}")
            if n_step == 1:  # the 1-step gather, byte for byte but for the sign of a zero reward
                for k in (0, 1, 3, 4):
                    assert np.array_equal(got[k], one[k]), NAMES[k]
                assert np.array_equal(got[2], one[2]) and (got[5] == 1).all()
                zeros = one[2] == 0
                assert not got[2][zeros].view(np.uint32).any()  # r + gamma * 0: a stored -0.0 comes back as +0.0
    # the wrapper of rlhip, and n_used = NULL
    s, a, ret, t, sn, nu = (x.cpu().numpy() for x in tr.gather_nstep(didx, 3, GAMMA))
    want = ref.gather_nstep(idx, 3, GAMMA)
    _same((s, a, ret, t, sn, nu), R.frame_major6(want) if want_frame_major else want, "rlhip wrapper")
    from rlhip._lib import call
    from rlhip.ops import ptr, stream_ptr

    b = idx.size
    s2, a2, ret2, t2, sn2, _ = _poisoned(tr, b, s.shape)
    call("rlhip_ring_gather_nstep", C.byref(tr.rb), ptr(didx), b, 3, GAMMA, ptr(s2), ptr(a2), ptr(ret2), ptr(t2), ptr(sn2), None, stream_ptr())
    _same(tuple(x.cpu().numpy() for x in (s2, a2, ret2, t2, sn2)), (s, a, ret, t, sn), "n_used = NULL")


STACKED = [(c, p) for c in R.STACKED_CASES for p in R.STACKED_PUSHES]


@pytest.mark.parametrize("case,pushes", STACKED, ids=[f"{c[0]}-{c[1]}-cap{c[2]}-{p}pushes" for c, p in STACKED])
def test_gather_stacked_nstep_equals_the_list_model(case, pushes):
    dtype, od, cap = case
    tr = _traces(dtype, od, 1, cap)
    ref = R.stacked_model(case, pushes, _sink(tr))
    assert len(tr) == len(ref) == min(pushes, cap)
    idx = R.exhaustive_batch(ref, pushes)
    didx = _dev(idx)
    for n_stack in R.STACKS:
        one = tuple(x.cpu().numpy() for x in tr.gather_stacked(didx, n_stack))
        for n_step in R.STACKED_NSTEPS:
            got = _gather_nstep(tr, didx, n_step, GAMMA, n_stack)
            _same(got, ref.gather_stacked_nstep(idx, n_stack, n_step, GAMMA), f"n_stack {n_stack}, n_step {n_step}")
            if n_step == 1:
                for k in (0, 1, 3, 4):
                    assert np.array_equal(got[k], one[k]), NAMES[k]
                assert np.array_equal(got[2], one[2])
    got = tuple(x.cpu().numpy() for x in tr.gather_stacked_nstep(didx, 4, 5, GAMMA))
    _same(got, ref.gather_stacked_nstep(idx, 4, 5, GAMMA), "rlhip wrapper")


@pytest.mark.parametrize("n_step", [1, 2, 3, 7, 32])
def test_action_return_and_terminal_equal_the_record_ring_fold(n_step):
    """the same (a, r, t) pushed into a frame ring and into a record ring: rlhip_ring_gather_nstep and rlhip_ring_fold_nstep give
    the same action, return (bit for bit) and terminal flag for every start that rlhip_ring_fold_nstep takes"""
    import rlhip as rl

    cap, n_env = 7, 5
    for pushes in (3, 2 * cap + 3):
        frames, records = _traces("f32", 6, n_env, cap), _traces("f32", 2, n_env, cap)
        assert records.records_layout
        rng = np.random.default_rng([n_step, pushes, 3])
        ref = R.fill(R.RingNStepRef(cap, n_env, 6, np.float32), rng, "f32", pushes, 0.25, _sink(frames))
        records.push_state_(_dev(np.zeros((2, n_env), np.float32)))
        for a, r, t in zip(ref.a, ref.r, ref.t):
            records.push_transition_(_dev(rng.standard_normal((2, n_env)).astype(np.float32)), _dev(a), _dev(r), _dev(t))
        idx = _dev(R.exhaustive_batch(ref, pushes))
        for gamma in R.GAMMAS:
            _, a, ret, t, _, _ = frames.gather_nstep(idx, n_step, gamma)
            folded, iota = rl.NStepBatchSampler(n_step, gamma, idx.numel()).fold(records, idx)
            _, fa, fr, ft, _ = folded.gather(iota)
            assert torch.equal(a, fa) and torch.equal(t, ft)
            assert torch.equal(ret.view(torch.int32), fr.view(torch.int32))


@pytest.mark.parametrize("case,n_stack", [(("u8", 7056, 1, 40, True), None), (("f32", 6, 5, 9, False), None), (("u8", 7056, 1, 40, True), 4)],
                         ids=["frame-major", "small", "stacked"])
def test_sampler_on_a_frame_ring_equals_sample_indices_then_gather_nstep(case, n_stack):
    import rlhip as rl

    dtype, od, n_env, cap, _ = case
    tr = _traces(dtype, od, n_env, cap)
    ref = R.fill(R.RingNStepRef(cap, n_env, od, np.uint8 if dtype == "u8" else np.float32), np.random.default_rng(5), dtype, cap + 4, 0.2,
                 _sink(tr))
    n, batch = 3, 64
    smp, twin = rl.NStepBatchSampler(n, GAMMA, batch, seed=7, n_stack=n_stack), rl.NStepBatchSampler(n, GAMMA, batch, seed=7)
    for draw in range(2):
        got = smp.sample(tr)
        idx = twin.sample_indices(tr, draw)
        assert smp.draw_ctr == draw + 1 and (idx // n_env).max().item() <= len(tr) - n
        s, a, ret, t, sn, nu = tr.gather_stacked_nstep(idx, n_stack, n, GAMMA) if n_stack else tr.gather_nstep(idx, n, GAMMA)
        assert set(got) == {"state", "action", "reward", "terminal", "next_state", "key", "n_steps"}
        assert torch.equal(got["key"], idx) and torch.equal(got["state"], s) and torch.equal(got["next_state"], sn)
        assert torch.equal(got["action"], a + 1) and torch.equal(got["reward"].view(torch.int32), ret.view(torch.int32))
        assert got["terminal"].dtype == torch.bool and torch.equal(got["terminal"].view(torch.uint8), t)
        assert torch.equal(got["n_steps"], nu) and got["n_steps"].dtype == torch.int32
        # ... and the model under the same indices
        hidx = idx.cpu().numpy()
        want = ref.gather_stacked_nstep(hidx, n_stack, n, GAMMA) if n_stack else ref.gather_nstep(hidx, n, GAMMA)
        _same(tuple(x.cpu().numpy() for x in (s, a, ret, t, sn, nu)), R.frame_major6(want) if tr.frame_major and not n_stack else want,
              f"draw {draw}")


@pytest.mark.parametrize("case", [("u8", 1024, 1, 9, True), ("u8", 7, 3, 9, False)], ids=["frame-major", "small"])
def test_a_prioritized_one_step_draw_feeds_gather_nstep(case):
    """any stored transition is a legal start: the indices of rlhip_ring_sample_prioritized (1-step traces, starts without n
    transitions ahead included) go straight into the n-step gather"""
    import rlhip as rl

    dtype, od, n_env, cap, fm = case
    tr = _traces(dtype, od, n_env, cap, cls=rl.CircularPrioritizedTraces, default_priority=1.5)
    ref = R.fill(R.RingNStepRef(cap, n_env, od, np.uint8), np.random.default_rng(11), dtype, cap + 5, 0.2, _sink(tr))
    idx, key, prio = tr.sample_prioritized(300, 3, 0)
    hidx = idx.cpu().numpy()
    assert hidx.min() >= 0 and hidx.max() < cap * n_env and (hidx // n_env).max() > cap - 4  # a start near the ring's end is in it
    for n_step in (1, 4):
        got = _gather_nstep(tr, idx, n_step, GAMMA)
        want = ref.gather_nstep(hidx, n_step, GAMMA)
        _same(got, R.frame_major6(want) if fm else want, f"n_step {n_step}")


def test_bounds_checked_build_validates_the_start_indices():
    """lib/librlhip_bounds.so (-DRLHIP_BOUNDS_CHECK), loaded by a child process through RLHIP_LIB_PATH: both n-step gathers return
    RLHIP_EINVAL for an index outside [0, length * n_env) instead of launching, and give the model's batch for valid ones"""
    import os
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    so = os.path.join(root, "reinforcementlearning.jl_amd", "lib", "librlhip_bounds.so")
    assert os.path.exists(so), "run python -c 'import __graft_entry__ as g; g.build()'"
    prog = r"""
import sys, numpy as np, torch
sys.path.insert(0, sys.argv[1] + "/tests"); sys.path.insert(0, sys.argv[1] + "/reinforcementlearning.jl_amd")
import rlhip
from rlhip._lib import RLHipArgumentError, lib
import ring_nstep_ref as R
import test_gpu_ring_nstep as T
print("checked_build", lib.rlhip_ring_bounds_checked_build())
case = ("u8", 1024, 1, 6, True)
tr = T._traces(*case[:4])
ref = R.plain_model(case, 9, T._sink(tr))
idx = R.exhaustive_batch(ref, 9)
T._same(T._gather_nstep(tr, T._dev(idx), 3, 0.99), R.frame_major6(ref.gather_nstep(idx, 3, 0.99)), "plain")
T._same(T._gather_nstep(tr, T._dev(idx), 3, 0.99, 4), ref.gather_stacked_nstep(idx, 4, 3, 0.99), "stacked")
print("valid: equal")
for bad_value in (len(ref), -1):
    bad = idx.copy(); bad[2] = bad_value
    for name, f in (("plain", lambda: tr.gather_nstep(T._dev(bad), 3, 0.99)), ("stacked", lambda: tr.gather_stacked_nstep(T._dev(bad), 4, 3, 0.99))):
        try:
            f(); print(name, bad_value, "no error")
        except RLHipArgumentError as e:
            print(name, bad_value, "EINVAL", "outside" in str(e))
"""
    r = subprocess.run([sys.executable, "-c", prog, root], capture_output=True, text=True, timeout=300, env=dict(os.environ, RLHIP_LIB_PATH=so))
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [ln for ln in r.stdout.splitlines() if ln.split(" ")[0] in ("checked_build", "valid:", "plain", "stacked")]
    assert lines == ["checked_build 1", "valid: equal", "plain 6 EINVAL True", "stacked 6 EINVAL True", "plain -1 EINVAL True",
                     "stacked -1 EINVAL True"], r.stdout + r.stderr
