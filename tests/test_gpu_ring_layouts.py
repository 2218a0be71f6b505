"""Every push and gather route of csrc/ring.hip that no other test fills through the push ABI and compares on stored content,
bit-exact against the list model of tests/ring_ref.py (and against oracle.Ring, itself pinned to the model on the CPU by
tests/test_ring_reference.py).  Everything runs through rlhip.CircularArraySARTSTraces, i.e. through the C ABI.

Route per case of ring_ref.CASES (dtype, obs_dim x n_env, capacity):
  f32   6 x 5    cap 7   frame = 120 B, no multiple of 16: push_art_kernel + copy1_kernel; gather_small_kernel<float>
  f32   6 x 8    cap 5   192 B: the fused push_transition_kernel with n16 = 12 > n = 8
  f32   5 x 300  cap 3   gathered batches that are no multiple of GATHER_TILE = 256; n_env beyond one workgroup of the trace loop
  f32   8 x 1    cap 9   single env, 32 B frame: below the frame-major bound
  u8    4 x 8    cap 6   32 B: the fused push with n16 = 2 < n = 8; gather_small_kernel<uint8_t>
  u8   32 x 3    cap 5   96 B: the fused push
  u8    7 x 3    cap 5   21 B: the copy1 fallback; slots land on unaligned offsets
  u8 1008 x 1    cap 4   16-aligned but < 1024 B: not frame-major
  u8 1030 x 1    cap 4   >= 1024 B but no multiple of 16: not frame-major
  u8 1024 x 1    cap 4   the smallest frame-major frame: gather_frames_kernel
  f32   1 x 37   cap 6   push_record_kernel<1> / gather_rec_kernel<1> with content and wrap
  f32   3 x 37   cap 6   push_record_kernel<3> / gather_rec_kernel<3> with content and wrap

Not covered: the grid-stride loops behind STREAM_GRID_CAP run only for frames of more than 4 GiB (2^20 workgroups x 256 lanes x
16 bytes)."""
import numpy as np
import pytest
import torch

import oracle
from ring_ref import CASES, RingRef, case_id, frame_major, random_frame, random_traces

pytestmark = pytest.mark.gpu

NAMES = ("state", "action", "reward", "terminal", "next_state")


def _dev(x):
    return torch.as_tensor(np.ascontiguousarray(x), device="cuda")


def _host(batch):
    return tuple(x.cpu().numpy() for x in batch)


def _same(got, want, where):
    for name, g, w in zip(NAMES, got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, (where, name, g.dtype, w.dtype, g.shape, w.shape)
        if not np.array_equal(g, w):
            bad = np.argwhere(g != w)
            raise AssertionError(f"{where}: {name} differs in {len(bad)} of {g.size} elements, first at {bad[0].tolist()}: "
                                 f"{g[tuple(bad[0])]!r} != {w[tuple(bad[0])]!r}")


def _traces(dtype, od, n_env, cap, cls=None, **kw):
    import rlhip

    cls = cls or rlhip.CircularArraySARTSTraces
    return cls(capacity=cap, n_env=n_env, obs_dim=od, dtype=torch.uint8 if dtype == "u8" else torch.float32, **kw)


def _np_dtype(dtype):
    return np.uint8 if dtype == "u8" else np.float32


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_push_then_gather_equals_the_list_model_after_every_push(case):
    dtype, od, n_env, cap, want_frame_major = case
    rng = np.random.default_rng([od, n_env, cap])
    tr = _traces(dtype, od, n_env, cap)
    assert tr.frame_major == want_frame_major  # the case still takes the kernel the table names
    assert tr.records_layout == (dtype == "f32" and od <= 4)
    ref = RingRef(cap, n_env, od, _np_dtype(dtype))
    ring = oracle.Ring(cap, n_env, od)
    f = random_frame(rng, dtype, od, n_env)
    tr.push_state_(_dev(f))
    ref.push_state(f)
    ring.push_state(f.astype(np.float32))
    assert len(tr) == 0
    seen = set()
    for k in range(1, 2 * cap + 4):  # fill, exactly full, two wraps
        f, (a, r, t) = random_frame(rng, dtype, od, n_env), random_traces(rng, n_env)
        tr.push_transition_(_dev(f), _dev(a), _dev(r), _dev(t))
        ref.push_transition(f, a, r, t)
        ring.push_transition(f.astype(np.float32), a, r, t)
        assert len(tr) == len(ref) == min(k, cap)
        total = len(ref) * n_env
        drawn = tr.sample_indices(300, 11, k)
        idx = torch.cat([torch.arange(total, dtype=torch.int64, device="cuda"), drawn])
        got = _host(tr.gather(idx))
        idx = idx.cpu().numpy()
        assert idx[total:].min() >= 0 and idx[total:].max() < total
        want = ref.gather(idx)
        _same(got, frame_major(want) if want_frame_major else want, f"push {k}")
        # ... and the oracle, which holds the same content as Float32
        s, a_, r_, t_, sn = got if not want_frame_major else (got[0].T, got[1], got[2], got[3], got[4].T)
        _same((s.astype(np.float32), a_, r_, t_, sn.astype(np.float32)), ring.gather(idx), f"push {k} (oracle)")
        # one multiplexed state trace: s' of (li, e) is s of (li + 1, e)
        assert np.array_equal(sn[:, :total - n_env], s[:, n_env:total])
        seen.update(np.unique(got[0]).tolist() if dtype == "u8" else ())
    if dtype == "u8":
        assert {0, 255} <= seen  # both ends of the range went through the ring


def test_push_from_a_misaligned_source_pointer():
    """a 96-byte frame is 16-byte aligned, a source that starts one byte into its allocation is not: the fused push must not be
    taken (push_art_kernel + copy1_kernel instead), and the content must not notice"""
    dtype, od, n_env, cap = "u8", 32, 3, 5
    rng = np.random.default_rng(96)
    tr = _traces(dtype, od, n_env, cap)
    ref = RingRef(cap, n_env, od, np.uint8)
    backing = torch.zeros(od * n_env + 64, dtype=torch.uint8, device="cuda")
    assert backing.data_ptr() % 16 == 0
    src = backing[1:1 + od * n_env].view(od, n_env)
    assert src.data_ptr() % 16 == 1 and src.is_contiguous()
    f = random_frame(rng, dtype, od, n_env)
    src.copy_(_dev(f))
    tr.push_state_(src)
    ref.push_state(f)
    for k in range(1, 2 * cap + 4):
        f, (a, r, t) = random_frame(rng, dtype, od, n_env), random_traces(rng, n_env)
        src.copy_(_dev(f))
        tr.push_transition_(src, _dev(a), _dev(r), _dev(t))
        ref.push_transition(f, a, r, t)
        idx = np.arange(len(ref) * n_env)
        _same(_host(tr.gather(_dev(idx))), ref.gather(idx), f"push {k}")
    assert not backing[0].item() and not backing[1 + od * n_env:].any().item()  # the pushes read, they never wrote


@pytest.mark.parametrize("od,n_env", [(16, 4), (4, 8), (7056, 3), (64, 300)], ids=lambda v: str(v))
def test_maxpool_pushes_of_a_vector_env(od, n_env):
    """rlhip_ring_push_state_maxpool / rlhip_ring_push_transition_maxpool with n_env > 1 (n16 = n, n16 < n, the Atari frame,
    n_env beyond one workgroup), alternating with the plain push within one fill: frames = max.(screen1, screen2), and the three
    traces land in the row of their transition"""
    cap = 5
    rng = np.random.default_rng([od, n_env])
    tr = _traces("u8", od, n_env, cap)
    assert not tr.frame_major
    ref = RingRef(cap, n_env, od, np.uint8)
    s1, s2 = random_frame(rng, "u8", od, n_env), random_frame(rng, "u8", od, n_env)
    tr.push_state_maxpool_(_dev(s1), _dev(s2))
    ref.push_state_maxpool(s1, s2)
    for k in range(1, 2 * cap + 4):
        s1, s2 = random_frame(rng, "u8", od, n_env), random_frame(rng, "u8", od, n_env)
        a, r, t = random_traces(rng, n_env)
        if k % 3 == 0:  # a plain push in between (pushes 3, 6, 9, 12: on either side of both wraps)
            tr.push_transition_(_dev(s1), _dev(a), _dev(r), _dev(t))
            ref.push_transition(s1, a, r, t)
        else:
            tr.push_transition_maxpool_(_dev(s1), _dev(s2), _dev(a), _dev(r), _dev(t))
            ref.push_transition_maxpool(s1, s2, a, r, t)
        if k in (cap - 1, cap, cap + 1, 2 * cap + 3):  # filling, exactly full, wrapped once, wrapped twice
            assert len(tr) == len(ref)
            idx = np.arange(len(ref) * n_env)
            _same(_host(tr.gather(_dev(idx))), ref.gather(idx), f"push {k}")


def test_frame_above_the_fused_push_bound():
    """a 16400 x 4096 UInt8 frame is 67 174 400 B > 64 MiB: rlhip_ring_push_transition leaves its fused kernel for push_art_kernel +
    copy16_kernel, and the max-pool push runs 16 400 workgroups.  Storage is compared on the device (about 0.4 GB); capacity 1 has
    two state slots, so pushed frame k lands in slot k % 2 and the one trace row is rewritten by every push."""
    od, n_env = 16400, 4096
    tr = _traces("u8", od, n_env, 1)
    assert od * n_env > 64 << 20 and not tr.frame_major
    g = torch.Generator(device="cuda").manual_seed(5)

    def screen():
        return torch.randint(0, 256, (od, n_env), dtype=torch.uint8, device="cuda", generator=g)

    def traces():
        return (torch.randint(0, 18, (n_env,), dtype=torch.int32, device="cuda", generator=g),
                torch.randn(n_env, device="cuda", generator=g),
                (torch.rand(n_env, device="cuda", generator=g) < 0.2).to(torch.uint8))

    prev = screen()
    tr.push_state_(prev)
    assert torch.equal(tr.state[0], prev) and not tr.state[1].any().item()
    for k in (1, 2, 3):
        f, (a, r, t) = screen(), traces()
        if k < 3:
            tr.push_transition_(f, a, r, t)
        else:  # the same size through the max-pool push
            s2 = screen()
            tr.push_transition_maxpool_(f, s2, a, r, t)
            f = torch.maximum(f, s2)
        assert len(tr) == 1
        assert torch.equal(tr.state[k % 2], f), f"push {k}: the new frame"
        assert torch.equal(tr.state[(k - 1) % 2], prev), f"push {k}: the frame before it was touched"
        assert torch.equal(tr.action[0], a) and torch.equal(tr.reward[0], r) and torch.equal(tr.terminal[0], t), f"push {k}: traces"
        # a handful of envs through the gather (element offsets up to 2 x 67 174 400)
        e = torch.tensor([0, 1, 255, 256, 2049, n_env - 2, n_env - 1], dtype=torch.int64, device="cuda")
        s, ga, gr, gt, sn = tr.gather(e)
        assert torch.equal(s, prev[:, e]) and torch.equal(sn, f[:, e]), f"push {k}: gather"
        assert torch.equal(ga, a[e]) and torch.equal(gr, r[e]) and torch.equal(gt, t[e]), f"push {k}: gathered traces"
        prev = f
    assert t.any().item() and not t.all().item() and f.min().item() == 0 and f.max().item() == 255


@pytest.mark.parametrize("dtype,od,n_env", [("u8", 4, 8), ("f32", 6, 5)], ids=["u8-4x8", "f32-6x5"])
def test_prioritized_draw_and_gather_of_layouts_without_a_fused_kernel(dtype, od, n_env):
    """rlhip_ring_sample_gather_prioritized on a ring that has no fused draw + gather kernel (its two-launch route): the batch is
    what the list model holds under the returned indices -- not what a second GPU call returns"""
    import rlhip

    cap, prio0 = 6, 1.5
    rng = np.random.default_rng([od, n_env, 7])
    tr = _traces(dtype, od, n_env, cap, cls=rlhip.CircularPrioritizedTraces, default_priority=prio0)
    assert not tr.frame_major and not tr.records_layout
    ref = RingRef(cap, n_env, od, _np_dtype(dtype))
    f = random_frame(rng, dtype, od, n_env)
    tr.push_state_(_dev(f))
    ref.push_state(f)
    for k in range(1, 2 * cap + 4):
        f, (a, r, t) = random_frame(rng, dtype, od, n_env), random_traces(rng, n_env)
        tr.push_transition_(_dev(f), _dev(a), _dev(r), _dev(t))
        ref.push_transition(f, a, r, t)
        if k in (1, cap - 1, cap, cap + 2, 2 * cap + 3):
            total = len(ref) * n_env
            for batch in (1, 300):
                (idx, key, prio), got = tr.sample_gather_prioritized(batch, 3, 10 * k + batch)
                idx = idx.cpu().numpy()
                assert idx.shape == (batch,) and idx.min() >= 0 and idx.max() < total
                assert (prio.cpu().numpy() == np.float32(prio0)).all()
                _same(_host(got), ref.gather(idx), f"push {k}, batch {batch}")
                if batch == 300:  # equal priorities: no stored transition is left out for long
                    assert len(np.unique(idx)) > total // 2
