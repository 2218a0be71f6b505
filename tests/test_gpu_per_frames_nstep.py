"""rlhip_ring_push_priority_nstep_frames, rlhip_ring_sample_gather_nstep_prioritized and rlhip_ring_sample_gather_stacked_nstep_prioritized
(csrc/per_nstep.hip, csrc/per_frames_nstep.hip) on the device, byte for byte against the two launches they replace AND against the
model of tests/per_frames_nstep_ref.py (list model of the ring, oracle.SumTree on leaves stated on the same lists).

Every ring is filled through the push ABI in step with the model, to both fill states of the n-step gather tests (not full; wrapped);
every output is poisoned with 0xA5 first.  Per (case, fill state) the trees of per_frames_nstep_ref.trees -- masked for n_step in
{1, 2, 3, capacity} by the new push after every transition (the device tree equals the model's bit for bit), each masked tree again
after a write-back with zeros among the values, and the unmasked tree gathered with n_step in {2, 3, capacity, 32} -- and per tree the
draws of per_frames_nstep_ref.draws: batch 1, 64, 257 (301 with 300 envs), draw_ctr 0 and 2^32 - 1, gamma 0.99 and 0.  What those draws
hold (no ring-end cut on a masked tree; terminal cuts, full windows, ring-end cuts, zero-filled members ...) is asserted from the model
alone in tests/test_per_frames_nstep_reference.py.

Route per plain case: f32 6 x 5 and f32 5 x 300 sample_gather_small_nstep_kernel<float>; u8 1030 x 1 sample_gather_small_nstep_kernel<uint8_t>;
u8 1024 x 1 and u8 7056 x 1 sample_gather_frames_nstep_kernel (wave 0's four-levels-per-trip descent over 3 levels); stacked cases
sample_gather_stacked_nstep_kernel (4 levels: one whole trip).  The depth test adds 17 levels (four trips and one level) and 6; the
stacked call's batch rule (fused up to 1536, its two launches beyond) is run on both sides."""
import ctypes as C

import numpy as np
import pytest
import torch

import per_frames_nstep_ref as P
import ring_nstep_ref as R
from ring_ref import case_id
from test_gpu_ring_nstep import _dev, _gather_nstep, _poisoned, _same, _sink

pytestmark = pytest.mark.gpu

DRAWN = ("idx", "key", "priority")


def _traces(dtype, od, n_env, cap, n_step):
    import rlhip

    return rlhip.CircularPrioritizedFrameTraces(capacity=cap, n_env=n_env, obs_dim=od, dtype=torch.uint8 if dtype == "u8" else torch.float32,
                                                default_priority=P.PRIORITY, n_step=n_step)


def _sink_for(dtype, od, n_env, cap):
    def make(n):
        tr = _traces(dtype, od, n_env, cap, n)
        return _sink(tr), tr
    return make


def _fused(tr, batch, n_step, gamma, ctr, n_stack=None, null=False):
    """the fused C ABI call on poisoned outputs -> ((idx, key, prio), (s, a, ret, t, sn, n_used)) as numpy; null: key / prio / n_used NULL"""
    from rlhip._lib import call
    from rlhip.ops import ptr, stream_ptr

    shape = (batch, n_stack, tr.obs_dim) if n_stack else ((batch, tr.obs_dim) if tr.frame_major else (tr.obs_dim, batch))
    s, a, ret, t, sn, nu = out = _poisoned(tr, batch, shape)
    dev = tr.state.device
    idx, key = (torch.full((batch,), -0x5A5A5A5A, dtype=torch.int64, device=dev) for _ in range(2))
    prio = torch.full((batch,), float("nan"), dtype=torch.float32, device=dev)
    opt = (lambda x: None) if null else ptr
    head = (C.byref(tr.rb), ptr(tr.priorities), batch) + ((n_stack,) if n_stack else ())
    call("rlhip_ring_sample_gather_stacked_nstep_prioritized" if n_stack else "rlhip_ring_sample_gather_nstep_prioritized", *head, n_step, gamma,
         P.SEED, ctr, ptr(idx), opt(key), opt(prio), ptr(s), ptr(a), ptr(ret), ptr(t), ptr(sn), opt(nu), stream_ptr())
    return tuple(x.cpu().numpy() for x in (idx, key, prio)), tuple(x.cpu().numpy() for x in out)


def _same_draw(got, want, where):
    for name, g, w in zip(DRAWN, got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, (where, name)
        assert np.array_equal(g.view(np.uint8), w.view(np.uint8)), f"{where}: {name} differs, first at {int(np.argmax(g != w))}: {g[g != w][:4]} != {w[g != w][:4]}"


def _check_tree(tr, ref, n_gather, n_stack, where, with_model=True):
    """every draw of the plan on one tree: fused == the two launches == the model"""
    fm = tr.frame_major and not n_stack
    for i, (batch, gamma, ctr) in enumerate(P.draws(tr.n_env)):
        at = f"{where}, n_step {n_gather}, batch {batch}, gamma {gamma}, draw_ctr {ctr}"
        drawn, got = _fused(tr, batch, n_gather, gamma, ctr, n_stack)
        two = tr.sample_prioritized(batch, P.SEED, ctr)
        _same_draw(drawn, tuple(x.cpu().numpy() for x in two), at + " (against rlhip_ring_sample_prioritized)")
        _same(got, _gather_nstep(tr, two[0], n_gather, gamma, n_stack), at + " (against the n-step gather)")
        if with_model:
            idx, key, prio = ref.draw(batch, P.SEED, ctr)
            _same_draw(drawn, (idx, key, prio), at + " (against the oracle's draw)")
            want = ref.gather_stacked_nstep(idx, n_stack, n_gather, gamma) if n_stack else ref.gather_nstep(idx, n_gather, gamma)
            _same(got, R.frame_major6(want) if fm else want, at + " (against the list model)")
        else:
            assert (got[5] == 1).all(), at  # a leaf outside the logical range: a one-step window
        if i == 1:  # NULL key_out / prio_out / n_used change nothing else
            drawn0, got0 = _fused(tr, batch, n_gather, gamma, ctr, n_stack, null=True)
            _same_draw(drawn0[:1], drawn[:1], at + " (NULL outputs)")
            _same(got0[:5], got[:5], at + " (NULL outputs)")
            assert (drawn0[1] == -0x5A5A5A5A).all() and np.isnan(drawn0[2]).all() and (got0[5].view(np.uint32) == 0xA5A5A5A5).all()


def _walk(make_ref, cap, sink_for, n_stack=None):
    seen = []
    for name, ref, gather_ns, tr, pending in P.trees(make_ref, cap, sink_for):
        assert len(tr) == len(ref)
        if pending is not None:  # the write-back the model has already applied
            tr.set_priority_(_dev(pending[0]), _dev(pending[1]))
        tree = tr.priorities.cpu().numpy()
        assert np.array_equal(tree.view(np.uint32), ref.st.tree.view(np.uint32)), f"{name}: the device tree is not the model's"
        if name.startswith("empty"):  # no mass: the draw ends on the clamp leaf, outside the logical range -- still the two launches'
            _check_tree(tr, ref, int(name.split(" ")[1]), n_stack, name, with_model=False)
        for n in gather_ns:
            _check_tree(tr, ref, n, n_stack, name)
        seen.append(name.split(" ")[0])
    assert {"masked", "written", "unmasked"} <= set(seen)


PLAIN = [(c, p) for c in P.PLAIN_CASES for p in R.plain_pushes(c[3])]


@pytest.mark.parametrize("case,pushes", PLAIN, ids=[f"{case_id(c)}-{p}pushes" for c, p in PLAIN])
def test_draw_and_gather_equal_the_two_launches_and_the_model(case, pushes):
    dtype, od, n_env, cap, want_frame_major = case
    probe = _traces(dtype, od, n_env, cap, 1)
    assert probe.frame_major == want_frame_major and not probe.records_layout  # the case still takes the kernel the table names
    _walk(lambda n, sink: P.plain_ref(case, pushes, n, sink), cap, _sink_for(dtype, od, n_env, cap))


STACKED = [(c, p, k) for c in P.STACKED_CASES for p in R.STACKED_PUSHES for k in P.STACKS]


@pytest.mark.parametrize("case,pushes,n_stack", STACKED, ids=[f"{c[0]}-{c[1]}-cap{c[2]}-{p}pushes-stack{k}" for c, p, k in STACKED])
def test_stacked_draw_and_gather_equal_the_two_launches_and_the_model(case, pushes, n_stack):
    dtype, od, cap = case
    _walk(lambda n, sink: P.stacked_ref(case, pushes, n, sink), cap, _sink_for(dtype, od, 1, cap), n_stack)


@pytest.mark.parametrize("batch", [1536, 1537])
def test_stacked_call_gives_the_same_bytes_on_both_sides_of_its_batch_rule(batch):
    """rlhip_ring_sample_gather_stacked_nstep_prioritized launches its fused kernel up to batch 1536 (STACKED_FUSED_MAX_BATCH,
    csrc/per_frames_nstep.hip) and the two launches it stands for beyond: the largest fused batch and the smallest one that is not"""
    case, n, n_stack = ("u8", 48, 12), 3, 4
    tr = _traces("u8", 48, 1, 12, n)
    ref = P.stacked_ref(case, 27, n, _sink(tr))
    drawn, got = _fused(tr, batch, n, 0.99, 5, n_stack)
    two = tr.sample_prioritized(batch, P.SEED, 5)
    _same_draw(drawn, tuple(x.cpu().numpy() for x in two), "against rlhip_ring_sample_prioritized")
    _same(got, _gather_nstep(tr, two[0], n, 0.99, n_stack), "against the n-step gather")
    idx, key, prio = ref.draw(batch, P.SEED, 5)
    _same_draw(drawn, (idx, key, prio), "against the oracle's draw")
    _same(got, ref.gather_stacked_nstep(idx, n_stack, n, 0.99), "against the list model")
    drawn0, got0 = _fused(tr, batch, n, 0.99, 5, n_stack, null=True)
    _same_draw(drawn0[:1], drawn[:1], "NULL outputs")
    _same(got0[:5], got[:5], "NULL outputs")
    assert (drawn0[1] == -0x5A5A5A5A).all() and np.isnan(drawn0[2]).all() and (got0[5].view(np.uint32) == 0xA5A5A5A5).all()


@pytest.mark.parametrize("od,cap,levels,n_stack", [(1024, 70_000, 17, None), (1024, 70_000, 17, 4), (7, 70_000, 17, None), (1024, 40, 6, None)],
                         ids=["frame-major-17-levels", "stacked-17-levels", "small-17-levels", "frame-major-6-levels"])
def test_descent_depth_that_is_no_multiple_of_its_stride(od, cap, levels, n_stack):
    """about 40 pushes into a ring of 70 000 (and of 40): mass only on the stored leaves, so the descent runs its full depth through a
    nearly empty tree -- 17 levels are four trips of four and one of one, 6 levels one of four and one of two"""
    tr = _traces("u8", od, 1, cap, 3)
    assert tr.frame_major == (od >= 1024) and tr.priorities.numel() == 2 ** (levels + 1)
    ref = P.PrioritizedFramesRef(cap, 1, od, np.uint8, 3)
    R.fill(ref, np.random.default_rng([od, cap, 41]), "u8", 41, 0.2, _sink(tr))
    assert np.array_equal(tr.priorities.cpu().numpy().view(np.uint32), ref.st.tree.view(np.uint32))
    _check_tree(tr, ref, 3, n_stack, "masked 3")
    key, prio = P.write_back(ref, cap)
    tr.set_priority_(_dev(key), _dev(prio))
    _check_tree(tr, ref, 3, n_stack, "written 3")


@pytest.mark.parametrize("case,n_stack", [(("u8", 7056, 1, 40), 4), (("u8", 7056, 1, 40), None), (("f32", 6, 5, 9), None)],
                         ids=["stacked", "frame-major", "small"])
def test_sampler_is_one_fused_call_equal_to_the_two_call_path(case, n_stack):
    import rlhip as rl

    dtype, od, n_env, cap = case
    n, batch, gamma = 3, 64, 0.99
    tr = _traces(dtype, od, n_env, cap, n)
    ref = P.PrioritizedFramesRef(cap, n_env, od, np.uint8 if dtype == "u8" else np.float32, n)
    R.fill(ref, np.random.default_rng(5), dtype, cap + 4, 0.2, _sink(tr))
    smp, twin = rl.NStepBatchSampler(n, gamma, batch, seed=7, n_stack=n_stack), rl.NStepBatchSampler(n, gamma, batch, seed=7, n_stack=n_stack)
    zeroed = set()  # keys whose priority a write-back below has set to 0
    for draw in range(3):
        got = smp.sample(tr)
        assert smp.draw_ctr == draw + 1
        # the two-call path, as NStepBatchSampler runs it over traces without the fused form
        idx = twin.sample_indices(tr, draw)
        s, a, ret, t, sn, nu = tr.gather_stacked_nstep(idx, n_stack, n, gamma) if n_stack else tr.gather_nstep(idx, n, gamma)
        assert set(got) == {"state", "action", "reward", "terminal", "next_state", "key", "priority", "n_steps"}
        assert torch.equal(got["key"], twin.key) and torch.equal(got["priority"].view(torch.int32), twin.priority.view(torch.int32))
        assert torch.equal(got["state"], s) and torch.equal(got["next_state"], sn) and torch.equal(got["action"], a + 1)
        assert torch.equal(got["reward"].view(torch.int32), ret.view(torch.int32))
        assert got["terminal"].dtype == torch.bool and torch.equal(got["terminal"].view(torch.uint8), t)
        assert torch.equal(got["n_steps"], nu) and got["n_steps"].dtype == torch.int32
        # ... and the model: the same keys, every window complete
        midx, mkey, mprio = ref.draw(batch, 7, draw)
        assert np.array_equal(got["key"].cpu().numpy(), mkey) and np.array_equal(got["priority"].cpu().numpy().view(np.uint32), mprio.view(np.uint32))
        assert np.array_equal(idx.cpu().numpy(), midx) and set(mkey.tolist()) <= ref.complete_starts()
        want = ref.gather_stacked_nstep(midx, n_stack, n, gamma) if n_stack else ref.gather_nstep(midx, n, gamma)
        _same(tuple(x.cpu().numpy() for x in (s, a, ret, t, sn, nu)), R.frame_major6(want) if tr.frame_major and not n_stack else want, f"draw {draw}")
        # priorities written back under the returned keys change the next draw as the model says
        newp = (0.25 + 4 * np.random.default_rng(draw).random(batch)).astype(np.float32)
        assert (mkey != mkey[0]).any()   # other keys keep the tree's mass ...
        newp[mkey == mkey[0]] = 0.0      # ... when the first drawn key leaves the distribution: no later draw returns it
        assert not set(mkey.tolist()) & zeroed
        zeroed.add(int(mkey[0]))
        tr.set_priority_(got["key"], _dev(newp))
        ref.st.update(mkey, newp)
        assert np.array_equal(tr.priorities.cpu().numpy().view(np.uint32), ref.st.tree.view(np.uint32))
    with pytest.raises(ValueError, match="n_step"):
        rl.NStepBatchSampler(2, gamma, batch, n_stack=n_stack).sample(tr)
