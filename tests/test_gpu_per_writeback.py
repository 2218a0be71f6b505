"""rlhip_per_writeback_f32 (csrc/per_writeback.hip): the priority power (|td| + eps)^alpha and the sum-tree write-back in ONE launch.

1. Against the two shipped launches, rlhip_per_priority_f32(td -> prio_out) then rlhip_sumtree_update(tree, key, prio_out), on a clone of
   the same consistent tree: the whole tree (tree[0] == 0 included) and prio_out must be EQUAL bytes.
2. Independently on the host: from the tree before the call and the device's prio_out, the leaves written one after the other in numpy
   (the last duplicate wins), every parent rebuilt as the Float32 left + right -- equal to tree[1 : 2P].
The cases are the smallest shapes that reach each path of the dispatch in csrc/sumtree_update.h (SMALL_UPDATE_MAX = 64, one workgroup
up to logP = 13, 128 workgroups below 2048 keys and 256 from there, LCAP = 1024, bl = min(logP - 13, 7), the sparse levels above):
    a  13 leaves, n = 1 / 37 / 64             the one-wave path; not a power of two
    b  5000 leaves (P = 2^13), n = 65 / 130   the general kernel, one workgroup
    c  2^15 leaves, n = 130 / 2100            128 and 256 workgroups
    d  2^15 leaves, n = 1100, keys in 0..3    one workgroup's share exceeds LCAP: the election on the leaf tags
    e  2^20 - 5 leaves, n = 130 / 2100        128-leaf block recompute (bl = 7)
    f  2^20 + 1 leaves, n = 2100              P = 2^21: the sparse-level loop above the blocks
Every case but n = 1 holds a duplicate key whose occurrences carry different |td| (asserted on the host before the launch)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

EPS = 1e-6
_BASE = {}


def _call(name, *args):
    from rlhip._lib import call
    from rlhip.ops import stream_ptr

    call(name, *args, stream_ptr())


def _base_tree(n_leaves):
    """a consistent tree with every leaf set: rlhip_sumtree_fill_range plus one random rlhip_sumtree_update.  Built once per size."""
    import rlhip
    from rlhip.ops import ptr

    if n_leaves not in _BASE:
        nodes = int(rlhip._lib.lib.rlhip_sumtree_nodes(n_leaves))
        tree = torch.zeros(nodes, dtype=torch.float32, device="cuda")
        _call("rlhip_sumtree_fill_range", ptr(tree), n_leaves, 0, n_leaves, 0.75)
        rng = np.random.default_rng(n_leaves)
        m = min(n_leaves, 3000)
        k = torch.as_tensor(rng.integers(0, n_leaves, m), device="cuda")
        p = torch.as_tensor((rng.random(m) ** 0.6).astype(np.float32), device="cuda")
        _call("rlhip_sumtree_update", ptr(tree), n_leaves, ptr(k), ptr(p), m)
        torch.cuda.synchronize()
        _BASE[n_leaves] = tree
    return _BASE[n_leaves]


def _inputs(n_leaves, n, key_hi, seed):
    """keys drawn with replacement from 0 .. key_hi - 1, td seeded normal with exact zeros and negatives; for n > 1 the first and the
    last item share a key and differ in |td|"""
    rng = np.random.default_rng(seed)
    keys = rng.integers(0, key_hi, n).astype(np.int64)
    td = rng.standard_normal(n).astype(np.float32)
    td[2::7] = 0.0
    if n > 1:
        keys[-1] = keys[0]
        td[0], td[-1] = 0.5, -1.25
        assert (td == 0).any() or n < 3
        assert (td < 0).any()
        order = {}
        for i, k in enumerate(keys.tolist()):
            order.setdefault(k, []).append(i)
        assert any(len(v) > 1 and len({abs(float(td[i])) for i in v}) > 1 for v in order.values()), "no observable duplicate"
    return keys, td


def _two_launches(tree, n_leaves, key, td, alpha):
    from rlhip.ops import ptr

    out = torch.full_like(td, -1.0)
    _call("rlhip_per_priority_f32", ptr(td), td.numel(), EPS, alpha, ptr(out))
    _call("rlhip_sumtree_update", ptr(tree), n_leaves, ptr(key), ptr(out), key.numel())
    return out


def _one_launch(tree, n_leaves, key, td, alpha):
    from rlhip.ops import ptr

    out = torch.full_like(td, -1.0)
    _call("rlhip_per_writeback_f32", ptr(tree), n_leaves, ptr(key), ptr(td), key.numel(), EPS, alpha, ptr(out))
    return out


def _host_tree(before, n_leaves, keys, prio):
    """the sequential reference: leaves one after the other, then every parent as the Float32 left + right"""
    t = before.copy()
    P = t.size // 2
    for k, p in zip(keys.tolist(), prio.tolist()):
        if 0 <= k < n_leaves:
            t[P + k] = np.float32(p)
    size = P // 2
    while size >= 1:
        nodes = np.arange(size, 2 * size)
        t[nodes] = t[2 * nodes] + t[2 * nodes + 1]
        size //= 2
    return t


def _check(n_leaves, keys, td, alpha):
    base = _base_tree(n_leaves)
    before = base.cpu().numpy()
    k, t = torch.as_tensor(keys, device="cuda"), torch.as_tensor(td, device="cuda")
    ref_tree, got_tree = base.clone(), base.clone()
    ref_out = _two_launches(ref_tree, n_leaves, k, t, alpha)
    got_out = _one_launch(got_tree, n_leaves, k, t, alpha)
    torch.cuda.synchronize()
    assert torch.equal(t.cpu(), torch.as_tensor(td)), "td was written"
    assert torch.equal(got_out, ref_out), "prio_out differs from rlhip_per_priority_f32"
    assert float(got_tree[0]) == 0.0 and float(ref_tree[0]) == 0.0
    bad = (got_tree != ref_tree).nonzero().flatten().tolist()
    assert torch.equal(got_tree, ref_tree), f"nodes {bad[:8]} differ from the two launches"
    host = _host_tree(before, n_leaves, keys, got_out.cpu().numpy())
    got = got_tree.cpu().numpy()
    assert host.dtype == np.float32 and np.array_equal(got[1:], host[1:]), "the tree is not the sequential write-back's"
    assert torch.equal(base.cpu(), torch.as_tensor(before)), "the shared base tree was written"
    return got_out.cpu().numpy(), got


CASES = [("a", 13, n, 13) for n in (1, 37, 64)] + [("b", 5000, n, 5000) for n in (65, 130)] + \
        [("c", 1 << 15, n, 1 << 15) for n in (130, 2100)] + [("d", 1 << 15, 1100, 4)] + \
        [("e", (1 << 20) - 5, n, (1 << 20) - 5) for n in (130, 2100)] + [("f", (1 << 20) + 1, 2100, (1 << 20) + 1)]


@pytest.mark.parametrize("alpha", [0.6, 1.0])
@pytest.mark.parametrize("case,n_leaves,n,key_hi", CASES)
def test_one_launch_equals_power_then_update_byte_for_byte(case, n_leaves, n, key_hi, alpha):
    keys, td = _inputs(n_leaves, n, key_hi, seed=n_leaves * 7 + n)
    out, _ = _check(n_leaves, keys, td, alpha)
    x = np.abs(td) + np.float32(EPS)
    want = x if alpha == 1.0 else np.power(x.astype(np.float64), np.float64(np.float32(alpha))).astype(np.float32)
    # a sanity bound on the value itself (the bits are pinned against rlhip_per_priority_f32 above): both sides round a Float64 power
    # once to Float32, and two Float64 pow implementations may differ in their last bit, so the results are at most one Float32 ulp
    # apart -- 2^-23 = 1.2e-7 relative
    np.testing.assert_allclose(out, want, rtol=1.2e-7, atol=0)


@pytest.mark.parametrize("n_leaves,n", [(13, 37), (5000, 130), (1 << 15, 2100)])
def test_out_of_range_keys_are_not_written_and_still_get_their_value(n_leaves, n):
    keys, td = _inputs(n_leaves, n, n_leaves, seed=n)
    keys[3], keys[5] = -1, n_leaves
    td[3], td[5] = 2.0, -3.0
    out, got = _check(n_leaves, keys, td, 0.6)
    np.testing.assert_allclose(out[[3, 5]], np.power(np.float64([2.0, 3.0]) + EPS, np.float64(np.float32(0.6))), rtol=2.4e-7)  # (+ eps's rounding)
    assert (out > 0).all()
    P = got.size // 2
    before = _base_tree(n_leaves).cpu().numpy()
    if n_leaves < P:  # the slot past the last leaf stays what it was
        assert got[P + n_leaves] == before[P + n_leaves]


def test_overlapping_prio_out_and_td_is_refused_before_any_launch():
    from rlhip._lib import RLHipArgumentError
    from rlhip.ops import ptr

    n_leaves, n = 5000, 130
    keys, td = _inputs(n_leaves, n, n_leaves, seed=1)
    tree = _base_tree(n_leaves).clone()
    k = torch.as_tensor(keys, device="cuda")
    buf = torch.zeros(2 * n, dtype=torch.float32, device="cuda")
    buf[:n] = torch.as_tensor(td)
    kept = buf.clone()
    for out in (buf[:n], buf[n - 1:2 * n - 1], buf[1:n + 1]):
        with pytest.raises(RLHipArgumentError, match="overlap"):
            _call("rlhip_per_writeback_f32", ptr(tree), n_leaves, ptr(k), ptr(buf[:n]), n, EPS, 0.6, ptr(out))
    with pytest.raises(RLHipArgumentError):
        _call("rlhip_per_writeback_f32", ptr(tree), n_leaves, ptr(k), ptr(buf[:n]), n, EPS, 0.6, None)
    # adjacent, not overlapping, is fine; n == 0 launches nothing
    _call("rlhip_per_writeback_f32", ptr(tree), n_leaves, ptr(k), ptr(buf[:n]), 0, EPS, 0.6, None)
    torch.cuda.synchronize()
    assert torch.equal(buf, kept) and torch.equal(tree, _base_tree(n_leaves))
    _call("rlhip_per_writeback_f32", ptr(tree), n_leaves, ptr(k), ptr(buf[:n]), n, EPS, 0.6, ptr(buf[n:]))
    torch.cuda.synchronize()
    assert torch.equal(buf[:n], kept[:n]) and float(buf[n:].min()) > 0
