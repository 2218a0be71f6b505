"""The optimiser contract of every learner -- clip_by_global_norm!, Optimisers.Adam with the running powers `bt = bt .* b`, Polyak --
bit for bit against the oracle (oracle/rlo_optim.c) on every dispatch path of csrc/optim.hip, and on the learner tails whose
"equals the unfused protocol" chain does not end in rlhip_clip_adam_f32.

What is compared, and how:
  p, m, v, the clipped gradient the kernels write back and beta_pow: np.array_equal (NaN positions included) with the oracle
  fed the same inputs.  beta_pow is the Float32 running product, compared with the host's Float32 running product.
  gn: both sides sum in Float64, in different orders -> within one Float32 ulp of the oracle's; the expected clip factor is
  then derived from the GPU's gn, in the kernels' order (g * grad_scale) * scale, so every other output stays bit-exact.
  An independent Float64 evaluation of the Optimisers.jl formula bounds m and v by 4 * 2^-24 relative and the update by
  12 * 2^-24 (a formula error shared by the oracle and the kernels): p = 0 before the first call makes p_after = -update exact,
  and every gradient of an element keeps the sign of its entering m, so that no sum cancels.  The bars are the rounding counts
  (unit roundoff 2^-24 per Float32 operation): m 2, v 3, the update 10.5 in the worst case (bias corrections, sqrt, + eps,
  the division and * lr on top of m and v) -- measured up to 4.2.
Inputs: gradient magnitudes 1e-9 .. 1e3 with exact zeros, non-zero m and v, three starting states of beta_pow (fresh, b^50,
b^1000), three calls enqueued back to back without a host sync (the last-out / separate-launch order of `bt .* b` across
launches).  The sizes come from the host code of csrc/optim.hip (tests/test_optim_dispatch_thresholds.py pins them).
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import oracle  # noqa: E402  (the checker)

LR, B1, B2, EPS = 3e-3, 0.9, 0.999, 1e-8
U = 2.0 ** -24
POOL = 1_000_003  # inputs beyond this many elements repeat with a prime period (no alignment with any launch geometry)
BIG = 1 << 22     # from here on the Float64 check reads a strided subsample
STATES = {"fresh": 1, "b^50": 50, "b^1000": 1000}  # t of the first call (beta_pow = Float32 running product b^t)


@pytest.fixture(scope="module")
def ops():
    import rlhip
    from rlhip import _lib, ops

    n = _lib.i32(0)
    _lib.call("rlhip_device_count", _lib.C.byref(n))
    assert n.value >= 1 and rlhip is not None
    return ops


@pytest.fixture(autouse=True)
def _free_device_memory():
    yield
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def host(t):
    return t.detach().cpu().numpy()


def running_pow(t):
    """(b1^t, b2^t) as Optimisers.Adam carries them: the Float32 product of t factors"""
    b = np.array([B1, B2], np.float32)
    bt = b.copy()
    for _ in range(t - 1):
        bt = bt * b
    return bt


def dview(a, mis):
    """a device copy of the host array; mis: a view one float into its allocation (4-byte aligned, not 16)"""
    n = a.size
    base = torch.empty(n + 4, dtype=torch.float32, device="cuda")
    v = base[1:1 + n] if mis else base[:n]
    v.copy_(torch.from_numpy(np.ascontiguousarray(a)))
    return v


def _pool(rng, n, f):
    return f(rng, n) if n <= POOL else np.resize(f(rng, POOL), n)


def _mag(rng, n, lo, hi):
    return np.power(10.0, rng.uniform(lo, hi, n)).astype(np.float32)


class Inputs:
    """one element-wise sign pattern s; every gradient is s * |g| (exact zeros mixed in), m on entry s * |m|, v on entry > 0"""

    def __init__(self, n, ncalls, seed):
        rng = np.random.default_rng(seed)
        self.s = _pool(rng, n, lambda r, k: np.where(r.random(k) < 0.5, -1.0, 1.0).astype(np.float32))

        def grad(r, k):
            g = _mag(r, k, -9, 3)
            g[r.random(k) < 1 / 16] = 0.0
            return g

        self.g = [self.s * _pool(rng, n, grad) for _ in range(ncalls)]
        self.m = self.s * _pool(rng, n, lambda r, k: _mag(r, k, -6, 1))
        self.v = _pool(rng, n, lambda r, k: _mag(r, k, -12, 4))
        self.p = np.zeros(n, np.float32)


def f64_check(g_applied, m0, v0, bt, m1, v1, update, sub):
    """Optimisers.Adam in Float64 from the same Float32 state: m, v within 4 * 2^-24 relative, the update within 12 * 2^-24"""
    g, m0, v0 = (np.asarray(x[sub], np.float64) for x in (g_applied, m0, v0))
    b1, b2 = float(np.float32(B1)), float(np.float32(B2))
    c1, c2 = 1.0 - float(bt[0]), 1.0 - float(bt[1])
    m = b1 * m0 + (1.0 - b1) * g
    v = b2 * v0 + (1.0 - b2) * (g * g)
    u = m / c1 / (np.sqrt(v / c2) + float(np.float32(EPS))) * float(np.float32(LR))
    for name, got, ref, bar in (("m", m1, m, 4), ("v", v1, v, 4), ("update", update, u, 12)):
        got = np.asarray(got[sub], np.float64)
        bad = np.abs(got - ref) > bar * U * np.abs(ref)
        assert not bad.any(), f"{name}: {int(bad.sum())} elements beyond {bar} * 2^-24 of Float64, e.g. {got[bad][:3]} vs {ref[bad][:3]}"


def expected_clip(g, grad_scale, clip_norm, gn_gpu):
    """the clipped gradient of the fused kernels, from the GPU's gn: (g * grad_scale) * scale, untouched when scale == 1"""
    gs = g * np.float32(grad_scale)
    gn = np.float32(gn_gpu)
    if np.float32(clip_norm) > 0 and np.float32(clip_norm) <= gn:
        scale = np.float32(clip_norm) / max(np.float32(clip_norm), gn)
        if scale != np.float32(1.0):
            with np.errstate(invalid="ignore"):  # +-Inf * 0 (gn = Inf): NaN, as on the GPU
                return gs * scale
    return gs


def assert_gn(gn_gpu, g_scaled):
    o = oracle.clip_by_global_norm(g_scaled.copy(), 1e30)  # the oracle's Float64 norm (clip far above: g left alone)
    if not np.isfinite(o):
        assert np.isnan(gn_gpu) if np.isnan(o) else gn_gpu == o, (gn_gpu, o)
        return
    assert abs(np.float32(gn_gpu) - np.float32(o)) <= np.spacing(np.float32(o)), (gn_gpu, o)


def eq(a, b, what):
    assert np.array_equal(a, b, equal_nan=True), f"{what}: {int(np.sum(~((a == b) | (np.isnan(a) & np.isnan(b)))))} elements differ"


class Streams:
    """streams made by the library (not torch's pool, which hands out at most 32 distinct ones per priority)"""

    def __init__(self):
        from rlhip import _lib

        self._lib, self.handles = _lib, []

    def new(self):
        h = C.c_void_p()
        self._lib.call("rlhip_stream_create", C.byref(h))
        self.handles.append(h)
        return torch.cuda.ExternalStream(h.value)

    def close(self):
        torch.cuda.synchronize()
        for h in self.handles:
            self._lib.call("rlhip_stream_destroy", h)


def beyond_the_slots(ops, streams):
    """a stream without a departure-counter slot: 64 slots per process and device, never recycled -- 65 new streams that each
    ask for one leave at least the last without"""
    p, g, m, v = (torch.ones(1, device="cuda") for _ in range(4))
    bp = torch.tensor([B1, B2], device="cuda")
    torch.cuda.synchronize()
    for _ in range(65):  # (every tensor allocated outside the streams: the caching allocator keeps no block of theirs)
        s = streams.new()
        with torch.cuda.stream(s):
            ops.adam_(p, g, m, v, bp)
        s.synchronize()
    return s


# ------------------------------------------------------------------------------------------------------------ rlhip_adam_f32
ADAM_CASES = [(0, False), (1, False), (65535, False),                          # adam_kernel, folded
              (65536, False), (65539, False), (1 << 22, False), (1 << 23, False),  # adam_vec4_kernel, folded; n % 4 tail
              ((1 << 23) + 1, False), (1 << 26, False),                        # adam_vec4_kernel + beta_pow_advance_kernel
              (65537, True), ((1 << 23) + 5, True)]                           # adam_kernel grid-stride (folded / two-launch)


def _adam_run(ops, n, mis, state, seed, stream=None):
    K = 3
    x = Inputs(n, K, seed)
    t0 = STATES[state]
    p, m, v = dview(x.p, mis), dview(x.m, mis), dview(x.v, mis)
    gd = [dview(g, mis) for g in x.g]
    bp = torch.tensor(running_pow(t0), device="cuda")
    p1 = (torch.empty_like(p), torch.empty_like(m), torch.empty_like(v))
    buf = torch.zeros(4, device="cuda")  # n = 0: a zero-size tensor has no data pointer -- the C ABI with a valid one
    torch.cuda.synchronize()
    with torch.cuda.stream(stream or torch.cuda.current_stream()):
        for k in range(K):  # back to back: no host sync between the calls
            if n == 0:
                ops.call("rlhip_adam_f32", ops.ptr(buf), ops.ptr(buf), ops.ptr(buf), ops.ptr(buf), ops.ptr(bp), 0, LR, B1, B2, EPS,
                         ops.stream_ptr())
            else:
                ops.adam_(p, gd[k], m, v, bp, LR, B1, B2, EPS)
            if k == 0:
                for dst, src in zip(p1, (p, m, v)):
                    dst.copy_(src)
    torch.cuda.synchronize()
    sub = slice(None, None, 97) if n > BIG else slice(None)
    po, mo, vo = x.p.copy(), x.m.copy(), x.v.copy()
    for k in range(K):
        oracle.adam(po, x.g[k], mo, vo, LR, B1, B2, EPS, t0 + k)
        if k == 0:
            for a, b, name in zip(p1, (po, mo, vo), "pmv"):
                eq(host(a), b, f"{name} after the first call")
    eq(host(p), po, "p")
    eq(host(m), mo, "m")
    eq(host(v), vo, "v")
    assert np.array_equal(host(bp), running_pow(t0 + K)), (host(bp), running_pow(t0 + K))
    # p = 0 before the first call: p_after = -update exactly
    f64_check(x.g[0], x.m, x.v, running_pow(t0), host(p1[1]), host(p1[2]), -host(p1[0]), sub)


@pytest.mark.parametrize("n,mis", ADAM_CASES)
def test_adam_bit_exact_vs_oracle(ops, n, mis):
    states = ["b^50"] if n >= 1 << 26 else list(STATES)
    for i, state in enumerate(states):
        _adam_run(ops, n, mis, state, seed=n + i)
        torch.cuda.empty_cache()


def test_adam_on_a_stream_without_a_departure_slot(ops):
    """a 65th distinct stream: `bt = bt .* b` as its own launch behind the update, below and above the streaming threshold"""
    streams = Streams()
    try:
        s = beyond_the_slots(ops, streams)
        for n in (4099, 65539):
            _adam_run(ops, n, False, "b^50", seed=7, stream=s)
    finally:
        streams.close()


# ------------------------------------------------------------------------------------------------------- rlhip_clip_adam_f32
# (grad_scale, clip) of the three back-to-back calls of a run; clip: a factor of the Float64 norm of g * grad_scale (away from the
# tie), "0" (disabled), "tie" (g = 3 e_0 + 4 e_(n-1), clip 5: gn == clip exactly, scale == 1, g untouched)
RUNS = [("fresh", [(0.5, "active"), (1.0, "inactive"), (1 / 3, "0")]),
        ("b^50", [(1.0, "tie"), (1 / 3, "active"), (1.0, "nan")]),
        ("b^1000", [(1.0, "active"), (0.5, "inf"), (0.5, "inactive")])]
CLIP_CASES = [(1, False), (4096, False), (4096, True),                # clip_adam_kernel<4>
              (4097, False), (4098, False), (4099, False), (8192, False),  # clip_adam_vec_kernel<2> (load4_guard tails)
              (8193, False), (12288, False),                           # clip_adam_vec_kernel<4>
              (4097, True), (12288, True),                             # clip_adam_kernel<16>
              (12289, False), (65536, False), ((1 << 20) + 3, False)]  # sumsq_scaled_partial_kernel + clip_adam_grid_kernel


def _clip_run(ops, n, mis, state, calls, seed, stream=None):
    x = Inputs(n, len(calls), seed)
    clips = []
    for k, (gs, mode) in enumerate(calls):
        g = x.g[k]
        if mode == "tie":
            g[:] = 0.0
            g[0], g[-1] = (3.0 * x.s[0], 4.0 * x.s[-1]) if n > 1 else (5.0 * x.s[0],) * 2
        elif mode in ("nan", "inf"):
            g[n // 2] = np.nan if mode == "nan" else -np.inf
            g[-1] = g[-1] if mode == "nan" or n == 1 else np.inf
        gn64 = float(np.sqrt(np.sum(np.square((g * np.float32(gs)).astype(np.float64)))))
        clips.append({"active": 0.37 * gn64, "inactive": 2.5 * gn64 + 1e-30, "0": 0.0, "tie": 5.0, "nan": 1.0,
                      "inf": 1.0}[mode])
    p, m, v = dview(x.p, mis), dview(x.m, mis), dview(x.v, mis)
    gd = [dview(g, mis) for g in x.g]
    bp = torch.tensor(running_pow(STATES[state]), device="cuda")
    gn = torch.zeros(len(calls), device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(stream or torch.cuda.current_stream()):
        for k, (gs, _) in enumerate(calls):
            ops.clip_adam_(p, gd[k], m, v, bp, gs, clips[k], LR, B1, B2, EPS, gn[k:k + 1])
    torch.cuda.synchronize()
    gn = host(gn)
    t0 = STATES[state]
    sub = slice(None, None, 97) if n > BIG else slice(None)
    po, mo, vo = x.p.copy(), x.m.copy(), x.v.copy()
    for k, (gs, mode) in enumerate(calls):
        assert_gn(gn[k], x.g[k] * np.float32(gs))
        gc = expected_clip(x.g[k], gs, clips[k], gn[k])
        if mode == "inactive":
            assert np.array_equal(gc, x.g[k] * np.float32(gs))
        if mode == "tie":
            assert gn[k] == 5.0 and np.array_equal(gc, x.g[k])
        eq(host(gd[k]), gc, f"clipped g of call {k} ({mode}, grad_scale {gs})")
        m0, v0 = mo.copy(), vo.copy()
        oracle.adam(po, gc, mo, vo, LR, B1, B2, EPS, t0 + k)
        if k == 0:
            first = (gc, m0, v0, po.copy(), mo.copy(), vo.copy(), gs, mode)
    eq(host(p), po, "p")
    eq(host(m), mo, "m")
    eq(host(v), vo, "v")
    assert np.array_equal(host(bp), running_pow(t0 + len(calls))), (host(bp), running_pow(t0 + len(calls)))
    # the first call in Float64 (its outputs are the oracle's, bit for bit: the final state above depends on them)
    gc, m0, v0, p1, m1, v1, gs, mode = first
    ref = x.g[0].astype(np.float64) * float(np.float32(gs))  # the clip: (g * grad_scale) * (clip / gn) -- three roundings
    if mode == "active" and np.float32(clips[0]) > 0:
        ref = ref * (float(np.float32(clips[0])) / float(gn[0]))
    assert np.all(np.abs(gc[sub] - ref[sub]) <= 3 * U * np.abs(ref[sub]))
    f64_check(gc, m0, v0, running_pow(t0), m1, v1, -p1, sub)


@pytest.mark.parametrize("n,mis", CLIP_CASES)
def test_clip_adam_bit_exact_vs_oracle(ops, n, mis):
    for i, (state, calls) in enumerate(RUNS):
        _clip_run(ops, n, mis, state, calls, seed=1000 + n + i)


def test_clip_adam_on_a_stream_without_a_departure_slot(ops):
    """the grid pair on a 65th distinct stream: no departure counter, `bt .* b` as its own launch, the shared partials block"""
    streams = Streams()
    try:
        s = beyond_the_slots(ops, streams)
        for n in (12289, 70001):
            _clip_run(ops, n, False, RUNS[0][0], RUNS[0][1], seed=n, stream=s)
    finally:
        streams.close()


# -------------------------------------------------------------------------------------------- rlhip_polyak_f32, rlhip_clip_by_global_norm_f32
@pytest.mark.parametrize("n,mis", [(1, False), (65535, False), (65536, False), (65539, False), (1 << 22, False), (1 << 26, False),
                                   ((1 << 20) + 1, True)])
def test_polyak_bit_exact_vs_oracle(ops, n, mis):
    rng = np.random.default_rng(n)
    dst = _pool(rng, n, lambda r, k: r.standard_normal(k, dtype=np.float32))
    srcs = [_pool(rng, n, lambda r, k: (r.standard_normal(k, dtype=np.float32) * 3)) for _ in range(3)]
    rhos = (0.0, 1.0, 0.995)
    d = dview(dst, mis)
    sd = [dview(s, mis) for s in srcs]
    for rho, s in zip(rhos, sd):  # back to back
        ops.polyak_(d, s, rho)
    torch.cuda.synchronize()
    o = dst.copy()
    for rho, s in zip(rhos, srcs):
        oracle.polyak(o, s, rho)
    eq(host(d), o, "polyak")


@pytest.mark.parametrize("n", [0, 1, 262144, 262145, 1 << 26])
def test_clip_by_global_norm_bit_exact_vs_oracle(ops, n):
    rng = np.random.default_rng(n + 5)
    g0 = _pool(rng, n, lambda r, k: (np.where(r.random(k) < 0.5, -1, 1) * _mag(r, k, -9, 3)).astype(np.float32))
    gn64 = float(np.sqrt(np.sum(np.square(g0.astype(np.float64)))))
    for clip in (0.37 * gn64 if n else 1.0, 2.5 * gn64 + 1.0):
        if n:
            d = dview(g0, False)
            gn = float(ops.clip_by_global_norm_(d, clip))
        else:  # (a zero-size tensor has no data pointer: the C ABI with a valid one and n = 0)
            buf, gnt = torch.full((4,), 7.0, device="cuda"), torch.full((1,), -1.0, device="cuda")
            ops.call("rlhip_clip_by_global_norm_f32", ops.ptr(buf), 0, clip, ops.ptr(gnt), ops.stream_ptr())
            gn, d = float(gnt), buf[:0]
            assert torch.equal(buf, torch.full((4,), 7.0, device="cuda"))
        assert_gn(gn, g0)
        # rlhip_clip_by_global_norm_f32 (basic.jl:23-26): no clip_norm > 0 guard, scale from the GPU's gn
        exp = g0.copy()
        if np.float32(clip) <= np.float32(gn):
            s = np.float32(clip) / max(np.float32(clip), np.float32(gn))
            if s != np.float32(1.0):
                exp = exp * s
        eq(host(d), exp, f"clip {clip}")
        if clip > gn64:
            assert np.array_equal(host(d), g0)
        else:
            o = g0.copy()
            ogn = oracle.clip_by_global_norm(o, clip)
            if np.float32(ogn) == np.float32(gn):
                eq(host(d), o, "oracle clip")
        del d
        torch.cuda.empty_cache()


# -------------------------------------------------------------------------------------------------------------- learner tails
def test_ppo_apply_pack_tail_vs_oracle(ops):
    """rlhip_ppo_apply_f32 of a two-layer policy (apply_pack_kernel: [grad_scale] -> clip -> Adam -> record refresh in one
    workgroup): the chain "update == grad + apply" of the PPO tests ends here, not in rlhip_clip_adam_f32"""
    import rlhip

    env = rlhip.CartPoleEnv(64, seed=1)
    pol = rlhip.PPOPolicy(env, update_freq=8, seed=1)
    n = pol.params.numel()
    assert pol.cfg.layers != 3 and n <= 16 * 1024  # the apply_pack_kernel route of rlhip_ppo_apply_f32
    lr, b1, b2, eps = (float(np.float32(getattr(pol.cfg, k))) for k in ("lr", "beta1", "beta2", "adam_eps"))
    x = Inputs(n, 3, 11)
    t0 = 50
    bt0 = np.array([np.float32(b1), np.float32(b2)], np.float32)
    bt = bt0.copy()
    for _ in range(t0 - 1):
        bt = bt * bt0
    pol.params.copy_(torch.from_numpy(x.p))
    pol.m.copy_(torch.from_numpy(x.m))
    pol.v.copy_(torch.from_numpy(x.v))
    pol.beta_pow.copy_(torch.from_numpy(bt))
    calls = [(0.5, 0.37), (1.0, 2.5), (1 / 3, 0.0)]
    clips = []
    gouts, gns = [], []
    for k, (gs, f) in enumerate(calls):
        gn64 = float(np.sqrt(np.sum(np.square((x.g[k] * np.float32(gs)).astype(np.float64)))))
        clips.append(f * gn64)
        pol.cfg.max_grad_norm = clips[-1]
        pol.grad.copy_(torch.from_numpy(x.g[k]))
        pol.apply_(gs)
        gouts.append(pol.grad.clone())
        gns.append(pol.gn.clone())
    torch.cuda.synchronize()
    po, mo, vo = x.p.copy(), x.m.copy(), x.v.copy()
    for k, (gs, _) in enumerate(calls):
        gn = float(host(gns[k])[0])
        assert_gn(gn, x.g[k] * np.float32(gs))
        gc = expected_clip(x.g[k], gs, clips[k], gn)
        eq(host(gouts[k]), gc, f"clipped g of call {k}")
        oracle.adam(po, gc, mo, vo, lr, b1, b2, eps, t0 + k)
    eq(host(pol.params), po, "p")
    eq(host(pol.m), mo, "m")
    eq(host(pol.v), vo, "v")
    b = bt
    for _ in range(len(calls)):
        b = b * bt0
    assert np.array_equal(host(pol.beta_pow), b)


def test_ppo3w_adam_pack_tail_vs_oracle(ops):
    """ppo3w_adam_pack_kernel (the 256-wide tail: norm from the partial sums, clip, Adam, bf16 re-pack, beta powers by the last
    workgroup out), reached through rlhip_dqn3_update_f32 at hidden 256; the raw gradient of each step from rlhip_dqn3_grad_f32
    on the same state"""
    import rlhip
    from rlhip import dqn

    ns, na, n, h, batch = 4, 2, 64, 256, 512
    tr = rlhip.CircularArraySARTSTraces(capacity=32, n_env=n, obs_dim=ns)
    tr.records.normal_()
    tr.action.random_(0, na)
    tr.reward.normal_()
    tr.terminal.copy_((torch.rand(tr.terminal.shape, device="cuda") < 0.1).to(torch.uint8))
    tr.rb.len_sa, tr.rb.len_rt = 33, 32
    tp = dqn.mlp3_init(ns, h, na, 2, 1)
    tpk = dqn.mlp3_pack(tp, ns, h, na)
    p = dqn.mlp3_init(ns, h, na, 1, 0)
    pk = dqn.mlp3_pack(p, ns, h, na)
    npar = p.numel()
    x = Inputs(npar, 1, 12)
    m, v = torch.from_numpy(x.m).cuda(), torch.from_numpy(x.v).cuda()
    t0 = 50
    bp = torch.tensor(running_pow(t0), device="cuda")
    g, graw, loss, gn = torch.empty_like(p), torch.empty_like(p), torch.empty(1, device="cuda"), torch.zeros(1, device="cuda")
    ws, ws_grad = dqn.dqn3_workspace(ns, h, na, batch), dqn.dqn3_workspace(ns, h, na, batch)
    gs = 0.5
    for it, f in enumerate((0.37, 2.5, 0.0)):
        dqn.dqn3_grad(tr, h, na, 0, p, pk, tp, tpk, batch, 0.99, 1.0, 7, it, None, ws_grad, graw, loss)
        g_raw = host(graw)
        gn64 = float(np.sqrt(np.sum(np.square((g_raw * np.float32(gs)).astype(np.float64)))))
        clip = f * gn64
        p0, m0, v0 = host(p), host(m), host(v)
        dqn.dqn3_update(tr, h, na, 0, p, pk, tp, tpk, batch, 0.99, 1.0, 7, it, ws, g, loss, m, v, bp, gs, clip, LR, B1, B2, EPS, gn)
        torch.cuda.synchronize()
        assert_gn(float(host(gn)[0]), g_raw * np.float32(gs))
        gc = expected_clip(g_raw, gs, clip, float(host(gn)[0]))
        eq(host(g), gc, f"clipped g of step {it}")
        oracle.adam(p0, gc, m0, v0, LR, B1, B2, EPS, t0 + it)
        eq(host(p), p0, f"p of step {it}")
        eq(host(m), m0, f"m of step {it}")
        eq(host(v), v0, f"v of step {it}")
        assert np.array_equal(host(bp), running_pow(t0 + it + 1))
        assert torch.equal(pk, dqn.mlp3_pack(p, ns, h, na))  # the re-pack is of the updated parameters
