"""Every instantiation the host dispatch of csrc/scans.hip can launch, through the entry point that reaches it, on the case
grids of tests/scan_cases.py: one test per row of scan_cases.ROUTES, every output array compared BYTE FOR BYTE (tobytes():
the sign of a zero and the bits of a NaN count) with the independent model tests/scan_ref.py.  tests/test_scan_reference.py
judges that model on the CPU; tests/test_scan_dispatch.py pins the conditions the routes were derived from.

Every array lives inside a larger allocation filled with a canary byte: the bytes in front of and behind each output must
come back untouched, and the alignment fall-back of the four-envs-per-lane route is reached by placing exactly one array one
element (terminal: one byte) into its allocation.  NaN bits are compared too: gfx950 creates the same NaN as the host for
an invalid operation and hands an input NaN on unchanged (tests/scan_ref.py).

The same module holds the small related cases: rlhip_huber_f32 over the block edges and the stride leg of its partial-sum
grid, rlhip_td_target_f32 / _n_f32 over both addressings, ties and infinite Q-values."""
import ctypes as C

import numpy as np
import pytest
import torch

import oracle
import scan_cases as SC
import scan_ref as R

pytestmark = pytest.mark.gpu
PAD, CANARY = 64, 0xA5


class Buf:
    """`nbytes` of device memory `shift` bytes past a 64-byte boundary inside a canary-filled allocation"""

    def __init__(self, nbytes=None, host=None, shift=0):
        if host is not None:
            host = np.ascontiguousarray(host).reshape(-1).view(np.uint8)
            nbytes = host.size
        self.nbytes, self.lo = int(nbytes), PAD + shift
        self.base = torch.full((self.nbytes + 2 * PAD,), CANARY, dtype=torch.uint8, device="cuda")
        if host is not None and nbytes:
            self.base[self.lo:self.lo + nbytes].copy_(torch.from_numpy(host.copy()))

    @property
    def ptr(self):  # an empty array has a NULL base pointer
        return C.c_void_p(self.base.data_ptr() + self.lo) if self.nbytes else None

    def host(self, dtype):
        b = self.base.cpu().numpy()
        assert (b[:self.lo] == CANARY).all(), "bytes in front of the array were written"
        assert (b[self.lo + self.nbytes:] == CANARY).all(), "bytes behind the array were written"
        return b[self.lo:self.lo + self.nbytes].copy().view(dtype)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _null():
    return Buf(0)


def run(rt, case, misaligned=None):
    """one call of the row's entry point on the case -> its outputs, time-major (reduced: (n,))"""
    from rlhip._lib import call

    c, s = case, SC.storage(case)
    esz = np.dtype(c.dtype).itemsize

    def buf(name, host=None, nbytes=None):
        shift = (1 if name == "term" else esz) if misaligned == name else 0
        return _null() if (host is None and nbytes is None) else Buf(nbytes, host, shift)
    r, v, term, init = buf("r", s["r"]), buf("v", s["v"]), buf("term", s["term"]), buf("init", s["init"])
    full = c.n * c.T * esz
    out = {}
    if rt.entry.startswith("rlhip_discount_rewards_reduced"):
        o = buf("out", nbytes=c.n * esz)
        call(rt.entry, o.ptr, r.ptr, s["n1"], s["n2"], c.gamma, term.ptr, init.ptr, c.dims, _stream())
        out["reduced"] = o
    elif rt.entry.startswith("rlhip_discount_rewards"):
        o = buf("out", nbytes=full)
        call(rt.entry, o.ptr, r.ptr, s["n1"], s["n2"], c.gamma, term.ptr, init.ptr, c.dims, _stream())
        out["scan"] = o
    elif rt.entry == "rlhip_gae_returns_f32":
        assert c.dims == 2
        out["gae"], out["returns"] = buf("adv", nbytes=full), buf("ret", nbytes=full)
        call(rt.entry, out["gae"].ptr, out["returns"].ptr, r.ptr, v.ptr, term.ptr, c.n, c.T, c.gamma, c.lam, _stream())
    else:
        out["gae"] = buf("adv", nbytes=full)
        call(rt.entry, out["gae"].ptr, r.ptr, v.ptr, s["n1"], s["n2"], c.gamma, c.lam, term.ptr, c.dims, _stream())
    torch.cuda.synchronize()
    if misaligned:  # exactly that array is off its alignment, by one element
        for name, b in (("r", r), ("v", v), ("term", term), ("adv", out.get("gae")), ("ret", out.get("returns"))):
            off = (b.base.data_ptr() + b.lo) % 16
            assert off == ((1 if name == "term" else esz) if name == misaligned else 0), (name, misaligned, off)
    for b in (r, v, term, init):
        b.host(np.uint8)  # the inputs' surroundings too
    return {k: (b.host(c.dtype) if k == "reduced" else np.ascontiguousarray(SC.from_storage(c, b.host(c.dtype)))) for k, b in out.items()}


def _bits(a):
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def same_bytes(got, want, tag):
    assert got.dtype == want.dtype and got.shape == want.shape, (tag, got.dtype, got.shape, want.shape)
    if got.tobytes() == want.tobytes():
        return
    d = np.argwhere(_bits(got) != _bits(want))
    first = [(tuple(int(x) for x in i), hex(int(_bits(got)[tuple(i)])), hex(int(_bits(want)[tuple(i)]))) for i in d[:5]]
    raise AssertionError(f"{tag}: {len(d)} of {got.size} cells differ from the model; (step, slice), kernel bits, model bits: {first}")


@pytest.mark.parametrize("route", [r.id for r in SC.ROUTES])
def test_route_equals_the_model_byte_for_byte(route):
    rt = SC.ROUTE[route]
    runs = 0
    for c in rt.cases():
        mod = SC.model(c)
        vec4_shape = c.dtype == np.float32 and c.dims == 2 and c.n % 4 == 0 and c.n * c.T >= SC.STREAM_MIN
        fall_back = bool(rt.misaligned) and vec4_shape  # this shape reaches the row only with one array off its alignment
        for mis in (rt.misaligned if fall_back else (None,)):
            got = run(rt, c, mis)
            assert set(got) == set(rt.outputs)
            for k in rt.outputs:
                same_bytes(got[k], getattr(mod, k), f"{rt.id} {c.id} {k}" + (f" ({mis} misaligned)" if mis else ""))
            runs += 1
        if route == "gae_vec4_f32":  # and the advantages of the fused form on the same inputs
            fused = run(SC.ROUTE["gae_vec4_ret_f32"], c)
            same_bytes(got["gae"], fused["gae"], f"{c.id}: rlhip_gae_f32 against rlhip_gae_returns_f32")
    assert runs >= len(rt.cases())


def test_ppo_policy_gae_equals_the_model():
    """rlhip_ppo_gae_f32 through PPOPolicy.gae_(): the trajectory's reward / value / terminal planes overwritten with one grid case"""
    import rlhip

    c = next(c for c in SC.ROUTE["gae_ret_f32"].cases() if (c.n, c.T) == (256, 33))
    assert c.has_term and c.dims == 2 and (c.gamma, c.lam) == (0.99, 0.95)
    env = rlhip.CartPoleEnv(c.n, seed=5)
    pol = rlhip.PPOPolicy(env, update_freq=c.T, seed=5, gamma=c.gamma, lam=c.lam)
    tr = pol.trajectory
    for plane, a in ((tr.reward, c.r), (tr.value, c.v), (tr.terminal, c.term)):
        assert tuple(plane.shape) == a.shape
        plane.copy_(torch.from_numpy(a.copy()))
    tr.adv.fill_(float("nan"))
    tr.ret.fill_(float("nan"))
    pol.gae_()
    torch.cuda.synchronize()
    mod = SC.model(c)
    same_bytes(tr.adv.cpu().numpy(), mod.gae, "PPOPolicy.gae_ adv")
    same_bytes(tr.ret.cpu().numpy(), mod.returns, "PPOPolicy.gae_ ret")


def test_reduced_scan_of_an_empty_matrix_through_ops():
    """len = 0 through rlhip.ops: empty tensors have no data pointer, the reduced form still returns init"""
    from rlhip import ops

    init = torch.tensor([1.5, -0.0, float("-inf")], device="cuda")
    out = ops.discount_rewards_reduced(torch.empty((0, 3), device="cuda"), 0.5, init=init, dims=2)
    same_bytes(out.cpu().numpy(), init.cpu().numpy(), "reduced, len = 0")


# -------------------------------------------------------------------------------------------------------------- huber
HUBER_N = (1, 255, 256, 257, 262143, 262144, 262145, (1 << 22) + 3)  # grid_for(n, 256, 1024) strides from 262145 on


def _ulps(a, b):
    a, b = np.float32(a), np.float32(b)
    assert a >= 0 and b >= 0 and np.isfinite(a) and np.isfinite(b), (a, b)
    return abs(int(a.view(np.uint32)) - int(b.view(np.uint32)))


@pytest.mark.parametrize("with_dq", [True, False], ids=["dq", "dq_null"])
@pytest.mark.parametrize("n", HUBER_N)
def test_huber_block_edges_and_stride_leg(n, with_dq):
    from rlhip._lib import call

    delta = np.float32(1.0 if HUBER_N.index(n) % 2 == 0 else 0.5)
    rng = np.random.default_rng(n)
    t = (rng.integers(-8, 9, n) / 4).astype(np.float32)
    q = (t + rng.standard_normal(n).astype(np.float32) * np.float32(1.5)).astype(np.float32)
    # |q - target| exactly delta, just below, just above, and 0, with either sign: at the head, and again at the tail
    # (the last block and, from 262145 on, the stride leg)
    plant = []
    for sgn in (1, -1):
        at = np.float32(0.0)  # q - 0 is exact on either side of the edge
        edge = np.float32(at + sgn * delta)
        plant += [(at, edge), (at, np.nextafter(edge, at)), (at, np.nextafter(edge, np.float32(sgn * 100))), (at, at)]
    for i, (tt, qq) in enumerate(plant):
        for j in (i, n - 1 - i):
            if 0 <= j < n and (j == i or n >= 2 * len(plant)):
                t[j], q[j] = tt, qq
    l, dq_m, loss_m = R.huber(q, t, delta)
    d = np.abs(q[:min(n, 8)] - t[:min(n, 8)])
    assert d[0] == delta and (n < 8 or (d[1] < delta < d[2] and d[3] == 0 and d[4] == delta and d[5] < delta < d[6]))
    qb, tb, loss, dq = Buf(host=q), Buf(host=t), Buf(4), (Buf(4 * n) if with_dq else _null())
    call("rlhip_huber_f32", qb.ptr, tb.ptr, n, float(delta), loss.ptr, dq.ptr, _stream())
    torch.cuda.synchronize()
    got = loss.host(np.float32)[0]
    # the per-sample losses are the model's Float32 values; only the order of the Float64 summation differs
    assert _ulps(got, loss_m) <= 1, (n, float(got), float(loss_m))
    if with_dq:
        same_bytes(dq.host(np.float32), dq_m, f"huber dq, n = {n}")


# ---------------------------------------------------------------------------------------------------------- td target
TD_N = (1, 255, 256, 257, 70001)


def _td_inputs(na, n, seed):
    rng = np.random.default_rng(seed)
    q = (rng.integers(-16, 17, (na, n)) / 8).astype(np.float32) * np.float32(1.37)
    r = rng.standard_normal(n).astype(np.float32)
    term = (rng.random(n) < 0.25).astype(np.uint8) * np.where(np.arange(n) % 2, 1, 255).astype(np.uint8)
    # planted columns: all actions tied, the maximum twice, +Inf / -Inf maxima on a non-terminal and on a terminal sample
    cols = [("tie_all", 0), ("tie_two", 0), ("pinf", 0), ("pinf", 1), ("ninf", 0), ("ninf", 1), ("pinf_last", 1)]
    for j, (kind, tm) in enumerate(cols):
        if j >= n:
            break
        term[j] = tm
        if kind == "tie_all":
            q[:, j] = 0.625
        elif kind == "tie_two":
            q[:, j] = -1.0
            q[0, j] = q[na - 1, j] = 2.5
        elif kind == "pinf":
            q[0, j] = np.inf
        elif kind == "ninf":
            q[:, j] = -np.inf
        else:
            q[na - 1, j] = np.inf
    return q, r, term


@pytest.mark.parametrize("addressing", ["soa", "julia"])
@pytest.mark.parametrize("na", [1, 2, 3, 4, 18])
def test_td_target_addressings_ties_and_infinities(na, addressing):
    from rlhip._lib import call, lib

    for n in TD_N:
        q, r, term = _td_inputs(na, n, 1000 * na + n)
        ks, is_ = (n, 1) if addressing == "soa" else (1, na)
        qb = Buf(host=q if addressing == "soa" else q.T)
        rb, tb = Buf(host=r), Buf(host=term)
        for n_step in (None, 1, 3, 32):
            out = Buf(4 * n)
            if n_step is None:
                gamma = 0.99
                call("rlhip_td_target_f32", qb.ptr, na, n, ks, is_, rb.ptr, tb.ptr, gamma, out.ptr, _stream())
            else:
                gamma = float(lib.rlhip_gamma_pow(0.99, n_step))
                assert gamma == oracle.gamma_pow(0.99, n_step)
                call("rlhip_td_target_n_f32", qb.ptr, na, n, ks, is_, rb.ptr, tb.ptr, 0.99, n_step, out.ptr, _stream())
            torch.cuda.synchronize()
            want = R.td_target(q, r, term, gamma)
            if n >= 7:
                assert np.isnan(want[3]) and np.isnan(want[5]) and want[2] == np.inf and want[4] == -np.inf  # gamma * 0 * Inf
            same_bytes(out.host(np.float32), want, f"td_target na = {na}, n = {n}, {addressing}, n_step = {n_step}")
