"""Case grids, census and route table for the reverse-time scans (TEST INFRASTRUCTURE ONLY; a helper, not a test module).

ROUTES has one row per kernel instantiation that the host dispatch of csrc/scans.hip can launch, with the entry point and the
condition that reaches it, derived from scan_geom / discount_impl / gae_impl (tests/test_scan_dispatch.py pins the literals
those conditions rest on, and the instantiation set of the code object):
    discount_impl<T, REDUCED>   always discount_kernel<T, REDUCED> (n_slices > 0; len > 0 unless REDUCED)
    gae_impl<T>                 streaming = n_slices * len >= 2^22
                                four envs per lane iff T is Float32, streaming, dims = 2 (env-major), n_slices % 4 == 0,
                                adv | r | v | ret 16-byte aligned and terminal (if any) 4-byte aligned: gae_vec4_kernel<ret, 8>
                                otherwise gae_kernel<T, ret, 128 / sizeof(T), streaming>
    `ret` is given by rlhip_gae_returns_f32 only (dims = 2), so gae_kernel<double, true, 16, *> is compiled and unreachable.

A case keeps its arrays TIME-MAJOR: r, term (T, n), v (T + 1, n), init (n,) -- row t is step t of every slice.  `math(case)`
gives the reference's mathematical arrays (what scan_ref.replay and the oracle take), `storage(case)` the flat device images
(the column-major storage of those matrices) with n1, n2.

Every grid carries PLANTED rows in fixed slices (slice j holds planted row j; a grid narrower than the list holds rows
(j + 3 * ordinal) mod K so that the narrow grids of a route cover the list between them), then, where n >= 80, the 16 patterns
of four terminal flags at one step in slices 16 .. 79 (one pattern per aligned group of four envs), then the random part.
`expected(case)` lists the planted rows the shape can hold; `census(case)` finds them again FROM THE ARRAYS ALONE.
    terminal rows   t_first, t_last, t_pair (two in a row), t_none, t_all, b_hi / b_lo (a terminal on either side of every
                    chunk boundary: steps b and b - 1 for b = T - k CH), t_far (terminals, none within a step of a boundary)
    special rows    GAE: V[T + 1] = +Inf / -Inf / NaN behind a terminal and behind a non-terminal last step; r = -0.0 and
                    V = +0.0 on a terminal step in front of a negative bootstrap and a negative carried gae
                    discount: r = +Inf / -Inf / NaN (the gain of that step) behind a terminal and behind a non-terminal step;
                    r = -0.0 on a terminal step in front of a negative gain; init = -Inf in front of a terminal last step
  The random part draws r and V from a standard normal and flags 10 % of its cells terminal (exactly floor(cells / 10), at
  least one, below 1000 cells; Bernoulli(0.1) above), so its terminal share lies in [2 %, 50 %] wherever it has two cells.
"""
import functools
import itertools
from types import SimpleNamespace

import numpy as np

import scan_ref as R

F32, F64 = np.float32, np.float64
STREAM_MIN = 1 << 22
N_SMALL = (1, 3, 4, 5, 255, 256, 257)
GAMMA_LAMBDA = ((0.99, 0.95), (1.0, 1.0), (0.0, 0.95), (0.99, 0.0))
VEC4_SHAPE, BELOW_SHAPE = (220756, 19), (220752, 19)   # 4 194 364 >= 2^22 > 4 194 288; 19 = 2 * 8 + 3
SCALAR_STREAM_SHAPE = (59919, 70)                      # odd n: never four per lane; 70 = 2 * 32 + 6
F64_STREAM_SHAPE = (113360, 37)                        # 37 = 2 * 16 + 5
assert VEC4_SHAPE[0] % 4 == 0 and VEC4_SHAPE[0] * VEC4_SHAPE[1] >= STREAM_MIN > BELOW_SHAPE[0] * BELOW_SHAPE[1]
assert SCALAR_STREAM_SHAPE[0] % 2 == 1 and SCALAR_STREAM_SHAPE[0] * SCALAR_STREAM_SHAPE[1] >= STREAM_MIN
assert F64_STREAM_SHAPE[0] * F64_STREAM_SHAPE[1] >= STREAM_MIN
NIBBLE_LO, NIBBLE_HI = 16, 80
SPECIALS = {"pinf": np.inf, "ninf": -np.inf, "nan": np.nan}
TERMINAL_ROWS = ("t_first", "t_last", "t_pair", "t_none", "t_all", "b_hi", "b_lo", "t_far")
GAE_ROWS = TERMINAL_ROWS + tuple(f"vlast_{x}_{w}" for w in ("term", "cont") for x in SPECIALS) + ("negzero",)
DISCOUNT_ROWS = TERMINAL_ROWS + tuple(f"gain_{x}_{w}" for w in ("term", "cont") for x in SPECIALS) + ("negzero", "init_ninf")
assert len(GAE_ROWS) <= NIBBLE_LO and len(DISCOUNT_ROWS) <= NIBBLE_LO


def t_values(ch):
    return (1, ch - 1, ch, ch + 1, 2 * ch + 3)


def boundaries(T, ch):
    """the steps b at which a chunk of ch steps ends: the scan walks i = T - 1 .. 0 and loads [b, b + ch) together"""
    return [T - k * ch for k in range(1, T // ch + 1) if T - k * ch > 0]


def _is(a, x):
    return np.isnan(a) if x != x else (a == x)


def _negzero(a):
    return (a == 0) & np.signbit(a)


# ----------------------------------------------------------------------------------------------------------- planted rows
def _terminal_steps(name, T, B):
    """the terminal steps of a planted terminal row, or None where the shape cannot hold it"""
    if name == "t_first":
        return [0]
    if name == "t_last":
        return [T - 1]
    if name == "t_pair":
        return None if T < 2 else [max(0, T // 2 - 1), max(0, T // 2 - 1) + 1]
    if name == "t_none":
        return []
    if name == "t_all":
        return list(range(T))
    if name == "b_hi":
        return list(B) or None
    if name == "b_lo":
        return [b - 1 for b in B] or None
    if name == "t_far":
        near = {b + d for b in B for d in (-2, -1, 0, 1)}
        far = [t for t in range(T) if t not in near]
        return far[::3] or None
    raise KeyError(name)


def expected(case):
    """the planted rows this case's shape can hold: name -> slice"""
    c = case
    rows = GAE_ROWS if c.kind == "gae" else DISCOUNT_ROWS
    K = len(rows)
    B = boundaries(c.T, c.ch)
    out = {}
    for j in range(min(c.n, K) if c.T >= 1 else 0):
        name = rows[(j + c.offset) % K]
        if name in TERMINAL_ROWS:
            ok = _terminal_steps(name, c.T, B) is not None and (c.has_term or name == "t_none")
        elif name.endswith("_cont"):
            ok = c.T >= (1 if c.kind == "gae" else 2)
        elif name.endswith("_term"):
            ok = c.has_term and c.T >= (1 if c.kind == "gae" else 2)
        elif name == "negzero":
            ok = c.has_term and c.T >= 2
        else:  # init_ninf
            ok = c.has_term and c.has_init and c.T >= 1
        if ok:
            out[name] = j
    return out


def _plant(c, r, v, term, init):
    T, B = c.T, boundaries(c.T, c.ch)
    for name, j in expected(c).items():
        if term is not None:
            term[:, j] = 0
        if name in TERMINAL_ROWS:
            for t in _terminal_steps(name, T, B):
                term[t, j] = 1
        elif name.startswith("vlast_"):
            v[T, j] = SPECIALS[name.split("_")[1]]
            if name.endswith("_term"):
                term[T - 1, j] = 1
        elif name.startswith("gain_"):
            r[T - 1, j] = SPECIALS[name.split("_")[1]]
            if name.endswith("_term"):
                term[T - 2, j] = 1
        elif name == "negzero":
            r[0, j], r[1, j], term[0, j] = -0.0, -1000.0, 1  # step 0: the reduced form returns this very element
            if c.kind == "gae":
                v[0, j], v[1, j] = 0.0, -3.0
        elif name == "init_ninf":
            init[j] = -np.inf
            term[T - 1, j] = 1


def random_from(case):
    """the first slice of the random part"""
    return NIBBLE_HI if case.n >= NIBBLE_HI else min(case.n, len(GAE_ROWS if case.kind == "gae" else DISCOUNT_ROWS))


def _build(kind, dtype, n, T, dims, gamma, lam, ch, has_term, init_kind, offset, seed):
    c = SimpleNamespace(kind=kind, dtype=dtype, n=n, T=T, dims=dims, gamma=gamma, lam=lam, ch=ch, has_term=has_term,
                        has_init=init_kind is not None, init_kind=init_kind, offset=offset if n < NIBBLE_LO else 0)
    c.id = (f"{kind}-{'f32' if dtype == F32 else 'f64'}-n{n}-T{T}-d{dims}-g{gamma}-l{lam}-"
            f"{'term' if has_term else 'noterm'}-init_{init_kind}-ch{ch}")
    rng = np.random.default_rng(seed)
    r = rng.standard_normal((T, n)).astype(dtype)
    v = rng.standard_normal((T + 1, n)).astype(dtype) if kind == "gae" else None
    init = rng.standard_normal(n).astype(dtype) if init_kind is not None else None
    term = None
    lo = random_from(c)
    if has_term:
        term = np.zeros((T, n), np.uint8)
        cells = T * (n - lo)
        if cells >= 1000:
            term[:, lo:] = rng.random((T, n - lo)) < 0.1
        elif cells >= 1:
            flat = np.zeros(cells, np.uint8)
            flat[rng.choice(cells, max(1, cells // 10), replace=False)] = 1
            term[:, lo:] = flat.reshape(T, n - lo)
        if n >= NIBBLE_HI and T >= 1:
            for p in range(16):
                for e in range(4):
                    term[T // 2, NIBBLE_LO + 4 * p + e] = (p >> e) & 1
        term[term != 0] = np.where(np.arange(int((term != 0).sum())) % 3 == 2, 255, 1)  # the kernels test != 0
    _plant(c, r, v, term, init)
    c.r, c.v, c.term, c.init = r, v, term, init
    for a in (r, v, term, init):
        if a is not None:
            a.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def build(kind, dtype, n, T, dims, gamma, lam, ch, has_term=True, init_kind=None, offset=0):
    seed = [1 if kind == "gae" else 2, 4 if dtype == F32 else 8, n, T, dims, ch, int(has_term), offset]
    return _build(kind, dtype, n, T, dims, gamma, lam, ch, has_term, init_kind, offset, seed)


# ---------------------------------------------------------------------------------------------------------------- views
def math(case):
    """the reference's arguments: dict(rewards, values, terminal, init, dims) of mathematical arrays"""
    c = case

    def m(a):
        return None if a is None else (a[:, 0] if c.dims == 0 else a if c.dims == 1 else a.T)
    init = c.init
    if init is not None and c.init_kind == "scalar":
        init = c.dtype(init[0])
    return dict(rewards=m(c.r), values=m(c.v), terminal=m(c.term), init=init, dims=c.dims)


def storage(case):
    """the device images: dict(r, v, term, init, n1, n2), flat C-contiguous arrays holding the column-major matrices"""
    c = case

    def s(a):
        if a is None:
            return None
        return np.ascontiguousarray(a if c.dims == 2 else a.T).reshape(-1)
    n1, n2 = (c.n, c.T) if c.dims == 2 else (c.T, c.n) if c.dims == 1 else (c.T, 1)
    init = None if c.init is None else np.ascontiguousarray(c.init[:1] if c.init_kind == "scalar" else c.init)
    return dict(r=s(c.r), v=s(c.v), term=s(c.term), init=init, n1=n1, n2=n2)


def from_storage(case, flat, extra=0):
    """a flat device image of a (T + extra, n) time-major array of this case -> that array"""
    c = case
    rows = c.T + extra
    return flat.reshape(rows, c.n) if c.dims == 2 else flat.reshape(c.n, rows).T


def time_major(case, a):
    """a mathematical array of this case (what replay returns) -> time-major (T, n)"""
    return None if a is None else R._time_major(a, case.dims)


def _replay(c, fault):
    m = math(c)
    out = R.replay(m["rewards"], c.gamma, c.lam if c.kind == "gae" else None, m["values"], m["terminal"], m["init"], c.dims,
                   fault=fault)
    return SimpleNamespace(**{k: time_major(c, a) if k != "reduced" else a for k, a in vars(out).items()})


@functools.lru_cache(maxsize=None)
def _model(case_id):
    return _replay(_BY_ID[case_id], None)


def model(case, fault=None):
    """scan_ref.replay on the case: time-major scan / gae / returns, reduced (n,).  The unfaulted result is computed once
    and shared between the tests that need it"""
    assert _BY_ID.setdefault(case.id, case) is case
    return _replay(case, fault) if fault else _model(case.id)


_BY_ID = {}


# --------------------------------------------------------------------------------------------------------------- census
def census(case):
    """What the arrays of a case hold, found from the arrays alone: dict(share = terminal share of the random part (None
    below two cells), rows = the planted rows present, nibbles = how many of the 16 four-flag patterns occur in an aligned
    group of four slices at one step, special = cells per special kind)"""
    c = case
    T, n = c.T, c.n
    B = boundaries(T, c.ch)
    lo = random_from(c)
    K = min(n, lo, NIBBLE_LO)
    t = None if c.term is None else (c.term[:, :K] != 0)
    rows = set()
    if t is None:
        rows.add("t_none")
    elif T >= 1 and K >= 1:
        cnt = t.sum(0)
        if t[0].any():
            rows.add("t_first")
        if t[T - 1].any():
            rows.add("t_last")
        if T >= 2 and (t[:-1] & t[1:]).any():
            rows.add("t_pair")
        if (cnt == 0).any():
            rows.add("t_none")
        if (cnt == T).any():
            rows.add("t_all")
        if B and all(t[b].any() for b in B):
            rows.add("b_hi")
        if B and all(t[b - 1].any() for b in B):
            rows.add("b_lo")
        near = sorted({b + d for b in B for d in (-2, -1, 0, 1) if 0 <= b + d < T})
        if ((cnt > 0) & (t[near].sum(0) == 0 if near else True)).any():
            rows.add("t_far")
    val = c.v if c.kind == "gae" else c.r  # the array whose element t + 1 step t carries: V[t + 1] / the gain of step t + 1
    if T >= 1 and K >= 1:
        nxt = val[1:T + 1 if c.kind == "gae" else T, :K]
        tt = np.zeros(nxt.shape, bool) if t is None else t[:nxt.shape[0]]
        for x, X in SPECIALS.items():
            pre = "vlast" if c.kind == "gae" else "gain"
            if (_is(nxt, X) & tt).any():
                rows.add(f"{pre}_{x}_term")
            if (_is(nxt, X) & ~tt).any():
                rows.add(f"{pre}_{x}_cont")
        if t is not None and T >= 2:
            z = _negzero(c.r[:T - 1, :K]) & t[:T - 1] & (c.r[1:, :K] < 0)
            if c.kind == "gae":
                z &= (c.v[1:T, :K] < 0) & (c.v[:T - 1, :K] == 0) & ~np.signbit(c.v[:T - 1, :K])
            if z.any():
                rows.add("negzero")
        if t is not None and c.init is not None and ((c.init[:K] == -np.inf) & t[T - 1]).any():
            rows.add("init_ninf")
    nib = 0
    if c.term is not None and n >= NIBBLE_HI and T >= 1:
        g = (c.term[:, NIBBLE_LO:NIBBLE_HI] != 0).reshape(T, 16, 4)
        nib = len(set((g * (1 << np.arange(4))).sum(2).reshape(-1).tolist()))
    share = None
    if c.term is not None and T * (n - lo) >= 2:
        share = float((c.term[:, lo:] != 0).mean())
    arrays = [a for a in (c.r, c.v, c.init) if a is not None]
    special = {x: int(sum(_is(a, X).sum() for a in arrays)) for x, X in SPECIALS.items()}
    special["negzero"] = int(sum(_negzero(a).sum() for a in arrays))
    return dict(share=share, rows=rows, nibbles=nib, special=special)


# --------------------------------------------------------------------------------------------------------------- routes
def _small(kind, dtype, ch, dims2_only=False, reduced=False):
    out = []
    for k, (n, T) in enumerate(itertools.product(N_SMALL, t_values(ch))):
        gamma, lam = GAMMA_LAMBDA[k % 4]
        if n == 1 and not dims2_only:
            dims = 0 if k % 2 == 0 else 2
        else:
            dims = 2 if (dims2_only or k % 3) else 1
        init_kind = None
        if kind == "discount" and k % 3:
            init_kind = "scalar" if dims == 0 else "slice"
        out.append(build(kind, dtype, n, T, dims, gamma, lam, ch, has_term=(k % 7 != 3), init_kind=init_kind, offset=3 * k))
    if reduced:  # len = 0: the reduced form returns init
        out.append(build(kind, dtype, 5, 0, 2, 0.99, 0.95, ch, has_term=True, init_kind="slice"))
        out.append(build(kind, dtype, 1, 0, 0, 0.99, 0.95, ch, has_term=False, init_kind="scalar"))
    return out


def _big(dtype, shape, dims, ch, has_term=True):
    return build("gae", dtype, shape[0], shape[1], dims, 0.99, 0.95, ch, has_term=has_term)


MISALIGNED = ("adv", "ret", "r", "v", "term")  # the alignment fall-back: exactly one array one element into its allocation


def _route(id, kernel, mangled, entry, condition, dtype, outputs, ch, cases, misaligned=()):
    return SimpleNamespace(id=id, kernel=kernel, mangled=mangled, entry=entry, condition=condition, dtype=dtype,
                           outputs=outputs, ch=ch, cases=cases, misaligned=misaligned)


ROUTES = (
    _route("discount_f32", "discount_kernel<float, false>", "discount_kernelIfLb0EE", "rlhip_discount_rewards_f32",
           "every call with n_slices > 0 and len > 0", F32, ("scan",), 4, lambda: _small("discount", F32, 4)),
    _route("discount_reduced_f32", "discount_kernel<float, true>", "discount_kernelIfLb1EE", "rlhip_discount_rewards_reduced_f32",
           "every call with n_slices > 0 (len = 0 returns init)", F32, ("reduced",), 4,
           lambda: _small("discount", F32, 4, reduced=True)),
    _route("discount_f64", "discount_kernel<double, false>", "discount_kernelIdLb0EE", "rlhip_discount_rewards_f64",
           "every call with n_slices > 0 and len > 0", F64, ("scan",), 4, lambda: _small("discount", F64, 4)),
    _route("discount_reduced_f64", "discount_kernel<double, true>", "discount_kernelIdLb1EE", "rlhip_discount_rewards_reduced_f64",
           "every call with n_slices > 0 (len = 0 returns init)", F64, ("reduced",), 4,
           lambda: _small("discount", F64, 4, reduced=True)),
    _route("gae_f32", "gae_kernel<float, false, 32, false>", "gae_kernelIfLb0ELi32ELb0EE", "rlhip_gae_f32",
           "n_slices * len < 2^22", F32, ("gae",), 32,
           lambda: _small("gae", F32, 32) + [_big(F32, BELOW_SHAPE, 2, 32)]),
    _route("gae_ret_f32", "gae_kernel<float, true, 32, false>", "gae_kernelIfLb1ELi32ELb0EE", "rlhip_gae_returns_f32",
           "n_env * T < 2^22", F32, ("gae", "returns"), 32,
           lambda: _small("gae", F32, 32, dims2_only=True) + [_big(F32, BELOW_SHAPE, 2, 32)]),
    _route("gae_stream_f32", "gae_kernel<float, false, 32, true>", "gae_kernelIfLb0ELi32ELb1EE", "rlhip_gae_f32",
           "n_slices * len >= 2^22 and not (dims = 2, n_slices % 4 == 0, adv | r | v 16-byte and terminal 4-byte aligned)",
           F32, ("gae",), 32,
           lambda: [_big(F32, SCALAR_STREAM_SHAPE, 2, 32), _big(F32, SCALAR_STREAM_SHAPE, 1, 32)]),
    _route("gae_ret_stream_f32", "gae_kernel<float, true, 32, true>", "gae_kernelIfLb1ELi32ELb1EE", "rlhip_gae_returns_f32",
           "n_env * T >= 2^22 and (n_env % 4 != 0 or one of adv | ret | r | v off 16 bytes or terminal off 4 bytes)",
           F32, ("gae", "returns"), 32,
           lambda: [_big(F32, SCALAR_STREAM_SHAPE, 2, 32), _big(F32, VEC4_SHAPE, 2, 32)], misaligned=MISALIGNED),
    _route("gae_f64", "gae_kernel<double, false, 16, false>", "gae_kernelIdLb0ELi16ELb0EE", "rlhip_gae_f64",
           "n_slices * len < 2^22", F64, ("gae",), 16, lambda: _small("gae", F64, 16)),
    _route("gae_stream_f64", "gae_kernel<double, false, 16, true>", "gae_kernelIdLb0ELi16ELb1EE", "rlhip_gae_f64",
           "n_slices * len >= 2^22", F64, ("gae",), 16, lambda: [_big(F64, F64_STREAM_SHAPE, 2, 16)]),
    _route("gae_vec4_f32", "gae_vec4_kernel<false, 8>", "gae_vec4_kernelILb0ELi8EE", "rlhip_gae_f32",
           "n_slices * len >= 2^22, dims = 2, n_slices % 4 == 0, adv | r | v 16-byte aligned, terminal 4-byte aligned",
           F32, ("gae",), 8, lambda: [_big(F32, VEC4_SHAPE, 2, 8), _big(F32, VEC4_SHAPE, 2, 8, has_term=False)]),
    _route("gae_vec4_ret_f32", "gae_vec4_kernel<true, 8>", "gae_vec4_kernelILb1ELi8EE", "rlhip_gae_returns_f32",
           "n_env * T >= 2^22, n_env % 4 == 0, adv | ret | r | v 16-byte aligned, terminal 4-byte aligned",
           F32, ("gae", "returns"), 8, lambda: [_big(F32, VEC4_SHAPE, 2, 8)]),
)
UNREACHABLE = {
    "gae_kernelIdLb1ELi16ELb0EE": "gae_kernel<double, true, 16, false>: gae_impl<double> instantiates it, no Float64 entry point passes ret",
    "gae_kernelIdLb1ELi16ELb1EE": "gae_kernel<double, true, 16, true>: gae_impl<double> instantiates it, no Float64 entry point passes ret",
}
ROUTE = {r.id: r for r in ROUTES}
assert len(ROUTE) == len(ROUTES) == 12


def applies(fault, route, case):
    """whether a planted misreading can show in this route's outputs on this case at all"""
    outs, needs = R.FAULT_APPLIES[fault]
    if not outs & set(route.outputs):
        return False
    if fault.startswith("chunk_carry_lost") and int(fault.split(":")[1]) != route.ch:
        return False
    have = {"terminal"} if case.has_term else set()
    if case.has_init:
        have |= {"init"} | ({"init_per_slice"} if case.init_kind == "slice" and case.n > 1 else set())
    return needs <= have


def route_applies(fault, route):
    return any(applies(fault, route, c) for c in route.cases())
