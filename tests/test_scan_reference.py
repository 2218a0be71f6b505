"""The independent model of the reverse-time scans (tests/scan_ref.py) against everything that can judge it without a GPU:
the oracle byte for byte on every case of every route's grid (tests/scan_cases.py), the reference's own known answers
(tests/golden/scans.json), its Float64 error bound, and the planted misreadings -- each must change at least one output byte
on every route it applies to, or the grid has a hole.  tests/test_gpu_scan_routes.py runs the same grids through the kernels."""
import json
import os

import numpy as np
import pytest

import oracle
import scan_cases as SC
import scan_ref as R

GOLDEN = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "scans.json")))
ROUTE_IDS = [r.id for r in SC.ROUTES]


def _oracle(case):
    """the oracle's outputs for a case, time-major like scan_cases.model's"""
    c, m = case, SC.math(case)
    out = {}
    if c.kind == "gae":
        o = oracle.generalized_advantage_estimation(m["rewards"], m["values"], c.gamma, c.lam, terminal=m["terminal"], dims=c.dims,
                                                    dtype=c.dtype)
        out["gae"] = SC.time_major(c, o)
        return out
    if c.T > 0:
        o = oracle.discount_rewards(m["rewards"], c.gamma, terminal=m["terminal"], init=m["init"], dims=c.dims, dtype=c.dtype)
        out["scan"] = SC.time_major(c, o)
    r = m["rewards"] if c.T > 0 or c.dims == 0 else np.zeros((c.n, 0), c.dtype)
    out["reduced"] = oracle.discount_rewards_reduced(r, c.gamma, terminal=m["terminal"], init=m["init"], dims=c.dims, dtype=c.dtype)
    return out


@pytest.mark.parametrize("route", ROUTE_IDS)
def test_replay_equals_the_oracle_byte_for_byte(route):
    bad = []
    for c in SC.ROUTE[route].cases():
        mod = SC.model(c)
        for k, o in _oracle(c).items():
            got = getattr(mod, k)
            assert got.dtype == o.dtype == c.dtype and got.shape == o.shape, (c.id, k, got.shape, o.shape)
            if got.tobytes() != o.tobytes():
                bad.append((c.id, k))
    assert not bad, bad


def _golden_args(case):
    r = np.array(case["reward_rows"] if "reward_rows" in case else case["reward"], dtype=float)
    v = case.get("values_rows", case.get("values"))
    term = case.get("terminal_rows", case.get("terminal"))
    return r, None if v is None else np.array(v, dtype=float), None if term is None else np.array(term)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_replay_gives_the_reference_s_known_answers(dtype):
    """tests/golden/scans.json under the tolerances tests/test_oracle_golden.py holds the oracle to"""
    f32 = dtype == np.float32
    n = 0
    for fn in ("discount_rewards", "discount_rewards_reduced", "generalized_advantage_estimation"):
        for case in GOLDEN[fn]:
            r, v, term = _golden_args(case)
            kw = dict(terminal=term, dims=case.get("dims", 0), dtype=dtype)
            if case.get("expect_error"):
                with pytest.raises(TypeError):
                    R.replay(r, case["gamma"], **kw)
                continue
            exp = np.array(case["expect_rows"] if "expect_rows" in case else case["expect"])
            if fn == "generalized_advantage_estimation":
                out = R.replay(r, case["gamma"], case["lam"], v, **kw).gae
                tol = dict(rtol=2e-6 if f32 else 1.5e-8, atol=1e-6 if f32 else 1e-12)
            else:
                m = R.replay(r, case["gamma"], init=case.get("init"), **kw)
                out = m.scan if fn == "discount_rewards" else m.reduced
                tol = dict(rtol=1e-6 if f32 else 1.5e-8)
            np.testing.assert_allclose(out.reshape(exp.shape) if out.size == exp.size else out, exp, err_msg=case["src"], **tol)
            n += 1
    assert n == 30  # every case of the file that is not a MethodError


def test_replay_lies_inside_the_float64_bound(capsys):
    """every finite Float32 cell of every grid: |replay - exact| <= the bound carried beside exact (no tolerance chosen)"""
    worst, cells = {}, 0
    for rt in SC.ROUTES:
        if rt.dtype != np.float32:
            continue
        for c in rt.cases():
            m, mod = SC.math(c), SC.model(c)
            ex = R.exact(m["rewards"], c.gamma, c.lam if c.kind == "gae" else None, m["values"], m["terminal"], m["init"], c.dims)
            for k in ("scan", "reduced", "gae", "returns"):
                got = getattr(mod, k)
                if got is None or got.size == 0:
                    continue
                val, bnd = getattr(ex, k), getattr(ex, k + "_bound")
                if k != "reduced":
                    val, bnd = SC.time_major(c, val), SC.time_major(c, bnd)
                fin = np.isfinite(val) & np.isfinite(bnd) & np.isfinite(got)
                assert np.array_equal(np.isfinite(got), np.isfinite(val)), (c.id, k)
                with np.errstate(invalid="ignore"):
                    err = np.abs(got.astype(np.float64) - val)[fin]
                b = bnd[fin]
                assert (err <= b).all(), (c.id, k, float((err - b).max()))
                if err.size:
                    ratio = float((err[b > 0] / b[b > 0]).max()) if (b > 0).any() else 0.0
                    worst[k] = max(worst.get(k, 0.0), ratio)
                    cells += int(fin.sum())
    with capsys.disabled():
        print(f"\nscan_ref.replay against scan_ref.exact: {cells} finite cells, largest error / bound: "
              + ", ".join(f"{k} {w:.3f}" for k, w in worst.items()))
    assert cells > 1e7 and set(worst) == {"scan", "reduced", "gae", "returns"}


def _differs(a, b):
    return any(x is not None and x.tobytes() != y.tobytes() for x, y in zip(a, b))


def test_every_planted_fault_is_caught_on_every_route_it_applies_to(capsys):
    table, holes = {}, []
    for rt in SC.ROUTES:
        cases = sorted(rt.cases(), key=lambda c: c.n * c.T)
        for fault in R.FAULTS:
            todo = [c for c in cases if SC.applies(fault, rt, c)]
            if not todo:
                table[fault, rt.id] = "-"
                continue
            hit = None
            for c in todo:
                good, bad = SC.model(c), SC.model(c, fault=fault)
                if _differs([getattr(good, k) for k in rt.outputs], [getattr(bad, k) for k in rt.outputs]):
                    hit = c
                    break
            table[fault, rt.id] = "x" if hit is not None else "HOLE"
            if hit is None:
                holes.append((fault, rt.id))
    with capsys.disabled():
        print("\nfault x route (x caught, - does not apply): columns " + " ".join(f"{i}={r.id}" for i, r in enumerate(SC.ROUTES)))
        for fault in R.FAULTS:
            print(f"  {fault:24s}" + " ".join(f"{table[fault, r.id]:>2s}" for r in SC.ROUTES))
    assert not holes, holes
    for fault in R.FAULTS:  # and no fault is planted for nothing
        assert any(table[fault, r.id] == "x" for r in SC.ROUTES), fault


@pytest.mark.parametrize("route", ROUTE_IDS)
def test_census_of_the_grids(route, capsys):
    """the conditions on the inputs alone: the terminal share of the random part, every planted row in every grid that can
    hold it, the 16 four-flag patterns wherever four envs can share a lane, and every special kind at least once per route"""
    rt = SC.ROUTE[route]
    seen, special, shares, nib = set(), {}, [], 0
    for c in rt.cases():
        cen = SC.census(c)
        want = set(SC.expected(c))
        assert want <= cen["rows"], (c.id, sorted(want - cen["rows"]))
        if cen["share"] is not None:
            assert 0.02 <= cen["share"] <= 0.5, (c.id, cen["share"])
            shares.append(cen["share"])
        if c.has_term and c.n >= SC.NIBBLE_HI and c.T >= 1:
            assert cen["nibbles"] == 16, (c.id, cen["nibbles"])
            nib += 1
        seen |= want
        for k, v in cen["special"].items():
            special[k] = special.get(k, 0) + v
    rows = SC.GAE_ROWS if rt.cases()[0].kind == "gae" else SC.DISCOUNT_ROWS
    assert seen == set(rows), sorted(set(rows) - seen)
    assert all(special[k] >= 1 for k in ("pinf", "ninf", "nan", "negzero")), special
    assert shares and nib
    with capsys.disabled():
        print(f"\n{rt.id}: {len(rt.cases())} cases, terminal share {min(shares):.3f} .. {max(shares):.3f}, planted rows {len(seen)}, "
              f"grids with the 16 patterns {nib}, special cells {special}")


def test_route_table_names_every_instantiation_once():
    assert len({r.mangled for r in SC.ROUTES}) == len(SC.ROUTES) == 12 and not set(SC.UNREACHABLE) & {r.mangled for r in SC.ROUTES}
    count = lambda pre: sum(r.kernel.startswith(pre) for r in SC.ROUTES)  # noqa: E731
    assert (count("discount_kernel<"), count("gae_kernel<float"), count("gae_kernel<double"), count("gae_vec4_kernel<")) == (4, 4, 2, 2)
    for want in ("gae_vec4_kernel<false, 8>", "gae_kernel<float, false, 32, true>", "gae_kernel<double, false, 16, true>"):
        assert want in {r.kernel for r in SC.ROUTES}
    for r in SC.ROUTES:  # the shapes reach the side of the threshold the row names
        for c in r.cases():
            stream = c.n * c.T >= SC.STREAM_MIN
            assert stream == ("stream" in r.id or "vec4" in r.id), (r.id, c.id)
            if "vec4" in r.id:
                assert c.n % 4 == 0 and c.dims == 2 and c.dtype == np.float32
            if r.id in ("gae_stream_f32", "gae_ret_stream_f32") and not r.misaligned:
                assert c.n % 4 or c.dims != 2
