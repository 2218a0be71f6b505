"""The kernels of csrc/dqn_batch.hip on the GPU, at the smallest shapes at which they can still go wrong.

  plan      rlhip_dqn_plan_obsn_f32: q_out and actions byte-equal to rlhip_mlp2_forward_f32 -> rlhip_eps_greedy_select_f32 (and, for
            relu, q_out byte-equal to oracle.mlp2_forward) -- ns in {5, 6, 16} x h in {4, 128, 256} x na in {1, 3, 4} x both activations,
            n in {1, 63, 257, 4096}, eps in {0, 0.3, 1}
  gradient  rlhip_dqn_grad_batch_f32 against the model of tests/dqn_batch_ref.py (the oracle's functions, composed) under F32_GRAD_TOL per
            tensor, loss 1e-4 relative, td rtol 1e-5 / atol 1e-6 (the bars of tests/test_gpu_f32_learner_matrix.py) -- ns in {5, 6, 16} x
            h in {4, 64, 128, 256} x na in {1, 3, 4} x both activations, batch in {1, 63, 64, 65, 512} (64 = the tile), one batch of
            64 x 256 + 1 (a workgroup takes a second tile), every combination of n_used / weights / double_dqn / td_out = NULL; two calls
            give the same bytes; an out-of-range action drops its sample and nothing else, and the bounds build refuses it."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import oracle  # noqa: E402
import dqn_batch_ref as ref  # noqa: E402
from conftest import F32_GRAD_TOL, ROOT, assert_grad_close  # noqa: E402
from test_gpu_bench_shapes import dev, host, note  # noqa: E402


@pytest.fixture(scope="module")
def rl():
    import rlhip

    oracle.use_all_cores(True)
    yield rlhip
    oracle.use_all_cores(False)


# ---------------------------------------------------------------------------------------------------------------- plan
@pytest.mark.parametrize("act", [0, 1], ids=["relu", "tanh"])
@pytest.mark.parametrize("na", [1, 3, 4])
@pytest.mark.parametrize("h", [4, 128, 256])
@pytest.mark.parametrize("ns", [5, 6, 16])
def test_plan_is_the_two_shipped_launches_byte_for_byte(rl, ns, h, na, act):
    from rlhip.dqn import dqn_plan_obsn
    from rlhip.ops import eps_greedy_select, mlp2_forward

    rng = np.random.default_rng(ns * 1000 + h * 10 + na + 5 * act)
    p_host = oracle.mlp2_init(ns, h, na, 3, 0) + (0.1 * rng.standard_normal(oracle.mlp2_nparams(ns, h, na))).astype(np.float32)
    p = dev(p_host)
    for n in (1, 63, 257, 4096):
        x_host = rng.standard_normal((ns, n)).astype(np.float32)
        x = dev(x_host)
        q_ref = mlp2_forward(p, ns, h, na, act, x)
        for eps in (0.0, 0.3, 1.0):
            step, base = 7 + n, 11
            a, q = dqn_plan_obsn(p, ns, h, na, act, x, eps, 5, base, step)
            a_ref = eps_greedy_select(q_ref, eps, 5, step, base)
            assert torch.equal(q, q_ref), f"n={n}: q_out differs from rlhip_mlp2_forward_f32"
            assert torch.equal(a, a_ref), f"n={n} eps={eps}: actions differ from rlhip_eps_greedy_select_f32"
            assert np.array_equal(host(a), oracle.eps_greedy_select(host(q_ref), eps, 5, step, env_id_base=base))
        if act == 0:
            assert np.array_equal(host(q_ref), oracle.mlp2_forward(p_host, ns, h, na, act, x_host)), f"n={n}: q_out differs from the oracle"
    # q_out = NULL: the actions alone
    a = torch.empty(4096, dtype=torch.int32, device="cuda")
    rl._lib.call("rlhip_dqn_plan_obsn_f32", C.c_void_p(p.data_ptr()), ns, h, na, act, C.c_void_p(x.data_ptr()), 4096, 0.3, 5, 11, 3,
                 C.c_void_p(a.data_ptr()), None, None)
    assert torch.equal(a, eps_greedy_select(q_ref, 0.3, 5, 3, 11))


@pytest.mark.parametrize("act", [0, 1], ids=["relu", "tanh"])
def test_plan_of_a_net_too_large_for_lds_staging(rl, act):
    """16 -> 1024 -> 4 has 21508 parameters, above the 12288 the plan kernel stages in LDS: the form with wave-uniform global loads"""
    from rlhip.dqn import dqn_plan_obsn
    from rlhip.ops import eps_greedy_select, mlp2_forward

    ns, h, na, n = 16, 1024, 4, 257
    assert oracle.mlp2_nparams(ns, h, na) > 12288 >= oracle.mlp2_nparams(16, 256, 4)
    rng = np.random.default_rng(act)
    p, x = dev(oracle.mlp2_init(ns, h, na, 3, 0)), dev(rng.standard_normal((ns, n)).astype(np.float32))
    q_ref = mlp2_forward(p, ns, h, na, act, x)
    for eps in (0.0, 0.3, 1.0):
        a, q = dqn_plan_obsn(p, ns, h, na, act, x, eps, 5, 11, 9)
        assert torch.equal(q, q_ref) and torch.equal(a, eps_greedy_select(q_ref, eps, 5, 9, 11))


# ------------------------------------------------------------------------------------------------------------ gradient
def _run(c, a=None, twice=False):
    """the case on the GPU -> (loss, grad, td or None)"""
    from rlhip.dqn import dqn_grad_batch

    ns, h, na, act = c["shape"]
    b = c["batch"]
    p, pt = dev(c["p"]), dev(c["pt"])
    args = (dev(c["s"]), dev(c["a"] if a is None else a), dev(c["r"]), dev(c["term"]), dev(c["sn"]))
    nu = None if c["n_used"] is None else dev(c["n_used"])
    w = None if c["weights"] is None else dev(c["weights"])
    out = []
    for _ in range(2 if twice else 1):
        td = torch.full((b,), -1.0, dtype=torch.float32, device="cuda") if c["td"] else None
        grad = torch.full_like(p, float("nan"))
        g, loss = dqn_grad_batch(ns, h, na, act, p, pt, *args, c["gamma"], c["delta"], nu, w, c["double_dqn"], grad=grad, td=td)
        out.append((float(loss), host(g).copy(), None if td is None else host(td).copy()))
    if twice:
        (l0, g0, t0), (l1, g1, t1) = out
        assert l0 == l1 and np.array_equal(g0, g1) and (t0 is None or np.array_equal(t0, t1)), "two calls on the same inputs differ"
    return out[0]


def _compare(c, got, want, tag):
    ns, h, na, _ = c["shape"]
    (loss, g, td), (lo, go, tdo) = got, want
    for name, part in ref.split(g, ns, h, na).items():
        o = ref.split(go, ns, h, na)[name]
        print(f"{tag} {name}: max|g - o| / max|o| = {np.abs(part - o).max() / max(np.abs(o).max(), 1e-30):.3e}")
        assert_grad_close(part, o, F32_GRAD_TOL, f"dqn_grad_batch {tag} {name}")
    assert abs(loss - lo) <= 1e-4 * max(abs(lo), 1e-6), f"{tag}: loss {loss} vs {lo}"
    if td is not None:
        np.testing.assert_allclose(td, tdo, rtol=1e-5, atol=1e-6, err_msg=tag)


GRID = ref.grid()


@pytest.mark.parametrize("shape,batches", GRID, ids=[f"ns{s[0]}-h{s[1]}-na{s[2]}-{'relu' if s[3] == 0 else 'tanh'}" for s, _ in GRID])
def test_gradient_against_the_model(rl, shape, batches):
    for b, k in batches:
        c = ref.make_case(*shape, b, seed=1000 + k, **ref.flags(k))
        _compare(c, _run(c, twice=(b in (ref.TILE + 1, 512))), ref.case_loss_grad(c), f"b={b} flags={k % 16}")


def test_gradient_with_a_second_tile_per_workgroup(rl):
    c = ref.make_case(16, 256, 3, 0, ref.BIG_BATCH, seed=77, **ref.flags(7))
    assert c["batch"] > ref.TILE * ref.MAX_ROWS
    _compare(c, _run(c, twice=True), ref.case_loss_grad(c), f"b={ref.BIG_BATCH}")


@pytest.mark.parametrize("k", [0, 15])
def test_out_of_range_action_drops_its_sample_only(rl, k):
    fl = ref.flags(k)
    fl["td"] = True
    c = ref.make_case(6, 128, 3, 1, 130, seed=4242 + k, **fl)
    a = c["a"].copy()
    a[[4, 70, 129]] = [3, -1, 1 << 30]
    got = _run(c, a=a)
    _compare(c, got, ref.case_loss_grad(c, dropped=(4, 70, 129)), f"dropped flags={k}")
    assert (got[2][[4, 70, 129]] == 0).all()
    # ... and the bounds-checked build refuses the batch (and takes the valid one)
    so = os.path.join(ROOT, "reinforcementlearning.jl_amd", "lib", "librlhip_bounds.so")
    assert os.path.exists(so), "run python -c 'import __graft_entry__ as g; g.build()'"
    lib = C.CDLL(so)
    f = lib.rlhip_dqn_grad_batch_f32
    f.restype, f.argtypes = C.c_int32, rl._lib._PROTOS["rlhip_dqn_grad_batch_f32"][1]
    lib.rlhip_last_error.restype = C.c_char_p
    ns, h, na, act = c["shape"]
    p, pt, s, r, t, sn = (dev(c[x]) for x in ("p", "pt", "s", "r", "term", "sn"))
    ws = torch.empty(int(rl._lib.lib.rlhip_dqn_batch_workspace_bytes(ns, h, na, 130)), dtype=torch.uint8, device="cuda")
    g, loss = torch.zeros_like(p), torch.zeros(1, device="cuda")
    P = lambda x: C.c_void_p(x.data_ptr())  # noqa: E731
    for acts, rc in ((a, -1), (c["a"], 0)):
        ad = dev(acts)
        got_rc = f(ns, h, na, act, P(p), P(pt), P(s), P(ad), P(r), P(t), P(sn), 130, c["gamma"], None, None, 0, 1.0, P(ws), P(g), P(loss), None, None)
        torch.cuda.synchronize()
        assert got_rc == rc, lib.rlhip_last_error()
        if rc:
            assert b"3 of 130 actions" in lib.rlhip_last_error()
    note("dqn_grad_batch out-of-range action", flags=k)
