"""Dueling distributional heads on the device (csrc/dist_dueling.hip, the dueling entry points of csrc/noisy.hip) against the models of
tests/dist_dueling_ref.py.

  fold / unfold      bit for bit the Float32 replay: both nets in one launch, pointers 4 bytes behind a 16-byte boundary, the refusals
  fold -> forward    rlhip_c51_forward_f32 / rlhip_qrdqn_forward_f32 on the folded vector against the float64 dueling model
  gradient           fold -> rlhip_c51_grad_batch_f32 -> unfold against float64 autograd with respect to the dueling vector; a* equal
  noisy forward/plan logits, probabilities, Q against the float64 model fed the replayed draws; actions = the selection kernel on q_out
  fused noisy folds  byte for byte the two-launch compositions, both tags, counter 0 and 2^32 - 1
  learner            three teacher-forced updates of RainbowLearner over each new approximator, the Adam bars of tests/test_gpu_c51_learner.py
Bars: the FLOOR is the Float32 replay's own distance from the float64 model on the same shape (the largest over the shape's cases,
never below u = 2^-24), relative to max|l| / max|g|; the kernel's bar is 4 x floor.  Measured (profiles/dist_dueling.md), gradient,
floor -> the worst kernel case: (2,4,1,2) 4.6e-7 -> 6.5e-7, (3,8,3,5) 1.3e-7 -> 2.6e-7, (4,128,2,51) 7.2e-7 -> 7.2e-7, (4,256,4,51)
1.6e-6 -> 1.6e-6; every test prints its figures before it asserts."""
import numpy as np
import pytest
import torch

import c51_ref as C
import dist_dueling_ref as D
import noisy_ref as N
import oracle
from heads_ref import F32
from test_gpu_bench_shapes import host
from test_gpu_noisy import SEED, U, _dev

pytestmark = pytest.mark.gpu
GRAD_CASES = [(b, dbl, ex) for b in (8, 24) for dbl in (False, True) for ex in (False, True)]
_FLOOR = {}


def _rl():
    import rlhip as rl

    return rl


def grad_floor(shape):
    """the replay's distance from the float64 model over the shape's gradient cases (computed once per shape); the gaps hold"""
    if shape not in _FLOOR:
        cases = {k: D.case(*shape, *k) for k in GRAD_CASES}
        models = {k: D.torch_model(c) for k, c in cases.items()}
        assert min(m["gap"] for m in models.values()) > 1e-3
        _FLOOR[shape] = (max(max(C.rel(D.replay_grad(cases[k])[0], models[k]["grad"]) for k in GRAD_CASES), U), cases, models)
    return _FLOOR[shape]


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("shape", D.SHAPES)
def test_fold_and_unfold_bit_for_bit(shape, offset):
    ops, (ns, h, na, K) = _rl().ops, shape
    rng = np.random.default_rng(sum(shape))
    nd, ne = C.nparams(ns, h, (1 + na) * K), C.nparams(ns, h, na * K)
    duel, duel2, g = rng.normal(0, 0.5, nd).astype(F32), rng.normal(0, 0.5, nd).astype(F32), rng.normal(0, 0.5, ne).astype(F32)
    eff, eff2 = (_dev(np.full(ne, np.nan), offset=offset) for _ in range(2))
    ops.dist_dueling_fold(_dev(duel, offset=offset), eff, *shape, _dev(duel2, offset=offset), eff2)
    assert np.array_equal(host(eff), D.fold(duel, *shape)) and np.array_equal(host(eff2), D.fold(duel2, *shape))
    single = ops.dist_dueling_fold(_dev(duel2, offset=offset), _dev(np.full(ne, np.nan), offset=1 - offset), *shape)
    assert torch.equal(single, eff2)
    gd = ops.dist_dueling_unfold_grad(_dev(g, offset=offset), _dev(np.full(nd, np.nan), offset=offset), *shape)
    assert np.array_equal(host(gd), D.unfold(g, *shape))


def test_the_fold_refuses_the_shape_beyond_256_rows_and_overlapping_vectors():
    rl = _rl()
    buf = torch.zeros(40000, device="cuda")
    with pytest.raises(rl.RLHipArgumentError, match="at most 256 rows"):  # (every other entry point: tests/test_dist_dueling_reference.py)
        rl.ops.dist_dueling_fold(buf, buf[20000:], *D.REFUSED)
    with pytest.raises(rl.RLHipArgumentError, match="overlap"):
        rl.ops.dist_dueling_fold(buf, buf[8:], 2, 4, 1, 2)  # eff inside the dueling vector's 32 floats
    with pytest.raises(rl.RLHipArgumentError, match="overlap"):
        rl.ops.dist_dueling_fold(buf, buf[100:], 2, 4, 1, 2, buf[200:], buf[110:])  # eff2 inside eff


def _close(name, got, r64, r32, floor_min=U):
    scale = np.abs(r64).max()
    floor = max(np.abs(np.asarray(r32, np.float64) - r64).max() / scale, floor_min)
    err = np.abs(host(got).astype(np.float64) - r64).max() / scale
    print(f"{name}: floor {floor:.3e}, kernel {err:.3e} of max = {scale:.3g}")
    assert err <= 4 * floor, name


@pytest.mark.parametrize("shape", D.SHAPES)
def test_fold_then_forward_against_the_float64_dueling_model(shape):
    rl, (ns, h, na, K) = _rl(), shape
    rng = np.random.default_rng(7 + sum(shape))
    duel, obs = rng.normal(0, 0.4, C.nparams(ns, h, (1 + na) * K)).astype(F32), rng.normal(0, 1, (ns, 19)).astype(F32)
    eff = rl.ops.dist_dueling_fold(_dev(duel), torch.empty(C.nparams(ns, h, na * K), device="cuda"), *shape)
    quiet = np.concatenate([duel, np.zeros_like(duel)])  # sigma = 0: the noisy model is the plain dueling network
    r64, r32 = (D.noisy_forward(quiet, ns, h, na, K, 0, obs, 0, 0, 0, dtype=t) for t in (np.float64, F32))
    rows = torch.empty((na * K, 19), device="cuda")
    qq = rl.qrdqn_forward(eff, ns, h, na, K, 0, _dev(obs), quantiles=rows)
    _close(f"qrdqn rows {shape}", rows, r64[0], r32[0])
    _close(f"qrdqn q {shape}", qq, r64[0].reshape(na, K, -1).mean(1), r32[0].reshape(na, K, -1).mean(1))
    if K >= 2:
        probs = torch.empty_like(rows)
        q = rl.c51_forward(eff, ns, h, na, K, 0, D.V_MIN, D.V_MAX, _dev(obs), probs=probs, logits=rows)
        for name, got, a, b in zip(("logits", "probs", "q"), (rows, probs, q), r64, r32):
            _close(f"c51 {name} {shape}", got, a, b)


@pytest.mark.parametrize("batch,double,extras", GRAD_CASES)
@pytest.mark.parametrize("shape", D.SHAPES)
def test_the_gradient_against_float64_autograd_of_the_dueling_loss(shape, batch, double, extras):
    rl, (ns, h, na, K) = _rl(), shape
    floor, cases, models = grad_floor(shape)
    c, m = cases[batch, double, extras], models[batch, double, extras]
    ne = C.nparams(ns, h, na * K)
    eff, eff_t = (torch.empty(ne, device="cuda") for _ in range(2))
    rl.ops.dist_dueling_fold(_dev(c["duel"]), eff, *shape, _dev(c["duel_t"]), eff_t)
    sel = torch.empty(batch, dtype=torch.int32, device="cuda")
    g_eff, loss = rl.c51_grad_batch(ns, h, na, K, c["act"], D.V_MIN, D.V_MAX, eff, eff_t, _dev(c["s"]), _dev(c["a"], np.int32), _dev(c["r"]),
                                    _dev(c["term"], np.uint8), _dev(c["sn"]), c["gamma"], None if c["n_used"] is None else _dev(c["n_used"], np.int32),
                                    None if c["weights"] is None else _dev(c["weights"]), double, sel=sel)
    g = rl.ops.dist_dueling_unfold_grad(g_eff, torch.empty(c["duel"].size, device="cuda"), *shape)
    err = C.rel(host(g), m["grad"])
    print(f"dueling gradient {shape} b{batch} double={double} extras={extras}: floor {floor:.3e}, kernel {err:.3e} of max|g|")
    assert np.array_equal(host(sel), m["sel"]), "a*"
    assert err <= 4 * floor and abs(float(loss) - m["loss"]) <= 1e-6 * max(1.0, abs(m["loss"]))


@pytest.mark.parametrize("n_of", [lambda t: 1, lambda t: t, lambda t: t + 1], ids=["one", "tile", "tile+1"])
@pytest.mark.parametrize("shape", D.SHAPES)
def test_the_per_env_noisy_dueling_forward_and_plan(shape, n_of):
    rl, (ns, h, na, K) = _rl(), shape
    n, M, rows, step, base = n_of(rl.noisy_plan_tile()), na * K, (1 + na) * K, 11, 2 ** 32 - 3
    rng = np.random.default_rng(n + sum(shape))
    noisy = host(rl.noisy_init(ns, h, rows, seed=3, sigma0=0.5)) + rng.normal(0, 0.05, 2 * C.nparams(ns, h, rows)).astype(F32)
    obs = rng.normal(0, 1, (ns, n)).astype(F32)
    args = (_dev(noisy), ns, h, na, K, 0, D.V_MIN, D.V_MAX, _dev(obs))
    logits, probs = (torch.empty((M, n), device="cuda") for _ in range(2))
    q = rl.noisy_c51_dueling_forward(*args, SEED, base, step, probs=probs, logits=logits)
    r64, r32 = (D.noisy_forward(noisy, ns, h, na, K, 0, obs, SEED, base, step, dtype=t) for t in (np.float64, F32))
    for name, got, a, b in zip(("logits", "probs", "q"), (logits, probs, q), r64, r32):
        _close(f"noisy dueling {name} {shape} n={n}", got, a, b)
    for eps in (0.0, 0.5):
        actions, qp = rl.noisy_c51_dueling_plan(*args, eps, SEED, base, step)
        assert torch.equal(qp, q) and torch.equal(actions, rl.ops.eps_greedy_select(qp, eps, SEED, step, base))
    # sigma = 0 and no advantage: every action's Q is the value head's Q, which is C51 on the value rows alone
    np_ = C.nparams(ns, h, rows)
    head = noisy[:np_].copy()
    D._head(head, ns, h, rows)[:, :M] = 0
    qv = rl.noisy_c51_dueling_forward(_dev(np.concatenate([head, np.zeros(np_, F32)])), *args[1:], SEED, base, step)
    val = np.concatenate([head[:h * ns + h], D._head(head, ns, h, rows)[:, M:].ravel()])
    want = rl.c51_forward(_dev(val), ns, h, 1, K, 0, D.V_MIN, D.V_MAX, args[-1])
    assert torch.equal(qv, want.expand(na, n))


@pytest.mark.parametrize("counter", [0, 2 ** 32 - 1])
@pytest.mark.parametrize("shape", D.SHAPES)
def test_the_fused_noisy_folds_are_the_two_launch_compositions(shape, counter):
    ops, (ns, h, na, K) = _rl().ops, shape
    rows, rng = (1 + na) * K, np.random.default_rng(counter % 97 + sum(shape))
    nd, ne = C.nparams(ns, h, rows), C.nparams(ns, h, na * K)
    noisy, noisy2, g = (_dev(rng.normal(0, 0.5, k).astype(F32), offset=1) for k in (2 * nd, 2 * nd, ne))
    mid, mid2, gmid = (torch.empty(nd, device="cuda") for _ in range(3))
    eff, eff2, fe, fe2 = (torch.full((ne,), np.nan, device="cuda") for _ in range(4))
    ops.noisy_fold(noisy, mid, ns, h, rows, SEED, counter, noisy2, mid2)  # tag 13 for the first pair, 14 for the second
    ops.dist_dueling_fold(mid, eff, *shape, mid2, eff2)
    ops.noisy_dueling_fold(noisy, fe, *shape, SEED, counter, noisy2, fe2)
    assert torch.equal(fe, eff) and torch.equal(fe2, eff2) and not torch.equal(eff, eff2)
    want, got = torch.empty(2 * nd, device="cuda"), torch.full((2 * nd,), np.nan, device="cuda")
    ops.noisy_unfold_grad(ops.dist_dueling_unfold_grad(g, gmid, *shape), want, ns, h, rows, SEED, counter)
    assert torch.equal(ops.noisy_dueling_unfold_grad(g, got, *shape, SEED, counter), want)


@pytest.mark.parametrize("form", [dict(), dict(per=True, per_beta=0.4, n_step=3, double_dqn=True)], ids=["uniform", "per-nstep3-double"])
@pytest.mark.parametrize("kind", ["dueling", "noisy-dueling", "noisy-dueling-two-launch", "qrdqn-dueling"])
def test_three_teacher_forced_updates_of_the_learners(kind, form):
    from test_gpu_c51_learner import CAP, N_ENV, PUSHES, _fill

    rl, form = _rl(), dict(form)
    ns, h, na, K, b, lr, gamma, seed = 4, 20, 3, 51, 33, 1e-3, 0.9, 11
    per, n_step, noisy = form.pop("per", False), form.get("n_step", 1), kind.startswith("noisy")
    if noisy:
        net = rl.NoisyDuelingApproximator(ns, h, na, K, lr=lr, seed=seed, fused=kind == "noisy-dueling")
    else:
        net = rl.DistDuelingApproximator(ns, h, na, K, lr=lr, seed=seed)
    tn = rl.TargetNetwork(net, sync_freq=2)
    if kind == "qrdqn-dueling":
        learner = rl.QRDQNLearner(tn, na, n_quantiles=K, batchsize=b, gamma=gamma, min_replay_history=N_ENV, seed=seed, **form)
    else:
        learner = rl.RainbowLearner(tn, na, n_atoms=K, v_min=D.V_MIN, v_max=D.V_MAX, batchsize=b, gamma=gamma, min_replay_history=N_ENV, seed=seed,
                                    **form)
    tr = rl.CircularPrioritizedTraces(CAP, N_ENV, ns, n_step=n_step, default_priority=2.0) if per else rl.CircularArraySARTSTraces(CAP, N_ENV, ns)
    traj = rl.Trajectory(_fill(tr, ns, np.random.default_rng(4242)), controller=rl.InsertSampleRatioController(ratio=1e9, threshold=1, n_inserted=PUSHES))
    trained, target = ("noisy_params", "target_noisy") if noisy else ("dueling_params", "target_dueling")
    shape, rows = (ns, h, na, K), (1 + na) * K
    for u in range(3):
        p0, t0, m, v = (host(x).copy() for x in (getattr(net, trained), getattr(tn, target), net.m, net.v))
        assert learner.optimise_(traj) is True and learner.n_updates == u + 1
        if kind == "qrdqn-dueling":  # the quantile loss has its own judges: here the unfold of the learner's gradient and a moving vector
            assert np.array_equal(host(net._grad.t), D.unfold(host(learner.grad), *shape)) and not np.array_equal(host(net.dueling_params), p0)
            continue
        s, a, r, t, sn, _ = (None if x is None else host(x) for x in learner._batch.t)
        fold = lambda p, tag: D.fold(N.fold(p, N.xi(seed, u, tag, ns, h, rows)).astype(F32) if noisy else p, *shape)  # noqa: E731
        c = dict(ns=ns, h=h, na=na, n_atoms=K, act=net.act, batch=b, v_min=D.V_MIN, v_max=D.V_MAX, params=fold(p0, N.TAG_ONLINE),
                 target=fold(t0, N.TAG_TARGET), s=s, sn=sn, a=a, r=r, term=t, n_used=None, weights=host(learner.is_weights).copy() if per else None,
                 double=learner.double_dqn, gamma=float(C.gamma_pow(gamma, n_step)))
        g = D.replay_grad(c)[0]
        if noisy:
            g = N.unfold(g, N.xi(seed, u, N.TAG_ONLINE, ns, h, rows)).astype(F32)
        pm = p0.copy()
        oracle.adam(pm, g, m, v, lr, 0.9, 0.999, 1e-8, u + 1)
        d = np.abs(host(getattr(net, trained)) - pm)
        q99, dmax = float(np.quantile(d, 0.99)), float(d.max())
        print(f"{kind} update {u}: |dp| q99 {q99:.2e} max {dmax:.2e}")
        assert q99 <= 0.02 * lr + 1e-7 and dmax <= 2.5 * lr + 1e-7
        assert np.array_equal(host(getattr(tn, target)), host(getattr(net, trained)) if (u + 1) % 2 == 0 else t0)
