"""DuelingNetwork Q-networks on the device: rlhip_dueling_fold_f32 / rlhip_dueling_unfold_grad_f32 (csrc/dueling.hip) bit for bit
against their numpy Float32 restatement, the UNCHANGED gradient entry points on the effective vector, and rlhip.DuelingApproximator
under DQNLearner / TargetNetwork / QBasedPolicy / the checkpoint -- against fold -> oracle -> unfold (tests/dueling_ref.py).
Rings hold host-made transitions (64 slots x 8 envs, wrapped), so every reference is computable without a device.

Bars (none of them new):
  fold / unfold                     bit-exact.
  gradients, f32                    F32_GRAD_TOL of max|g| (tests/conftest.py); loss rel 1e-4, td rtol 1e-5 / atol 1e-6
                                    (tests/test_gpu_learners.py:312, tests/test_gpu_double_dqn.py:228).
  gradients, bf16                   per tensor BF16_GRAD_TOL with its bulk bars (conftest.assert_grad_close), loss 2e-5 max(1, |ref|),
                                    td relu 2e-5 (1 + ref) / tanh 5e-3 (1 + ref): tests/test_gpu_bf16_learner_matrix.py:147-152.
  learner parameters, per step      teacher-forced single updates: |dp| q99 <= 0.02 lr (two-layer) / 0.2 lr (bf16), max <= 2.5 lr --
                                    the per-step bar of the plain learner, tests/test_gpu_dqn_agent_vs_oracle.py:144 (tests/
                                    test_gpu_learners.py holds no DQNLearner loop of its own; this is the project's bar for one).
  Double DQN                        samples whose top-two gap of the online Q(s') is below 1e-5 are left out of the comparison of y (their
                                    share <= 2 %, asserted on the oracle alone); y under the Q tolerances of tests/test_gpu_double_dqn.py."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import oracle  # noqa: E402
import dueling_ref as dr  # noqa: E402
from conftest import BF16_GRAD_TOL, F32_GRAD_TOL, assert_grad_close  # noqa: E402
from double_dqn_ref import compose, forward, top_two_gap, trained_nets  # noqa: E402
from test_gpu_bench_shapes import dev, host, note  # noqa: E402

GAMMA, LR, BATCH = 0.97, 1e-3, 64
NA = {4: 2, 3: 3, 2: 3}  # obs_dim -> actions: the three (ns, na) pairs of the MFMA learners
_NETS = {}


def _nets(layers, ns, h, na, act):
    """(online, target) dueling vectors whose Q-values have separated: trained plain nets, their head as adv, a Glorot val head"""
    key = (layers, ns, h, na, act)
    if key not in _NETS:
        p, pt = trained_nets(layers, ns, h, na, act, seed=3 + ns + h + na + act, steps=150 if layers == 2 else 40, batch=128)
        rng = np.random.default_rng(h + act)
        _NETS[key] = (dr.make(ns, h, na, layers, p, rng), dr.make(ns, h, na, layers, pt, rng))
    return _NETS[key]


def _ring(rl, ns, na, seed, prioritized=False, n_env=8, cap=64):
    """64 slots x 8 envs of host-made transitions, wrapped, in a device ring and an oracle.Ring"""
    rng = np.random.default_rng(seed)
    cls = rl.CircularPrioritizedTraces if prioritized else rl.CircularArraySARTSTraces
    tr = cls(capacity=cap, n_env=n_env, obs_dim=ns)
    oring = oracle.Ring(cap, n_env, ns)
    o = rng.standard_normal((ns, n_env)).astype(np.float32)
    tr.push_state_(dev(o))
    oring.push_state(o)
    for _ in range(cap + 5):
        o = (o + 0.3 * rng.standard_normal((ns, n_env))).astype(np.float32)
        a = rng.integers(0, na, n_env).astype(np.int32)
        r = rng.standard_normal(n_env).astype(np.float32)
        t = (rng.random(n_env) < 0.1).astype(np.uint8)
        tr.push_transition_(dev(o), dev(a), dev(r), dev(t))
        oring.push_transition(o, a, r, t)
    torch.cuda.synchronize()
    assert tr.rb.head_sa != 0, "the ring has not wrapped"
    return tr, oring


def _approx(rl, layers, ns, h, na, act, d, **kw):
    return rl.DuelingApproximator(ns, h, na, act=("relu", "tanh")[act], layers=layers, dueling_params=d, lr=LR, **kw)


def _set_target(tn, dt):
    from rlhip import dqn

    net = tn.network
    tn.target_dueling.copy_(dev(dt))
    dqn.fold_dueling(tn.target_dueling, tn.target, net.n_in, net.hidden, net.n_out, net.layers)
    if net.layers == 3:
        dqn.mlp3_pack(tn.target, net.n_in, net.hidden, net.n_out, tn.target_packed)


def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------------ the two kernels, bit for bit
FOLD_CASES = [(2, 4, 1, 1), (2, 2, 5, 3), (2, 4, 64, 4), (2, 4, 128, 2), (2, 3, 256, 3)] + \
             [(3, ns, h, NA[ns]) for ns in (4, 3, 2) for h in (128, 256)]


@pytest.mark.parametrize("layers,ns,h,na", FOLD_CASES)
def test_fold_and_unfold_are_bit_exact(layers, ns, h, na):
    from rlhip import dqn

    rng = np.random.default_rng(ns * 1000 + h + na)
    n, nd = dr.plain_nparams(ns, h, na, layers), dr.nparams(ns, h, na, layers)
    assert dqn.dueling_nparams(ns, h, na, layers) == nd
    d, d2, g = (rng.standard_normal(k).astype(np.float32) for k in (nd, nd, n))
    PAD, CANARY = 8, 777.0
    for shift in (0, 1):  # 0: 16-byte aligned pointers (float4 copies and a scalar tail); 1: the element-by-element path
        def buf(k):
            t = torch.full((k + 2 * PAD,), CANARY, dtype=torch.float32, device="cuda")
            return t, t[PAD + shift:PAD + shift + k]

        def src(x):
            t = torch.zeros(x.size + 4, dtype=torch.float32, device="cuda")
            t[shift:shift + x.size] = dev(x)
            return t[shift:shift + x.size]

        (E, e), (E2, e2), (U, u) = buf(n), buf(n), buf(nd)
        D, D2, G = src(d), src(d2), src(g)
        assert (e.data_ptr() % 16 == 0) == (shift == 0)
        dqn.fold_dueling(D, e, ns, h, na, layers)
        dqn.unfold_dueling_grad(G, u, ns, h, na, layers)
        torch.cuda.synchronize()
        assert np.array_equal(_bits(host(e)), _bits(dr.fold(d, ns, h, na, layers))), f"fold differs (shift {shift})"
        assert np.array_equal(_bits(host(u)), _bits(dr.unfold(g, ns, h, na, layers))), f"unfold differs (shift {shift})"
        one = host(e).copy()
        # the two-net form equals two one-net calls
        e.fill_(CANARY)
        dqn.fold_dueling(D, e, ns, h, na, layers, duel2=D2, eff2=e2)
        torch.cuda.synchronize()
        assert np.array_equal(_bits(host(e)), _bits(one)) and np.array_equal(_bits(host(e2)), _bits(dr.fold(d2, ns, h, na, layers)))
        for whole, k in ((E, n), (E2, n), (U, nd)):  # nothing outside the outputs was written
            w = host(whole)
            assert (w[:PAD + shift] == CANARY).all() and (w[PAD + shift + k:] == CANARY).all()
        assert np.array_equal(host(D), d) and np.array_equal(host(G), g)
    if na == 1:
        o, k = dr.offsets(ns, h, na, layers)["Wadv"]
        assert not host(u)[o:o + k + na].any()  # x - x / 1


# ------------------------------------------------------------------------------------------------ one gradient, then unfold
def _per_tensor(layers, g, ref, ns, h, na, tag):
    if layers == 2:
        return assert_grad_close(g, ref, F32_GRAD_TOL, tag)
    for name, (o, n) in dr.offsets(ns, h, na, layers).items():
        assert np.abs(ref[o:o + n]).max() > 0, f"{tag} {name}: zero reference gradient"
        assert_grad_close(g[o:o + n], ref[o:o + n], BF16_GRAD_TOL, f"{tag} {name}")


@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("entry,layers,h", [("idx", 2, 128), ("idx_w", 2, 128), ("dqn3", 3, 128), ("dqn3", 3, 256)])
def test_shipped_gradient_entry_on_the_effective_vector_then_unfold(entry, layers, h, act):
    import rlhip as rl
    from rlhip import dqn
    from rlhip._lib import call
    from rlhip.ops import ptr, stream_ptr

    ns, na = 4, 2
    tr, oring = _ring(rl, ns, na, seed=11 + h + act)
    d, dt = _nets(layers, ns, h, na, act)
    net = _approx(rl, layers, ns, h, na, act, d)
    tn = rl.TargetNetwork(net)
    _set_target(tn, dt)
    idx = oring.sample_indices(BATCH, 5, 2)
    s, a, r, t, sn = oring.gather(idx)
    assert t.any() and not t.all()
    w = W = None
    if entry == "idx_w":
        w = oracle.per_is_weights(((np.random.default_rng(3).random(BATCH) + 1e-3) ** 0.6).astype(np.float32), 0.4)
        W = dev(w)
    ref_loss, ref, pe, pte = dr.composed(layers, ns, h, na, act, d, dt, s, a, r, t, sn, GAMMA, weights=w)
    assert np.array_equal(_bits(host(net.params)), _bits(pe)) and np.array_equal(_bits(host(tn.target)), _bits(pte))
    I = dev(idx)
    ws = (dqn.dqn_workspace if layers == 2 else dqn.dqn3_workspace)(ns, h, na, BATCH)
    g, loss, td = torch.empty_like(net.params), torch.empty(1, device="cuda"), torch.zeros(BATCH, device="cuda")
    if entry == "idx":
        call("rlhip_dqn_grad_idx_f32", C.byref(tr.rb), h, na, act, ptr(net.params), ptr(tn.target), BATCH, ptr(I), GAMMA, 1.0, ptr(ws),
             ptr(g), ptr(loss), ptr(td), stream_ptr())
    elif entry == "idx_w":
        call("rlhip_dqn_grad_idx_w_f32", C.byref(tr.rb), h, na, act, ptr(net.params), ptr(tn.target), BATCH, ptr(I), ptr(W), GAMMA, 1.0,
             ptr(ws), ptr(g), ptr(loss), ptr(td), stream_ptr())
    else:
        dqn.dqn3_grad(tr, h, na, act, net.params, net.packed, tn.target, tn.target_packed, BATCH, GAMMA, 1.0, 0, 0, idx=I, workspace=ws,
                      grad=g, loss=loss, td=td)
    gd = dqn.unfold_dueling_grad(g, torch.empty_like(net.dueling_params), ns, h, na, layers)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(host(gd)), _bits(dr.unfold(host(g), ns, h, na, layers)))
    gd, loss, td = host(gd), float(loss), host(td)
    qa = forward(layers, pe, ns, h, na, act, s)[a, np.arange(BATCH)]
    ref_td = np.abs(qa - (r + np.float32(GAMMA) * (1 - t.astype(np.float32)) * forward(layers, pte, ns, h, na, act, sn).max(0)))
    terr = np.abs(td - ref_td)
    print(f"{entry} layers={layers} h={h} act={act}: loss {loss:.6f} vs {ref_loss:.6f}, max|g - ref| / max|ref| = "
          f"{np.abs(gd - ref).max() / np.abs(ref).max():.2e}, max td error {terr.max():.2e}")
    if layers == 2:
        assert loss == pytest.approx(ref_loss, rel=1e-4)
        np.testing.assert_allclose(td, ref_td, rtol=1e-5, atol=1e-6)
    else:
        assert abs(loss - ref_loss) <= 2e-5 * max(1.0, abs(ref_loss))
        assert (terr / (1 + ref_td)).max() <= (2e-5 if act == 0 else 5e-3)
    _per_tensor(layers, gd, ref, ns, h, na, f"dueling {entry} h={h} act={act}")


# ------------------------------------------------------------------------------------------------ the learner
def _step_bars(layers, d_gpu, d_ref, tag):
    e = np.abs(d_gpu - d_ref)
    q99, dmax = float(np.quantile(e, 0.99)), float(e.max())
    print(f"{tag}: |dp| q99 {q99:.3e} max {dmax:.3e}")
    assert q99 <= (0.02 if layers == 2 else 0.2) * LR and dmax <= 2.5 * LR, f"{tag}: |dp| q99 {q99:.2e} max {dmax:.2e}"
    return q99, dmax


def _assert_folded(net, tn):
    """the vectors the kernels read are the folds of the trained ones, bit for bit"""
    a = (net.n_in, net.hidden, net.n_out, net.layers)
    assert np.array_equal(_bits(host(net.params)), _bits(dr.fold(host(net.dueling_params), *a)))
    assert np.array_equal(_bits(host(tn.target)), _bits(dr.fold(host(tn.target_dueling), *a)))


@pytest.mark.parametrize("rho", [0.0, 0.5])
def test_learner_ten_updates_teacher_forced_vs_oracle_loop(rho):
    """DQNLearner.optimise_ x 10 with a DuelingApproximator; before every update the host loop receives the device state (dueling
    vectors, Adam moments), then both run ONE update: ring_sample_indices -> gather -> fold -> oracle gradient -> unfold -> clip -> Adam
    on the dueling vector -> every third update polyak on the dueling vectors + fold"""
    import rlhip as rl

    layers, ns, h, na, act, K, sync = 2, 4, 128, 2, 0, 10, 3
    tr, oring = _ring(rl, ns, na, seed=31)
    traj = rl.Trajectory(tr)
    traj.controller.on_insert_(10 ** 6)
    d, dt = _nets(layers, ns, h, na, act)
    net = _approx(rl, layers, ns, h, na, act, d)
    tn = rl.TargetNetwork(net, sync_freq=sync, rho=rho)
    _set_target(tn, dt)
    learner = rl.DQNLearner(tn, batchsize=BATCH, gamma=GAMMA, min_replay_history=1, seed=5, max_grad_norm=0.5)
    assert learner.grad.numel() == dr.plain_nparams(ns, h, na, layers) and net.m.numel() == dr.nparams(ns, h, na, layers)
    n_opt, worst, clipped = 0, (0.0, 0.0), 0
    d0 = host(net.dueling_params).copy()
    for k in range(K):
        p, pt, m, v = (host(x).copy() for x in (net.dueling_params, tn.target_dueling, net.m, net.v))
        assert learner.optimise_(traj)
        torch.cuda.synchronize()
        s, a, r, t, sn = oring.gather(oring.sample_indices(BATCH, 5, k))
        ref_loss, g, _, _ = dr.composed(layers, ns, h, na, act, p, pt, s, a, r, t, sn, GAMMA)
        assert float(learner.loss) == pytest.approx(ref_loss, rel=1e-4)
        gn = oracle.clip_by_global_norm(g, 0.5)  # the global norm of the DUELING gradient
        clipped += gn > 0.5
        assert float(net.gn) == pytest.approx(gn, rel=1e-5)
        oracle.adam(p, g, m, v, LR, 0.9, 0.999, 1e-8, k + 1)
        due, n_opt = oracle.target_sync_due(n_opt, sync)
        if due:
            oracle.polyak(pt, p, rho)
        assert tn.n_optimise == n_opt
        q99, dmax = _step_bars(layers, host(net.dueling_params), p, f"update {k} (rho {rho})")
        worst = (max(worst[0], q99), max(worst[1], dmax))
        assert np.abs(host(tn.target_dueling) - pt).max() <= dmax + 1e-12
        if due and rho == 0.0:
            assert torch.equal(tn.target_dueling, net.dueling_params)
        _assert_folded(net, tn)
    assert clipped >= 1, "max_grad_norm = 0.5 never clipped: the norm over the dueling gradient is not exercised"
    assert np.median(np.abs(host(net.dueling_params) - d0)) > LR
    note("DQNLearner with a DuelingApproximator x 10, teacher-forced", rho=rho, dp_q99_worst_step=worst[0], dp_max_worst_step=worst[1])


@pytest.mark.parametrize("form,layers,h", [("double", 2, 128), ("double", 3, 128), ("nstep", 2, 128), ("per", 2, 128)])
def test_one_update_composed_with_double_dqn_nstep_and_prioritized_replay(form, layers, h):
    import rlhip as rl

    ns, na, act = 4, 2, 0
    prioritized = form == "per"
    tr, oring = _ring(rl, ns, na, seed=41 + h, prioritized=prioritized)
    traj = rl.Trajectory(tr)
    traj.controller.on_insert_(10 ** 6)
    d, dt = _nets(layers, ns, h, na, act)
    net = _approx(rl, layers, ns, h, na, act, d)
    tn = rl.TargetNetwork(net, sync_freq=1, rho=0.5)
    _set_target(tn, dt)
    kw = {"double": dict(double_dqn=True), "nstep": dict(n_step=3), "per": dict(per_beta=0.4)}[form]
    learner = rl.DQNLearner(tn, batchsize=BATCH, gamma=GAMMA, min_replay_history=1, seed=5, max_grad_norm=0.5, **kw)
    p, pt = d.copy(), dt.copy()
    m, v = np.zeros_like(p), np.zeros_like(p)
    pe, pte = dr.fold(p, ns, h, na, layers), dr.fold(pt, ns, h, na, layers)
    gamma, w, key = GAMMA, None, None
    if form == "nstep":
        idx = oracle.ring_sample_indices_nstep(oring, BATCH, 3, 5, 0)
        s, a, r, t, sn = oracle.ring_gather_nstep(oring, idx, 3, GAMMA)
        gamma = oracle.gamma_pow(GAMMA, 3)
    elif prioritized:
        st = oracle.SumTree(tr.n_leaves)
        st.tree[:] = host(tr.priorities)
        idx, key, prio = oracle.ring_sample_prioritized(oring, st, BATCH, 5, 0)
        w = oracle.per_is_weights(prio, 0.4)
        s, a, r, t, sn = oring.gather(idx)
    else:
        idx = oring.sample_indices(BATCH, 5, 0)
        s, a, r, t, sn = oring.gather(idx)
    left_out = np.zeros(BATCH, bool)
    if form == "double":  # the oracle alone: the share of samples too close to a tie of the online Q(s') is a condition on the nets
        y, astar, q, qt = compose(layers, ns, h, na, act, pe, pte, r, t, sn, gamma)
        left_out = top_two_gap(q) < 1e-5
        print(f"double layers={layers}: left out {left_out.mean():.4f}, smallest gap {top_two_gap(q).min():.3e}")
        assert left_out.mean() <= 0.02
    assert learner.optimise_(traj)
    torch.cuda.synchronize()
    if prioritized:
        assert np.array_equal(host(learner._key), key)
    if form == "double":
        assert np.array_equal(host(learner._idx), idx)
        gy = host(learner._double._folded.gather(learner._double._iota)[2])
        qtol = 2e-6 + 2e-5 * np.abs(y) if layers == 2 else 2e-5 * (1 + np.abs(y))
        assert np.all(np.abs(gy - y)[~left_out] <= qtol[~left_out]), np.abs(gy - y)[~left_out].max()
        assert np.array_equal(gy[t != 0], r[t != 0])
        y[left_out] = gy[left_out]  # a left-out sample takes the device's selection: it is not part of the comparison
        r, t = y, np.ones(BATCH, np.uint8)
    if layers == 2:
        ref_loss, g = oracle.dqn_loss_grad(ns, h, na, act, pe, pte, s, a, r, t, sn, gamma, 1.0, weights=w)
    else:
        ref_loss, g, _ = oracle.dqn3_loss_grad(ns, h, na, act, pe, pte, s, a, r, t, sn, gamma, 1.0, weights=w)
    assert abs(float(learner.loss) - ref_loss) <= (1e-4 if layers == 2 else 2e-5) * max(1.0, abs(ref_loss))
    if prioritized:  # the write-back: (|Q(s, a) - y| + eps)^alpha under the sampled keys
        tgt = r + np.float32(gamma) * (1 - t.astype(np.float32)) * forward(layers, pte, ns, h, na, act, sn).max(0)
        ref_prio = oracle.per_priority(np.abs(forward(layers, pe, ns, h, na, act, s)[a, np.arange(BATCH)] - tgt), 1e-6, 0.6)
        np.testing.assert_allclose(host(learner.td), ref_prio, rtol=1e-3, atol=1e-6)
        st.update(key, host(learner.td))  # the oracle's tree, as it stood before the update, with the device's priorities written in
        after = host(tr.priorities)
        assert np.array_equal(after[st.P:st.P + tr.n_leaves], st.tree[st.P:st.P + tr.n_leaves]), "leaves differ: other keys written"
        np.testing.assert_allclose(after, st.tree, rtol=1e-5, atol=1e-6)
    gd = dr.unfold(g, ns, h, na, layers)
    oracle.clip_by_global_norm(gd, 0.5)
    oracle.adam(p, gd, m, v, LR, 0.9, 0.999, 1e-8, 1)
    oracle.polyak(pt, p, 0.5)
    _, dmax = _step_bars(layers, host(net.dueling_params), p, f"{form} layers={layers}")
    assert np.abs(host(tn.target_dueling) - pt).max() <= dmax + 1e-12
    assert np.abs(p - d).max() > 0.5 * LR
    _assert_folded(net, tn)
    if layers == 3:  # the bf16 fragments follow the folded vectors
        from rlhip import dqn

        assert torch.equal(net.packed, dqn.mlp3_pack(net.params, ns, h, na)) and torch.equal(tn.target_packed, dqn.mlp3_pack(tn.target, ns, h, na))


@pytest.mark.parametrize("layers,h", [(2, 128), (3, 128), (3, 256)])
def test_plan_equals_the_plan_of_a_plain_network_on_the_effective_vector(layers, h):
    import rlhip as rl

    ns, na, act, n = 4, 2, 0, 256
    d, _ = _nets(layers, ns, h, na, act)
    net = _approx(rl, layers, ns, h, na, act, d)
    plain = rl.HipApproximator(ns, h, na, act="relu", params=net.params, layers=layers)
    env = rl.CartPoleEnv(n, seed=4)
    out = []
    for A in (net, plain):
        pol = rl.QBasedPolicy(rl.DQNLearner(rl.TargetNetwork(A), batchsize=BATCH), rl.EpsilonGreedyExplorer(0.0, seed=1))
        out.append((pol.plan_(env).clone(), pol._q.clone()))
    torch.cuda.synchronize()
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])
    lit = dr.literal_q(d, ns, h, na, act, host(env.state().to(torch.float32)), layers)
    assert np.abs(host(out[0][1]) - lit).max() <= (1e-5 if layers == 2 else 1e-3) * (1 + np.abs(lit).max())  # it IS the dueling Q
    x = env.state().to(torch.float32)
    assert torch.equal(net.forward(x), plain.forward(x))  # forward(A, x) is the existing forward on the effective vector


@pytest.mark.parametrize("layers", [2, 3])
def test_checkpoint_resume_is_bit_identical(tmp_path, layers):
    import rlhip as rl

    ns, h, na, act = 4, 128, 2, 0
    tr, _ = _ring(rl, ns, na, seed=51)
    traj = rl.Trajectory(tr)
    traj.controller.on_insert_(10 ** 6)
    d, dt = _nets(layers, ns, h, na, act)

    def build(vec, seed):
        net = _approx(rl, layers, ns, h, na, act, vec, seed=seed)
        tn = rl.TargetNetwork(net, sync_freq=3, rho=0.5)
        return rl.DQNLearner(tn, batchsize=BATCH, gamma=GAMMA, min_replay_history=1, seed=seed, max_grad_norm=0.5)

    whole, first = build(d, 5), build(d, 5)
    for L in (whole, first):
        _set_target(L.approximator, dt)
    for _ in range(10):
        assert whole.optimise_(traj)
    for _ in range(5):
        assert first.optimise_(traj)
    path = str(tmp_path / "ck.npz")
    rl.save_checkpoint(path, first)
    with np.load(path) as z:
        assert {"approximator/network/dueling_params", "approximator/target_dueling", "approximator/network/params",
                "approximator/target"} <= set(z.files) and not [k for k in z.files if "/_grad" in k]
        assert z["approximator/network/m"].shape == (dr.nparams(ns, h, na, layers),)
    second = build(np.zeros_like(d), 99)  # fresh objects: other weights, other seed
    rl.load_checkpoint(path, second)
    for _ in range(5):
        assert second.optimise_(traj)
    torch.cuda.synchronize()
    a, b = rl.state_dict(whole), rl.state_dict(second)
    assert set(a) == set(b)
    for k in a:
        if "workspace" in k or k == "grad":
            continue  # scratch
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k
    assert whole.n_updates == second.n_updates == 10 and not np.array_equal(a["approximator/network/dueling_params"], d)
