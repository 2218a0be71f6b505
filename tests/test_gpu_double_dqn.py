"""Double DQN on the device: rlhip_dqn_fold_double_f32 / rlhip_dqn3_fold_double_f32 (csrc/dqn_double.hip), the unchanged gradient
entry points on the folded ring, and DQNLearner(double_dqn=True) -- against the target composed from the oracle's own functions
(tests/double_dqn_ref.py).  Rings are filled through the push ABI from real env steps.

Bars (none of them new):
  Q tolerance, f32   |x - ref| <= 2e-6 + 2e-5 |ref|: the q_out comparison of the plan kernels, tests/test_gpu_f32_learner_matrix.py:347
  Q tolerance, bf16  |x - ref| / (1 + |ref|) <= 2e-5 (relu: every sample; tanh: >= 99.9 % of them, max 5e-3): tests/test_gpu_dqn3.py:23-28
  a* must agree wherever the oracle's top-two gap of Q(s') exceeds four times that tolerance; the share of samples below that gap is a
  CONDITION on the test's nets and batches (<= 1 % f32, <= 5 % bf16), asserted on the oracle alone before the GPU is looked at.
  Gradients: F32_GRAD_TOL / BF16_GRAD_TOL per tensor (tests/conftest.py); td_out: the bars of the explicit-index tests
  (test_gpu_f32_learner_matrix.py:293; three-layer, relu and tanh alike, EVERY sample within 1e-4 (1 + ref): test_gpu_dqn3.py:142);
  learner parameters: tests/test_gpu_dqn_agent_vs_oracle.py:82-84."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import oracle  # noqa: E402
from conftest import BF16_GRAD_TOL, F32_GRAD_TOL, assert_grad_close  # noqa: E402
from double_dqn_ref import compose, forward, loss_grad, top_two_gap, trained_nets  # noqa: E402
from test_gpu_bench_shapes import dev, host, note  # noqa: E402

ENV = {4: ("cartpole", 2), 3: ("pendulum", 3), 2: ("mountaincar", 3)}  # obs_dim -> (env, its number of discrete actions)
GAMMA = 0.97
_NETS = {}


def _nets(layers, ns, h, na, act):
    key = (layers, ns, h, na, act)
    if key not in _NETS:
        _NETS[key] = trained_nets(layers, ns, h, na, act, seed=7 + ns + h + na + act, steps=300 if layers == 2 else 120)
    return _NETS[key]


def _filled(rl, ns, n_env=96, cap=24, pushes=40, seed=0, prioritized=False):
    """a wrapped ring (pushes > capacity) of real transitions under uniformly random actions, mirrored into an oracle ring"""
    name, na_env = ENV[ns]
    kw = {} if name == "cartpole" else {"max_steps": 11}  # short episodes: terminal transitions in every ring
    env = rl.HipVecEnv(name, n_env, continuous=False, seed=seed + 1, **kw)
    cls = rl.CircularPrioritizedTraces if prioritized else rl.CircularArraySARTSTraces
    tr = cls(capacity=cap, n_env=n_env, obs_dim=ns)
    oring = oracle.Ring(cap, n_env, ns)
    g = torch.Generator(device="cpu").manual_seed(seed)
    obs = env.state().to(torch.float32)
    tr.push_state_(obs)
    oring.push_state(host(obs))
    for _ in range(pushes):
        a0 = torch.randint(0, na_env, (n_env,), generator=g, dtype=torch.int32).cuda()
        env.act0_(a0)
        nobs, r, t = env.state().to(torch.float32), env.reward().to(torch.float32), env._done
        tr.push_transition_(nobs, a0, r, t)
        oring.push_transition(host(nobs), host(a0), host(r), host(t))
    torch.cuda.synchronize()
    return tr, oring


def _qtol(layers, ref):
    return 2e-6 + 2e-5 * np.abs(ref) if layers == 2 else 2e-5 * (1 + np.abs(ref))


def _assert_within(layers, act, x, ref, what):
    err = np.abs(x - ref) / _qtol(layers, ref)
    print(f"{what}: max |x - ref| / tol = {err.max():.3f}, share within = {(err <= 1).mean():.5f}")
    if layers == 2 or act == 0:
        assert err.max() <= 1.0, f"{what}: {err.max():.3f} x the Q tolerance"
    else:  # the tanh bar of the bf16 forward: test_gpu_dqn3.py:28
        assert (err <= 1).mean() >= 0.999 and (np.abs(x - ref) / (1 + np.abs(ref))).max() <= 5e-3, what


def _index_revealing_target(layers, ns, h, na):
    """a target net with Qt(s') = (1, 2, .., na) for every s': y = r + gamma * (a* + 1) reads the GPU's a* off exactly"""
    n = oracle.mlp2_nparams(ns, h, na) if layers == 2 else oracle.mlp3_nparams(ns, h, na)
    p = np.zeros(n, np.float32)
    p[-na:] = np.arange(1, na + 1, dtype=np.float32)
    return p


def _fold(rl, tr, idx, layers, ns, h, na, act, p, pt, gamma, fold=None, in_place=False):
    from rlhip import dqn

    net = rl.HipApproximator(ns, h, na, act=("relu", "tanh")[act], params=p, layers=layers)
    dpt = dev(pt)
    ptk = dqn.mlp3_pack(dpt, ns, h, na) if layers == 3 else None
    fold = fold or rl.DoubleTargetFold()
    folded, iota = fold.fold(tr, None if in_place else idx, net, dpt, ptk, gamma, in_place=in_place)
    torch.cuda.synchronize()
    return folded, iota, net, dpt, ptk


CASES2 = [(4, 0, 64, 2, 32), (4, 1, 100, 4, 333), (4, 0, 256, 2, 4096), (3, 1, 64, 3, 4096), (3, 0, 100, 4, 32), (3, 1, 256, 3, 333),
          (2, 0, 256, 3, 333), (2, 1, 100, 4, 4096), (2, 0, 64, 3, 32), (4, 1, 256, 3, 4096)]
CASES3 = [(4, 0, 128, 2, 333), (4, 1, 128, 2, 4096), (4, 0, 256, 2, 4096), (3, 0, 128, 3, 32), (3, 1, 256, 3, 333), (2, 0, 128, 3, 4096),
          (2, 1, 256, 3, 32), (2, 0, 256, 3, 333)]


@pytest.mark.parametrize("layers,ns,act,h,na,batch", [(2,) + c for c in CASES2] + [(3,) + c for c in CASES3])
def test_fold_double_vs_composed_oracle(layers, ns, act, h, na, batch):
    import rlhip as rl

    tr, oring = _filled(rl, ns, seed=ns + h)
    assert tr.rb.head_sa != 0, "the ring has not wrapped"
    p, pt = _nets(layers, ns, h, na, act)
    idx = oring.sample_indices(batch, 11, 3)
    s, a, r, t, sn = oring.gather(idx)
    assert t.any() and not t.all()
    # the oracle alone: the share of samples too close to a tie to pin a* is a condition on this test's nets and batches
    y, astar, q, qt = compose(layers, ns, h, na, act, p, pt, r, t, sn, GAMMA)
    decisive = top_two_gap(q) > 4 * _qtol(layers, q).max(0)
    left_out = 1.0 - decisive.mean()
    print(f"layers={layers} ns={ns} act={act} h={h} na={na} batch={batch}: left out {left_out:.4f}")
    assert left_out <= (0.01 if layers == 2 else 0.05), f"{left_out:.4f} of the samples sit within 4 x the Q tolerance of a tie"
    didx = dev(idx)
    folded, iota, *_ = _fold(rl, tr, didx, layers, ns, h, na, act, p, pt, GAMMA)
    # stored fields: s, a, s' and terminal = 1 bit for bit, iota, zero pads
    gs, ga, gy, gt, gsn = (host(x) for x in folded.gather(iota))
    assert np.array_equal(host(iota), np.arange(batch)) and len(folded) == 1 and folded.n_env == batch
    assert np.array_equal(gs.view(np.uint32), s.view(np.uint32)) and np.array_equal(gsn.view(np.uint32), sn.view(np.uint32))
    assert np.array_equal(ga, a) and np.array_equal(gt, np.ones(batch, np.uint8))
    rec = folded.records.view(torch.int32)[0]
    assert int(rec[:, 6].min()) == 1 and int(rec[:, 6].max()) == 1 and int(rec[:, 7].abs().max()) == 0 and int(rec[:, 12:].abs().max()) == 0
    assert int(rec[:, ns:4].abs().max() if ns < 4 else 0) == 0
    # the target
    assert np.array_equal(gy[t != 0], r[t != 0]), "a terminal sample must give y = r exactly"
    _assert_within(layers, act, gy[decisive], y[decisive], "y on the decisive samples")
    # the selection, read off exactly through a target net whose values are the action numbers
    prev = _index_revealing_target(layers, ns, h, na)
    folded2, iota2, *_ = _fold(rl, tr, didx, layers, ns, h, na, act, p, prev, 1.0)
    gy2 = host(folded2.gather(iota2)[2])
    live = t == 0
    gstar = np.rint(gy2 - r).astype(np.int64) - 1
    assert np.all(np.abs((gy2 - r)[live] - (gstar[live] + 1)) < 1e-3) and np.array_equal(gy2[~live], r[~live])
    both = decisive & live
    assert np.array_equal(gstar[both], astar[both]), f"{int((gstar[both] != astar[both]).sum())} decisive selections differ"
    note("double DQN fold vs composed oracle", layers=layers, ns=ns, act=act, h=h, na=na, batch=batch, left_out=float(left_out),
         selections_differing_anywhere=int((gstar[live] != astar[live]).sum()))


@pytest.mark.parametrize("layers,h", [(2, 128), (3, 128), (3, 256)])
def test_fold_double_in_place_on_an_nstep_ring(layers, h):
    import rlhip as rl

    ns, na, act, n_step, batch = 4, 2, 0, 3, 1000
    tr, oring = _filled(rl, ns, seed=5)
    p, pt = _nets(layers, ns, h, na, act)
    smp = rl.NStepBatchSampler(n_step, GAMMA, batch, seed=3)
    idx = smp.sample_indices(tr, 2)
    nfold, niota = smp.fold(tr, idx)
    s, a, R, t, sn = oracle.ring_gather_nstep(oring, host(idx), n_step, GAMMA)
    gn = oracle.gamma_pow(GAMMA, n_step)
    assert smp.gamma_n == gn
    y, astar, q, qt = compose(layers, ns, h, na, act, p, pt, R, t, sn, gn)
    decisive = top_two_gap(q) > 4 * _qtol(layers, q).max(0)
    assert 1.0 - decisive.mean() <= (0.01 if layers == 2 else 0.05)
    out, oiota, *_ = _fold(rl, nfold, niota, layers, ns, h, na, act, p, pt, gn)                  # into a ring of its own
    ref = [host(x).copy() for x in out.gather(oiota)]
    same, siota, *_ = _fold(rl, nfold, niota, layers, ns, h, na, act, p, pt, gn, in_place=True)  # ... and in place
    assert same is nfold and np.array_equal(host(siota), np.arange(batch)) and np.array_equal(host(niota), np.arange(batch))
    assert len(nfold) == 1
    with pytest.raises(ValueError):  # the in-place form walks the ring's own records: it takes no indices
        rl.DoubleTargetFold().fold(nfold, niota.flip(0), rl.HipApproximator(ns, h, na, params=p, layers=layers), dev(pt), None, gn,
                                   in_place=True)
    got = [host(x) for x in nfold.gather(niota)]
    for g, o in zip(got, ref):
        assert np.array_equal(g.view(np.uint8), o.view(np.uint8))
    assert np.array_equal(got[0], s) and np.array_equal(got[1], a) and np.array_equal(got[4], sn) and got[3].all()
    assert np.array_equal(got[2][t != 0], R[t != 0])
    _assert_within(layers, act, got[2][decisive], y[decisive], "in-place n-step y")


def _per_tensor(layers, g, og, ns, h, na, tag):
    if layers == 2:
        return assert_grad_close(g, og, F32_GRAD_TOL, tag)
    o = 0
    for name, n in (("W1", h * ns), ("b1", h), ("W2", h * h), ("b2", h), ("W3", na * h), ("b3", na)):
        assert_grad_close(g[o:o + n], og[o:o + n], BF16_GRAD_TOL, f"{tag} {name}")
        o += n


@pytest.mark.parametrize("layers,ns,h,na,act,weighted", [(2, 4, 128, 2, 0, False), (2, 3, 100, 3, 1, True), (2, 2, 256, 4, 0, True),
                                                         (3, 4, 128, 2, 0, False), (3, 4, 256, 2, 0, True), (3, 3, 128, 3, 1, False)])
def test_unchanged_gradient_kernels_on_the_folded_ring(layers, ns, h, na, act, weighted):
    """the GPU's own folded y into oracle.dqn[3]_loss_grad(reward = y, terminal = 1) against the shipped gradient entry points"""
    import rlhip as rl
    from rlhip import dqn
    from rlhip._lib import call
    from rlhip.ops import ptr, stream_ptr

    batch = 1000
    tr, oring = _filled(rl, ns, seed=21 + ns)
    p, pt = _nets(layers, ns, h, na, act)
    idx = oring.sample_indices(batch, 5, 1)
    folded, iota, net, dpt, ptk = _fold(rl, tr, dev(idx), layers, ns, h, na, act, p, pt, GAMMA)
    s, a, y, t1, sn = (host(x) for x in folded.gather(iota))
    w = W = None
    if weighted:
        w = oracle.per_is_weights(((np.random.default_rng(3).random(batch) + 1e-3) ** 0.6).astype(np.float32), 0.4)
        W = dev(w)
    ol, og = loss_grad(layers, ns, h, na, act, p, pt, s, a, y, sn, GAMMA, weights=w)
    outs = []
    for gamma in (GAMMA, 0.0):  # terminal = 1: the discount handed to the gradient call cannot reach a single bit
        ws = (dqn.dqn_workspace if layers == 2 else dqn.dqn3_workspace)(ns, h, na, batch)
        g, loss, td = torch.empty_like(net.params), torch.empty(1, device="cuda"), torch.zeros(batch, device="cuda")
        if layers == 2 and not weighted:
            call("rlhip_dqn_grad_idx_f32", C.byref(folded.rb), h, na, act, ptr(net.params), ptr(dpt), batch, ptr(iota), gamma, 1.0,
                 ptr(ws), ptr(g), ptr(loss), ptr(td), stream_ptr())
        elif layers == 2:
            call("rlhip_dqn_grad_idx_w_f32", C.byref(folded.rb), h, na, act, ptr(net.params), ptr(dpt), batch, ptr(iota), ptr(W), gamma,
                 1.0, ptr(ws), ptr(g), ptr(loss), ptr(td), stream_ptr())
        elif not weighted:
            dqn.dqn3_grad(folded, h, na, act, net.params, net.packed, dpt, ptk, batch, gamma, 1.0, 0, 0, idx=iota, workspace=ws, grad=g,
                          loss=loss, td=td)
        else:
            call("rlhip_dqn3_grad_w_f32", C.byref(folded.rb), h, na, act, ptr(net.params), ptr(net.packed), ptr(dpt), ptr(ptk), batch,
                 ptr(iota), ptr(W), gamma, 1.0, ptr(ws), ptr(g), ptr(loss), ptr(td), stream_ptr())
        torch.cuda.synchronize()
        outs.append((host(g), float(loss), host(td)))
    (g, loss, td), (g0, loss0, td0) = outs
    assert np.array_equal(g, g0) and loss == loss0 and np.array_equal(td, td0)
    assert abs(loss - ol) <= (1e-4 if layers == 2 else 2e-5) * max(1.0, abs(ol))
    _per_tensor(layers, g, og, ns, h, na, f"gradient on the folded ring, layers={layers} h={h}")
    qa = forward(layers, p, ns, h, na, act, s)[a, np.arange(batch)]
    ref_td = np.abs(qa - y)
    if layers == 2:
        np.testing.assert_allclose(td, ref_td, rtol=1e-5, atol=1e-6)
    else:
        terr = np.abs(td - ref_td) / (1 + ref_td)
        print(f"td_out layers=3 h={h} act={act}: max |td - ref| / (1 + ref) = {terr.max():.3e}, share within 1e-4 = {(terr <= 1e-4).mean():.5f}")
        assert np.all(terr <= 1e-4), terr.max()  # every sample, relu and tanh alike: test_gpu_dqn3.py:142


@pytest.mark.parametrize("act", [0, 1])
def test_folded_target_passes_the_target_line_bit_exactly(act):
    """online = target, hidden 256: the wide plan kernel and the gradient kernel sum Q(s) in the same order, so |q_out[a] - y|
    recomputed on the host from the plan kernel's q_out must equal td_out bit for bit -- y reached the Huber line unchanged"""
    import rlhip as rl
    from rlhip import dqn
    from rlhip._lib import call
    from rlhip.ops import ptr, stream_ptr

    ns, h, na, batch = 4, 256, 2, 2048
    tr, oring = _filled(rl, ns, seed=9)
    p, _ = _nets(2, ns, h, na, act)
    idx = oring.sample_indices(batch, 2, 0)
    folded, iota, net, dpt, _ = _fold(rl, tr, dev(idx), 2, ns, h, na, act, p, p, GAMMA)
    s, a, y, _, _ = folded.gather(iota)
    _, q = dqn.dqn_plan(net.params, ns, h, na, act, s.contiguous(), 0.0, 0, 0, 0)
    ws = dqn.dqn_workspace(ns, h, na, batch)
    g, loss, td = torch.empty_like(net.params), torch.empty(1, device="cuda"), torch.zeros(batch, device="cuda")
    call("rlhip_dqn_grad_idx_f32", C.byref(folded.rb), h, na, act, ptr(net.params), ptr(dpt), batch, ptr(iota), GAMMA, 1.0, ptr(ws),
         ptr(g), ptr(loss), ptr(td), stream_ptr())
    torch.cuda.synchronize()
    qa = host(q)[host(a), np.arange(batch)]
    assert np.array_equal(host(td).view(np.uint32), np.abs(qa - host(y)).astype(np.float32).view(np.uint32))


def _learner(rl, layers, h, seed, prioritized=False, **kw):
    net = rl.HipApproximator(4, h, 2, seed=seed, layers=layers)
    tn = rl.TargetNetwork(net, sync_freq=4)
    return rl.DQNLearner(tn, batchsize=256, gamma=GAMMA, min_replay_history=1, seed=seed, max_grad_norm=0.5, **kw), tn, net


@pytest.mark.parametrize("form,layers,h", [("uniform", 2, 128), ("nstep", 2, 128), ("per", 2, 128), ("uniform", 3, 128), ("per", 3, 256),
                                           ("per0", 2, 128), ("per0", 3, 128)])
def test_learner_ten_updates_vs_oracle_loop(form, layers, h):
    """DQNLearner(double_dqn=True).optimise_ x 10 against compose -> clip -> adam -> sync from the oracle's functions; the drawn
    indices (and keys) bit-exact at every update.  "per0" is prioritized replay without importance weights (per_beta = 0, the default):
    the unweighted `_idx` entry on the folded ring, priorities still written back under the original keys"""
    import rlhip as rl

    ns, na, act, K, lr, batch = 4, 2, 0, 10, 1e-3, 256
    prioritized = form in ("per", "per0")
    tr, oring = _filled(rl, ns, seed=31, prioritized=prioritized)
    traj = rl.Trajectory(tr)
    traj.controller.on_insert_(10 ** 6)
    kw = dict(n_step=3) if form == "nstep" else (dict(per_beta=0.4) if form == "per" else {})
    learner, tn, net = _learner(rl, layers, h, 5, double_dqn=True, **kw)
    assert form != "per0" or learner.per_beta == 0.0
    p, pt = host(net.params).copy(), host(tn.target).copy()
    p0 = p.copy()
    m, v = np.zeros_like(p), np.zeros_like(p)
    st = oracle.SumTree(tr.n_leaves) if prioritized else None
    n_opt = 0
    for k in range(K):
        gamma, w, key = GAMMA, None, None
        if form == "nstep":
            idx = oracle.ring_sample_indices_nstep(oring, batch, 3, 5, k)
            s, a, r, t, sn = oracle.ring_gather_nstep(oring, idx, 3, GAMMA)
            gamma = oracle.gamma_pow(GAMMA, 3)
        else:
            if prioritized:  # the oracle draws from the GPU's tree as it stands before this update
                st.tree[:] = host(tr.priorities)
                idx, key, prio = oracle.ring_sample_prioritized(oring, st, batch, 5, k)
                w = oracle.per_is_weights(prio, 0.4) if form == "per" else None
            else:
                idx = oring.sample_indices(batch, 5, k)
            s, a, r, t, sn = oring.gather(idx)
        if form == "nstep":  # (the learner folds its n-step draw; the double fold then takes that ring's iota)
            assert np.array_equal(host(learner._nstep.sample_indices(tr, k)), idx) and learner._nstep.gamma_n == gamma
        assert learner.optimise_(traj)
        torch.cuda.synchronize()
        assert np.array_equal(host(learner._idx), idx if form != "nstep" else np.arange(batch)), f"update {k}: other transitions drawn"
        if prioritized:
            assert np.array_equal(host(learner._key), key)
        y, *_ = compose(layers, ns, h, na, act, p, pt, r, t, sn, gamma)
        if prioritized:  # the write-back: (|Q(s, a) - y| + eps)^alpha under the original keys
            ref_prio = oracle.per_priority(np.abs(forward(layers, p, ns, h, na, act, s)[a, np.arange(batch)] - y), 1e-6, 0.6)
            np.testing.assert_allclose(host(learner.td), ref_prio, rtol=1e-3 if layers == 2 else 2e-2, atol=1e-6)
        _, g = loss_grad(layers, ns, h, na, act, p, pt, s, a, y, sn, gamma, weights=w)
        oracle.clip_by_global_norm(g, 0.5)
        oracle.adam(p, g, m, v, lr, 0.9, 0.999, 1e-8, k + 1)
        due, n_opt = oracle.target_sync_due(n_opt, 4)
        if due:
            oracle.polyak(pt, p, 0.0)
    d = np.abs(host(net.params) - p)
    q99, dmax = float(np.quantile(d, 0.99)), float(d.max())
    note("DQNLearner(double_dqn=True) x 10 vs oracle loop", form=form, layers=layers, h=h, dp_q99=q99, dp_max=dmax,
         moved_q50=float(np.median(np.abs(p - p0))))
    print(f"{form} layers={layers}: |dp| q99 {q99:.3e} max {dmax:.3e}")
    assert np.median(np.abs(p - p0)) > lr
    assert q99 < (0.2 if layers == 2 else 2.0) * lr and dmax < K * 2 * lr
    assert np.abs(host(tn.target) - pt).max() <= dmax + 1e-12


@pytest.mark.parametrize("form", ["uniform", "nstep", "per"])
def test_flag_off_is_bit_identical_to_a_learner_without_the_keyword(form):
    import rlhip as rl

    extra = dict(n_step=3) if form == "nstep" else (dict(per_beta=0.4) if form == "per" else {})

    def ten_updates(negate_target=False, **kw):
        tr, _ = _filled(rl, 4, seed=31, prioritized=form == "per")
        traj = rl.Trajectory(tr)
        traj.controller.on_insert_(10 ** 6)
        learner, tn, net = _learner(rl, 2, 128, 5, **extra, **kw)
        if negate_target:  # a target net that ranks the actions unlike the online net: argmax Q(s') != argmax Qt(s') on most samples
            tn.target.neg_()
        for _ in range(10):
            assert learner.optimise_(traj)
        torch.cuda.synchronize()
        return host(net.params).copy(), host(tn.target).copy(), host(net.m).copy()

    for x, y in zip(ten_updates(), ten_updates(double_dqn=False)):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
    # ... and the flag does change the update where it can: the two nets must disagree about the best action (a freshly synchronised
    # target agrees with the online net on nearly every sample) and the TD errors must sit in Huber's quadratic zone (beyond delta the
    # gradient is sign(td) / batch whatever the target: the n-step returns of this ring, ~2.9 against Q ~ 0.1, saturate delta = 1 on
    # every sample, and DQN and Double DQN are then the same update bit for bit)
    kw = dict(negate_target=True, huber_delta=100.0)
    assert not np.array_equal(ten_updates(**kw)[0], ten_updates(double_dqn=True, **kw)[0])


def test_fold_double_argument_validation():
    import rlhip as rl
    from rlhip._lib import RLHipArgumentError, call
    from rlhip.ops import ptr, stream_ptr

    tr, _ = _filled(rl, 4, pushes=3)
    idx = torch.zeros(8, dtype=torch.int64, device="cuda")
    ok = rl.CircularArraySARTSTraces(capacity=1, n_env=8, obs_dim=4)
    net = rl.HipApproximator(4, 64, 2, seed=1)
    net3 = rl.HipApproximator(4, 128, 2, seed=1, layers=3)

    def fold2(src, dst, h=64, na=2, batch=8):
        call("rlhip_dqn_fold_double_f32", C.byref(src.rb), h, na, 0, ptr(net.params), ptr(net.params), ptr(idx), batch, 0.9,
             C.byref(dst.rb), None, None, stream_ptr())

    fold2(tr, ok)
    with pytest.raises(RLHipArgumentError):   # folded ring of the wrong width
        fold2(tr, rl.CircularArraySARTSTraces(capacity=1, n_env=9, obs_dim=4))
    with pytest.raises(RLHipArgumentError):   # not a record ring
        fold2(rl.CircularArraySARTSTraces(capacity=4, n_env=8, obs_dim=6), ok)
    with pytest.raises(RLHipArgumentError):   # obs_dim outside 2..4
        fold2(rl.CircularArraySARTSTraces(capacity=4, n_env=8, obs_dim=1), rl.CircularArraySARTSTraces(capacity=1, n_env=8, obs_dim=1))
    with pytest.raises(RLHipArgumentError):   # more actions than the learners take
        fold2(tr, ok, na=5)
    with pytest.raises(RLHipArgumentError):   # hidden width the gradient kernel does not take
        fold2(tr, ok, h=258)
    with pytest.raises(RLHipArgumentError):   # in place on a ring that is not a folded one
        fold2(tr, tr, batch=tr.n_env)
    ws = torch.empty(int(rl._lib.lib.rlhip_dqn_double_workspace_bytes(4, 64, 2, 8, 3)), dtype=torch.uint8, device="cuda")
    with pytest.raises(RLHipArgumentError):   # three-layer form: hidden must be 128 / 256
        call("rlhip_dqn3_fold_double_f32", C.byref(tr.rb), 64, 2, 0, ptr(net3.params), ptr(net3.packed), ptr(net3.params),
             ptr(net3.packed), ptr(idx), 8, 0.9, C.byref(ok.rb), None, ptr(ws), stream_ptr())
    torch.cuda.synchronize()


def test_bounds_checked_build_refuses_an_out_of_range_index_in_both_folds():
    """lib/librlhip_bounds.so (-DRLHIP_BOUNDS_CHECK), as tests/test_gpu_edges.py drives it: both fold entry points give the default
    build's bits for valid indices and RLHIP_EINVAL, before any launch, for an index outside [0, length * n_env).  The bad index is
    handed to the checked build only."""
    import os
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    so = os.path.join(root, "reinforcementlearning.jl_amd", "lib", "librlhip_bounds.so")
    assert os.path.exists(so), "run python -c 'import __graft_entry__ as g; g.build()'"
    prog = r"""
import sys, torch
sys.path.insert(0, sys.argv[1] + "/tests"); sys.path.insert(0, sys.argv[1] + "/reinforcementlearning.jl_amd"); sys.path.insert(0, sys.argv[1])
import rlhip as rl
from rlhip._lib import RLHipArgumentError, lib
from test_gpu_double_dqn import _filled
checked = int(lib.rlhip_ring_bounds_checked_build())
print("checked_build", checked)
tr, _ = _filled(rl, 4, pushes=5)
idx = tr.sample_indices(64, seed=3, draw_ctr=0)
for layers, h in ((2, 64), (3, 128)):
    net = rl.HipApproximator(4, h, 2, seed=1, layers=layers)
    tn = rl.TargetNetwork(net, sync_freq=10)
    fold = rl.DoubleTargetFold()
    folded, iota = fold.fold(tr, idx, net, tn.target, tn.target_packed, 0.9)
    torch.cuda.synchronize()
    print("sum", layers, float(folded.records.double().sum()))
    if checked:
        bad = idx.clone(); bad[5] = tr.n_transitions()
        try:
            fold.fold(tr, bad, net, tn.target, tn.target_packed, 0.9); print("fold:", layers, "no error")
        except RLHipArgumentError as e:
            print("fold:", layers, "EINVAL", "outside" in str(e))
"""
    outs = {}
    for name, env_extra in (("default", {}), ("bounds", {"RLHIP_LIB_PATH": so})):
        r = subprocess.run([sys.executable, "-c", prog, root], capture_output=True, text=True, timeout=300, env=dict(os.environ, **env_extra))
        assert r.returncode == 0, r.stdout + r.stderr
        outs[name] = [ln for ln in r.stdout.splitlines() if ln.split(" ")[0] in ("checked_build", "sum", "fold:")]
    assert outs["default"][0] == "checked_build 0" and outs["bounds"][0] == "checked_build 1"
    assert outs["default"][1:] == [ln for ln in outs["bounds"] if ln.startswith("sum")], "valid folds differ between the two builds"
    assert [ln for ln in outs["bounds"] if ln.startswith("fold:")] == ["fold: 2 EINVAL True", "fold: 3 EINVAL True"]


def test_checkpoint_with_the_flag_loads_into_a_learner_built_without_it(tmp_path):
    """the flag is state, the fold's ring is not: a learner constructed with the default that loads a double_dqn = True checkpoint
    makes its DoubleTargetFold at the next update and continues bit-identically to the learner that wrote the checkpoint"""
    import rlhip as rl

    def make(**kw):
        tr, _ = _filled(rl, 4, seed=31)
        traj = rl.Trajectory(tr)
        traj.controller.on_insert_(10 ** 6)
        learner, tn, net = _learner(rl, 2, 128, 5, **kw)
        return traj, learner, net

    traj, learner, net = make(double_dqn=True)
    for _ in range(3):
        assert learner.optimise_(traj)
    path = str(tmp_path / "ck.npz")
    rl.save_checkpoint(path, {"learner": learner})
    traj2, learner2, net2 = make()
    rl.load_checkpoint(path, {"learner": learner2})
    assert learner2.double_dqn is True
    for _ in range(3):
        assert learner.optimise_(traj) and learner2.optimise_(traj2)
    torch.cuda.synchronize()
    assert np.array_equal(host(net.params).view(np.uint32), host(net2.params).view(np.uint32))


@pytest.mark.parametrize("layers,vec_steps", [(2, 6500), (3, 3000)])
def test_double_dqn_learns_cartpole(layers, vec_steps):
    """the criterion of tests/test_gpu_learn.py::test_dqn_learns_cartpole, on the per-stage loop (the fused vec-step is plain DQN)"""
    import rlhip as rl
    from test_gpu_learn import _random_policy_episode_length

    n, cap, chunk = 4096, 256, 500
    base = _random_policy_episode_length(rl)
    assert 15.0 < base < 30.0, base
    env = rl.CartPoleEnv(n, seed=5)
    net = rl.HipApproximator(4, 128, 2, seed=5, layers=layers)
    learner = rl.DQNLearner(rl.TargetNetwork(net, sync_freq=100), batchsize=512, min_replay_history=n, seed=5, double_dqn=True)
    policy = rl.QBasedPolicy(learner, rl.EpsilonGreedyExplorer(0.01, kind="exp", decay_steps=500, seed=5))
    tr = rl.CircularArraySARTSTraces(capacity=cap, n_env=n, obs_dim=4)
    agent = rl.Agent(policy, rl.Trajectory(tr))
    with pytest.raises(NotImplementedError):
        rl.run_fused_dqn(agent, env, rl.StopAfterNSteps(1))
    curve = []
    for _ in range(vec_steps // chunk):
        rl.run(agent, env, rl.StopAfterNSteps(chunk))
        idx = torch.arange(len(tr) * n, device="cuda")
        term = tr.gather(idx)[3]
        curve.append(round(len(tr) * n / max(1.0, float(term.sum())), 1))
    note(f"Double DQN learns CartPole, layers={layers}", random_policy_ep_len=round(base, 1), ep_len_per_500_vec_steps=curve,
         updates=learner.n_updates)
    print(f"layers={layers}: random {base:.1f}, curve {curve}")
    assert learner.n_updates == (vec_steps // chunk) * chunk and torch.isfinite(net.params).all()
    assert max(curve) >= 2.0 * base, f"mean episode length never reached 2 x the random policy's {base:.1f}: {curve}"
    assert sum(c >= 2.0 * base for c in curve) >= 3, f"fewer than three 500-step windows above 2 x random ({base:.1f}): {curve}"


@pytest.mark.parametrize("layers,form", [(2, "uniform"), (3, "uniform"), (2, "per"), (2, "nstep")])
def test_checkpoint_resume_with_double_dqn_is_bit_identical(tmp_path, layers, form):
    import rlhip

    def build(seed):
        n = 160
        env = rlhip.CartPoleEnv(n, seed=seed)
        net = rlhip.HipApproximator(4, 128, 2, seed=seed, layers=layers)
        extra = dict(n_step=3) if form == "nstep" else (dict(per_beta=0.4) if form == "per" else {})
        learner = rlhip.DQNLearner(rlhip.TargetNetwork(net, sync_freq=5), batchsize=128, min_replay_history=2 * n, seed=seed,
                                   max_grad_norm=1.0, double_dqn=True, **extra)
        policy = rlhip.QBasedPolicy(learner, rlhip.EpsilonGreedyExplorer(0.05, kind="exp", decay_steps=30, seed=seed))
        traces = (rlhip.CircularPrioritizedTraces if form == "per" else rlhip.CircularArraySARTSTraces)(capacity=16, n_env=n, obs_dim=4)
        return env, rlhip.Agent(policy, rlhip.Trajectory(traces))

    path = str(tmp_path / "ck.npz")
    env, agent = build(6)
    saved = []

    def hook_fn(t, policy, e):
        if t == 20:
            saved.append(rlhip.save_checkpoint(path, {"agent": agent, "env": env}))

    rlhip.run(agent, env, rlhip.StopAfterNSteps(45), rlhip.DoEveryNSteps(hook_fn, n=20))
    assert saved and saved[0] > 20
    with np.load(path) as z:
        assert bool(z["agent/policy/learner/double_dqn"]) and not [k for k in z.files if "_double" in k]  # the flag, not the scratch
    env2, agent2 = build(99)
    rlhip.load_checkpoint(path, {"agent": agent2, "env": env2})
    rlhip.run(agent2, env2, rlhip.StopAfterNSteps(25))
    torch.cuda.synchronize()
    a, b = rlhip.state_dict({"agent": agent, "env": env}), rlhip.state_dict({"agent": agent2, "env": env2})
    assert set(a) == set(b)
    for k in a:
        if "workspace" in k or k.endswith("/grad") or "/_q" in k or "_nstep/_" in k or k.endswith("/_idx"):
            continue    # scratch
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k
    assert agent2.policy.learner.n_updates > 30
