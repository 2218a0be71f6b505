"""Every reachable instantiation of the three-layer bf16 MFMA learner kernels (tests/bf16_learner_matrix.py) against the oracle.

One case per row of the table, the row's id in the test id.  The comparisons are against oracle/ (Float64 accumulation, the
same bf16 roundings), with the protocols and bars of the per-feature files: gradients per tensor under BF16_GRAD_TOL and its
bulk bars (conftest.assert_grad_close), Q-values and values under the forward bar of tests/test_gpu_dqn3.py (_assert_q_close),
actions bit for bit against oracle.eps_greedy_select on the GPU's own Q, rollouts as tests/test_gpu_ppo3w.py
test_rollout_matches_oracle.  The update rows compare rlhip_dqn3_update_f32 with grad -> clip + Adam -> pack bit for bit (the
gradient rows pin the gradient to the oracle).  The decision-free cases of each DQN gradient form are
tests/test_gpu_bf16_tight.py::test_dqn3_grad_tight and test_dqn3_grad_tight_batches.

The inputs are chosen so that an error is visible, and each case asserts it: every tensor of the reference gradient is non-zero,
DQN batches have samples in both Huber branches, greedy plans pick at least two actions, the fused act resets a quarter of the
envs.  Where a comparison spans tens of thousands of outputs (rollouts of 2^15 + 1 envs, TD errors of large batches) the tanh /
Gaussian outputs take the flip rule of _assert_q_close, and observations after an env step the tolerance of the fused act
(ocml's and glibc's sin / cos differ in the last bit now and then).
"""
import ctypes as C
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import bf16_learner_matrix as M  # noqa: E402
import oracle  # noqa: E402
from conftest import BF16_GRAD_TOL, assert_grad_close  # noqa: E402

KIND = {"cartpole": 0, "pendulum": 1, "mountaincar": 2}
GAMMA, DELTA = 0.99, 1.0


@pytest.fixture(scope="module")
def rl():
    import rlhip

    oracle.use_all_cores(True)  # batches up to 131 072 samples through a Float64 128-wide forward / backward
    yield rlhip
    oracle.use_all_cores(False)


def dev(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).cuda()


def host(t):
    return t.detach().cpu().numpy()


def ids(rows):
    return [r["id"] for r in rows]


def _rows(rows, pred):
    sel = [r for r in rows if pred(r)]
    return dict(argvalues=sel, ids=ids(sel))


# ------------------------------------------------------------------------------------------------------------ helpers
def _assert_q_close(q, ref, act):
    """tests/test_gpu_dqn3.py::_assert_q_close"""
    err = np.abs(q - ref) / (1 + np.abs(ref))
    if act == 0:
        assert err.max() <= 2e-5, err.max()
    else:
        assert (err <= 2e-5).mean() >= 0.999 and err.max() <= 5e-3, ((err <= 2e-5).mean(), err.max())


def _layout(ns, h, nout):
    return (("W1", h * ns), ("b1", h), ("W2", h * h), ("b2", h), ("W3", nout * h), ("b3", nout))


def _net(ns, h, na, seed):
    """oracle init with non-zero biases (every bias path exercised): tests/test_gpu_dqn3.py::_net at either width"""
    p = oracle.mlp3_init(ns, h, na, seed, 0)
    rng = np.random.default_rng(seed)
    o = 0
    for name, n in _layout(ns, h, na):
        if name[0] == "b":
            p[o:o + n] = rng.standard_normal(n).astype(np.float32) * 0.1
        o += n
    return p


def _check(g, ref, nets, tag, q99_tol=None):
    """nets: [(name, ns, h, nout)] in the order they sit in the flat vector; one bar per tensor, each reference tensor non-zero"""
    o = 0
    for net, ns, h, nout in nets:
        for name, sz in _layout(ns, h, nout):
            assert np.abs(ref[o:o + sz]).max() > 0, f"{tag} {net}.{name}: zero reference gradient"
            assert_grad_close(g[o:o + sz], ref[o:o + sz], BF16_GRAD_TOL, f"bf16 matrix {tag} {net}.{name}", q99_tol=q99_tol)
            o += sz
    assert o == g.size


def _ring(rl, ns, na, rng, n_env=64, cap=40, steps=57):
    """the same transitions in a GPU record ring and an oracle.Ring (tests/test_gpu_dqn3.py::_fill_ring); wraps"""
    traces = rl.CircularArraySARTSTraces(capacity=cap, n_env=n_env, obs_dim=ns)
    oring = oracle.Ring(cap, n_env, ns)
    obs = rng.standard_normal((ns, n_env)).astype(np.float32)
    traces.push_state_(dev(obs))
    oring.push_state(obs)
    for _ in range(steps):
        nobs = rng.standard_normal((ns, n_env)).astype(np.float32)
        a = rng.integers(0, na, n_env).astype(np.int32)
        r = (rng.standard_normal(n_env) * 2).astype(np.float32)
        term = (rng.random(n_env) < 0.2).astype(np.uint8)
        traces.push_transition_(dev(nobs), dev(a), dev(r), dev(term))
        oring.push_transition(nobs, a, r, term)
    return traces, oring


def _td_ref(ns, h, na, act, tp, rq, s, a, r, t, sn):
    qn = oracle.mlp3_forward(tp, ns, h, na, act, sn)
    ref_td = np.abs(rq[a, np.arange(a.size)] - (r + GAMMA * (1 - t.astype(np.float32)) * qn.max(0)))
    quad = float((ref_td < DELTA).mean())
    assert 0.05 < quad < 0.95, f"both Huber branches are meant to occur: {quad:.3f} of the samples on the quadratic one"
    return ref_td


# ------------------------------------------------------------------------------------------------ DQN gradient (h = 128)
@pytest.mark.parametrize("row", **_rows(M.DQN3_GRAD, lambda r: True))
def test_dqn3_gradient_vs_oracle(rl, row):
    """rlhip_dqn3_grad_f32 on the inline draw against oracle.dqn3_loss_grad, per tensor; explicit indices equal the inline
    draw, a second launch is bit-identical, the TD errors match; tanh rows also run rlhip_dqn3_grad_w_f32 (IS weights)"""
    from rlhip import dqn
    from rlhip._lib import call
    from rlhip.ops import ptr, stream_ptr

    env, act, batch, h = row["env"], row["act"], row["batch"], row["hidden"]
    ns, na = M.ENVS[env], M.DQN_NA[env]
    rng = np.random.default_rng(zlib.crc32(row["id"].encode()))
    traces, oring = _ring(rl, ns, na, rng)
    p, tp = _net(ns, h, na, 11 + act), _net(ns, h, na, 12 + ns)
    pd, tpd = dev(p), dev(tp)
    packed, tpacked = dqn.mlp3_pack(pd, ns, h, na), dqn.mlp3_pack(tpd, ns, h, na)
    ws = dqn.dqn3_workspace(ns, h, na, batch)
    td = torch.zeros(batch, device="cuda")
    g, loss = dqn.dqn3_grad(traces, h, na, act, pd, packed, tpd, tpacked, batch, GAMMA, DELTA, 7, 3, workspace=ws, td=td)
    gh, lh = host(g).copy(), float(loss)
    idx = oring.sample_indices(batch, 7, 3)
    s, a, r, t, sn = oring.gather(idx)
    rl_, rg, rq = oracle.dqn3_loss_grad(ns, h, na, act, p, tp, s, a, r, t, sn, GAMMA, DELTA)
    ref_td = _td_ref(ns, h, na, act, tp, rq, s, a, r, t, sn)
    assert abs(lh - rl_) <= 2e-5 * max(1.0, abs(rl_))
    _check(gh, rg, [("q", ns, h, na)], f"{row['id']} (batch={batch})")
    # TD errors: relu within the forward bar; tanh within its every-output bound -- a sample's TD error passes through the h1 of
    # two nets, so the rare bf16 flips of h1 are twice as frequent as for one Q output (measured 0.12 - 0.2 % of the samples)
    terr = np.abs(host(td) - ref_td) / (1 + ref_td)
    assert terr.max() <= (2e-5 if act == 0 else 5e-3), terr.max()
    # explicit indices (the prioritized path) give the same result as the inline draw; a second launch is bit-identical
    I = dev(idx)
    g2, loss2 = dqn.dqn3_grad(traces, h, na, act, pd, packed, tpd, tpacked, batch, GAMMA, DELTA, 0, 0, idx=I, workspace=ws)
    assert np.array_equal(host(g2), gh) and float(loss2) == lh
    g3, _ = dqn.dqn3_grad(traces, h, na, act, pd, packed, tpd, tpacked, batch, GAMMA, DELTA, 7, 3, workspace=ws)
    assert np.array_equal(host(g3), gh)
    if row["batch"] == M.D3_MAX_BATCH:  # the largest batch one launch takes; one more sample is refused
        with pytest.raises(rl._lib.RLHipError, match="too large"):
            dqn.dqn3_grad(traces, h, na, act, pd, packed, tpd, tpacked, batch + 1, GAMMA, DELTA, 7, 3)
    if row["isw"]:
        prio = ((rng.random(batch) + 1e-3) ** 0.6).astype(np.float32)
        w = oracle.per_is_weights(prio, 0.4)
        assert w.min() < 0.5 * w.max()
        gw, lw, tdw = torch.empty_like(pd), torch.empty(1, device="cuda"), torch.zeros(batch, device="cuda")
        call("rlhip_dqn3_grad_w_f32", C.byref(traces.rb), h, na, act, ptr(pd), ptr(packed), ptr(tpd), ptr(tpacked), batch, ptr(I),
             ptr(dev(w)), GAMMA, DELTA, ptr(ws), ptr(gw), ptr(lw), ptr(tdw), stream_ptr())
        rlw, rgw, _ = oracle.dqn3_loss_grad(ns, h, na, act, p, tp, s, a, r, t, sn, GAMMA, DELTA, weights=w)
        assert abs(float(lw) - rlw) <= 2e-5 * max(1.0, abs(rlw))
        _check(host(gw), rgw, [("q", ns, h, na)], f"{row['id']} IS weights (batch={batch})")
        assert np.array_equal(host(tdw), host(td))


@pytest.mark.parametrize("row", **_rows(M.DQN3_UPDATE, lambda r: True))
def test_dqn3_update_equals_grad_clip_adam_pack(rl, row):
    """rlhip_dqn3_update_f32 (gradient, then d3_apply_kernel: reduce + clip + Adam + bf16 re-pack behind a grid barrier) ==
    rlhip_dqn3_grad_f32 + rlhip_clip_adam_f32 + rlhip_mlp3_pack_bf16, bit for bit, over repeated calls, at a batch that reaches
    the row's gradient form (tests/test_gpu_dqn3.py::test_dqn3_update_is_bit_identical_to_grad_clip_adam_pack)"""
    from rlhip import dqn, ops

    env, act, batch, h = row["env"], row["act"], row["batch"], row["hidden"]
    ns, na = M.ENVS[env], M.DQN_NA[env]
    rng = np.random.default_rng(zlib.crc32(row["id"].encode()))
    traces, _ = _ring(rl, ns, na, rng)
    tp = dev(_net(ns, h, na, 2))
    tpk = dqn.mlp3_pack(tp, ns, h, na)
    st = []
    for _ in range(2):
        p = dev(_net(ns, h, na, 1))
        st.append(dict(p=p, pk=dqn.mlp3_pack(p, ns, h, na), m=torch.zeros_like(p), v=torch.zeros_like(p), g=torch.empty_like(p),
                       bp=torch.tensor([0.9, 0.999], device="cuda"), loss=torch.empty(1, device="cuda"),
                       gn=torch.zeros(1, device="cuda"), ws=dqn.dqn3_workspace(ns, h, na, batch)))
    a, b = st
    p0 = a["p"].clone()
    for it, clip in enumerate((0.5, 0.0, 1e6)):
        dqn.dqn3_grad(traces, h, na, act, a["p"], a["pk"], tp, tpk, batch, GAMMA, DELTA, 7, it, None, a["ws"], a["g"], a["loss"])
        ops.clip_adam_(a["p"], a["g"], a["m"], a["v"], a["bp"], 0.5, clip, 1e-2, 0.9, 0.999, 1e-8, a["gn"])
        dqn.mlp3_pack(a["p"], ns, h, na, a["pk"])
        dqn.dqn3_update(traces, h, na, act, b["p"], b["pk"], tp, tpk, batch, GAMMA, DELTA, 7, it, b["ws"], b["g"], b["loss"],
                        b["m"], b["v"], b["bp"], 0.5, clip, 1e-2, 0.9, 0.999, 1e-8, b["gn"])
        for k in ("p", "pk", "m", "v", "g", "bp", "loss", "gn"):
            assert torch.equal(a[k], b[k]), (it, k)
        assert float(a["g"].abs().max()) > 0
    assert not torch.equal(a["p"], p0)


# ----------------------------------------------------------------------------------------------------------- DQN plans
def _plan_case(rl, row, n, rng):
    from rlhip import dqn

    env, act, h = row["env"], row["act"], row["hidden"]
    ns, na = M.ENVS[env], M.DQN_NA[env]
    p = _net(ns, h, na, 3 + ns + act)
    x = rng.standard_normal((ns, n)).astype(np.float32)
    pd, xd = dev(p), dev(x)
    packed = dqn.mlp3_pack(pd, ns, h, na)
    _, q = dqn.dqn3_plan(pd, packed, ns, h, na, act, xd, want_actions=False)
    qh = host(q)
    _assert_q_close(qh, oracle.mlp3_forward(p, ns, h, na, act, x), act)
    for eps in (0.0, 0.3):
        a, q2 = dqn.dqn3_plan(pd, packed, ns, h, na, act, xd, eps, 17, 5, 42)
        assert torch.equal(q2, q)
        ah = host(a)
        assert np.array_equal(ah, oracle.eps_greedy_select(qh.astype(np.float32), eps, 17, 42, env_id_base=5))
        if eps == 0.0:
            share = np.bincount(ah, minlength=na) / n
            assert np.sort(share)[-2] >= 0.05, f"the greedy actions do not spread over two actions: {share}"


@pytest.mark.parametrize("row", **_rows(M.DQN3_PLAN + M.DQN3W, lambda r: r["kernel"] in ("mlp3_plan32_kernel", "mlp3_plan_kernel",
                                                                                         "dqn3w_plan_kernel")))
def test_dqn3_plan_vs_oracle(rl, row):
    """rlhip_dqn3_plan_f32: Q within the forward bar of oracle.mlp3_forward, actions bit for bit against
    oracle.eps_greedy_select on the GPU's Q (greedy and eps = 0.3); the 128-row kernel at n = 2^15 + 1 and a larger ragged n"""
    rng = np.random.default_rng(zlib.crc32(row["id"].encode()))
    for n in (row["n"],) + ((row["n2"],) if "n2" in row else ()):
        _plan_case(rl, row, n, rng)


# --------------------------------------------------------------------------------------------------- fused DQN act
@pytest.mark.parametrize("row", **_rows(M.DQN3_ACT, lambda r: True))
def test_fused_dqn3_act_vs_oracle(rl, row):
    """rlhip_dqn3_act_f32 (plan! + act! + push! in one launch, mlp3_plan32_kernel<.., ActTail<P>>) called directly
    (tests/test_gpu_f32_learner_matrix.py::test_fused_dqn_act_vs_oracle): Q on the observations the kernel read within the
    forward bar; actions bit-exact with oracle.eps_greedy_select on the GPU's Q; the oracle env started from the GPU's state and
    stepped with those actions gives the same terminal flags, step and reset counters bit for bit (rewards too, except
    Pendulum's: within 2e-6); the ring records equal an oracle.Ring fed the same states and transitions.  A quarter of the envs
    start at t = max_steps, so resets happen."""
    from rlhip import dqn
    from rlhip._lib import call
    from rlhip.ops import ptr, stream_ptr
    from rlhip.trajectory import CircularArraySARTSTraces

    env_name, h, act, n = row["env"], row["hidden"], row["act"], row["n"]
    kind = KIND[env_name]
    env = rl.HipVecEnv(env_name, n, seed=13, env_id_base=7, continuous=False, max_steps=40)
    ns, na = env.odim, len(env.action_space())
    assert (ns, na) == (M.ENVS[env_name], M.DQN_NA[env_name])
    assert int(rl._lib.lib.rlhip_dqn3_act_supported(kind, n, h, na)) == 1
    rng = np.random.default_rng(zlib.crc32(row["id"].encode()))
    p = _net(ns, h, na, 9 + act)
    t0 = np.where(rng.random(n) < 0.25, 40, rng.integers(0, 30, n)).astype(np.int32)  # CartPole ends at t > max_steps
    raw = env.raw_state().clone()
    if env_name == "cartpole":  # the reset states are within +-0.05: spread them (|x| < 1.5, |theta| < 0.15: no termination)
        raw *= torch.tensor([30.0, 20.0, 3.0, 20.0], device=raw.device)[:, None]
    env.set_raw_state(raw, t0)
    tr = CircularArraySARTSTraces(capacity=4, n_env=n, obs_dim=ns)
    ref = oracle.Ring(4, n, ns)
    obs0 = host(env.state()).copy()
    tr.push_state_(env.state())
    ref.push_state(obs0)
    oenv = oracle.VecEnv(kind, n, seed=13, env_id_base=7, continuous=False, max_steps=40)
    oenv.set_state([host(env.raw_state()[k]) for k in range(env.sdim)], host(env._t))
    oenv.episode[:] = host(env._episode).view(np.uint32)
    eps, xseed, step = 0.3, 17, 5
    P = dev(p)
    packed = dqn.mlp3_pack(P, ns, h, na)
    actions = torch.zeros(n, dtype=torch.int32, device="cuda")
    q = torch.zeros((na, n), device="cuda")
    obs, last_obs = dev(obs0), torch.zeros((ns, n), device="cuda")  # obs: read (this step's), rewritten (the next one's)
    call("rlhip_dqn3_act_f32", kind, C.byref(env.cfg), C.byref(env._st), n, ptr(P), ptr(packed), h, na, act, eps, xseed, step,
         env.seed, env.env_id_base, C.byref(tr.rb), ptr(actions), ptr(q), ptr(obs), ptr(last_obs), stream_ptr())
    env._obs_valid = False
    gq, ga = host(q), host(actions)
    # the fused kernel is rlhip_dqn3_plan_f32 (pinned by the dqn3_plan32 rows) followed by act! + push!, bit for bit
    pa, pq = dqn.dqn3_plan(P, packed, ns, h, na, act, dev(obs0), eps, xseed, env.env_id_base, step)
    assert np.array_equal(host(pq), gq) and np.array_equal(host(pa), ga)
    _assert_q_close(gq, oracle.mlp3_forward(p, ns, h, na, act, obs0), act)
    assert np.array_equal(ga, oracle.eps_greedy_select(gq, eps, seed=xseed, step=step, env_id_base=env.env_id_base))
    assert np.bincount(ga, minlength=na).min() > 0
    oenv.step(ga)
    done = host(env._done)
    assert np.array_equal(done, oenv.done) and np.array_equal(host(env._t), oenv.t)
    assert np.array_equal(host(env._episode).view(np.uint32), oenv.episode)
    assert 0.2 <= done.mean() <= 0.5, f"{done.mean():.3f} of the envs terminated"
    if env_name == "pendulum":
        np.testing.assert_allclose(host(env.reward()), oenv.reward, rtol=2e-6, atol=1e-7)
    else:
        assert np.array_equal(host(env.reward()), oenv.reward)
    oatol = 2e-5 if env_name == "pendulum" else 1e-7
    np.testing.assert_allclose(host(obs), oenv.obs(), rtol=2e-6, atol=oatol)
    np.testing.assert_allclose(host(last_obs), oenv.last_obs, rtol=2e-6, atol=oatol)
    assert np.array_equal(host(obs), host(env.state())), "obs is not state(env) after the step"
    ref.push_transition(host(obs), ga, host(env.reward()), done)
    assert len(tr) == len(ref) == 1
    idx = np.arange(n, dtype=np.int64)
    for g_, o_ in zip((host(x) for x in tr.gather(dev(idx))), ref.gather(idx)):
        assert np.array_equal(g_, o_)


# ------------------------------------------------------------------------------------------------------- PPO rollouts
@pytest.mark.parametrize("row", **_rows(M.PPO3 + M.PPO3W, lambda r: "rollout" in r["id"]))
def test_ppo3_rollout_vs_oracle(rl, row):
    """the whole T-step rollout (one launch) against oracle.ppo_rollout (tests/test_gpu_ppo3w.py::test_rollout_matches_oracle):
    step 0 sees the same observations, values / actions within the forward bar (tanh: the bar of _assert_q_close), discrete
    actions agree where not at a near-tie, envs whose actions all agree have identical trajectories; the fused GAE equals the
    stand-alone scan"""
    env_name, act, h, n, T = row["env"], row["act"], row["hidden"], row["n"], row["T"]
    cont = M.PPO_ENVS[env_name]
    env = rl.HipVecEnv(env_name, n, seed=5)
    pol = rl.PPOPolicy(env, update_freq=T, hidden=h, seed=5, layers=3, act=act)
    params = host(pol.params)
    oenv = oracle.VecEnv(env_name, n, seed=5)
    ocfg = oracle.ppo_default(hidden=h, continuous=int(cont), layers=3, act=act)
    otr = oracle.PPOTraj(oracle.KIND[env_name], n, T, continuous=cont)
    oracle.ppo_rollout(oenv, T, ocfg, params, otr, 0)
    pol.rollout_()
    tr = pol.trajectory
    v, ov = host(tr.value), otr.value
    vtol = 1e-4 if (cont or act == 1) else 2e-5
    flip = act == 1 or cont  # Pendulum: an obs differing in its last bit can move an h1 element across a bf16 rounding boundary

    def close(x, ref, tol):
        err = np.abs(x - ref) / (1 + np.abs(ref))
        if not flip:
            assert err.max() <= tol, err.max()
        else:
            assert (err <= tol).mean() >= 0.999 and err.max() <= 5e-3, ((err <= tol).mean(), err.max())

    if cont:
        np.testing.assert_allclose(host(tr.obs[0]), otr.obs[0], rtol=0, atol=2e-7)
    else:
        assert np.array_equal(host(tr.obs[0]), otr.obs[0])
    close(v[0], ov[0], vtol)
    if cont:
        af, oaf = host(tr.action_f).reshape(T, n), otr.action_f.reshape(T, n)
        close(af[0], oaf[0], 1e-4)
        assert np.quantile(np.abs(host(tr.logp[0]) - otr.logp[0]), 0.999) <= 1e-3
        assert af[0].std() > 0.1
    else:
        ai, oai = host(tr.action_i), otr.action_i
        assert 0.1 <= ai[0].mean() <= 0.9, f"action 1 taken by {ai[0].mean():.3f} of the envs"
        agree = ai == oai
        assert agree[0].mean() >= 0.995
        same = agree.all(0)
        assert same.mean() >= 0.95
        for name in ("reward", "terminal"):
            assert np.array_equal(host(getattr(tr, name))[:, same], getattr(otr, name)[:, same])
        np.testing.assert_allclose(host(tr.obs)[:, :, same], otr.obs[:, :, same], rtol=2e-6, atol=1e-7)
        close(v[:, same], ov[:, same], 1e-4)
    adv = host(tr.adv).copy()
    pol.gae_()
    assert np.array_equal(host(tr.adv), adv)


# ------------------------------------------------------------------------------------------------------ PPO gradients
def _oracle_ppo_grad(pol, params, cont, ocfg, epoch, mb, n, T, nmb):
    tr = pol.trajectory
    total = n * T
    bm = total // nmb
    f = np.array([oracle.permute(pol.seed, epoch, total, mb * bm + b) for b in range(bm)])
    t, i = f // n, f % n
    obs = host(tr.obs)[t, :, i].T.copy()
    action = host(tr.action_f).reshape(T, n)[t, i][None, :] if cont else host(tr.action_i)[t, i]
    ns = obs.shape[0]
    return oracle.ppo_loss_grad(ocfg, ns, 1 if cont else 2, params, obs, action, host(tr.logp)[t, i], host(tr.adv)[t, i],
                                host(tr.ret)[t, i])


def _w3_pad(on):
    """rlhip_debug_w3_dzf_pad_info (csrc/ppo3w.hip, not part of the ABI): 0 / 1 force the backward kernel's LDS copy, 2 = by
    the chip's clock, < 0 query.  Returns (kernel of the next launch, mode)"""
    from rlhip import _lib

    fn = _lib.lib.rlhip_debug_w3_dzf_pad_info
    fn.restype, fn.argtypes = C.c_int32, [C.c_int32, C.POINTER(C.c_double)]
    info = (C.c_double * 6)()
    v = fn(on, info)
    return v, int(info[0])


class _Forced:
    """force128 (ppo3.hip) and the backward LDS copy (ppo3w.hip) for one row; restores both afterwards"""

    def __init__(self, row):
        self.row = row

    def __enter__(self):
        from rlhip import _lib

        self.force = _lib.lib.rlhip_debug_ppo3_force128
        self.force.restype = C.c_int32
        self.mode0 = _w3_pad(-1)[1]
        assert self.force(1 if self.row.get("force128") else 0) == 0
        if "pad" in self.row:
            assert _w3_pad(self.row["pad"])[0] == self.row["pad"]
        return self

    def __exit__(self, *exc):
        self.force(0)
        _w3_pad(self.mode0)
        assert _w3_pad(-1)[1] == self.mode0


def _ppo_q99(row):
    # the one documented bulk override of the suite: Gaussian + tanh at a small 256-wide micro-batch (tests/test_gpu_ppo3w.py)
    small = row["n"] * row["T"] // row["nmb"] < 1000
    return 3e-4 if (row["hidden"] == 256 and M.PPO_ENVS[row["env"]] and row["act"] == 1 and small) else None


@pytest.mark.parametrize("row", **_rows(M.PPO3 + M.PPO3W, lambda r: "rollout" not in r["id"] and not r.get("rec")))
def test_ppo3_gradient_vs_oracle(rl, row):
    """rlhip_ppo_grad_f32 (layers = 3) on the last micro-batch of a GPU rollout against oracle.ppo_loss_grad on the same
    permuted samples (tests/test_gpu_ppo3.py::test_grad_matches_oracle): every tensor of actor and critic, the four loss
    terms; a second launch is bit-identical"""
    env_name, act, h, n, T, nmb = row["env"], row["act"], row["hidden"], row["n"], row["T"], row["nmb"]
    cont = M.PPO_ENVS[env_name]
    env = rl.HipVecEnv(env_name, n, seed=5)
    pol = rl.PPOPolicy(env, update_freq=T, hidden=h, seed=5, layers=3, act=act, n_microbatches=nmb)
    pol.rollout_()
    pol.gae_()
    ocfg = oracle.ppo_default(hidden=h, continuous=int(cont), layers=3, n_microbatches=nmb, act=act)
    epoch, mb = 1, nmb - 1
    with _Forced(row):
        pol.grad_(epoch, mb)
        g, losses = host(pol.grad).copy(), host(pol.losses).copy()
        pol.grad_(epoch, mb)
        assert np.array_equal(host(pol.grad), g) and np.array_equal(host(pol.losses), losses)
    og, ol = _oracle_ppo_grad(pol, host(pol.params), cont, ocfg, epoch, mb, n, T, nmb)
    assert np.all(np.abs(losses - ol) <= 2e-4 * (1 + np.abs(ol))), (losses, ol)
    ns = env.odim
    _check(g, og, [("actor", ns, h, 2), ("critic", ns, h, 1)], f"{row['id']} (bm={n * T // nmb})", q99_tol=_ppo_q99(row))


@pytest.mark.parametrize("row", **_rows(M.PPO3W, lambda r: r.get("rec", False)))
def test_ppo3w_update_on_the_record_copy_vs_oracle(rl, row):
    """rlhip_ppo_update_f32 at hidden = 256 builds the record copy of the trajectory (ppo3w_build_rec_kernel) and gathers the
    micro-batch from it (ppo3w_gather_rec_kernel).  One epoch, one micro-batch, clipping off: the gradient the tail leaves in
    the gradient buffer and its loss line against oracle.ppo_loss_grad at the parameters before the step"""
    env_name, act, h, n, T = row["env"], row["act"], row["hidden"], row["n"], row["T"]
    cont = M.PPO_ENVS[env_name]
    env = rl.HipVecEnv(env_name, n, seed=5)
    pol = rl.PPOPolicy(env, update_freq=T, hidden=h, seed=5, layers=3, act=act, n_microbatches=1, n_epochs=1, max_grad_norm=1e9)
    pol.rollout_()
    p0 = host(pol.params).copy()
    pol.update_()
    g, losses = host(pol.grad).copy(), host(pol.losses).copy()
    assert not np.array_equal(host(pol.params), p0)
    ocfg = oracle.ppo_default(hidden=h, continuous=int(cont), layers=3, n_microbatches=1, act=act)
    og, ol = _oracle_ppo_grad(pol, p0, cont, ocfg, 0, 0, n, T, 1)
    assert np.all(np.abs(losses - ol) <= 2e-4 * (1 + np.abs(ol))), (losses, ol)
    ns = env.odim
    _check(g, og, [("actor", ns, h, 2), ("critic", ns, h, 1)], f"{row['id']} (bm={n * T})")


# ------------------------------------------------------------------------------------------- DQN gradient (h = 256)
@pytest.mark.parametrize("row", **_rows(M.DQN3W, lambda r: r["kernel"] != "dqn3w_plan_kernel"))
def test_dqn3w_gradient_vs_oracle(rl, row):
    """rlhip_dqn3_grad_f32 at hidden = 256 with the row's backward LDS copy forced: per tensor against oracle.dqn3_loss_grad"""
    from rlhip import dqn

    env, act, batch, h = row["env"], row["act"], row["batch"], row["hidden"]
    ns, na = M.ENVS[env], M.DQN_NA[env]
    rng = np.random.default_rng(zlib.crc32(row["id"].encode()))
    traces, oring = _ring(rl, ns, na, rng)
    p, tp = _net(ns, h, na, 11 + act), _net(ns, h, na, 12 + ns)
    pd, tpd = dev(p), dev(tp)
    packed, tpacked = dqn.mlp3_pack(pd, ns, h, na), dqn.mlp3_pack(tpd, ns, h, na)
    with _Forced(row):
        g, loss = dqn.dqn3_grad(traces, h, na, act, pd, packed, tpd, tpacked, batch, GAMMA, DELTA, 7, 3)
        gh = host(g).copy()
        g2, _ = dqn.dqn3_grad(traces, h, na, act, pd, packed, tpd, tpacked, batch, GAMMA, DELTA, 7, 3)
        assert np.array_equal(host(g2), gh)
    idx = oring.sample_indices(batch, 7, 3)
    s, a, r, t, sn = oring.gather(idx)
    rl_, rg, rq = oracle.dqn3_loss_grad(ns, h, na, act, p, tp, s, a, r, t, sn, GAMMA, DELTA)
    _td_ref(ns, h, na, act, tp, rq, s, a, r, t, sn)
    assert abs(float(loss) - rl_) <= 2e-5 * max(1.0, abs(rl_))
    _check(gh, rg, [("q", ns, h, na)], f"{row['id']} (batch={batch})")
