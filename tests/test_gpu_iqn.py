"""The IQN kernels and IQNLearner on the device against the float64 model of tests/iqn_ref.py.

Levels      tau_out of forward / plan and of both gradient draws = the oracle's Philox words mapped by the header's rule.
Kernels     quantiles, Q, targets, per-sample losses, loss and every block of the gradient against float64 torch (autograd), on levels
            mapped from the oracle's Philox words (which the same test checks the kernel drew); a second call returns the same bytes.
Decisions   float64 and Float32 may disagree only at a relu sign or an a* tie: every case's seed is chosen so that, in the reference,
            every relu pre-activation of psi and phi has |z| >= 1e-4 and the a* margin is >= 1e-4; asserted, no case is dropped.
Bar         max(1e-6, 4 x FLOOR).  FLOOR is the largest distance of the SAME model evaluated in Float32 torch on the CPU from the float64
            model over these cases (gradients relative to max|g|, quantiles / targets to max|theta|): 3.33e-7 (the forward case "max";
            per case in profiles/iqn.md), so the bar is 1.33e-6.  The bar is never taken from the kernel.
Learner     eight update forms teacher-forced against iqn_grad_batch -> clip_adam_ on the same batch; checkpoint resume; CartPole."""
import functools

import numpy as np
import pytest
import torch

import iqn_ref as R
import oracle

pytestmark = pytest.mark.gpu

FLOOR = 3.33e-7
BAR = max(1e-6, 4.0 * FLOOR)
ZMIN = MARGIN = 1e-4
TAG_PLAN, TAG_ONLINE, TAG_TARGET = 9, 10, 11
KAPPA, GAMMA, SEED, CTR = 1.0, 0.9, 77, 5
F32 = np.float32
host = lambda x: x.detach().cpu().numpy()  # noqa: E731


def philox_levels(n_levels, idx, t, tag, seed=SEED):
    """(n_levels, len(idx)) levels of the header's rule from the oracle's Philox"""
    w = [[oracle.philox(seed, int(i), n // 4, t, tag)[n % 4] for i in idx] for n in range(n_levels)]
    return R.levels(w)


def make_net(rng, ns, h, na, nc, safe):
    """biases away from zero and weights small enough that few (safe: no) relu pre-activations come near zero"""
    sgn = lambda n: rng.choice([-1.0, 1.0], n)  # noqa: E731
    W1 = rng.uniform(-1, 1, h * ns) * (0.25 / ns if safe else 0.5 / np.sqrt(ns))
    Wp = rng.uniform(-1, 1, h * nc) * (0.4 / nc if safe else 0.6 / np.sqrt(nc))
    return np.concatenate([W1, rng.uniform(0.3, 1.0, h) * sgn(h), Wp, rng.uniform(0.5, 1.5, h) * sgn(h),
                           rng.uniform(-2, 2, na * h) / np.sqrt(h), rng.uniform(-0.5, 0.5, na)]).astype(F32)


#            ns  h   na nc  N   N'  batch act double seed
GRAD = {"b1": (2, 32, 1, 2, 1, 1, 1, 0, False, 0), "b9-tanh": (4, 32, 2, 64, 5, 3, 9, 1, True, 0), "b9-wide": (16, 256, 4, 64, 5, 3, 9, 0, False, 0),
        "b9-levels": (4, 32, 3, 32, 32, 64, 9, 0, True, 0), "b67": (5, 64, 4, 6, 5, 3, 67, 0, True, 0), "b67-tanh": (3, 32, 2, 34, 3, 5, 67, 1, False, 0),
        "multi-tile": (4, 32, 2, 4, 2, 1, 8 * 256 + 3, 0, False, 0),  # (8 * 256 + 3: more tiles than workgroups)
        # the smallest network the kernels take: the register chains carry into a full second tile (workgroup 0) and into a tile of one
        # valid sample (workgroup 1)
        "carry-smallest": (2, 32, 1, 2, 1, 1, 8 * 256 + 9, 0, True, 0)}
CARRY = ("multi-tile", "carry-smallest")  # asserted below: more than one tile per workgroup


@functools.lru_cache(maxsize=None)
def grad_case(name, dtype=torch.float64):
    ns, h, na, nc, N, Np, b, act, double, seed = GRAD[name]
    rng = np.random.default_rng([seed, b, h])
    safe = b > 1000
    c = dict(dims=(ns, h, na, nc), N=N, Np=Np, b=b, act=act, double=double, params=make_net(rng, ns, h, na, nc, safe),
             target=make_net(rng, ns, h, na, nc, safe), s=rng.uniform(-1, 1, (ns, b)).astype(F32), sn=rng.uniform(-1, 1, (ns, b)).astype(F32),
             a=rng.integers(0, na, b).astype(np.int32), r=rng.normal(0.2, 1.0, b).astype(F32), term=(rng.uniform(size=b) < 0.2).astype(np.uint8),
             n_used=rng.integers(0, 4, b).astype(np.int32), weights=rng.uniform(0.3, 1.0, b).astype(F32))
    if b > 1:
        c["a"][b // 2] = na  # one action out of range: its sample contributes nothing
    c["tau"] = philox_levels(N, range(b), CTR, TAG_ONLINE)
    c["taup"] = philox_levels(Np, range(b), CTR, TAG_TARGET)
    t = lambda k: torch.tensor(c[k].astype(np.float64) if c[k].dtype.kind == "f" else c[k]).to(dtype if c[k].dtype.kind == "f" else torch.int64)  # noqa: E731
    p = t("params").requires_grad_(True)
    out = R.loss(p, t("target"), c["dims"], act, KAPPA, t("s"), t("a"), t("r"), t("term"), t("sn"), GAMMA, t("tau"), t("taup"), t("n_used"),
                 t("weights"), double)
    out["grad"] = torch.autograd.grad(out["loss"], p)[0]
    c["ref"] = {k: (v.detach().double().numpy() if torch.is_tensor(v) else v) for k, v in out.items()}
    return c


def rel(x, ref, scale=None):
    ref = np.asarray(ref, np.float64)
    return float(np.abs(np.asarray(x, np.float64) - ref).max() / (np.abs(ref).max() if scale is None else scale))


def blocks(g, dims):
    ns, h, na, nc = dims
    return np.split(g, np.cumsum([h * ns, h, h * nc, h, na * h]))


@pytest.mark.parametrize("L", [1, 4, 5, 64])
def test_levels_are_the_philox_words_of_the_header(L):
    import rlhip as rl

    ns, h, na, nc, n, base, step = 3, 32, 2, 4, 9, 1000, 6
    net = rl.IQNApproximator(ns, h, na, nc, seed=1)
    x = torch.randn(ns, n, device="cuda")
    tau = torch.empty(L, n, device="cuda")
    tau2 = torch.empty(L, n, device="cuda")
    rl.iqn_forward(net.params, ns, h, na, nc, L, 0, x, SEED, base, step, tau=tau)
    rl.iqn_plan(net.params, ns, h, na, nc, L, 0, x, 0.1, SEED, base, step, tau=tau2)
    want = philox_levels(L, range(base, base + n), step, TAG_PLAN)
    assert np.array_equal(host(tau), want.astype(F32)) and torch.equal(tau, tau2)
    Np = {1: 64, 4: 5, 5: 4, 64: 1}[L]
    to, tt = torch.empty(L, n, device="cuda"), torch.empty(Np, n, device="cuda")
    a, r, term = torch.zeros(n, dtype=torch.int32, device="cuda"), torch.zeros(n, device="cuda"), torch.zeros(n, dtype=torch.uint8, device="cuda")
    rl.iqn_grad_batch(ns, h, na, nc, L, Np, 0, KAPPA, net.params, net.params, x, a, r, term, x, GAMMA, SEED, CTR, tau=to, tau_target=tt)
    assert np.array_equal(host(to), philox_levels(L, range(n), CTR, TAG_ONLINE).astype(F32))
    assert np.array_equal(host(tt), philox_levels(Np, range(n), CTR, TAG_TARGET).astype(F32))


#           ns  h    na nc  K   n  act seed
FWD = {"min": (2, 32, 1, 2, 1, 1, 0, 0), "max": (16, 256, 4, 64, 64, 9, 0, 2), "n33": (4, 32, 4, 64, 5, 33, 1, 0), "k64": (3, 64, 2, 10, 64, 33, 0, 0)}


@functools.lru_cache(maxsize=None)
def fwd_case(name, dtype=torch.float64):
    ns, h, na, nc, K, n, act, seed = FWD[name]
    rng = np.random.default_rng([seed, n, h, 1])
    c = dict(params=make_net(rng, ns, h, na, nc, False), x=rng.uniform(-1, 1, (ns, n)).astype(F32), tau=philox_levels(K, range(40, 40 + n), 3, TAG_PLAN))
    th, zpsi, zphi = R.net(torch.tensor(c["params"]).to(dtype), (ns, h, na, nc), act, torch.tensor(c["x"]).to(dtype), torch.tensor(c["tau"]).to(dtype))
    c["th"] = th.double().numpy()
    c["zmin"] = min(float(zphi.abs().min()), float(zpsi.abs().min()) if act == 0 else np.inf)
    return c


@pytest.mark.parametrize("name", list(FWD))
def test_forward_and_plan(name):
    import rlhip as rl

    ns, h, na, nc, K, n, act, _ = FWD[name]
    c = fwd_case(name)
    assert c["zmin"] >= ZMIN, f"{name}: a relu pre-activation of the reference is {c['zmin']:.1e} from zero; choose another seed"
    p, x = torch.tensor(c["params"]).cuda(), torch.tensor(c["x"]).cuda()
    th, tau = torch.empty(na * K, n, device="cuda"), torch.empty(K, n, device="cuda")
    q = rl.iqn_forward(p, ns, h, na, nc, K, act, x, SEED, 40, 3, quantiles=th, tau=tau)
    assert np.array_equal(host(tau), c["tau"].astype(F32))
    want = c["th"].transpose(1, 0, 2).reshape(na * K, n)  # row k + K o
    eth, eq = rel(host(th), want), rel(host(q), c["th"].mean(0), np.abs(want).max())
    print(f"iqn forward {name}: quantiles {eth:.2e}, Q {eq:.2e} of max|theta| (bar {BAR:.1e})")
    assert eth <= BAR and eq <= BAR
    actions, q2 = rl.iqn_plan(p, ns, h, na, nc, K, act, x, 0.3, SEED, 40, 3)
    assert torch.equal(q2, q), "plan's Q differs from forward's"
    assert torch.equal(actions, rl.ops.eps_greedy_select(q, 0.3, SEED, 3, env_id_base=40))


@pytest.mark.parametrize("name", list(GRAD))
def test_gradient_against_float64_autograd(name):
    import rlhip as rl

    c = grad_case(name)
    ref, (ns, h, na, nc), N, Np, b = c["ref"], c["dims"], c["N"], c["Np"], c["b"]
    assert ref["zmin"] >= ZMIN and ref["margin"] >= MARGIN, f"{name}: reference decisions too close (|z| {ref['zmin']:.1e}, a* margin {ref['margin']:.1e})"
    if name in CARRY:
        rows = int(rl._lib.lib.rlhip_iqn_workspace_bytes(ns, h, na, nc, N, Np, b)) // (4 * (rl.iqn_nparams(ns, h, na, nc) + 1))
        assert rows >= 1 and 8 * rows < b, f"{name}: {rows} workgroups for {b} samples: no workgroup takes a second tile"
    d = {k: torch.tensor(c[k]).cuda() for k in ("params", "target", "s", "sn", "a", "r", "term", "n_used", "weights")}
    outs = []
    for _ in range(2):
        o = dict(ql=torch.empty(b, device="cuda"), target=torch.empty(Np, b, device="cuda"), sel=torch.empty(b, dtype=torch.int32, device="cuda"),
                 tau=torch.empty(N, b, device="cuda"), tau_target=torch.empty(Np, b, device="cuda"))
        o["grad"], o["loss"] = rl.iqn_grad_batch(ns, h, na, nc, N, Np, c["act"], KAPPA, d["params"], d["target"], d["s"], d["a"], d["r"], d["term"],
                                                 d["sn"], GAMMA, SEED, CTR, d["n_used"], d["weights"], c["double"], **o)
        outs.append({k: host(v) for k, v in o.items()})
    g = outs[0]
    assert all(np.array_equal(outs[0][k], outs[1][k]) for k in g), "two calls differ"
    assert np.array_equal(g["tau"], c["tau"].astype(F32)) and np.array_equal(g["tau_target"], c["taup"].astype(F32))
    assert np.array_equal(g["sel"], ref["sel"])
    if b > 1:
        assert g["ql"][b // 2] == 0.0 and ref["ql"][b // 2] == 0.0  # the action out of range
    gmax = np.abs(ref["grad"]).max()
    errs = dict(target=rel(g["target"], ref["target"]), ql=rel(g["ql"], ref["ql"]), loss=rel(g["loss"], ref["loss"], max(abs(float(ref["loss"])), 1e-30)))
    for nm, gb, rb in zip(("dW1", "db1", "dWphi", "dbphi", "dW2", "db2"), blocks(g["grad"], c["dims"]), blocks(ref["grad"], c["dims"])):
        errs[nm] = rel(gb, rb, gmax)
    print(f"iqn gradient {name}: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()) + f" (bar {BAR:.1e})")
    assert max(errs.values()) <= BAR, errs


# ------------------------------------------------------------------------------------------------------------------ learner
N_ENV, CAP, PUSHES, NA = 8, 24, 30, 3
FORMS = {"uniform-records": dict(ns=4), "nstep3-records": dict(ns=4, n_step=3, double_dqn=True), "per-records": dict(ns=4, per=True, per_beta=0.4),
         "per-nstep3-records": dict(ns=3, per=True, per_beta=0.4, n_step=3, double_dqn=True), "uniform-frames": dict(ns=6, double_dqn=True),
         "nstep3-frames": dict(ns=6, n_step=3), "per-frames": dict(ns=6, per=True, per_beta=0.5), "per-nstep3-frames": dict(ns=6, per=True, per_beta=0.5, n_step=3, double_dqn=True)}


@pytest.mark.parametrize("form", list(FORMS))
def test_an_update_is_the_gradient_entry_then_clip_adam(form):
    import rlhip as rl

    kw = dict(FORMS[form])
    ns, per, n_step = kw.pop("ns"), kw.pop("per", False), kw.get("n_step", 1)
    h, nc, b, seed = 32, 8, 33, 11
    rng = np.random.default_rng(4242)
    up = lambda x: torch.tensor(np.ascontiguousarray(x), device="cuda")  # noqa: E731
    net = rl.IQNApproximator(ns, h, NA, nc, act="tanh" if n_step > 1 else "relu", lr=1e-3, seed=seed)
    tn = rl.TargetNetwork(net, sync_freq=2)
    learner = rl.IQNLearner(tn, NA, N=5, N_target=3, K=4, batchsize=b, gamma=0.9, min_replay_history=N_ENV, seed=seed, max_grad_norm=0.5, per_eps=1e-3, **kw)
    if per:
        tr = (rl.CircularPrioritizedFrameTraces if ns > 4 else rl.CircularPrioritizedTraces)(CAP, N_ENV, ns, n_step=n_step, default_priority=2.0)
    else:
        tr = rl.CircularArraySARTSTraces(CAP, N_ENV, ns)
    tr.push_state_(up(rng.normal(0, 1, (ns, N_ENV)).astype(F32)))
    for _ in range(PUSHES):
        tr.push_transition_(up(rng.normal(0, 1, (ns, N_ENV)).astype(F32)), up(rng.integers(0, NA, N_ENV).astype(np.int32)),
                            up(rng.normal(0.2, 1.0, N_ENV).astype(F32)), up((rng.uniform(size=N_ENV) < 0.15).astype(np.uint8)))
    traj = rl.Trajectory(tr, controller=rl.InsertSampleRatioController(ratio=1e9, threshold=1, n_inserted=PUSHES))
    for u in range(3):
        p0, t0, m, v, bp = (x.clone() for x in (net.params, tn.target, net.m, net.v, net.beta_pow))
        assert learner.optimise_(traj) is True and learner.n_updates == u + 1 and learner.draw_ctr == u + 1
        s, a, r, t, sn, n_used = learner._batch.t
        folded = n_step > 1 and ns <= 4  # the record rings fold the window: one discount gamma^n
        gamma = float(oracle.gamma_pow(0.9, n_step)) if folded else 0.9
        weights = learner.is_weights if per else None
        ql = torch.empty(b, device="cuda")
        grad, loss = rl.iqn_grad_batch(ns, h, NA, nc, 5, 3, net.act, 1.0, p0, t0, s, a, r, t, sn, gamma, seed, u, n_used, weights, learner.double_dqn, ql=ql)
        assert torch.equal(loss, learner.loss) and float(loss) > 0
        if per:  # (ql + eps)^alpha of the UNWEIGHTED loss was written back in place
            assert torch.allclose(learner.ql, (ql + 1e-3) ** 0.6, rtol=1e-5)
        rl.ops.clip_adam_(p0, grad, m, v, bp, 1.0, 0.5, 1e-3, 0.9, 0.999, 1e-8, torch.zeros(1, device="cuda"))
        assert torch.equal(grad, learner.grad)  # (both clipped in place)
        assert torch.equal(p0, net.params) and torch.equal(tn.target, net.params if (u + 1) % 2 == 0 else t0)


def _agent(rl, n=64, seed=5):
    env = rl.CartPoleEnv(n, seed=seed)
    learner = rl.IQNLearner(rl.TargetNetwork(rl.IQNApproximator(4, 64, 2, 16, seed=seed), sync_freq=10), 2, N=8, N_target=8, K=8, batchsize=64,
                            min_replay_history=5 * n, seed=seed)
    policy = rl.QBasedPolicy(learner, rl.EpsilonGreedyExplorer(0.05, kind="exp", decay_steps=20, seed=seed))
    return env, rl.Agent(policy, rl.Trajectory(rl.CircularArraySARTSTraces(64, n, 4)))


def test_run_and_a_checkpoint_continues_bit_identically():
    import rlhip as rl

    env, agent = _agent(rl)
    learner = agent.policy.learner
    rl.run(agent, env, rl.StopAfterNSteps(20))
    sd = rl.state_dict({"env": env, "agent": agent})
    rl.run(agent, env, rl.StopAfterNSteps(20))
    assert learner.vec_steps == 40 and learner.n_updates == 36
    q, th, tau = learner.quantiles(env.state(), step=7)
    assert q.shape == (2, 64) and th.shape == (8, 2, 64) and tau.shape == (8, 64)
    assert float((th.mean(0) - q).abs().max()) <= 1e-5 * max(1.0, float(q.abs().max()))
    env2, agent2 = _agent(rl)
    rl.load_state_dict({"env": env2, "agent": agent2}, sd)
    rl.run(agent2, env2, rl.StopAfterNSteps(20))
    l2 = agent2.policy.learner
    for x, y in ((learner.approximator.network.params, l2.approximator.network.params), (learner.approximator.target, l2.approximator.target),
                 (learner.approximator.network.v, l2.approximator.network.v), (learner.grad, l2.grad), (env.state(), env2.state())):
        assert torch.equal(x, y), "the run does not continue bit-identically from the checkpoint"
    with pytest.raises(NotImplementedError, match="IQNLearner"):
        rl.run_fused_dqn(agent, env, rl.StopAfterNSteps(1))


LEARN_STEPS = 2000  # from the measured curve (profiles/iqn.md): 3 x random is cleared after 1000 vec-steps; the cap is QR-DQN's 6500


def test_it_learns_cartpole():
    import rlhip as rl
    from test_gpu_learn import _random_policy_episode_length

    n, cap, chunk = 4096, 256, 500
    base = _random_policy_episode_length(rl)
    assert 15.0 < base < 30.0, base
    env = rl.CartPoleEnv(n, seed=5)
    net = rl.IQNApproximator(4, 128, 2, 64, seed=5)
    learner = rl.IQNLearner(rl.TargetNetwork(net, sync_freq=100), 2, N=32, N_target=32, K=32, batchsize=512, min_replay_history=n, seed=5)
    policy = rl.QBasedPolicy(learner, rl.EpsilonGreedyExplorer(0.01, kind="exp", decay_steps=500, seed=5))
    tr = rl.CircularArraySARTSTraces(capacity=cap, n_env=n, obs_dim=4)
    agent = rl.Agent(policy, rl.Trajectory(tr))
    curve = []
    for _ in range(LEARN_STEPS // chunk):
        rl.run(agent, env, rl.StopAfterNSteps(chunk))
        term = tr.gather(torch.arange(len(tr) * n, device="cuda"))[3]
        curve.append(round(len(tr) * n / max(1.0, float(term.sum())), 1))
    print(f"IQNLearner on CartPole: random {base:.1f}, mean episode length per {chunk} vec-steps {curve}, updates {learner.n_updates}")
    assert torch.isfinite(net.params).all()
    assert max(curve) >= 3.0 * 21.6, f"mean episode length never reached 3 x the random policy's 21.6: {curve}"
