"""The FQF kernels and FQFLearner on the device against the float64 model of tests/fqf_ref.py.

Stage 1     tau_out, tau_hat_out, ent_out of the gradient entry (and of forward) against the model's own fraction stage.
Stage 2     everything behind the levels with the model teacher-forced on the kernel's own tau_out: sel_out equal; quantiles, Q,
            target_out, ql_out, loss, grad_out and frac_grad_out relative to the largest reference magnitude of the output.
Bars        4 x FLOOR[output].  A floor is the largest distance, over these cases, of the SAME model evaluated in Float32 torch on the
            CPU from the float64 model (stage 2: both forced on the Float32 model's levels); per case in profiles/fqf.md.  The bars are
            never taken from the kernel.
Ties        no case is left out: every seed is chosen so that the model's top-two gap of Q(s') is >= 100 x the Q floor; asserted.
Envelope    the NEW cases launch what the one-axis cases never reach: the corner of the envelope (17 dW1 elements per thread, the unit
            blocks wave + 4 of dWphi, Wf filling the phi buffer), h 160 (block 4 is wave 0's alone), a second tile per workgroup (every
            chain carried: registers, the MFMA accumulators, dWf | dbf through the partial row) and n_used outside 0 .. 32.  Their floors
            exceed the constants, so a new case's bar is 4 x max(FLOOR[k], the case's own floor), the floor computed here on the CPU by
            the method above.  Beside the a* rule they assert the same rule for relu signs: the model's smallest |pre-activation| is
            >= 100 x the largest distance of the Float32 model's pre-activations from the float64 model's.  tests/test_fqf_reference.py
            asserts both rules for every case without a GPU.
Bytes       plan = forward + eps_greedy_select, also with env ids that wrap 2^32; two gradient calls return the same bytes.
Learner     three updates on a prioritized n-step record ring against the gradient entry and the model; IQN's eight update forms
            teacher-forced against the gradient entry -> clip_adam_; checkpoint resume; the fused loops' refusal; CartPole."""
import functools

import numpy as np
import pytest
import torch

import fqf_ref as R
from test_gpu_iqn import CAP, FORMS, N_ENV, NA, PUSHES  # the eight update forms and the ring they are drawn from

pytestmark = pytest.mark.gpu

KAPPA, GAMMA, ENT = 1.0, 0.9, 0.05
FLOOR = dict(tau=1.76e-7, that=1.98e-7, ent=1.82e-7, th=5.85e-7, q=1.98e-7, target=1.68e-7, ql=1.24e-7, loss=9.36e-8, grad=3.86e-7, frac=3.15e-6)
BAR = {k: 4.0 * v for k, v in FLOOR.items()}
F32 = np.float32
host = lambda x: x.detach().cpu().numpy()  # noqa: E731

# one axis at a time around the base shape; every case with batch > 1 has a terminal sample and an action outside 0 .. na - 1
BASE = dict(ns=4, h=64, na=2, N=5, nc=4, b=9, act=0, double=False, null=False, seed=0, safe=False, n_used=None, term_at=0)
CASES = {"base": {}, "ns2": dict(ns=2), "ns6": dict(ns=6), "h32": dict(h=32), "h96": dict(h=96), "na1": dict(na=1), "na3": dict(na=3),
         "N2": dict(N=2), "N32": dict(N=32), "nc2": dict(nc=2), "nc64": dict(nc=64, seed=64), "b1": dict(b=1), "b8": dict(b=8), "b20": dict(b=20),
         "tanh": dict(act=1), "double": dict(double=True), "null": dict(null=True)}  # null: weights and n_used are NULL
# (nc64: seed 0 left a pre-activation 2.4e-4 from zero, under the relu-sign rule's 3.9e-4; FLOOR keeps the seed-0 figures)
CORNER = dict(ns=16, h=256, na=4, nc=64, N=32)  # every bound of the envelope at once: 160064 of 163840 bytes of LDS
# safe: IQN's recipe for ~1e7 pre-activations (no relu comes near zero).  carry-*: more tiles than workgroups, so workgroup 0 takes a
# full second tile and workgroup 1 a tile of 9 - 8 = 1 or 3 samples; at the corner's row size the cap is 138 workgroups, not 256
NEW = {"corner": dict(CORNER, double=True, seed=468), "corner-tanh": dict(CORNER, act=1, seed=331), "h160": dict(h=160, na=4, nc=34),
       "carry-smallest": dict(ns=2, h=32, na=1, nc=2, N=2, b=8 * 256 + 9, double=True, safe=True), "carry-base": dict(b=8 * 256 + 3, safe=True),
       "carry-wide": dict(CORNER, b=8 * 138 + 3, safe=True),
       # (the terminal sample is not sample 0: a terminal sample has no discount to check, and -5 is its n_used)
       "nused-edges": dict(n_used=(-5, 0, 1, 31, 32, 33, 1000, 2 ** 31 - 1, 2), term_at=2)}
CARRY = ("carry-smallest", "carry-base", "carry-wide")  # asserted below: more than one tile per workgroup
CASES.update(NEW)


def make_nets(rng, ns, h, na, nc, N, safe=False):
    """biases away from zero, so that few (safe, the recipe of test_gpu_iqn.make_net: no) relu pre-activations come near zero; fraction
    logits spread enough for uneven fractions"""
    sgn = lambda n: rng.choice([-1.0, 1.0], n)  # noqa: E731
    s1, sp = (0.25 / ns, 0.4 / nc) if safe else (0.5 / np.sqrt(ns), 0.6 / np.sqrt(nc))
    q = lambda: np.concatenate([rng.uniform(-1, 1, h * ns) * s1, rng.uniform(0.3, 1.0, h) * sgn(h),  # noqa: E731
                                rng.uniform(-1, 1, h * nc) * sp, rng.uniform(0.5, 1.5, h) * sgn(h),
                                rng.uniform(-2, 2, na * h) / np.sqrt(h), rng.uniform(-0.5, 0.5, na)]).astype(F32)
    return q(), q(), np.concatenate([rng.uniform(-2, 2, N * h) / np.sqrt(h), rng.uniform(-0.5, 0.5, N)]).astype(F32)


@functools.lru_cache(maxsize=None)
def case(name):
    k = dict(BASE, **CASES[name])
    ns, h, na, nc, N, b = (k[x] for x in ("ns", "h", "na", "nc", "N", "b"))
    rng = np.random.default_rng([k["seed"], b, h, N])
    c = dict(k, dims=(ns, h, na, nc))
    c["params"], c["target"], c["frac"] = make_nets(rng, ns, h, na, nc, N, k["safe"])
    c.update(s=rng.uniform(-1, 1, (ns, b)).astype(F32), sn=rng.uniform(-1, 1, (ns, b)).astype(F32), a=rng.integers(0, na, b).astype(np.int32),
             r=rng.normal(0.2, 1.0, b).astype(F32), term=np.zeros(b, np.uint8), n_used=rng.integers(0, 4, b).astype(np.int32),
             weights=rng.uniform(0.3, 1.0, b).astype(F32))
    if k["n_used"] is not None:
        c["n_used"] = np.array(k["n_used"], np.int32)
    if b > 1:
        c["term"][k["term_at"]], c["a"][b // 2] = 1, na
    return c


def model(name, dtype=torch.float64, tau=None):
    """the model on a case -> numpy outputs; tau: teacher-forced levels ((N + 1, b) array)"""
    c = case(name)
    t = lambda v: torch.tensor(v.astype(np.float64)).to(dtype) if v.dtype.kind == "f" else torch.tensor(v.astype(np.int64))  # noqa: E731
    p, pf = t(c["params"]).requires_grad_(True), t(c["frac"]).requires_grad_(True)
    opt = (None, None) if c["null"] else (t(c["n_used"]), t(c["weights"]))
    out = R.loss(p, t(c["target"]), pf, c["dims"], c["N"], c["act"], KAPPA, ENT, t(c["s"]), t(c["a"]), t(c["r"]), t(c["term"]), t(c["sn"]), GAMMA,
                 *opt, c["double"], None if tau is None else t(np.asarray(tau)))
    out["grad"], out["fgrad"] = torch.autograd.grad(out["loss"], p)[0], torch.autograd.grad(out["frac_loss"], pf)[0]
    with torch.no_grad():
        f = R.forward(p, pf, c["dims"], c["N"], c["act"], t(c["s"]), out["tau"])
    out.update(th=f["th"], q=f["q"])
    return {k: (v.detach().double().numpy() if torch.is_tensor(v) else v) for k, v in out.items()}


def rel(x, ref, scale=None):
    ref = np.asarray(ref, np.float64)
    return float(np.abs(np.asarray(x, np.float64) - ref).max() / max(np.abs(ref).max() if scale is None else scale, 1e-30))


def distances(got, ref):
    """the distance of every output (stage 2 names) from the reference"""
    return dict(th=rel(got["th"], ref["th"]), q=rel(got["q"], ref["q"], np.abs(ref["th"]).max()), target=rel(got["target"], ref["target"]),
                ql=rel(got["ql"], ref["ql"]), loss=rel(got["loss"], ref["loss"]), grad=rel(got["grad"], ref["grad"]),
                frac=rel(got["fgrad"], ref["fgrad"]))


@functools.lru_cache(maxsize=None)
def floors(name):
    """the case's own Float32 floor per output, on the CPU: stage 1 each model on its own fractions, stage 2 both on the Float32 model's
    levels -> (floor, the float64 model on its own fractions, decisions: both models' a* margin / zmin / sel and `zdist`, the largest
    distance of a Float32 pre-activation from its float64 one)"""
    own = model(name)
    own["zs"] = None  # (the largest arrays of a case: held no longer than needed)
    m32 = model(name, torch.float32)
    m64 = model(name, tau=m32["tau"])
    fl = dict(tau=rel(m32["tau"], own["tau"]), that=rel(m32["that"], own["that"]), ent=rel(m32["ent"], own["ent"], max(1.0, np.abs(own["ent"]).max())),
              **distances(m32, m64))
    zdist = max(float((a.double() - b).abs().max()) for a, b in zip(m32["zs"], m64["zs"]))
    dec = dict(zdist=zdist, zmin=min(m64["zmin"], own["zmin"]), margin=min(m64["margin"], own["margin"]), thmax=float(np.abs(m64["th"]).max()),
               sel=(m32["sel"], m64["sel"], own["sel"]))
    return fl, own, dec


def bars(name):
    """-> (floor, bar) per output: an old case's bar is the constant's, a new case's 4 x max(the constant, the case's own floor)"""
    if name not in NEW:
        return FLOOR, BAR
    fl = {k: max(FLOOR[k], v) for k, v in floors(name)[0].items()}
    return fl, {k: 4.0 * v for k, v in fl.items()}


def decisions_hold(name, ref, fl):
    """the a* rule (every case) and the relu-sign rule (new cases) on the model `ref`; fl: the floors of the case's bars"""
    assert ref["margin"] >= 100 * fl["q"] * np.abs(ref["th"]).max(), f"{name}: a* margin {ref['margin']:.1e}; choose another seed"
    if name in NEW:
        zdist = floors(name)[2]["zdist"]
        assert ref["zmin"] >= 100 * zdist, f"{name}: a pre-activation is {ref['zmin']:.1e} from zero, 100 x the Float32 distance is {100 * zdist:.1e}"


def device_case(name):
    c = case(name)
    d = {k: torch.tensor(c[k]).cuda() for k in ("params", "target", "frac", "s", "sn", "a", "r", "term", "n_used", "weights")}
    if c["null"]:
        d["n_used"] = d["weights"] = None
    return c, d


@pytest.mark.parametrize("name", list(CASES))
def test_gradient_entry_against_the_float64_model(name):
    import rlhip as rl

    c, d = device_case(name)
    (ns, h, na, nc), N, b = c["dims"], c["N"], c["b"]
    if name in CARRY:
        rows = int(rl._lib.lib.rlhip_fqf_workspace_bytes(ns, h, na, nc, N, b)) // (4 * (rl.iqn_nparams(ns, h, na, nc) + rl.fqf_frac_nparams(h, N) + 1))
        assert rows >= 1 and 8 * rows < b, f"{name}: {rows} workgroups for {b} samples: no workgroup takes a second tile"
    outs = []
    for _ in range(2):
        o = dict(ql=torch.empty(b, device="cuda"), target=torch.empty(N, b, device="cuda"), sel=torch.empty(b, dtype=torch.int32, device="cuda"),
                 tau=torch.empty(N + 1, b, device="cuda"), tau_hat=torch.empty(N, b, device="cuda"), ent=torch.empty(b, device="cuda"))
        o["grad"], o["fgrad"], o["loss"] = rl.fqf_grad_batch(ns, h, na, nc, N, c["act"], KAPPA, ENT, d["params"], d["target"], d["frac"], d["s"],
                                                             d["a"], d["r"], d["term"], d["sn"], GAMMA, d["n_used"], d["weights"], c["double"], **o)
        outs.append({k: host(v) for k, v in o.items()})
    g = outs[0]
    assert all(np.array_equal(outs[0][k], outs[1][k]) for k in g), "two calls differ"
    own = floors(name)[1] if name in NEW else model(name)  # stage 1: the model's own fractions
    fl, bar = bars(name)
    assert g["tau"][0].max() == 0.0 and g["tau"][N].min() == 1.0 and (np.diff(g["tau"], axis=0) >= 0).all()
    e1 = dict(tau=rel(g["tau"], own["tau"]), that=rel(g["tau_hat"], own["that"]), ent=rel(g["ent"], own["ent"], max(1.0, np.abs(own["ent"]).max())))
    ref = model(name, tau=g["tau"])  # stage 2: teacher-forced on the kernel's levels
    decisions_hold(name, ref, fl)
    assert np.array_equal(g["sel"], ref["sel"])
    if b > 1:
        assert g["ql"][b // 2] == 0.0 and ref["ql"][b // 2] == 0.0  # the action out of range
    th, ftau, fthat = torch.empty(na * N, b, device="cuda"), torch.empty(N + 1, b, device="cuda"), torch.empty(N, b, device="cuda")
    g["q"] = host(rl.fqf_forward(d["params"], d["frac"], ns, h, na, nc, N, c["act"], d["s"], quantiles=th, tau=ftau, tau_hat=fthat))
    g["th"] = host(th).reshape(na, N, b).transpose(1, 0, 2)
    assert np.array_equal(host(ftau), g["tau"]) and np.array_equal(host(fthat), g["tau_hat"]), "forward and the gradient entry place different levels"
    errs = dict(e1, **distances(g, ref))
    if name in NEW:
        print(f"fqf {name} floor: " + ", ".join(f"{k} {v:.2e}" for k, v in floors(name)[0].items()))
    print(f"fqf {name}: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert all(errs[k] <= bar[k] for k in errs), {k: (v, bar[k]) for k, v in errs.items() if v > bar[k]}


@pytest.mark.parametrize("name", ["corner", "corner-tanh"])
def test_forward_at_the_corner_of_the_envelope(name):
    """n = T + 1 = 9 envs: a full tile and a tile of one"""
    import rlhip as rl

    c, d = device_case(name)
    (ns, h, na, nc), N, b = c["dims"], c["N"], c["b"]
    (fl, bar), own = bars(name), floors(name)[1]
    th, tau, that = torch.empty(na * N, b, device="cuda"), torch.empty(N + 1, b, device="cuda"), torch.empty(N, b, device="cuda")
    g = dict(q=host(rl.fqf_forward(d["params"], d["frac"], ns, h, na, nc, N, c["act"], d["s"], quantiles=th, tau=tau, tau_hat=that)))
    g.update(th=host(th).reshape(na, N, b).transpose(1, 0, 2), tau=host(tau), that=host(that))
    assert g["tau"][0].max() == 0.0 and g["tau"][N].min() == 1.0 and (np.diff(g["tau"], axis=0) >= 0).all()
    with torch.no_grad():  # stage 2: the model forced on forward's levels
        t = lambda v: torch.tensor(np.asarray(v, np.float64))  # noqa: E731
        ref = R.forward(t(c["params"]), t(c["frac"]), c["dims"], N, c["act"], t(c["s"]), t(g["tau"]))
    thmax = float(ref["th"].abs().max())
    errs = dict(tau=rel(g["tau"], own["tau"]), that=rel(g["that"], own["that"]), th=rel(g["th"], ref["th"].numpy()), q=rel(g["q"], ref["q"].numpy(), thmax))
    print(f"fqf forward {name} floor: " + ", ".join(f"{k} {fl[k]:.2e}" for k in errs))
    print(f"fqf forward {name}: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert all(errs[k] <= bar[k] for k in errs), {k: (v, bar[k]) for k, v in errs.items() if v > bar[k]}


@pytest.mark.parametrize("name", ["base", "corner"])
def test_plan_with_env_ids_that_wrap(name):
    """n = 2 T + 1 = 17 envs from env_id_base = 2^32 - 3: the ids wrap inside the first tile"""
    import rlhip as rl

    c, d = device_case(name)
    (ns, h, na, nc), N, n, base = c["dims"], c["N"], 17, 2 ** 32 - 3
    x = torch.tensor(np.random.default_rng([7, h]).uniform(-1, 1, (ns, n)).astype(F32)).cuda()
    q = rl.fqf_forward(d["params"], d["frac"], ns, h, na, nc, N, c["act"], x)
    for eps in (0.0, 0.3):
        actions, q2 = rl.fqf_plan(d["params"], d["frac"], ns, h, na, nc, N, c["act"], x, eps, 77, base, 3)
        assert torch.equal(q2, q), "plan's Q differs from forward's"
        assert torch.equal(actions, rl.ops.eps_greedy_select(q, eps, 77, 3, env_id_base=base))


@pytest.mark.parametrize("name", ["base", "N32", "b20", "tanh"])
def test_plan_is_forward_then_eps_greedy_select(name):
    import rlhip as rl

    c, d = device_case(name)
    (ns, h, na, nc), N, b = c["dims"], c["N"], c["b"]
    tau, that = torch.empty(N + 1, b, device="cuda"), torch.empty(N, b, device="cuda")
    q = rl.fqf_forward(d["params"], d["frac"], ns, h, na, nc, N, c["act"], d["s"], tau=tau, tau_hat=that)
    gt = torch.empty(N + 1, b, device="cuda")
    rl.fqf_grad_batch(ns, h, na, nc, N, c["act"], KAPPA, ENT, d["params"], d["target"], d["frac"], d["s"], d["a"], d["r"], d["term"], d["sn"], GAMMA, tau=gt)
    assert torch.equal(tau, gt), "forward and the gradient entry place different levels on the same states"
    actions, q2 = rl.fqf_plan(d["params"], d["frac"], ns, h, na, nc, N, c["act"], d["s"], 0.3, 77, 40, 3)
    assert torch.equal(q2, q), "plan's Q differs from forward's"
    assert torch.equal(actions, rl.ops.eps_greedy_select(q, 0.3, 77, 3, env_id_base=40))


@pytest.mark.parametrize("kw", [dict(N=1), dict(N=33), dict(h=48)], ids=str)
def test_envelope_edges_are_refused(kw):
    import rlhip as rl

    a = dict(dict(ns=4, h=64, na=2, nc=4, N=5), **kw)
    assert rl._lib.lib.rlhip_fqf_workspace_bytes(a["ns"], a["h"], a["na"], a["nc"], a["N"], 9) == -1
    x = torch.zeros(a["ns"], 9, device="cuda")
    p = torch.zeros(rl.iqn_nparams(a["ns"], a["h"], a["na"], a["nc"]) + 64, device="cuda")
    with pytest.raises(rl._lib.RLHipArgumentError):
        rl.fqf_forward(p, torch.zeros(a["N"] * a["h"] + a["N"], device="cuda"), a["ns"], a["h"], a["na"], a["nc"], a["N"], 0, x)
    with pytest.raises(ValueError):
        rl.FQFLearner(rl.TargetNetwork(rl.FQFApproximator(a["ns"], a["h"], a["na"], a["N"], a["nc"])), a["na"], a["N"], a["nc"])


# ------------------------------------------------------------------------------------------------------------------ learner
def test_three_updates_on_a_prioritized_nstep_record_ring():
    import oracle
    import rlhip as rl

    ns, h, na, nc, N, b, seed, n_env, n_step = 3, 32, 3, 8, 5, 33, 11, 8, 3
    rng = np.random.default_rng(4242)
    up = lambda x: torch.tensor(np.ascontiguousarray(x), device="cuda")  # noqa: E731
    net = rl.FQFApproximator(ns, h, na, N, nc, act="tanh", lr=1e-3, frac_lr=1e-4, seed=seed)
    net.frac_params.mul_(100.0)  # (the paper's x 0.01 initialisation leaves the fractions uniform to the last bits)
    tn = rl.TargetNetwork(net, sync_freq=2)
    learner = rl.FQFLearner(tn, na, N, nc, ent_coef=ENT, batchsize=b, gamma=0.9, min_replay_history=n_env, seed=seed, per_eps=1e-3, per_beta=0.4,
                            n_step=n_step, double_dqn=True)
    tr = rl.CircularPrioritizedTraces(24, n_env, ns, n_step=n_step, default_priority=2.0)
    tr.push_state_(up(rng.normal(0, 1, (ns, n_env)).astype(F32)))
    for _ in range(30):
        tr.push_transition_(up(rng.normal(0, 1, (ns, n_env)).astype(F32)), up(rng.integers(0, na, n_env).astype(np.int32)),
                            up(rng.normal(0.2, 1.0, n_env).astype(F32)), up((rng.uniform(size=n_env) < 0.15).astype(np.uint8)))
    traj = rl.Trajectory(tr, controller=rl.InsertSampleRatioController(ratio=1e9, threshold=1, n_inserted=30))
    gamma = float(oracle.gamma_pow(0.9, n_step))  # the record rings fold the window: one discount gamma^n
    for u in range(3):
        p0, t0, f0 = net.params.clone(), tn.target.clone(), net.frac_params.clone()
        st = [x.clone() for x in (net.m, net.v, net.beta_pow, net.frac_m, net.frac_v, net.frac_beta_pow)]
        assert learner.optimise_(traj) is True and learner.n_updates == u + 1
        s, a, r, t, sn, n_used = learner._batch.t
        ql, tau = torch.empty(b, device="cuda"), torch.empty(N + 1, b, device="cuda")
        grad, fgrad, loss = rl.fqf_grad_batch(ns, h, na, nc, N, net.act, 1.0, ENT, p0, t0, f0, s, a, r, t, sn, gamma, n_used, learner.is_weights,
                                              True, ql=ql, tau=tau)
        assert torch.equal(loss, learner.loss) and torch.equal(grad, learner.grad) and torch.equal(fgrad, net.frac_grad)
        assert torch.allclose(learner.ql, (ql + 1e-3) ** 0.6, rtol=1e-5)  # (ql + eps)^alpha of the UNWEIGHTED loss, written back in place
        t64 = lambda x: x.detach().cpu().double() if x.dtype.is_floating_point else x.detach().cpu().long()  # noqa: E731
        p, pf = t64(p0).requires_grad_(True), t64(f0).requires_grad_(True)
        ref = R.loss(p, t64(t0), pf, (ns, h, na, nc), N, net.act, 1.0, ENT, t64(s), t64(a), t64(r), t64(t), t64(sn), gamma, None if n_used is None else t64(n_used),
                     t64(learner.is_weights), True, t64(tau))
        eg = rel(host(grad), torch.autograd.grad(ref["loss"], p)[0].numpy())
        ef = rel(host(fgrad), torch.autograd.grad(ref["frac_loss"], pf)[0].numpy())
        print(f"fqf learner update {u}: grad {eg:.2e}, frac grad {ef:.2e}")
        assert eg <= BAR["grad"] and ef <= BAR["frac"]
        rl.ops.clip_adam_(p0, grad, st[0], st[1], st[2], 1.0, 0.0, 1e-3, 0.9, 0.999, 1e-8, torch.zeros(1, device="cuda"))
        rl.ops.clip_adam_(f0, fgrad, st[3], st[4], st[5], 1.0, 0.0, 1e-4, 0.9, 0.999, 1e-8, torch.zeros(1, device="cuda"))
        assert torch.equal(p0, net.params) and torch.equal(f0, net.frac_params)
        assert torch.equal(tn.target, net.params if (u + 1) % 2 == 0 else t0)  # the target network is the quantile vector's


@pytest.mark.parametrize("form", list(FORMS))
def test_an_update_is_the_gradient_entry_then_clip_adam(form):
    """IQN's eight update forms (test_gpu_iqn.FORMS).  The frame rings (ns 6) hand the kernel a per-sample n_used with the unfolded
    gamma; the record rings fold the window to one discount gamma^n.  The 3-step forms clip (0.5), the 1-step forms do not, so there
    the learner's gradients are the entry's bytes before any scaling"""
    import oracle
    import rlhip as rl

    kw = dict(FORMS[form])
    ns, per, n_step = kw.pop("ns"), kw.pop("per", False), kw.get("n_step", 1)
    h, nc, N, b, seed = 32, 8, 5, 33, 11
    clip = 0.5 if n_step > 1 else 0.0
    rng = np.random.default_rng(4242)
    up = lambda x: torch.tensor(np.ascontiguousarray(x), device="cuda")  # noqa: E731
    net = rl.FQFApproximator(ns, h, NA, N, nc, act="tanh" if n_step > 1 else "relu", lr=1e-3, frac_lr=1e-4, seed=seed)
    net.frac_params.mul_(100.0)  # (the paper's x 0.01 initialisation leaves the fractions uniform to the last bits)
    tn = rl.TargetNetwork(net, sync_freq=2)
    learner = rl.FQFLearner(tn, NA, N, nc, ent_coef=ENT, batchsize=b, gamma=0.9, min_replay_history=N_ENV, seed=seed, max_grad_norm=clip, per_eps=1e-3, **kw)
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
        p0, t0, f0 = net.params.clone(), tn.target.clone(), net.frac_params.clone()
        st = [x.clone() for x in (net.m, net.v, net.beta_pow, net.frac_m, net.frac_v, net.frac_beta_pow)]
        assert learner.optimise_(traj) is True and learner.n_updates == u + 1
        s, a, r, t, sn, n_used = learner._batch.t
        folded = n_step > 1 and ns <= 4  # the record rings fold the window: one discount gamma^n
        assert folded or n_step == 1 or n_used is not None, "an unfolded window needs its per-sample n_used"
        gamma = float(oracle.gamma_pow(0.9, n_step)) if folded else 0.9
        weights = learner.is_weights if per else None
        ql = torch.empty(b, device="cuda")
        grad, fgrad, loss = rl.fqf_grad_batch(ns, h, NA, nc, N, net.act, 1.0, ENT, p0, t0, f0, s, a, r, t, sn, gamma, n_used, weights,
                                              learner.double_dqn, ql=ql)
        assert torch.equal(loss, learner.loss) and float(loss) > 0
        if clip == 0.0:
            assert torch.equal(grad, learner.grad) and torch.equal(fgrad, net.frac_grad)
        if per:  # (ql + eps)^alpha of the UNWEIGHTED loss was written back in place
            assert torch.allclose(learner.ql, (ql + 1e-3) ** 0.6, rtol=1e-5)
        rl.ops.clip_adam_(p0, grad, st[0], st[1], st[2], 1.0, clip, 1e-3, 0.9, 0.999, 1e-8, torch.zeros(1, device="cuda"))
        rl.ops.clip_adam_(f0, fgrad, st[3], st[4], st[5], 1.0, clip, 1e-4, 0.9, 0.999, 1e-8, torch.zeros(1, device="cuda"))
        assert torch.equal(grad, learner.grad) and torch.equal(fgrad, net.frac_grad)  # (each clipped in place by its own norm)
        assert torch.equal(p0, net.params) and torch.equal(f0, net.frac_params)
        assert torch.equal(tn.target, net.params if (u + 1) % 2 == 0 else t0)  # the target network is the quantile vector's


def _agent(rl, n=64, seed=5):
    env = rl.CartPoleEnv(n, seed=seed)
    net = rl.FQFApproximator(4, 64, 2, 8, 16, frac_lr=1e-4, seed=seed)
    learner = rl.FQFLearner(rl.TargetNetwork(net, sync_freq=10), 2, 8, 16, batchsize=64, min_replay_history=5 * n, seed=seed)
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
    q, th, tau, that = learner.quantiles(env.state())
    assert q.shape == (2, 64) and th.shape == (8, 2, 64) and tau.shape == (9, 64) and that.shape == (8, 64)
    env2, agent2 = _agent(rl)
    rl.load_state_dict({"env": env2, "agent": agent2}, sd)
    rl.run(agent2, env2, rl.StopAfterNSteps(20))
    n1, n2 = learner.approximator.network, agent2.policy.learner.approximator.network
    for x, y in ((n1.params, n2.params), (n1.frac_params, n2.frac_params), (n1.frac_v, n2.frac_v), (learner.approximator.target, agent2.policy.learner.approximator.target),
                 (learner.grad, agent2.policy.learner.grad), (env.state(), env2.state())):
        assert torch.equal(x, y), "the run does not continue bit-identically from the checkpoint"
    with pytest.raises(NotImplementedError, match="FQFLearner"):
        rl.run_fused_dqn(agent, env, rl.StopAfterNSteps(1))


# the measured curve (profiles/fqf.md) first clears 3 x random in the chunk that ends at 1250 vec-steps; 1.25 x 1250 = 1563, taken up
# to whole chunks of 250
LEARN_STEPS = 1750


def test_it_learns_cartpole():
    import rlhip as rl

    n, chunk = 4096, 250
    env = rl.CartPoleEnv(n, seed=5)
    net = rl.FQFApproximator(4, 128, 2, 32, 64, frac_lr=1e-5, seed=5)
    learner = rl.FQFLearner(rl.TargetNetwork(net, sync_freq=100), 2, 32, 64, batchsize=512, min_replay_history=n, seed=5)
    policy = rl.QBasedPolicy(learner, rl.EpsilonGreedyExplorer(0.01, kind="exp", decay_steps=500, seed=5))
    tr = rl.CircularArraySARTSTraces(capacity=256, n_env=n, obs_dim=4)
    agent = rl.Agent(policy, rl.Trajectory(tr))
    curve = []
    for _ in range(LEARN_STEPS // chunk):
        rl.run(agent, env, rl.StopAfterNSteps(chunk))
        term = tr.gather(torch.arange(len(tr) * n, device="cuda"))[3]
        curve.append(round(len(tr) * n / max(1.0, float(term.sum())), 1))
    print(f"FQFLearner on CartPole: mean episode length per {chunk} vec-steps {curve}, updates {learner.n_updates}")
    assert torch.isfinite(net.params).all() and torch.isfinite(net.frac_params).all()
    assert max(curve) >= 3.0 * 21.6, f"mean episode length never reached 3 x the random policy's 21.6: {curve}"
