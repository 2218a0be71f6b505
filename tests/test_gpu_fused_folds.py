"""The fused vec-step for folded learners on the device.

1. rlhip_dqn_sample_fold_f32 (csrc/dqn_sample_fold.hip: draw + n-step window + Double DQN target in one launch) against the shipped
   composition rlhip_ring_sample_indices[_nstep] -> rlhip_ring_fold_nstep -> rlhip_dqn_fold_double_f32: byte equality of the folded
   records, idx_out and iota_out.  Source ring: capacity 5 x 8 envs, 12 pushes (wrapped: windows straddle the physical wrap) of a
   CartPole with max_steps = 3, so every env ends an episode every third step and two of three 3-step windows hold a terminal before
   their last step (asserted on the oracle's mirror of the ring, >= 1/4 of the sampled windows).
2. The same kernel against the oracle for one configuration: records from rlo_ring_gather_nstep (integer fields and R bit-exact),
   targets from tests/double_dqn_ref.py; y on the decisive samples within |x - ref| <= 2e-6 + 2e-5 |ref|, the bar of the fold targets
   in tests/test_gpu_double_dqn.py:62 (used at :128 and :171).
3. rlhip.run against rlhip.run_fused_dqn_folded on two identically built agents: everything bit-identical, counters equal, then five
   more steps with the roles swapped.
4. The plain learner through the new entry point against run_fused_dqn; a refused call moves nothing."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import oracle  # noqa: E402
from double_dqn_ref import compose, top_two_gap, trained_nets  # noqa: E402
from test_gpu_bench_shapes import dev, host  # noqa: E402

GAMMA = 0.97
SEED, CTR = 11, 3  # the sampler's seed and draw counter of every kernel case
_SRC = {}


def _source(rl):
    """(traces, the oracle's mirror): capacity 5 x 8 envs, 12 pushes of CartPole(max_steps = 3) under random actions.  Built once."""
    if not _SRC:
        n_env, cap = 8, 5
        env = rl.HipVecEnv("cartpole", n_env, continuous=False, seed=3, max_steps=3)
        tr = rl.CircularArraySARTSTraces(capacity=cap, n_env=n_env, obs_dim=4)
        oring = oracle.Ring(cap, n_env, 4)
        g = torch.Generator(device="cpu").manual_seed(5)
        obs = env.state().to(torch.float32)
        tr.push_state_(obs)
        oring.push_state(host(obs))
        for _ in range(12):
            a0 = torch.randint(0, 2, (n_env,), generator=g, dtype=torch.int32).cuda()
            env.act0_(a0)
            nobs, r, t = env.state().to(torch.float32), env.reward().to(torch.float32), env._done
            tr.push_transition_(nobs, a0, r, t)
            oring.push_transition(host(nobs), host(a0), host(r), host(t))
        torch.cuda.synchronize()
        assert len(tr) == cap and tr.rb.head_sa != 0, "the ring has not wrapped"
        _SRC["v"] = (tr, oring, tr.records.clone())
    return _SRC["v"]


def _source32(rl):
    """the longest window: capacity 34 x 4 envs, 40 pushes of made-up transitions (head_sa = 6, so a 32-step window crosses the state
    trace's wrap slot).  Terminal flags written here: env 0 never ends, env e ends every 3 + 2 e pushes.  Built once."""
    if "v32" not in _SRC:
        n_env, cap = 4, 34
        rng = np.random.default_rng(32)
        tr = rl.CircularArraySARTSTraces(capacity=cap, n_env=n_env, obs_dim=4)
        oring = oracle.Ring(cap, n_env, 4)
        obs = rng.standard_normal((4, n_env)).astype(np.float32)
        tr.push_state_(dev(obs))
        oring.push_state(obs)
        for k in range(40):
            nobs = rng.standard_normal((4, n_env)).astype(np.float32)
            a = rng.integers(0, 2, n_env).astype(np.int32)
            r = (rng.standard_normal(n_env) * 2).astype(np.float32)
            t = np.array([e > 0 and k % (3 + 2 * e) == 0 for e in range(n_env)], np.uint8)
            tr.push_transition_(dev(nobs), dev(a), dev(r), dev(t))
            oring.push_transition(nobs, a, r, t)
        torch.cuda.synchronize()
        assert len(tr) == cap and tr.rb.head_sa == 6
        _SRC["v32"] = (tr, oring, tr.records.clone())
    return _SRC["v32"]


def _nets(ns, h, na, seed=0):
    return oracle.mlp2_init(ns, h, na, 40 + seed, 0), oracle.mlp2_init(ns, h, na, 40 + seed, 1)


def _terminal_before_last(oring, idx, n_step):
    """share of the sampled windows with a terminal flag before their last step, read off the oracle's ring"""
    hits = 0
    for fj in idx:
        t = [oring.gather(np.array([fj + k * oring.rb.n_env], np.int64))[3][0] for k in range(n_step - 1)]
        hits += bool(np.any(t))
    return hits / len(idx)


def _composition(rl, tr, batch, n_step, double, h, na, act, p, pt):
    """what DQNLearner issues today -> (records of the folded ring as int32 (batch, 16), idx, iota)"""
    net = rl.HipApproximator(4, h, na, act=("relu", "tanh")[act], params=p) if double else None
    smp = rl.NStepBatchSampler(n_step, GAMMA, batch, seed=SEED)
    idx = smp.sample_indices(tr, CTR) if n_step > 1 else tr.sample_indices(batch, SEED, CTR)
    if n_step > 1 or not double:  # (n_step = 1 without the double fold: the window fold of one step, a record copy)
        folded, iota = smp.fold(tr, idx)
        if double:
            folded, iota = rl.DoubleTargetFold().fold(folded, None, net, dev(pt), None, smp.gamma_n, in_place=True)
    else:
        folded, iota = rl.DoubleTargetFold().fold(tr, idx, net, dev(pt), None, GAMMA)
    torch.cuda.synchronize()
    assert len(folded) == 1
    return folded.records.view(torch.int32)[0].clone(), idx.clone(), iota.clone()


def _kernel(rl, tr, batch, n_step, double, h, na, act, p, pt, want_idx=True):
    from rlhip._lib import call
    from rlhip.ops import ptr, stream_ptr

    folded = rl.CircularArraySARTSTraces(capacity=1, n_env=batch, obs_dim=4)
    idx = torch.full((batch,), -1, dtype=torch.int64, device="cuda")
    iota = torch.full((batch,), -1, dtype=torch.int64, device="cuda")
    dp, dpt = (dev(p), dev(pt)) if double else (None, None)
    call("rlhip_dqn_sample_fold_f32", C.byref(tr.rb), batch, n_step, int(double), GAMMA, SEED, CTR, h, na, act,
         ptr(dp) if double else None, ptr(dpt) if double else None, C.byref(folded.rb), ptr(idx) if want_idx else None, ptr(iota),
         stream_ptr())
    torch.cuda.synchronize()
    assert len(folded) == 1 and (folded.rb.head_sa, folded.rb.len_sa, folded.rb.head_rt) == (0, 2, 0)
    assert int(folded.records.view(torch.int32)[1].abs().max()) == 0, "a slot other than 0 was written"
    return folded.records.view(torch.int32)[0].clone(), idx, iota


def _check(rl, batch, n_step, double, h, na, act, nets=None, source=_source):
    tr, oring, snapshot = source(rl)
    p, pt = nets or _nets(4, h, na)
    ref, ridx, riota = _composition(rl, tr, batch, n_step, double, h, na, act, p, pt)
    if n_step > 1:  # the condition on the cases, on the reference alone: terminals INSIDE the windows
        share = _terminal_before_last(oring, host(ridx), n_step)
        print(f"n_step={n_step} batch={batch}: {share:.2f} of the windows hold a terminal before their last step")
        assert batch < 8 or share >= 0.25
    got, idx, iota = _kernel(rl, tr, batch, n_step, double, h, na, act, p, pt)
    assert torch.equal(idx, ridx), "other start indices drawn"
    assert torch.equal(iota, riota) and torch.equal(iota.cpu(), torch.arange(batch))
    differing = (got != ref).any(1).nonzero().flatten().tolist()
    assert not differing, f"records {differing[:8]} differ: kernel {got[differing[0]].tolist()} composition {ref[differing[0]].tolist()}"
    assert torch.equal(tr.records, snapshot), "the source ring was written"
    return got, idx


MATRIX = [(n, 0, b, 64, 2, 0) for n in (1, 3, 5) for b in (1, 37, 130)] + \
         [(n, 1, b, h, na, act) for n in (1, 3, 5) for b in (1, 37) for h in (4, 64, 256) for na in (2, 3) for act in (0, 1)] + \
         [(n, 1, 130, h, na, act) for n, h, na, act in ((1, 256, 3, 1), (3, 64, 2, 0), (5, 4, 3, 0), (3, 256, 2, 1))]


@pytest.mark.parametrize("n_step,double,batch,h,na,act", MATRIX)
def test_sample_fold_equals_the_shipped_composition_byte_for_byte(n_step, double, batch, h, na, act):
    import rlhip as rl

    _check(rl, batch, n_step, double, h, na, act)


@pytest.mark.parametrize("double", [0, 1])
def test_sample_fold_at_the_longest_window(double):
    """n_step = 32, the bound of the ABI, on a ring whose windows cross the wrap slot: the conditions on the drawn windows are asserted
    on the composition's index list before the kernel runs (the composition is pinned to the oracle at n_step = 32 by test_gpu_nstep.py)"""
    import rlhip as rl

    n_step, batch = 32, 37
    tr, oring, _ = _source32(rl)
    idx = host(rl.NStepBatchSampler(n_step, GAMMA, batch, seed=SEED).sample_indices(tr, CTR))
    env0 = idx[idx % tr.n_env == 0]
    assert len(env0) >= 1 and _terminal_before_last(oring, env0, n_step) == 0, "no window of the full 32 steps (env 0) was drawn"
    assert tr.rb.head_sa + env0.min() // tr.n_env <= tr.capacity < tr.rb.head_sa + env0.min() // tr.n_env + n_step, "no wrap inside it"
    assert _terminal_before_last(oring, idx, n_step) > 0, "no drawn window is cut short by a terminal"
    _check(rl, batch, n_step, double, 64, 2, 0, source=_source32)


@pytest.mark.parametrize("n_step,na", [(1, 2), (3, 3), (5, 4)])
def test_ties_select_the_first_action(n_step, na):
    """head weights and biases zero: every Q(s') is equal, a* must be action 0 -- read off a target net whose values are the action numbers"""
    import rlhip as rl

    h, batch = 64, 37
    p, _ = _nets(4, h, na)
    p = p.copy()
    p[4 * h + h:] = 0.0
    pt = np.zeros_like(p)
    pt[-na:] = np.arange(1, na + 1, dtype=np.float32)  # Qt(s') = (1, 2, .., na) for every s'
    got, _ = _check(rl, batch, n_step, 1, h, na, 0, nets=(p, pt))
    plain, _, _ = _kernel(rl, _source(rl)[0], batch, n_step, 0, h, na, 0, p, pt)
    R, t = host(plain[:, 5].view(torch.float32)), host(plain[:, 6])
    y = host(got[:, 5].view(torch.float32))
    geff = np.float32(oracle.gamma_pow(GAMMA, n_step))
    assert np.array_equal(y, (R + geff * np.where(t != 0, np.float32(0), np.float32(1)) * np.float32(1.0)).astype(np.float32))
    assert int(got[:, 6].min()) == 1 and int(got[:, 6].max()) == 1


def test_idx_out_is_optional():
    import rlhip as rl

    tr, _, _ = _source(rl)
    p, pt = _nets(4, 64, 2)
    a, _, _ = _kernel(rl, tr, 37, 3, 1, 64, 2, 0, p, pt)
    b, idx, _ = _kernel(rl, tr, 37, 3, 1, 64, 2, 0, p, pt, want_idx=False)
    assert torch.equal(a, b) and int(idx.max()) == -1


@pytest.mark.parametrize("act", [0, 1])
def test_sample_fold_vs_the_oracle(act):
    import rlhip as rl

    ns, h, na, n_step, batch = 4, 64, 2, 3, 130
    tr, oring, _ = _source(rl)
    p, pt = trained_nets(2, ns, h, na, act, seed=7 + act, steps=300)
    idx = oracle.ring_sample_indices_nstep(oring, batch, n_step, SEED, CTR)
    s, a, R, t, sn = oracle.ring_gather_nstep(oring, idx, n_step, GAMMA)
    assert _terminal_before_last(oring, idx, n_step) >= 0.25 and t.any() and not t.all()
    gn = oracle.gamma_pow(GAMMA, n_step)
    y, astar, q, qt = compose(2, ns, h, na, act, p, pt, R, t, sn, gn)
    tol = 2e-6 + 2e-5 * np.abs(q)  # tests/test_gpu_double_dqn.py:62
    decisive = top_two_gap(q) > 4 * tol.max(0)
    assert 1.0 - decisive.mean() <= 0.01, "a condition on this test's nets, on the oracle alone"
    # the n-step record, no double fold: every field bit-exact
    rec, gidx, _ = _kernel(rl, tr, batch, n_step, 0, h, na, act, p, pt)
    assert np.array_equal(host(gidx), idx)
    f = host(rec).view(np.float32)
    i = host(rec)
    assert np.array_equal(f[:, :4].T.view(np.uint32), s.view(np.uint32))
    assert np.array_equal(f[:, 8:12].T.view(np.uint32), sn.view(np.uint32))
    assert np.array_equal(i[:, 4], a) and np.array_equal(i[:, 6], t.astype(np.int32))
    assert np.array_equal(f[:, 5].view(np.uint32), R.astype(np.float32).view(np.uint32)), "R is not bit-exact"
    assert not i[:, 7].any() and not i[:, 12:].any()
    # ... and with it: y
    rec2, _, _ = _kernel(rl, tr, batch, n_step, 1, h, na, act, p, pt)
    f2, i2 = host(rec2).view(np.float32), host(rec2)
    assert np.array_equal(i2[:, :5], i[:, :5]) and np.array_equal(i2[:, 7:], i[:, 7:]) and (i2[:, 6] == 1).all()
    gy = f2[:, 5]
    assert np.array_equal(gy[t != 0], R[t != 0]), "a terminal window must give y = R exactly"
    err = np.abs(gy - y) / (2e-6 + 2e-5 * np.abs(y))
    print(f"act={act}: max |y - ref| / tol on the decisive samples = {err[decisive].max():.3f}")
    assert err[decisive].max() <= 1.0


# ------------------------------------------------------------------------------------------------ the loops
def _build(rl, kind, layers, h, n_step, double, dueling):
    n = 64
    env = rl.HipVecEnv(kind, n, seed=4, continuous=False)
    na = len(env.action_space())
    cls = rl.DuelingApproximator if dueling else rl.HipApproximator
    net = cls(env.odim, h, na, seed=4, layers=layers)
    tn = rl.TargetNetwork(net, sync_freq=3)
    learner = rl.DQNLearner(tn, batchsize=32, gamma=GAMMA, min_replay_history=5 * n, seed=4, max_grad_norm=1.0, n_step=n_step,
                            double_dqn=double)
    policy = rl.QBasedPolicy(learner, rl.EpsilonGreedyExplorer(0.05, kind="exp", decay_steps=20, seed=4))
    traces = rl.CircularArraySARTSTraces(capacity=16, n_env=n, obs_dim=env.odim)
    return NSpace(env=env, net=net, tn=tn, learner=learner, policy=policy, traces=traces, agent=rl.Agent(policy, rl.Trajectory(traces)))


class NSpace:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def _assert_same(x, y, layers, dueling):
    pairs = [("params", x.net.params, y.net.params), ("target", x.tn.target, y.tn.target), ("m", x.net.m, y.net.m), ("v", x.net.v, y.net.v),
             ("beta_pow", x.net.beta_pow, y.net.beta_pow), ("loss", x.learner.loss, y.learner.loss), ("td", x.learner.td, y.learner.td),
             ("ring records", x.traces.records, y.traces.records), ("env state", x.env._s, y.env._s), ("env t", x.env._t, y.env._t),
             ("observation", x.env.state(), y.env.state())]
    if dueling:
        pairs += [("dueling params", x.net.dueling_params, y.net.dueling_params), ("target dueling", x.tn.target_dueling, y.tn.target_dueling)]
    if layers == 3:
        pairs += [("packed", x.net.packed, y.net.packed), ("target packed", x.tn.target_packed, y.tn.target_packed)]
    for name, a, b in pairs:
        assert torch.equal(a, b), f"{name} differ"
    for f in ("head_rt", "len_rt", "head_sa", "len_sa"):
        assert getattr(x.traces.rb, f) == getattr(y.traces.rb, f), f
    assert (x.learner.n_updates, x.learner.draw_ctr, x.learner.vec_steps) == (y.learner.n_updates, y.learner.draw_ctr, y.learner.vec_steps)
    assert x.policy.explorer.step == y.policy.explorer.step and x.tn.n_optimise == y.tn.n_optimise
    assert (x.agent.trajectory.controller.n_inserted, x.agent.trajectory.controller.n_sampled) == \
           (y.agent.trajectory.controller.n_inserted, y.agent.trajectory.controller.n_sampled)


LOOPS = [("cartpole", 2, 128, 3, False, False), ("cartpole", 2, 128, 1, True, False), ("cartpole", 2, 128, 3, True, False),
         ("cartpole", 2, 128, 3, True, True), ("cartpole", 2, 128, 1, False, True), ("cartpole", 3, 128, 3, True, False),
         ("cartpole", 3, 128, 1, True, True), ("mountaincar", 2, 128, 3, True, False)]


@pytest.mark.parametrize("kind,layers,h,n_step,double,dueling", LOOPS)
def test_fused_folded_loop_is_bit_identical_to_the_per_stage_loop(kind, layers, h, n_step, double, dueling):
    import rlhip as rl

    x, y = (_build(rl, kind, layers, h, n_step, double, dueling) for _ in range(2))
    steps = 45  # > capacity: the ring wraps; updates from step 5 on, a target sync every third
    rl.run(x.agent, x.env, rl.StopAfterNSteps(steps))
    rl.run_fused_dqn_folded(y.agent, y.env, rl.StopAfterNSteps(steps))
    torch.cuda.synchronize()
    assert x.learner.n_updates > 20 and x.learner.vec_steps == steps
    _assert_same(x, y, layers, dueling)
    assert float(x.net.params.sub(_build(rl, kind, layers, h, n_step, double, dueling).net.params).abs().max()) > 0, "nothing was learnt"
    # and the two can be interleaved: the roles swapped
    rl.run_fused_dqn_folded(x.agent, x.env, rl.StopAfterNSteps(5))
    rl.run(y.agent, y.env, rl.StopAfterNSteps(5))
    torch.cuda.synchronize()
    _assert_same(x, y, layers, dueling)


@pytest.mark.parametrize("layers", [2, 3])
def test_plain_learner_through_the_new_entry_point_equals_run_fused_dqn(layers):
    import rlhip as rl

    x, y = (_build(rl, "cartpole", layers, 128, 1, False, False) for _ in range(2))
    rl.run_fused_dqn(x.agent, x.env, rl.StopAfterNSteps(45))
    rl.run_fused_dqn_folded(y.agent, y.env, rl.StopAfterNSteps(45))
    torch.cuda.synchronize()
    assert x.learner.n_updates > 20
    _assert_same(x, y, layers, False)


def test_nstep_warm_up_on_the_device():
    """min_replay_history = 0 and n_step = 5: the first four vec-steps store no full window -- both loops count them and draw nothing"""
    import rlhip as rl

    x, y = (_build(rl, "cartpole", 2, 128, 5, True, False) for _ in range(2))
    for b in (x, y):
        b.learner.min_replay_history = 0
    rl.run(x.agent, x.env, rl.StopAfterNSteps(7))
    rl.run_fused_dqn_folded(y.agent, y.env, rl.StopAfterNSteps(7))
    torch.cuda.synchronize()
    assert x.learner.n_updates == 3 and x.learner.vec_steps == 7
    _assert_same(x, y, 2, False)


def test_a_refused_call_moves_nothing():
    import rlhip as rl
    from rlhip._lib import RLHipArgumentError

    y = _build(rl, "cartpole", 2, 128, 3, True, False)
    rl.run_fused_dqn_folded(y.agent, y.env, rl.StopAfterNSteps(8))
    torch.cuda.synchronize()
    rb = y.traces.rb
    before = (rb.head_sa, rb.len_sa, rb.head_rt, rb.len_rt)
    kept = [t.clone() for t in (y.traces.records, y.env._s, y.env._t, y.env.state(), y.net.params, y.net.m)]
    y.net.hidden = 130  # not a multiple of 4: RLHIP_EINVAL from the checks in front of the first launch
    with pytest.raises(RLHipArgumentError, match="multiple of 4"):
        rl.run_fused_dqn_folded(y.agent, y.env, rl.StopAfterNSteps(1))
    y.net.hidden = 128
    torch.cuda.synchronize()
    assert before == (rb.head_sa, rb.len_sa, rb.head_rt, rb.len_rt)
    for a, b in zip(kept, (y.traces.records, y.env._s, y.env._t, y.env.state(), y.net.params, y.net.m)):
        assert torch.equal(a, b)
