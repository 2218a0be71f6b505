"""The fused vec-step of a prioritized-replay DQN learner on the device: rlhip.run against rlhip.run_fused_dqn_prioritized
(rlhip_dqn_vec_step_per_f32, one C call per vec-step, with rlhip_per_writeback_f32 as its priority write-back) on two identically
built agents -- parameters, optimiser state, trajectory, sum-tree, the learner's batch vectors and every host counter bit-identical,
then five more steps with the roles swapped.  The pattern of tests/test_gpu_fused_folds.py, over CircularPrioritizedTraces."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

GAMMA = 0.97


def _schedule(n_updates):
    """beta annealed towards 1 with the update count"""
    return min(1.0, 0.4 + 0.02 * n_updates)


class NSpace:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def _build(rl, kind, layers, n_step, double, dueling, beta, batch=32, capacity=16):
    n, h = 64, 128
    env = rl.HipVecEnv(kind, n, seed=4, continuous=False)
    na = len(env.action_space())
    cls = rl.DuelingApproximator if dueling else rl.HipApproximator
    net = cls(env.odim, h, na, seed=4, layers=layers)
    tn = rl.TargetNetwork(net, sync_freq=3)
    learner = rl.DQNLearner(tn, batchsize=batch, gamma=GAMMA, min_replay_history=5 * n, seed=4, max_grad_norm=1.0, n_step=n_step,
                            double_dqn=double, per_beta=beta)
    policy = rl.QBasedPolicy(learner, rl.EpsilonGreedyExplorer(0.05, kind="exp", decay_steps=20, seed=4))
    traces = rl.CircularPrioritizedTraces(capacity=capacity, n_env=n, obs_dim=env.odim, n_step=n_step)
    return NSpace(env=env, net=net, tn=tn, learner=learner, policy=policy, traces=traces, agent=rl.Agent(policy, rl.Trajectory(traces)))


def _assert_same(x, y, layers, dueling):
    pairs = [("params", x.net.params, y.net.params), ("target", x.tn.target, y.tn.target), ("m", x.net.m, y.net.m), ("v", x.net.v, y.net.v),
             ("beta_pow", x.net.beta_pow, y.net.beta_pow), ("loss", x.learner.loss, y.learner.loss), ("td", x.learner.td, y.learner.td),
             ("ring records", x.traces.records, y.traces.records), ("env state", x.env._s, y.env._s), ("env t", x.env._t, y.env._t),
             ("observation", x.env.state(), y.env.state()),
             ("sum-tree", x.traces.priorities, y.traces.priorities), ("is_weights", x.learner.is_weights, y.learner.is_weights),
             ("key", x.learner._key, y.learner._key), ("prio", x.learner._prio, y.learner._prio)]
    if dueling:
        pairs += [("dueling params", x.net.dueling_params, y.net.dueling_params), ("target dueling", x.tn.target_dueling, y.tn.target_dueling)]
    if layers == 3:
        pairs += [("packed", x.net.packed, y.net.packed), ("target packed", x.tn.target_packed, y.tn.target_packed)]
    assert (x.learner._idx is None) == (y.learner._idx is None), "_idx is set by one loop only"
    if x.learner._idx is not None:
        pairs.append(("idx", x.learner._idx, y.learner._idx))
    for name, a, b in pairs:
        assert torch.equal(a, b), f"{name} differ"
    for f in ("head_rt", "len_rt", "head_sa", "len_sa"):
        assert getattr(x.traces.rb, f) == getattr(y.traces.rb, f), f
    assert (x.learner.n_updates, x.learner.draw_ctr, x.learner.vec_steps) == (y.learner.n_updates, y.learner.draw_ctr, y.learner.vec_steps)
    assert x.policy.explorer.step == y.policy.explorer.step and x.tn.n_optimise == y.tn.n_optimise
    assert (x.agent.trajectory.controller.n_inserted, x.agent.trajectory.controller.n_sampled) == \
           (y.agent.trajectory.controller.n_inserted, y.agent.trajectory.controller.n_sampled)


def _assert_tree_consistent(traces):
    """node == left + right in Float32 for every internal node, tree[0] == 0: checked on the host"""
    t = traces.priorities.cpu().numpy()
    P = t.size // 2
    nodes = np.arange(1, P)
    assert t[0] == 0.0
    assert np.array_equal(t[nodes], t[2 * nodes] + t[2 * nodes + 1]), "a parent is not left + right of its children"
    assert t[1] > 0.0


def _both_loops(rl, steps, more, layers, dueling, **kw):
    x, y = (_build(rl, layers=layers, dueling=dueling, **kw) for _ in range(2))
    rl.run(x.agent, x.env, rl.StopAfterNSteps(steps))
    rl.run_fused_dqn_prioritized(y.agent, y.env, rl.StopAfterNSteps(steps))
    torch.cuda.synchronize()
    assert x.learner.vec_steps == steps
    _assert_same(x, y, layers, dueling)
    _assert_tree_consistent(y.traces)
    if more:  # and the two can be interleaved: the roles swapped
        rl.run_fused_dqn_prioritized(x.agent, x.env, rl.StopAfterNSteps(more))
        rl.run(y.agent, y.env, rl.StopAfterNSteps(more))
        torch.cuda.synchronize()
        _assert_same(x, y, layers, dueling)
        _assert_tree_consistent(x.traces)
    return x, y


#        kind, layers, n_step, double, dueling, beta
LOOPS = [("cartpole", 2, 1, False, False, 0.0), ("cartpole", 2, 1, False, False, 0.4), ("cartpole", 2, 3, False, False, 0.4),
         ("cartpole", 2, 1, True, False, 0.4), ("cartpole", 2, 3, True, True, _schedule), ("cartpole", 3, 3, True, False, 0.4),
         ("cartpole", 3, 1, False, True, 0.0), ("mountaincar", 2, 3, False, False, 0.4)]


@pytest.mark.parametrize("kind,layers,n_step,double,dueling,beta", LOOPS)
def test_fused_prioritized_loop_is_bit_identical_to_the_per_stage_loop(kind, layers, n_step, double, dueling, beta):
    import rlhip as rl

    kw = dict(kind=kind, n_step=n_step, double=double, beta=beta)
    x, _ = _both_loops(rl, 45, 5, layers, dueling, **kw)  # 45 > capacity: the ring wraps; updates from step 5 on, a sync every third
    assert x.learner.n_updates > 20
    fresh = _build(rl, layers=layers, dueling=dueling, **kw)
    assert float(x.net.params.sub(fresh.net.params).abs().max()) > 0, "nothing was learnt"
    if not (callable(beta) or beta > 0):
        assert torch.equal(x.learner.is_weights, fresh.learner.is_weights), "beta = 0 computes no weights"


@pytest.mark.parametrize("capacity,steps", [(16, 45), (256, 20)])
def test_batch_130_takes_the_general_write_back_inside_the_loop(capacity, steps):
    """130 keys: past the one-wave write-back.  Capacity 16 x 64 envs = 2^10 leaves, one workgroup; capacity 256 = 2^14 leaves, 128"""
    import rlhip as rl

    x, _ = _both_loops(rl, steps, 5, 2, False, kind="cartpole", n_step=1, double=False, beta=0.4, batch=130, capacity=capacity)
    assert x.learner.n_updates >= 15 and x.traces.n_leaves == capacity * 64


def test_nstep_warm_up_on_the_device():
    """min_replay_history = 0 and n_step = 5: the first four vec-steps store no full window -- both loops count them and draw nothing"""
    import rlhip as rl

    x, y = (_build(rl, "cartpole", 2, 5, True, False, 0.4) for _ in range(2))
    for b in (x, y):
        b.learner.min_replay_history = 0
    rl.run(x.agent, x.env, rl.StopAfterNSteps(7))
    rl.run_fused_dqn_prioritized(y.agent, y.env, rl.StopAfterNSteps(7))
    torch.cuda.synchronize()
    assert (x.learner.n_updates, x.learner.vec_steps, x.learner.draw_ctr) == (3, 7, 3)
    assert (y.learner.n_updates, y.learner.vec_steps, y.learner.draw_ctr) == (3, 7, 3)
    _assert_same(x, y, 2, False)
    _assert_tree_consistent(y.traces)


def test_a_refused_call_moves_nothing():
    import rlhip as rl
    from rlhip._lib import RLHipArgumentError

    y = _build(rl, "cartpole", 2, 3, True, False, 0.4)
    rl.run_fused_dqn_prioritized(y.agent, y.env, rl.StopAfterNSteps(8))
    torch.cuda.synchronize()
    rb = y.traces.rb
    before = (rb.head_sa, rb.len_sa, rb.head_rt, rb.len_rt)
    watched = lambda: (y.traces.records, y.traces.priorities, y.env._s, y.env._t, y.env.state(), y.net.params, y.net.m,  # noqa: E731
                       y.learner.td, y.learner._key)
    kept = [t.clone() for t in watched()]
    y.net.hidden = 130  # not a multiple of 4: RLHIP_EINVAL from the checks in front of the first launch
    with pytest.raises(RLHipArgumentError, match="multiple of 4"):
        rl.run_fused_dqn_prioritized(y.agent, y.env, rl.StopAfterNSteps(1))
    y.net.hidden = 128
    torch.cuda.synchronize()
    assert before == (rb.head_sa, rb.len_sa, rb.head_rt, rb.len_rt)
    for a, b in zip(kept, watched()):
        assert torch.equal(a, b)
