"""GPU tests of the drop-in surface: run(policy, env, stop, hook) on the vector env, Agent + trajectory +
DQN learner end to end, and the multi-process gradient all-reduce with the real kernels (2 ranks sharing
one GPU over `gloo`, because RCCL refuses two ranks on one device)."""
import ctypes as C
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import oracle  # noqa: E402


@pytest.fixture(scope="module")
def rl():
    import rlhip

    return rlhip


def test_config1_random_policy_cartpole_run(rl):
    """BASELINE configs[0]: run(RandomPolicy(), CartPoleEnv(), StopAfterNSteps(1_000), hook) (README.md:44-51)."""
    seed = 123
    env = rl.CartPoleEnv(1, T=torch.float64, seed=seed)
    hook = rl.StepsPerEpisode() + rl.TotalBatchRewardPerEpisode(1)
    rl.run(rl.RandomPolicy(seed=seed), env, rl.StopAfterNSteps(1000), hook)
    steps = hook.hooks[0].steps
    # oracle: the same Philox EXPLORE draws (step counter starts at 1), same env stream
    ref = oracle.VecEnv("cartpole", 1, seed=seed, dtype=np.float64)
    lens, cur = [], 0
    for step in range(1, 1001):
        w = oracle.philox(seed, 0, 0, step, oracle.TAG["EXPLORE"])
        ref.step(np.array([oracle.lib().rlo_randint(w[2], 2)], np.int32))
        cur += 1
        if ref.done[0]:
            lens.append(cur)
            cur = 0
    if cur:
        lens.append(cur)
    assert steps == lens
    assert sum(steps) == 1000
    rewards = hook.hooks[1].rewards[0]
    assert rewards == [float(l - 1) for l in lens[:len(rewards)]]  # terminal step pays 0


def test_run_with_ppo_agent_stepwise_updates(rl):
    n, T = 128, 8
    env = rl.CartPoleEnv(n, seed=4)
    pol = rl.PPOPolicy(env, update_freq=T)
    p0 = pol.params.clone()
    hook = rl.BatchStepsPerEpisode(n)
    rl.run(rl.PPOAgent(pol), env, rl.StopAfterNSteps(3 * T), hook)
    assert pol.update_ctr == 3 and pol.vec_step == 3 * T and not torch.equal(p0, pol.params)
    assert sum(len(s) for s in hook.steps) > 0
    # the fused loop gives the identical parameters (same streams, same kernels)
    env2 = rl.CartPoleEnv(n, seed=4)
    pol2 = rl.PPOPolicy(env2, update_freq=T)
    rl.run_fused_ppo(pol2, env2, 3)
    assert torch.equal(pol.params, pol2.params)


def test_dqn_agent_end_to_end(rl):
    """4096-way CartPole + QBasedPolicy(DQN, 2-layer MLP) (BASELINE configs[1] shape, shortened)."""
    n = 1024
    env = rl.CartPoleEnv(n, seed=2)
    net = rl.HipApproximator(4, 128, 2, lr=1e-3, seed=2)
    learner = rl.DQNLearner(rl.TargetNetwork(net, sync_freq=100), batchsize=512, min_replay_history=n, seed=2)
    explorer = rl.EpsilonGreedyExplorer(0.01, kind="exp", decay_steps=500, seed=2)
    policy = rl.QBasedPolicy(learner, explorer)
    traces = rl.CircularArraySARTSTraces(capacity=64, n_env=n, obs_dim=4)
    agent = rl.Agent(policy, rl.Trajectory(traces))
    p0 = net.params.clone()
    rl.run(agent, env, rl.StopAfterNSteps(150), rl.EmptyHook())
    assert len(traces) == 64  # ring wrapped
    assert learner.n_updates == 150  # one update per vec-step once min_replay_history is reached (after step 1)
    assert torch.isfinite(learner.loss).all() and not torch.equal(p0, net.params)
    assert explorer.step == 151
    assert learner.approximator.n_optimise == 150 % 100
    # target network lags: last sync at update 100
    assert not torch.equal(learner.approximator.target, net.params)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _gpu_worker(rank, world, port, q, extra_env=None):
    os.environ.update(extra_env or {})
    os.environ.update(RANK=str(rank), LOCAL_RANK="0", WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1",
                      MASTER_PORT=str(port))
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for p in (root, os.path.join(root, "reinforcementlearning.jl_amd")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import torch
    import torch.distributed as dist

    import rlhip
    from rlhip import dist as rdist

    torch.cuda.set_device(0)
    dist.init_process_group("gloo")
    n_per, T = 256, 8
    base, n = rdist.env_shard(rank, n_per)
    env = rlhip.CartPoleEnv(n, seed=77, env_id_base=base)
    import json

    kw = json.loads(os.environ.get("RLHIP_TEST_PPO_KW", "{}"))
    pol = rlhip.PPOPolicy(env, update_freq=T, seed=77, process_group=dist.group.WORLD, **kw)
    pol.rollout_()
    pol.update_()
    torch.cuda.synchronize()
    same = rdist.params_checksum_equal(pol.params.cpu(), dist.group.WORLD)
    expect_p2p = os.environ.get("RLHIP_NO_P2P", "0") != "1" and "RLHIP_TEST_FAIL_EXPORT_RANK" not in os.environ
    q.put((rank, pol.params.cpu().numpy(), pol.trajectory.obs.cpu().numpy(), same and (
        (getattr(pol, "_p2p", None) is not None) == expect_p2p), pol._hipcomm.transport()))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("mode", ["p2p_fused", "p2p_unfused", "p2p_host_loop", "library_allreduce", "layers3_hidden256",
                                  "layers3_hidden256_library"])
def test_two_ranks_one_gpu_gradient_allreduce(rl, mode):
    """every variant of the exchange step: the fused reduce + peer exchange + clip + Adam kernel, the separate p2p
    kernel (one C call / host loop), and the torch.distributed all-reduce fallback; and the 3-layer 256-wide actor / critic
    (csrc/ppo3w.hip: gradient kernels -> exchange of the 134 403-float gradient -> clip + Adam per optimiser step)"""
    import json

    import torch.multiprocessing as mp

    wide = {"RLHIP_TEST_PPO_KW": json.dumps({"layers": 3, "hidden": 256})}
    extra = {"p2p_fused": {}, "p2p_unfused": {"RLHIP_P2P_UNFUSED": "1"}, "p2p_host_loop": {"RLHIP_P2P_HOST_LOOP": "1"},
             "library_allreduce": {"RLHIP_NO_P2P": "1"}, "layers3_hidden256": wide,
             "layers3_hidden256_library": dict(wide, RLHIP_NO_P2P="1")}[mode]
    world, port = 2, _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_gpu_worker, args=(r, world, port, q, extra)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=300) for _ in range(world)], key=lambda x: x[0])
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    (_, p0, obs0, s0, _t0), (_, p1, obs1, s1, _t1) = res
    assert np.array_equal(p0, p1) and s0 and s1  # replicas bit-identical after 16 all-reduced steps
    # one process owning both shards: same rollouts (global env ids), nearly the same update
    n_per, T = 256, 8
    env = rl.CartPoleEnv(2 * n_per, seed=77)
    pol = rl.PPOPolicy(env, update_freq=T, seed=77, **json.loads(extra.get("RLHIP_TEST_PPO_KW", "{}")))
    pol.rollout_()
    assert np.array_equal(pol.trajectory.obs.cpu().numpy(), np.concatenate([obs0, obs1], axis=2))
    if "RLHIP_TEST_PPO_KW" in extra:
        return
    # (the micro-batch composition differs -- each rank permutes its own shard -- so parameters are close,
    #  not equal: both are valid PPO updates of the same data)
    pol.update_()
    d = np.abs(pol.params.cpu().numpy() - p0)
    assert np.quantile(d, 0.9) < 5e-3


@pytest.mark.parametrize("layers,kind,hidden", [(2, "cartpole", 128), (3, "cartpole", 128), (2, "mountaincar", 128),
                                                (3, "mountaincar", 128), (3, "cartpole", 256), (3, "pendulum", 128), (2, "pendulum", 128)])
def test_fused_dqn_vec_step_is_bit_identical_to_the_per_step_protocol(layers, kind, hidden):
    """rlhip_dqn_vec_step_f32 (one C call per vec-step) against run(): same kernels in the same order, so the
    parameters, target network, replay ring, env state and every counter must end bit-identical."""
    import rlhip

    def build():
        n = 192
        env = rlhip.HipVecEnv(kind, n, seed=4, continuous=False)
        na = len(env.action_space())
        net = rlhip.HipApproximator(env.odim, hidden, na, seed=4, layers=layers)
        tn = rlhip.TargetNetwork(net, sync_freq=7)
        learner = rlhip.DQNLearner(tn, batchsize=256, min_replay_history=5 * n, seed=4, max_grad_norm=1.0)
        policy = rlhip.QBasedPolicy(learner, rlhip.EpsilonGreedyExplorer(0.05, kind="exp", decay_steps=20, seed=4))
        traces = rlhip.CircularArraySARTSTraces(capacity=16, n_env=n, obs_dim=env.odim)
        return env, net, tn, learner, policy, traces, rlhip.Agent(policy, rlhip.Trajectory(traces))

    e1, n1, t1, l1, p1, tr1, a1 = build()
    e2, n2, t2, l2, p2, tr2, a2 = build()
    steps = 45  # > capacity: the ring wraps; > min_replay_history / n: updates and target syncs happen
    rlhip.run(a1, e1, rlhip.StopAfterNSteps(steps))
    rlhip.run_fused_dqn(a2, e2, rlhip.StopAfterNSteps(steps))
    torch.cuda.synchronize()
    assert l1.n_updates == l2.n_updates > 30 and l1.draw_ctr == l2.draw_ctr
    assert p1.explorer.step == p2.explorer.step and t1.n_optimise == t2.n_optimise
    for a, b in ((n1.params, n2.params), (t1.target, t2.target), (n1.m, n2.m), (n1.v, n2.v), (l1.loss, l2.loss),
                 (tr1.state, tr2.state), (tr1.action, tr2.action), (tr1.reward, tr2.reward),
                 (tr1.terminal, tr2.terminal), (e1._s, e2._s), (e1._t, e2._t), (e1.state(), e2.state())):
        assert torch.equal(a, b)
    assert (tr1.rb.head_rt, tr1.rb.len_rt, tr1.rb.head_sa, tr1.rb.len_sa) == \
           (tr2.rb.head_rt, tr2.rb.len_rt, tr2.rb.head_sa, tr2.rb.len_sa)
    if layers == 3:
        assert torch.equal(n1.packed, n2.packed) and torch.equal(t1.target_packed, t2.target_packed)
    # and the two can be interleaved: continue the per-step agent with the fused loop
    rlhip.run_fused_dqn(a1, e1, rlhip.StopAfterNSteps(5))
    rlhip.run(a2, e2, rlhip.StopAfterNSteps(5))
    torch.cuda.synchronize()
    assert torch.equal(n1.params, n2.params) and torch.equal(tr1.state, tr2.state)


def test_device_episode_stats_hook_matches_host_hooks():
    """DeviceEpisodeStats (hooks.hip: no per-step sync) against the host-side BatchStepsPerEpisode /
    TotalBatchRewardPerEpisode hooks on the same run."""
    import rlhip

    n = 300
    env = rlhip.CartPoleEnv(n, seed=8)
    pol = rlhip.RandomPolicy(env.action_space(), seed=8)
    dev_hook = rlhip.DeviceEpisodeStats(n)
    h_steps, h_rew = rlhip.BatchStepsPerEpisode(n), rlhip.TotalBatchRewardPerEpisode(n)
    rlhip.run(pol, env, rlhip.StopAfterNSteps(120), rlhip.ComposedHook(dev_hook, h_steps, h_rew))
    assert sum(len(s) for s in h_steps.steps) > n  # random CartPole episodes last ~20 steps
    assert dev_hook.steps == h_steps.steps
    assert dev_hook.rewards == h_rew.rewards
    rec = dev_hook.records()
    assert (rec["steps"] > 0).all() and (np.diff(rec["vec_step"].astype(np.int64)) >= 0).all()
    small = rlhip.DeviceEpisodeStats(n, log_capacity=4)
    rlhip.run(pol, env, rlhip.StopAfterNSteps(60), small)
    with pytest.raises(OverflowError):
        small.records()


def _p2p_worker(rank, world, port, q):
    os.environ.update(RANK=str(rank), LOCAL_RANK="0", WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1",
                      MASTER_PORT=str(port))
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for p in (root, os.path.join(root, "reinforcementlearning.jl_amd")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import torch
    import torch.distributed as dist

    import rlhip  # noqa: F401
    from rlhip.dist import P2PAllReduce

    torch.cuda.set_device(0)
    dist.init_process_group("gloo")
    p2p = P2PAllReduce.create(dist.group.WORLD, 3331, torch.device("cuda"))
    ok = p2p is not None
    outs = []
    if ok:
        g = torch.Generator(device="cpu").manual_seed(100 + rank)
        for it in range(40):  # many back-to-back calls: exercises the double buffering
            x = torch.randn(3331, generator=g).cuda()
            outs.append((x.cpu().numpy(), p2p.all_reduce_(x.clone()).cpu().numpy()))
        ok = not p2p.failed()
    q.put((rank, ok, outs))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 4, 8])
def test_p2p_allreduce_ranks_sharing_one_gpu(world):
    """one-shot IPC all-reduce (p2p.hip) between `world` processes sharing the GPU: passes its own self-test against
    torch.distributed, then 40 back-to-back sums equal ((x0 + x1) + x2) + ... exactly (rank-order summation) on every
    rank"""
    import torch.multiprocessing as mp

    port = _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_p2p_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=300) for _ in range(world)], key=lambda x: x[0])
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    assert all(ok for _, ok, _ in res), "the P2P path did not validate on this box (the product then uses the library all-reduce)"
    outs = [o for _, _, o in res]
    for it in range(len(outs[0])):
        acc = np.zeros_like(outs[0][it][0])
        for r in range(world):
            acc = acc + outs[r][it][0]  # float32 adds in rank order, starting from +0
        for r in range(world):
            assert np.array_equal(outs[r][it][1], acc)


def test_four_ranks_one_gpu_fused_exchange_keeps_replicas_identical(rl):
    """the fused reduce + peer exchange + clip + Adam kernel with four ranks (53 spinning workgroups per rank on the
    shared GPU): all replicas end bit-identical after 16 optimiser steps"""
    import torch.multiprocessing as mp

    world, port = 4, _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_gpu_worker, args=(r, world, port, q, {})) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=300) for _ in range(world)], key=lambda x: x[0])
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    assert all(r[3] for r in res)
    for r in res[1:]:
        assert np.array_equal(r[1], res[0][1])


def _run_gpu_workers(world, extra):
    import torch.multiprocessing as mp

    port = _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_gpu_worker, args=(r, world, port, q, extra)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=600) for _ in range(world)], key=lambda x: x[0])
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    return res


def test_eight_ranks_one_gpu_fused_exchange_keeps_replicas_identical(rl):
    """world = 8, the size of the target node: the fused reduce + peer exchange + clip + Adam kernel with
    eight slots / eight flags per exchange, eight processes sharing this box's one GPU.  The policy is 4 -> 64 -> {2, 1}
    (14 spinning workgroups per rank): with the headline's 53 per rank, seven ranks' spinners (371 workgroups of 1024 threads)
    would hold every CU of the one shared device and starve the eighth rank's gradient launch -- an artefact of eight ranks on
    ONE device (on the node every rank owns its GPU), bounded by the exchange's timeout but not worth provoking."""
    import json

    res = _run_gpu_workers(8, {"RLHIP_TEST_PPO_KW": json.dumps({"hidden": 64})})
    assert all(r[3] for r in res), [r[4] for r in res]
    assert all(r[4].startswith("p2p") for r in res)
    for r in res[1:]:
        assert np.array_equal(r[1], res[0][1])


def test_a_rank_that_fails_its_export_switches_every_rank_to_the_fallback(rl):
    """rank 1's rlhip_comm_export `fails` (injected).  No rank hangs; every rank reports the peer-to-peer path
    as not active with the failing rank's message, the update runs over the fallback collective and the replicas end
    bit-identical."""
    res = _run_gpu_workers(2, {"RLHIP_TEST_FAIL_EXPORT_RANK": "1"})
    assert all(r[3] for r in res), [r[4] for r in res]
    for r in res:
        assert "injected rlhip_comm_export failure" in r[4] and not r[4].startswith("p2p"), r[4]
    assert np.array_equal(res[0][1], res[1][1])


def test_bench_preflight_two_ranks_one_device():
    """`bench.py --gpus 2 --preflight`: one JSON report with the peer-access row, the per-peer IPC round trip,
    the set-up verdict with its reason and one exchange checked on the host, per rank; exit status 0; a few seconds."""
    import json

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, RLHIP_BENCH_SINGLE_DEVICE="1", RLHIP_BENCH_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--preflight"], env=env, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    d = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert d["world"] == 2 and len(d["preflight"]) == 2 and d["exchange_ok_on_every_rank"] is True
    for rk, rep in enumerate(d["preflight"]):
        peer = str(1 - rk)
        assert rep["rank"] == rk and rep["can_access_peer"][peer] is True and rep["ipc_round_trip"][peer] == "ok", rep
        assert rep["comm"]["why"] and rep["comm"]["setup_error"] is None and rep["exchange"]["correct"] and not rep["exchange"]["timeout"]
    assert d["p2p_active_on_every_rank"] == all(rep["comm"]["p2p_active"] for rep in d["preflight"])


def test_bench_eight_ranks_on_one_device_prints_the_contract_line():
    """bare `python bench.py --gpus 8` with all eight ranks on this box's one GPU: the contract line at the
    world size of the target node, `p2p_timeouts` false, `replicas_bit_identical` true.  RLHIP_P2P_UNFUSED=1: the exchange runs
    as its own small kernel instead of inside the 53-workgroup reduce kernel, whose spinners from seven ranks would occupy
    every CU of the one shared device (see the eight-rank test above)."""
    import json

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, RLHIP_BENCH_SINGLE_DEVICE="1", RLHIP_BENCH_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0",
               RLHIP_P2P_UNFUSED="1")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "8", "--steps", "3", "--warmup", "1",
                        "--full", "--no-extras"], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    d = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert d["n_gpus"] == 8 and d["steps"] == 3 and d["scaling"] == "weak" and d["value"] > 0
    assert d["config"]["n_envs_per_gpu"] == 4096 and d["replicas_bit_identical"] is True
    assert d["p2p_timeouts"] is False and d["gradient_allreduce"].startswith("p2p"), d["gradient_allreduce"]
    assert np.isfinite(d["final_loss"])


def test_bench_plain_line_and_dumped_outputs_repeat(tmp_path):
    """a plain `bench.py --gpus 1` (no --full): the contract fields and no side legs; --dump-outputs writes the last timed
    step's arrays as float32 .npy files, and a second run with the same arguments writes the same bits"""
    import json

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    dumps = []
    for run in range(2):
        d_out = tmp_path / f"out{run}"
        r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "7", "--warmup", "2",
                            "--dump-outputs", str(d_out)], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        assert len(lines) == 1
        d = json.loads(lines[0])
        assert d["metric"] == "env_steps_per_sec" and d["unit"] == "env-steps/s" and d["higher_is_better"] is True
        assert d["dtype"] == "f32" and d["steps"] == 7 and d["ms_per_step"] > 0
        assert abs(d["value"] - 4096 * 32 * 1e3 / d["ms_per_step"]) <= 1e-3 * d["value"]
        assert not {"roofline", "roofline_extra", "cpu_baseline", "kernels", "ms_per_step_no_preheat"} & set(d)
        arrays = {f.name: np.load(f) for f in sorted(d_out.glob("*.npy"))}
        assert set(arrays) == {"params.npy", "adam_m.npy", "adam_v.npy", "losses.npy", "obs.npy", "action.npy", "reward.npy",
                               "terminal.npy", "logp.npy", "value.npy", "adv.npy", "ret.npy"}
        assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in arrays.values())
        assert arrays["obs.npy"].shape == (33, 4, 4096) and arrays["params.npy"].size == 3331
        dumps.append(arrays)
    for k, a in dumps[0].items():
        assert np.array_equal(a, dumps[1][k]), k


@pytest.mark.parametrize("layers,prioritized", [(2, False), (3, False), (2, True)])
def test_checkpoint_resume_of_a_dqn_agent_is_bit_identical(tmp_path, layers, prioritized):
    """save_checkpoint / load_checkpoint (rlhip/checkpoint.py; the JLD2 hook recipe docs/src/How_to_use_hooks.md:122-167):
    agent + env exported mid-run from a DoEveryNSteps hook, restored into FRESH objects, continue -> the same bits
    as the uninterrupted run (parameters, Adam state, target, ring, priorities, env state, every counter)"""
    import rlhip

    def build(seed):
        n = 160
        env = rlhip.CartPoleEnv(n, seed=seed)
        net = rlhip.HipApproximator(4, 128, 2, seed=seed, layers=layers)
        learner = rlhip.DQNLearner(rlhip.TargetNetwork(net, sync_freq=5), batchsize=128, min_replay_history=2 * n,
                                   seed=seed, max_grad_norm=1.0)
        policy = rlhip.QBasedPolicy(learner, rlhip.EpsilonGreedyExplorer(0.05, kind="exp", decay_steps=30, seed=seed))
        traces = (rlhip.CircularPrioritizedTraces if prioritized else rlhip.CircularArraySARTSTraces)(
            capacity=16, n_env=n, obs_dim=4)
        return env, rlhip.Agent(policy, rlhip.Trajectory(traces))

    path = str(tmp_path / "ck.npz")
    env, agent = build(6)
    saved = []

    def hook_fn(t, policy, e):   # DoEveryNSteps(f; n): f(t, policy, env)
        if t == 20:
            saved.append(rlhip.save_checkpoint(path, {"agent": agent, "env": env}))

    rlhip.run(agent, env, rlhip.StopAfterNSteps(45), rlhip.DoEveryNSteps(hook_fn, n=20))
    assert saved and saved[0] > 20
    env2, agent2 = build(99)        # different seed: every bit must come from the checkpoint
    rlhip.load_checkpoint(path, {"agent": agent2, "env": env2})
    rlhip.run(agent2, env2, rlhip.StopAfterNSteps(25))
    torch.cuda.synchronize()
    a, b = rlhip.state_dict({"agent": agent, "env": env}), rlhip.state_dict({"agent": agent2, "env": env2})
    assert set(a) == set(b)
    import numpy as np
    for k in a:
        if "workspace" in k or k.endswith("/grad") or "/_q" in k:
            continue    # scratch
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k
    assert agent2.policy.learner.n_updates > 30


def test_checkpoint_resume_of_a_ppo_policy_is_bit_identical(tmp_path):
    import numpy as np
    import rlhip

    def build(seed):
        env = rlhip.CartPoleEnv(256, seed=seed)
        return env, rlhip.PPOPolicy(env, update_freq=16, hidden=64, seed=seed)

    env, pol = build(3)
    rlhip.run_fused_ppo(pol, env, 3)
    rlhip.save_checkpoint(str(tmp_path / "p.npz"), {"policy": pol, "env": env})
    rlhip.run_fused_ppo(pol, env, 3)
    env2, pol2 = build(77)
    rlhip.load_checkpoint(str(tmp_path / "p.npz"), {"policy": pol2, "env": env2})
    rlhip.run_fused_ppo(pol2, env2, 3)
    torch.cuda.synchronize()
    for x, y in ((pol.params, pol2.params), (pol.m, pol2.m), (pol.v, pol2.v), (pol.beta_pow, pol2.beta_pow),
                 (env._s, env2._s), (env._episode, env2._episode), (pol.trajectory.obs, pol2.trajectory.obs)):
        assert torch.equal(x, y)
    assert (pol.vec_step, pol.update_ctr) == (pol2.vec_step, pol2.update_ctr)
    assert not np.array_equal(rlhip.state_dict(pol)["params"], rlhip.state_dict(build(3)[1])["params"])


def test_debug_timer_reports_device_time_per_run_loop_section():
    """RLCore.timer with enable_debug_timings (RLCore/test/core/base.jl:41-57): the sections of run.jl:46-72, each with
    the device time between two HIP events on the compute stream"""
    import rlhip

    n = 4096
    env = rlhip.CartPoleEnv(n, seed=2)
    net = rlhip.HipApproximator(4, 128, 2, seed=2)
    learner = rlhip.DQNLearner(rlhip.TargetNetwork(net, sync_freq=10), batchsize=512, min_replay_history=n, seed=2)
    agent = rlhip.Agent(rlhip.QBasedPolicy(learner, rlhip.EpsilonGreedyExplorer(0.05, seed=2)),
                        rlhip.Trajectory(rlhip.CircularArraySARTSTraces(capacity=32, n_env=n, obs_dim=4)))
    rlhip.timer.reset_()
    rlhip.enable_debug_timings()
    try:
        rlhip.run(agent, env, rlhip.StopAfterNSteps(700))   # > the resolve batch: events are recycled
    finally:
        rlhip.disable_debug_timings()
    d = rlhip.timer.todict()
    assert list(d)[:4] == ["plan!", "push!(policy) PreActStage", "push!(hook) PreActStage", "act!"]
    assert all(v["ncalls"] == 700 for v in d.values())
    for k in ("plan!", "act!", "push!(policy) PostActStage", "optimise! PostActStage"):
        assert 700 * 1e-3 < d[k]["device_ms"] < 700 * 2.0, (k, d[k])       # 1 us .. 2 ms of device time per call
    assert d["optimise! PostActStage"]["device_ms"] > d["push!(hook) PostActStage"]["device_ms"]
    print(rlhip.timer)
    n_before = len(d)
    rlhip.run(agent, env, rlhip.StopAfterNSteps(3))          # disabled again: nothing is recorded
    assert rlhip.timer.todict()["plan!"]["ncalls"] == 700 and len(rlhip.timer.todict()) == n_before


@pytest.mark.parametrize("form", ["torch.distributed.run", "bare"])
def test_bench_two_ranks_on_one_device_prints_the_contract_line(form):
    """bench.py --gpus 2 as the driver launches it -- under torch.distributed.run (one rank per process), and BARE
    (`python bench.py --gpus 2`, the form the driver uses at N = 1: bench.py must then launch its ranks itself, VERDICT r3
    item 3) -- both ranks on this box's single GPU via the RLHIP_BENCH_SINGLE_DEVICE test hook: the JSON contract line, the
    exchange mode, the all-reduce report of SURVEY 8(e), no peer-to-peer timeouts"""
    import json

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, RLHIP_BENCH_SINGLE_DEVICE="1", RLHIP_BENCH_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0")  # RCCL refuses two ranks on one device
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    tail = [os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "5", "--warmup", "2", "--full"]
    if form == "bare":
        cmd = [sys.executable] + tail
    else:
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
               "127.0.0.1", "--master-port", str(_free_port())] + tail
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["steps"] == 5 and d["scaling"] == "weak" and d["value"] > 0
    assert d["metric"] == "env_steps_per_sec" and d["config"]["n_envs_per_gpu"] == 4096
    assert d["replicas_bit_identical"] is True  # every rank applied the same reduced gradients: same parameters, bit for bit
    ar = d["allreduce"]
    assert "error" not in ar and ar["world"] == 2 and ar["gradient_bytes"] == 3331 * 4
    assert ar["library_us_at_gradient_size"] > 0 and len(ar["library_sweep"]) == 5
    if d["gradient_allreduce"].startswith("p2p"):
        assert d["p2p_timeouts"] is False and ar["p2p_us_at_gradient_size"] > 0
    # the sweep through the product's own collective (rlhip_allreduce_grads), next to torch.distributed's
    sweep = ar["abi_sweep"]
    assert isinstance(sweep, list) and [r["bytes"] for r in sweep] == [4 << 10, 64 << 10, 1 << 20, 16 << 20, 256 << 20], sweep
    assert ar["abi_sweep_p2p"]["cap_bytes"] == 16 << 20
    if ar["abi_sweep_p2p"]["active"]:
        assert all(r["transport"] == "p2p kernel" and r["us"] > 0 for r in sweep[:4]), sweep
    assert sweep[4]["transport"].startswith("none")  # gloo group: no RCCL behind the ABI for 256 MB
    assert "abi_sweep_timeout" not in ar


def _grid_barrier_probe():
    """one PPO update (reduce_apply_kernel<APPLY_GRID>) + a few 3-layer DQN updates (d3_apply_kernel): parameter bytes"""
    import rlhip

    env = rlhip.CartPoleEnv(512, seed=3)
    pol = rlhip.PPOPolicy(env, update_freq=8, seed=3)
    pol.rollout_()
    pol.update_()
    n = 128
    e2 = rlhip.CartPoleEnv(n, seed=5)
    net = rlhip.HipApproximator(4, 128, 2, seed=5, layers=3)
    tn = rlhip.TargetNetwork(net, sync_freq=3)
    learner = rlhip.DQNLearner(tn, batchsize=64, min_replay_history=2 * n, seed=5, max_grad_norm=1.0)
    policy = rlhip.QBasedPolicy(learner, rlhip.EpsilonGreedyExplorer(0.1, seed=5))
    agent = rlhip.Agent(policy, rlhip.Trajectory(rlhip.CircularArraySARTSTraces(capacity=8, n_env=n, obs_dim=4)))
    rlhip.run_fused_dqn(agent, e2, rlhip.StopAfterNSteps(12))
    # 3-layer PPO: gradient + fused optimiser tail (d3_apply_kernel with two nets: reduce, loss line, norm, clip, Adam,
    # bf16 re-pack of both W2) -- or, without the grid barrier, reduce / clip_adam / pack as separate launches
    e3 = rlhip.HipVecEnv("pendulum", 256, seed=9)
    p3 = rlhip.PPOPolicy(e3, update_freq=8, hidden=128, seed=9, layers=3)
    p3.rollout_()
    p3.update_()
    torch.cuda.synchronize()
    return (pol.params.cpu().numpy().tobytes() + net.params.cpu().numpy().tobytes() + p3.params.cpu().numpy().tobytes()
            + p3.losses.cpu().numpy().tobytes()), learner.n_updates


def test_grid_barrier_kernels_while_another_stream_saturates_the_device():
    """the spin-barrier kernels (occupancy-sized grids, csrc/common.h grid_barrier_capacity) must
    finish -- with the same bits -- while a second stream keeps every CU busy with thousands of streaming workgroups"""
    import rlhip
    from rlhip._lib import call
    from rlhip.ops import ptr

    quiet, nup = _grid_barrier_probe()
    assert nup >= 8
    big = rlhip.HipVecEnv("cartpole", 1 << 22, seed=1, packed_episode=True)
    acts = torch.randint(0, 2, (1 << 22,), dtype=torch.int32, device="cuda")
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        for _ in range(400):  # ~40 us x 400 of 4096-workgroup launches queued on the side stream
            call("rlhip_env_step", big.kind, 0, C.byref(big.cfg), C.byref(big._st), big.n, ptr(acts), 1, big.seed, 0, None,
                 None, C.c_void_p(side.cuda_stream))
    busy, _ = _grid_barrier_probe()  # enqueued while the side stream is saturating the device
    torch.cuda.synchronize()
    assert busy == quiet


def test_barrier_free_fallback_of_the_optimiser_tails_is_bit_identical():
    """RLHIP_GRID_BARRIER_CAP=0 (what a device too small for co-residency gets): the last-arriver reduce_apply variant
    and the unfused 3-layer tail produce the same parameters as the grid-barrier kernels"""
    import hashlib

    src = ("import os, sys, hashlib\n"
           "sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
           "import torch\n"
           "import tests.test_gpu_run as t\n"
           "b, n = t._grid_barrier_probe()\n"
           "print('HASH', hashlib.sha256(b).hexdigest(), n)\n") % (
        os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
        os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "reinforcementlearning.jl_amd"))
    env = dict(os.environ, RLHIP_GRID_BARRIER_CAP="0")
    r = subprocess.run([sys.executable, "-c", src], env=env, capture_output=True, text=True, timeout=600,
                       cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    assert r.returncode == 0, r.stderr[-2000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("HASH")][0].split()
    here, nup = _grid_barrier_probe()
    assert line[1] == hashlib.sha256(here).hexdigest() and int(line[2]) == nup


@pytest.mark.parametrize("fused", [False, True])
def test_dqn_update_freq_and_sample_ratio_controller_gate_the_updates(fused):
    """`update_freq` and the trajectory's InsertSampleRatioController were stored but never consulted.
    update_freq = 4 -> one optimiser step every fourth vec-step after the warm-up; ratio = 0.5 -> every second; both
    loops (per-step protocol and one-call-per-step) gate identically and end with identical parameters."""
    import rlhip

    def build(update_freq, ratio):
        n = 64
        env = rlhip.CartPoleEnv(n, seed=3)
        net = rlhip.HipApproximator(4, 128, 2, seed=3)
        learner = rlhip.DQNLearner(rlhip.TargetNetwork(net, sync_freq=5), batchsize=32, min_replay_history=4 * n, seed=3,
                                   update_freq=update_freq)
        policy = rlhip.QBasedPolicy(learner, rlhip.EpsilonGreedyExplorer(0.1, seed=3))
        traj = rlhip.Trajectory(rlhip.CircularArraySARTSTraces(capacity=32, n_env=n, obs_dim=4),
                                controller=rlhip.InsertSampleRatioController(ratio=ratio, threshold=1))
        return env, learner, net, rlhip.Agent(policy, traj)

    runner = rlhip.run_fused_dqn if fused else rlhip.run
    counts = {}
    for uf, ratio in ((1, 1.0), (4, 1.0), (1, 0.5)):
        env, learner, net, agent = build(uf, ratio)
        runner(agent, env, rlhip.StopAfterNSteps(44))
        torch.cuda.synchronize()
        counts[(uf, ratio)] = learner.n_updates
        assert learner.vec_steps == 44 and learner.draw_ctr == learner.n_updates
    assert counts[(1, 1.0)] == 41          # warm-up: 4 vec-steps of 64 transitions, then every step
    assert counts[(4, 1.0)] == 11          # vec-steps 4, 8, ..., 44
    assert 19 <= counts[(1, 0.5)] <= 23    # n_sampled <= (n_inserted - 1) / 2
    with pytest.raises(ValueError):
        rlhip.DQNLearner(rlhip.TargetNetwork(rlhip.HipApproximator(4, 128, 2)), update_freq=0)
