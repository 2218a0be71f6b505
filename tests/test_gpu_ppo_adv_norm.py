"""PPO advantage normalisation on the GPU (rlhip_ppo_cfg.normalize_advantage = 1, csrc/ppo_advnorm.hip) against the oracle:
the normalised values and {mean, std} of rlhip_ppo_adv_normalize_f32, the flag-on gradients of every learner family, the
update loop, the device-counter and graph paths, and learning on Pendulum."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import oracle  # noqa: E402
from conftest import BF16_GRAD_TOL, F32_GRAD_TOL, assert_grad_close  # noqa: E402


@pytest.fixture(scope="module")
def rl():
    import rlhip

    return rlhip


def dev(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).cuda()


def host(t):
    return t.detach().cpu().numpy()


def _oracle_norm(x):
    """oracle/rlo_learn.c's branch: sequential Float64 sums (np.cumsum adds in order), corrected std, clamp, one rounding"""
    x = x.astype(np.float64)
    bm = x.size
    mu = np.cumsum(x)[-1] / bm
    s2 = np.cumsum((x - mu) * (x - mu))[-1]
    sd = min(max(np.sqrt(s2 / (bm - 1 if bm > 1 else 1)), 1e-8), 1000.0)
    return ((x - mu) / sd).astype(np.float32), mu, sd


def _perm(seed, epoch, total, mb, bm):
    return np.array([oracle.permute(seed, epoch, total, mb * bm + b) for b in range(bm)])


def _normalize(rl, cfg, n, T, adv, seed, epoch, mb):
    from rlhip._lib import call
    from rlhip.ops import ptr, stream_ptr

    out = torch.full((T, n), float("nan"), dtype=torch.float32, device="cuda")
    stats = torch.zeros(2, dtype=torch.float64, device="cuda")
    call("rlhip_ppo_adv_normalize_f32", C.byref(cfg), n, T, ptr(adv), seed, epoch, mb, ptr(out), ptr(stats), stream_ptr())
    torch.cuda.synchronize()
    return host(out).reshape(-1), host(stats)


@pytest.mark.parametrize("n,T", [(256, 16), (4096, 32), (4096, 128)])
@pytest.mark.parametrize("dist", ["shifted", "constant", "wide"])
def test_normalised_values_vs_oracle(rl, n, T, dist):
    from rlhip.ppo import make_ppo_cfg

    nmb, seed, epoch = 4, 17, 5
    cfg = make_ppo_cfg(n_microbatches=nmb, normalize_advantage=1)
    rng = np.random.default_rng(n + T)
    if dist == "shifted":  # mean far from 0, std far from 1
        a = 300.0 + 40.0 * rng.standard_normal(n * T)
    elif dist == "constant":  # std 0 -> clamped to 1e-8
        a = np.full(n * T, 3.25)
    else:  # std above 1000 -> clamped to 1000
        a = -800.0 + 5e4 * rng.standard_normal(n * T)
    a = a.astype(np.float32)
    adv = dev(a.reshape(T, n))
    total, bm = n * T, (n * T) // nmb
    for mb in ((0, 3) if total <= 4096 * 32 else (2,)):
        out, stats = _normalize(rl, cfg, n, T, adv, seed, epoch, mb)
        perm = _perm(seed, epoch, total, mb, bm)
        o, mu, sd = _oracle_norm(a[perm])
        g = out[perm]
        # entries of the other micro-batches are untouched
        rest = np.ones(total, bool)
        rest[perm] = False
        assert np.isnan(out[rest]).all()
        # mu / sd: the GPU sums in a fixed tree, the oracle sequentially -- bm additions of |x| <= max|x| apart
        bound = bm * 2.0 ** -52 * np.abs(a[perm].astype(np.float64)).sum() / bm
        assert abs(stats[0] - mu) <= bound, (stats[0], mu)
        assert abs(stats[1] - sd) <= bm * 2.0 ** -52 * sd, (stats[1], sd)
        if dist == "constant":
            assert stats[1] == 1e-8 and not g.any()
        if dist == "wide":
            assert stats[1] == 1000.0
        ulp = np.abs(g.view(np.int32).astype(np.int64) - o.view(np.int32).astype(np.int64))
        assert ulp.max() <= 1, f"{ulp.max()} ulp"
        assert (ulp == 0).mean() >= 0.999, f"bit-equal share {(ulp == 0).mean():.5f}"
        # run to run: bit-identical
        out2, stats2 = _normalize(rl, cfg, n, T, adv, seed, epoch, mb)
        assert np.array_equal(out2.view(np.int32), out.view(np.int32)) and np.array_equal(stats2, stats)


def _pair(rl, kind, n, T, seed=3, hidden=256, **kw):
    env = rl.HipVecEnv(kind, n, seed=seed)
    pol = rl.PPOPolicy(env, update_freq=T, hidden=hidden, normalize_advantage=1, **kw)
    ocfg = oracle.ppo_default(continuous=int(env.continuous), hidden=hidden, normalize_advantage=1, **kw)
    return env, pol, ocfg


def _micro(pol, tr, epoch_ctr, mb):
    n, T = tr.n, tr.T
    total = n * T
    bm = total // pol.cfg.n_microbatches
    perm = _perm(pol.seed, epoch_ctr, total, mb, bm)
    t, i = perm // n, perm % n
    obs = host(tr.obs)[t, :, i].T.copy()
    flat = lambda x: host(x).reshape(-1)[perm]  # noqa: E731
    act = host(tr.action_f)[t, 0, i][None, :] if tr.continuous else host(tr.action_i).reshape(-1)[perm]
    return obs, act, flat(tr.logp), flat(tr.adv), flat(tr.ret)


def _scaled_adv(pol, scale, shift):
    """GAE advantages moved far from mean 0 / std 1, so that the normalisation is visible in the gradient"""
    pol.trajectory.adv.mul_(scale).add_(shift)


@pytest.mark.parametrize("kind,hidden,act,n,T,nmb", [("cartpole", 256, 0, 256, 16, 4), ("cartpole", 64, 1, 256, 16, 4),
                                                     ("pendulum", 256, 0, 256, 16, 4), ("mountaincar", 128, 0, 256, 16, 4),
                                                     ("cartpole", 256, 0, 100, 7, 3)])
def test_two_layer_gradient_vs_oracle(rl, kind, hidden, act, n, T, nmb):
    env, pol, ocfg = _pair(rl, kind, n, T, hidden=hidden, act=act, n_microbatches=nmb)
    pol.rollout_()
    pol.gae_()
    _scaled_adv(pol, 30.0, 200.0)
    rng = np.random.default_rng(1)
    p2 = (host(pol.params) + rng.standard_normal(pol.np) * 0.02).astype(np.float32)
    pol.params.copy_(dev(p2))
    tr = pol.trajectory
    off = oracle.ppo_default(continuous=int(env.continuous), hidden=hidden, act=act, n_microbatches=nmb)
    for epoch_ctr, mb in ((0, 0), (5, nmb - 1)):
        pol.grad_(epoch_ctr, mb)
        obs, a, lp, adv, ret = _micro(pol, tr, epoch_ctr, mb)
        g, losses = oracle.ppo_loss_grad(ocfg, env.odim, pol.na, p2, obs, a, lp, adv, ret)
        assert_grad_close(host(pol.grad), g, F32_GRAD_TOL, f"ppo_grad normalised {kind} h={hidden} mb={mb}")
        np.testing.assert_allclose(host(pol.losses), losses, rtol=1e-4, atol=1e-6)
        g_off, _ = oracle.ppo_loss_grad(off, env.odim, pol.na, p2, obs, a, lp, adv, ret)
        assert np.abs(g_off - g).max() / np.abs(g).max() > 1e3 * F32_GRAD_TOL
        # grad_fresh reads the same plane
        pol.grad_(epoch_ctr, mb, records_fresh=True)
        assert_grad_close(host(pol.grad), g, F32_GRAD_TOL, f"ppo_grad_fresh normalised {kind} h={hidden} mb={mb}")


@pytest.mark.parametrize("hidden", [128, 256])
@pytest.mark.parametrize("kind", ["cartpole", "pendulum"])
def test_layers3_gradient_vs_oracle(rl, kind, hidden):
    n, T = 96, 9
    env, pol, ocfg = _pair(rl, kind, n, T, seed=5, hidden=hidden, layers=3, n_microbatches=2)
    pol.rollout_()
    pol.gae_()
    _scaled_adv(pol, 30.0, -500.0)
    tr = pol.trajectory
    params = host(pol.params)
    ns, na = env.odim, pol.na
    off = oracle.ppo_default(continuous=int(env.continuous), hidden=hidden, layers=3, n_microbatches=2)
    for epoch, mb in ((0, 0), (3, 1)):
        pol.grad_(epoch, mb)
        g = host(pol.grad)
        obs, a, lp, adv, ret = _micro(pol, tr, epoch, mb)
        og, ol = oracle.ppo_loss_grad(ocfg, ns, na, params, obs, a, lp, adv, ret)
        assert np.all(np.abs(host(pol.losses) - ol) <= 2e-4 * (1 + np.abs(ol)))
        np_a = pol.np_actor
        for name, x, y in (("actor", g[:np_a], og[:np_a]), ("critic", g[np_a:], og[np_a:])):
            o = 0
            nout = (2 if name == "actor" else 1)
            for tname, sz in (("W1", hidden * ns), ("b1", hidden), ("W2", hidden * hidden), ("b2", hidden),
                              ("W3", nout * hidden), ("b3", nout)):
                assert_grad_close(x[o:o + sz], y[o:o + sz], BF16_GRAD_TOL, f"ppo3 normalised h={hidden} {name} {tname}")
                o += sz
        g_off, _ = oracle.ppo_loss_grad(off, ns, na, params, obs, a, lp, adv, ret)
        assert np.abs(g_off - og).max() / np.abs(og).max() > 10 * BF16_GRAD_TOL


@pytest.mark.parametrize("kind,n,T,hidden,layers", [("cartpole", 256, 16, 256, 2), ("cartpole", 4096, 32, 256, 2),
                                                    ("pendulum", 256, 16, 256, 2), ("cartpole", 256, 16, 128, 3),
                                                    ("pendulum", 256, 16, 256, 3)])
def test_update_equals_manual_sequence_and_tracks_oracle(rl, kind, n, T, hidden, layers):
    envA, polA, ocfg = _pair(rl, kind, n, T, hidden=hidden, layers=layers)
    envB, polB, _ = _pair(rl, kind, n, T, hidden=hidden, layers=layers)
    polA.rollout_()
    polB.rollout_()
    for p in (polA, polB):
        _scaled_adv(p, 30.0, 200.0)
    p0 = host(polA.params).copy()
    polA._adv_ready = True
    polA.update_()
    for e in range(polB.cfg.n_epochs):
        for mb in range(polB.cfg.n_microbatches):
            polB.grad_(e, mb)
            polB.apply_(1.0)
    polB.update_ctr += 1
    if layers == 2:  # layers = 3: the update fuses the bf16 re-pack (tests/test_gpu_ppo3*.py); compare with the oracle only
        assert torch.equal(polA.params, polB.params)
        assert torch.equal(polA.m, polB.m) and torch.equal(polA.v, polB.v) and torch.equal(polA.beta_pow, polB.beta_pow)
    tr = polA.trajectory
    otr = oracle.PPOTraj(oracle.KIND[kind], n, T, continuous=envA.continuous)
    for name in ("obs", "logp", "value", "reward", "terminal", "adv", "ret"):
        getattr(otr, name)[...] = host(getattr(tr, name)).reshape(getattr(otr, name).shape)
    if envA.continuous:
        otr.action_f[...] = host(tr.action_f).reshape(otr.action_f.shape)
    else:
        otr.action_i[...] = host(tr.action_i)
    po, mo, vo = p0.copy(), np.zeros_like(p0), np.zeros_like(p0)
    oracle.use_all_cores(True)
    try:
        steps, _ = oracle.ppo_update(oracle.KIND[kind], ocfg, otr, po, mo, vo, 0, polA.seed, 0)
    finally:
        oracle.use_all_cores(False)
    assert steps == polA.cfg.n_epochs * polA.cfg.n_microbatches
    d = np.abs(host(polA.params) - po)
    q99 = 2e-4 if layers == 2 else 2e-3
    assert np.quantile(d, 0.99) < q99, f"99th percentile |dp| = {np.quantile(d, 0.99):.2e}"
    assert d.max() < steps * 2 * 1e-3
    assert np.abs(po - p0).max() > 1e-3


def test_device_counters_graph_replay_and_determinism(rl):
    n, T = 512, 8
    pols = []
    for _ in range(4):
        env = rl.CartPoleEnv(n, seed=9)
        pols.append(rl.PPOPolicy(env, update_freq=T, normalize_advantage=1))
    a, b, c, d = pols
    for _ in range(2):
        for p in pols:
            p.rollout_()
            p.update_()
    b.sync_counters_()
    c.capture_graph_(warmup=0)
    for it in range(3):
        a.rollout_()
        a.update_()
        d.rollout_()
        d.update_()
        b.iteration_dc_()
        c.replay_()
        torch.cuda.synchronize()
        assert torch.equal(a.params, d.params), f"two eager runs differ at iteration {it}"
        assert torch.equal(a.params, b.params), f"device-counter path differs at iteration {it}"
        assert torch.equal(a.params, c.params), f"graph replay differs at iteration {it}"
    # and the flag changed the learner at all
    env = rl.CartPoleEnv(n, seed=9)
    plain = rl.PPOPolicy(env, update_freq=T)
    for _ in range(5):
        plain.rollout_()
        plain.update_()
    assert not torch.equal(plain.params, a.params)


def _pendulum_returns(rl, normalize, iters=60):
    n, T = 1024, 200
    env = rl.HipVecEnv("pendulum", n, seed=21)
    pol = rl.PPOPolicy(env, update_freq=T, hidden=64, seed=21, lr=3e-4, normalize_advantage=normalize)
    out = []
    for _ in range(iters):
        pol.rollout_()
        out.append(float(pol.trajectory.reward.mean()) * 200)  # mean reward per step x episode length
        pol.update_()
    return np.array(out)


def test_pendulum_learns_with_normalised_advantages(rl):
    r = _pendulum_returns(rl, 1)
    first, last = r[:5].mean(), r[-5:].mean()
    print(f"pendulum mean episode return: {first:.1f} -> {last:.1f}")
    assert last > first + LEARN_MARGIN, f"{first:.1f} -> {last:.1f}"


# measured on an MI355X with these seeds: -1325.4 -> -718.3 (+607) with the flag, -1285.2 -> -1009.3 (+276) without it;
# the bar is half the measured gain with the flag
LEARN_MARGIN = 300.0


def test_gather_form_for_many_microbatches(rl):
    """n_microbatches > 64 takes the gather form: the same contract"""
    from rlhip.ppo import make_ppo_cfg

    n, T, nmb, seed, epoch = 256, 16, 100, 17, 2
    cfg = make_ppo_cfg(n_microbatches=nmb, normalize_advantage=1)
    a = (300.0 + 40.0 * np.random.default_rng(7).standard_normal(n * T)).astype(np.float32)
    adv = dev(a.reshape(T, n))
    bm = n * T // nmb
    for mb in (0, 57, 99):
        out, stats = _normalize(rl, cfg, n, T, adv, seed, epoch, mb)
        perm = _perm(seed, epoch, n * T, mb, bm)
        o, mu, sd = _oracle_norm(a[perm])
        ulp = np.abs(out[perm].view(np.int32).astype(np.int64) - o.view(np.int32).astype(np.int64))
        assert ulp.max() <= 1 and abs(stats[0] - mu) <= 2.0 ** -52 * np.abs(a[perm]).sum() and abs(stats[1] - sd) <= bm * 2.0 ** -52 * sd


def test_sharded_comm_update_refuses_world_above_one(rl):
    """rlhip_ppo_update_comm_f32 with a two-rank communicator (never set up: no peer, no launch) refuses the flag"""
    from rlhip import _lib
    from rlhip.ppo import make_ppo_cfg

    h = C.c_void_p()
    _lib.call("rlhip_comm_init", 0, 2, None, 1 << 16, C.byref(h))
    try:
        on = make_ppo_cfg(normalize_advantage=1)
        traj = _lib.PPOTraj()
        rc = _lib.lib.rlhip_ppo_update_comm_f32(0, C.byref(on), 256, 16, C.byref(traj), None, None, None, None, 0, 0, None,
                                               None, None, h, None)
        assert rc == -1 and b"world > 1" in _lib.lib.rlhip_last_error()
    finally:
        _lib.lib.rlhip_comm_destroy(h)


def test_single_rank_group_grad_dc_graph_and_comm_route_equal_update(rl):
    """world = 1 with a process group: update_() takes rlhip_ppo_update_comm_f32 (step by step through the gradient calls),
    the captured iteration takes rlhip_ppo_grad_dc_f32 + all-reduce + apply; both equal the single-GPU update bit for bit"""
    import os

    import torch.distributed as dist

    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29519")
    created = False
    if not dist.is_initialized():
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
        created = True
    try:
        n, T = 256, 8
        envs = [rl.CartPoleEnv(n, seed=3) for _ in range(3)]
        ref = rl.PPOPolicy(envs[0], update_freq=T, normalize_advantage=1)
        eager = rl.PPOPolicy(envs[1], update_freq=T, process_group=dist.group.WORLD, normalize_advantage=1)
        graph = rl.PPOPolicy(envs[2], update_freq=T, process_group=dist.group.WORLD, normalize_advantage=1)
        for p in (eager, graph):
            p._force_dist = True
        graph.capture_graph_(warmup=1)
        for p in (ref, eager):
            for _ in range(2):
                p.rollout_()
                p.update_()
        graph.replay_()
        torch.cuda.synchronize()
        assert torch.equal(ref.params, eager.params)
        assert torch.equal(ref.params, graph.params)
    finally:
        if created:
            dist.destroy_process_group()
