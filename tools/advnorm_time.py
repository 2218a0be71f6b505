"""PPO advantage normalisation (profiles/advnorm.md): event timing of update_() with and without normalize_advantage, and the Pendulum learning curves"""
import json, sys, time
import numpy as np, torch
sys.path.insert(0, "reinforcementlearning.jl_amd"); sys.path.insert(0, ".")  # run from the repository root
import rlhip

def upd_time(kind, n, T, layers, hidden, norm, reps=20, gather=0):
    rlhip._lib.lib.rlhip_debug_advnorm_gather(gather)  # 1: the gather form (the A / B of profiles/advnorm.md)
    env = rlhip.HipVecEnv(kind, n, seed=3)
    pol = rlhip.PPOPolicy(env, update_freq=T, hidden=hidden, layers=layers, normalize_advantage=norm)
    pol.rollout_()
    for _ in range(3):
        pol._adv_ready = True; pol.update_()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        pol._adv_ready = True; pol.update_()
    e.record(); torch.cuda.synchronize()
    return s.elapsed_time(e) / reps * 1e3

mode = sys.argv[1]
if mode == "time":
    res = []
    for kind, n, T, layers, hidden in (("cartpole", 4096, 32, 2, 256), ("pendulum", 4096, 128, 2, 256), ("pendulum", 4096, 128, 3, 128)):
        for rep in range(2):
            for norm in (0, 1):
                us = upd_time(kind, n, T, layers, hidden, norm)
                res.append(dict(kind=kind, n=n, T=T, layers=layers, hidden=hidden, normalize=norm, rep=rep, us_per_update=round(us, 1)))
                print(json.dumps(res[-1]), flush=True)
elif mode == "ab":  # same box, alternated: flag off, binned form, gather form
    for kind, n, T, layers, hidden in (("cartpole", 4096, 32, 2, 256), ("pendulum", 4096, 128, 2, 256), ("pendulum", 4096, 128, 3, 128)):
        for rep in range(2):
            r = [round(upd_time(kind, n, T, layers, hidden, norm, gather=g), 1) for norm, g in ((0, 0), (1, 0), (1, 1))]
            print(json.dumps(dict(kind=kind, n=n, T=T, layers=layers, rep=rep, off_us=r[0], binned_us=r[1], gather_us=r[2])), flush=True)
elif mode == "trace":
    for kind, n, T, layers, hidden in (("cartpole", 4096, 32, 2, 256), ("pendulum", 4096, 128, 2, 256), ("pendulum", 4096, 128, 3, 128)):
        upd_time(kind, n, T, layers, hidden, 1, reps=10)
        upd_time(kind, n, T, layers, hidden, 1, reps=10, gather=1)
    torch.cuda.synchronize()
elif mode == "learn":
    sys.path.insert(0, "tests")
    from test_gpu_ppo_adv_norm import _pendulum_returns
    out = {}
    for norm in (1, 0):
        r = _pendulum_returns(rlhip, norm)
        out[norm] = r.tolist()
        print(norm, "first5", r[:5].mean(), "last5", r[-5:].mean(), flush=True)
