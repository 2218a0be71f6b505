"""n-step gathers of a frame ring (profiles/ring_nstep.md): event timing of rlhip_ring_gather_nstep against rlhip_ring_gather, and of
rlhip_ring_gather_stacked_nstep against rlhip_ring_gather_stacked, on the Atari-shaped ring -- UInt8 frames of 84 x 84 = 7056 bytes,
one env, capacity 2^17 (0.9 GB: beyond the caches), batch 4096, a fresh index vector for every launch (drawn before the timed
blocks by rlhip_ring_sample_indices_nstep, the same vectors for both members of a pair).  Everything goes through the C ABI on
outputs allocated once.  The two members of a pair alternate in ONE process, block by block, after a settle phase of untimed
launches; the median, minimum and maximum over the blocks are printed per series, then the ratio of the medians and the share of
8 TB/s that the algorithmic bytes of a launch reach.

    python tools/bench_ring_nstep.py [--rounds 5] [--reps 400] [--capacity 131072] [--batch 4096] [--n-step 3] [--n-stack 4]

The ring is filled in place (random frames, rewards, terminals at --p-term) and its host counters are set to "full": pushing 2^17
frames one launch at a time would only test the push.  One JSON line per series, times in microseconds per launch."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--reps", type=int, default=400)
ap.add_argument("--capacity", type=int, default=1 << 17)
ap.add_argument("--batch", type=int, default=4096)
ap.add_argument("--frame", type=int, default=7056)
ap.add_argument("--n-step", type=int, default=3)
ap.add_argument("--n-stack", type=int, default=4)
ap.add_argument("--p-term", type=float, default=0.005)
args = ap.parse_args()
assert args.rounds >= 3, "a pair alternates at least three times"
tree = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, tree)
sys.path.insert(0, os.path.join(tree, "reinforcementlearning.jl_amd"))

import torch  # noqa: E402

import rlhip as rl  # noqa: E402
from rlhip._lib import call  # noqa: E402
from rlhip.ops import ptr, stream_ptr  # noqa: E402

assert torch.cuda.is_available(), "a timing needs the GPU"
SETTLE_S, HBM_BPS = 0.3, 8e12
cap, b, fb, n, k = args.capacity, args.batch, args.frame, args.n_step, args.n_stack

tr = rl.CircularArraySARTSTraces(capacity=cap, n_env=1, obs_dim=fb, dtype=torch.uint8)
assert tr.frame_major
g = torch.Generator(device="cuda").manual_seed(1)
for lo in range(0, cap + 1, 4096):  # (in slices: randint has no uint8 fill of 0.9 GB in one piece everywhere)
    hi = min(lo + 4096, cap + 1)
    tr.state[lo:hi] = torch.randint(0, 256, (hi - lo, fb, 1), dtype=torch.uint8, device="cuda", generator=g)
tr.action.copy_(torch.randint(0, 18, (cap, 1), dtype=torch.int32, device="cuda", generator=g))
tr.reward.copy_(torch.randn(cap, 1, device="cuda", generator=g))
tr.terminal.copy_((torch.rand(cap, 1, device="cuda", generator=g) < args.p_term).to(torch.uint8))
tr.rb.len_rt, tr.rb.len_sa = cap, cap + 1  # full, heads at 0
assert len(tr) == cap

n_vec = 2 * args.reps  # index vectors: no launch of a block repeats one
idx = torch.empty((n_vec, b), dtype=torch.int64, device="cuda")
for v in range(n_vec):
    call("rlhip_ring_sample_indices_nstep", C.byref(tr.rb), b, n, 7, v, ptr(idx[v]), stream_ptr())


def outputs(per_sample):
    u8 = lambda m: torch.empty(m, dtype=torch.uint8, device="cuda")  # noqa: E731
    return (u8(b * per_sample), torch.empty(b, dtype=torch.int32, device="cuda"), torch.empty(b, dtype=torch.float32, device="cuda"),
            u8(b), u8(b * per_sample), torch.empty(b, dtype=torch.int32, device="cuda"))


def launches():
    s, a, r, t, sn, nu = plain = outputs(fb)
    S, A, R, T, SN, NU = stacked = outputs(k * fb)
    ctr = [0]

    def nxt():
        ctr[0] = (ctr[0] + 1) % n_vec
        return ptr(idx[ctr[0]])

    def one(_keep=plain):
        call("rlhip_ring_gather", C.byref(tr.rb), nxt(), b, ptr(s), ptr(a), ptr(r), ptr(t), ptr(sn), stream_ptr())

    def nstep(_keep=plain):
        call("rlhip_ring_gather_nstep", C.byref(tr.rb), nxt(), b, n, 0.99, ptr(s), ptr(a), ptr(r), ptr(t), ptr(sn), ptr(nu), stream_ptr())

    def one_stacked(_keep=stacked):
        call("rlhip_ring_gather_stacked", C.byref(tr.rb), nxt(), b, k, ptr(S), ptr(A), ptr(R), ptr(T), ptr(SN), stream_ptr())

    def nstep_stacked(_keep=stacked):
        call("rlhip_ring_gather_stacked_nstep", C.byref(tr.rb), nxt(), b, k, n, 0.99, ptr(S), ptr(A), ptr(R), ptr(T), ptr(SN), ptr(NU),
             stream_ptr())

    return (one, nstep, nu), (one_stacked, nstep_stacked, NU)


def settle(f):
    t_end = time.perf_counter() + SETTLE_S
    while time.perf_counter() < t_end:
        for _ in range(8):
            f()
        torch.cuda.synchronize()


def block(f):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(args.reps):
        f()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / args.reps * 1e3


def pair(name, f1, fn, bytes1, bytesn):
    settle(f1)
    settle(fn)
    us1, usn = [], []
    for _ in range(args.rounds):  # alternated: 1-step block, n-step block
        us1.append(block(f1))
        usn.append(block(fn))
    m1, mn = statistics.median(us1), statistics.median(usn)
    for series, us, m, nbytes in ((f"{name}_1step", us1, m1, bytes1), (f"{name}_nstep", usn, mn, bytesn)):
        print(json.dumps(dict(series=series, us=[round(m, 2), round(min(us), 2), round(max(us), 2)], bytes=int(nbytes),
                              tb_per_s=round(nbytes / m / 1e6, 3), share_of_8tbs=round(nbytes / (m * 1e-6) / HBM_BPS, 3))), flush=True)
    print(json.dumps(dict(pair=name, ratio_nstep_over_1step=round(mn / m1, 4))), flush=True)


props = torch.cuda.get_device_properties(0)
print(json.dumps(dict(device=props.name, cus=props.multi_processor_count, torch=torch.__version__, hip=torch.version.hip, capacity=cap,
                      batch=b, frame_bytes=fb, n_step=n, n_stack=k, p_term=args.p_term, rounds=args.rounds, reps=args.reps,
                      settle_s=SETTLE_S, columns="[median, min, max] us per launch")), flush=True)
(one, nstep, nu), (one_stacked, nstep_stacked, NU) = launches()
# algorithmic bytes of a launch (frames only; the scalars are < 0.1 %): plain -- two frames read, two written, either form; stacked --
# n_stack + 1 frames read by the 1-step form, n_stack + min(ns, n_stack) by the n-step form (the union of two stacks that lie ns
# apart; zero-filled members are not read: an upper bound), 2 n_stack written by both
nstep_stacked()
torch.cuda.synchronize()
ns = NU.to(torch.int64)
print(json.dumps(dict(mean_n_used=round(float(ns.double().mean()), 4), share_cut=round(float((ns < n).double().mean()), 4))), flush=True)
read_n = float((k + torch.clamp(ns, max=k)).double().mean())
pair("gather", one, nstep, 4 * fb * b, 4 * fb * b)
pair("gather_stacked", one_stacked, nstep_stacked, (k + 1 + 2 * k) * fb * b, (read_n + 2 * k) * fb * b)
