"""Prioritized n-step replay on a frame ring (profiles/per_frames_nstep.md): event timing of the fused draw + n-step gather
(rlhip_ring_sample_gather_nstep_prioritized, rlhip_ring_sample_gather_stacked_nstep_prioritized) against the two launches it replaces
(rlhip_ring_sample_prioritized, then rlhip_ring_gather_nstep / rlhip_ring_gather_stacked_nstep on its indices), on the Atari-shaped
ring of tools/bench_ring_nstep.py -- UInt8 frames of 84 x 84 = 7056 bytes, one env, capacity 2^17 (0.9 GB: beyond the caches), full,
terminals at --p-term -- under a tree masked for --n-step whose priorities have been written back at random (a quarter of them 0).
Every launch draws with a draw counter of its own, so no launch of a block repeats a batch.  Everything goes through the C ABI on
outputs allocated once.  The two members of a pair alternate in ONE process, block by block, after a settle phase of untimed launches;
per series the median, minimum and maximum over the blocks are printed, then per pair the ratio of the medians next to the spread
between blocks, (max - min) / median of the wider series: the fused form meets its bar when fused - two <= that spread.

    python tools/bench_per_frames_nstep.py [--rounds 5] [--reps 400] [--capacity 131072] [--batch 32,512,4096] [--n-step 3] [--n-stack 4]

The ring is filled in place and its host counters are set to "full" (pushing 2^17 frames one launch at a time would only test the
push); with both heads at 0 the leaf of logical frame li is li, so the masked tree is: leaves 0 .. capacity - n_step written, the newest
n_step - 1 left at 0.  One JSON line per series and per pair, times in microseconds per launch (a pair of launches for the composition).
RLHIP_LIB_PATH selects another build of the library (how the one-barrier schedule of the frame-major kernel was timed)."""
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
ap.add_argument("--batch", type=str, default="32,512,4096")
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
SETTLE_S = 0.3
cap, fb, n, k = args.capacity, args.frame, args.n_step, args.n_stack
batches = [int(x) for x in args.batch.split(",")]

tr = rl.CircularPrioritizedFrameTraces(capacity=cap, n_env=1, obs_dim=fb, dtype=torch.uint8, default_priority=1.0, n_step=n)
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
# the masked tree, then the write-back: every complete start once, in random order, a quarter of the priorities 0
starts = cap - n + 1
call("rlhip_sumtree_fill_range", ptr(tr.priorities), tr.n_leaves, 0, starts, 1.0, stream_ptr())
keys = torch.randperm(starts, device="cuda", generator=g)
prio = torch.rand(starts, device="cuda", generator=g) * 4 + 0.01
prio[torch.rand(starts, device="cuda", generator=g) < 0.25] = 0.0
tr.set_priority_(keys, prio)
leaves = tr.priorities[tr.priorities.numel() // 2:][:cap]
assert float(leaves[starts:].sum()) == 0.0 and float(tr.priorities[1]) > 0.0


def outputs(b, per_sample):
    u8 = lambda m: torch.empty(m, dtype=torch.uint8, device="cuda")  # noqa: E731
    i64 = lambda: torch.empty(b, dtype=torch.int64, device="cuda")  # noqa: E731
    return (i64(), i64(), torch.empty(b, dtype=torch.float32, device="cuda"), u8(b * per_sample), torch.empty(b, dtype=torch.int32, device="cuda"),
            torch.empty(b, dtype=torch.float32, device="cuda"), u8(b), u8(b * per_sample), torch.empty(b, dtype=torch.int32, device="cuda"))


def launches(b):
    idx, key, pr, s, a, r, t, sn, nu = plain = outputs(b, fb)
    IDX, KEY, PR, S, A, R, T, SN, NU = stacked = outputs(b, k * fb)
    rb, tp, ctr = C.byref(tr.rb), ptr(tr.priorities), [0]

    def nxt():
        ctr[0] += 1
        return ctr[0]

    def two(_keep=plain):
        call("rlhip_ring_sample_prioritized", rb, tp, b, 7, nxt(), ptr(idx), ptr(key), ptr(pr), stream_ptr())
        call("rlhip_ring_gather_nstep", rb, ptr(idx), b, n, 0.99, ptr(s), ptr(a), ptr(r), ptr(t), ptr(sn), ptr(nu), stream_ptr())

    def fused(_keep=plain):
        call("rlhip_ring_sample_gather_nstep_prioritized", rb, tp, b, n, 0.99, 7, nxt(), ptr(idx), ptr(key), ptr(pr), ptr(s), ptr(a), ptr(r),
             ptr(t), ptr(sn), ptr(nu), stream_ptr())

    def two_stacked(_keep=stacked):
        call("rlhip_ring_sample_prioritized", rb, tp, b, 7, nxt(), ptr(IDX), ptr(KEY), ptr(PR), stream_ptr())
        call("rlhip_ring_gather_stacked_nstep", rb, ptr(IDX), b, k, n, 0.99, ptr(S), ptr(A), ptr(R), ptr(T), ptr(SN), ptr(NU), stream_ptr())

    def fused_stacked(_keep=stacked):
        call("rlhip_ring_sample_gather_stacked_nstep_prioritized", rb, tp, b, k, n, 0.99, 7, nxt(), ptr(IDX), ptr(KEY), ptr(PR), ptr(S), ptr(A),
             ptr(R), ptr(T), ptr(SN), ptr(NU), stream_ptr())

    return (two, fused, nu), (two_stacked, fused_stacked, NU)


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


def pair(name, b, f2, f1):
    settle(f2)
    settle(f1)
    us2, us1 = [], []
    for _ in range(args.rounds):  # alternated: a block of the two launches, a block of the fused one
        us2.append(block(f2))
        us1.append(block(f1))
    m2, m1 = statistics.median(us2), statistics.median(us1)
    for series, us, m in ((f"{name}_two_launches", us2, m2), (f"{name}_fused", us1, m1)):
        print(json.dumps(dict(series=series, batch=b, us=[round(m, 2), round(min(us), 2), round(max(us), 2)])), flush=True)
    spread = max((max(us) - min(us)) / statistics.median(us) for us in (us2, us1))
    print(json.dumps(dict(pair=name, batch=b, ratio_fused_over_two=round(m1 / m2, 4), spread_between_blocks=round(spread, 4),
                          fused_within_spread=bool(m1 / m2 - 1.0 <= spread))), flush=True)


props = torch.cuda.get_device_properties(0)
print(json.dumps(dict(device=props.name, cus=props.multi_processor_count, torch=torch.__version__, hip=torch.version.hip,
                      lib=os.path.basename(os.environ.get("RLHIP_LIB_PATH", "default")), capacity=cap, frame_bytes=fb, n_step=n, n_stack=k, p_term=args.p_term,
                      rounds=args.rounds, reps=args.reps, settle_s=SETTLE_S, columns="[median, min, max] us per launch (pair of launches)")),
      flush=True)
for b in batches:
    (two, fused, nu), (two_stacked, fused_stacked, NU) = launches(b)
    fused()
    torch.cuda.synchronize()
    assert 1 <= int(nu.min()) and int(nu.max()) <= n
    print(json.dumps(dict(batch=b, mean_n_used=round(float(nu.double().mean()), 4), share_cut_by_a_terminal=round(float((nu < n).double().mean()), 4))),
          flush=True)
    pair("gather", b, two, fused)
    pair("gather_stacked", b, two_stacked, fused_stacked)
