"""The host-side dispatch of csrc/optim.hip decides which kernel a size reaches; tests/test_gpu_optimiser_contract.py picks its
sizes and alignments from these thresholds.  A re-tune that moves one of them would leave a branch of that matrix untested
without any test failing -- this test fails instead (CPU only: it reads the source)."""
import os
import re

SRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "reinforcementlearning.jl_amd", "csrc", "optim.hip")

# (pattern, count): every literal the matrix depends on, exactly as often as the dispatch uses it today
PINNED = [
    (r"constexpr int64_t STREAM_MIN_N = 1 << 16;", 1),       # scalar / streaming kernels of Adam and Polyak
    (r"n <= \(\(int64_t\)1 << 23\)", 1),                     # Adam: beta powers folded into the update / a launch of their own
    (r"n >= STREAM_MIN_N && aligned16\(params, grad, m, v\)", 1),
    (r"n >= STREAM_MIN_N && aligned16\(dst, src\)", 1),
    (r"if \(per > 12\)", 1),                                  # clip_adam: grid pair beyond 12 k parameters
    (r"aligned && per > 4 && per <= 32", 1),                  # clip_adam_vec_kernel for aligned 4 k .. 12 k
    (r"if \(per <= 8\) LAUNCH_CAV\(2\);", 1),
    (r"else if \(per <= 16\) LAUNCH_CAV\(4\);", 1),
    (r"if \(per <= 4\) LAUNCH_CA\(4\);", 1),                  # clip_adam_kernel<4> / <16> (unaligned) below
    (r"else if \(per <= 16\) LAUNCH_CA\(16\);", 1),
    (r"& 15\) == 0\)", 2),                                    # the 16-byte alignment tests (aligned16 and clip_adam's)
    (r"const int nb = grid_for\(n, 256, 256\);", 1),         # clip_adam grid pair: <= 256 workgroups, grid-stride beyond
    (r"int nb = grid_for\(n > 0 \? n : 1, 256, 1024\);", 1),  # clip_by_global_norm partials: <= 1024 workgroups
    (r"constexpr int DEPART_SLOTS = 64;", 1),                # the 65th stream has no departure counter
]


def test_optim_dispatch_thresholds_match_the_contract_matrix():
    src = open(SRC).read()
    moved = [(p, n, len(re.findall(p, src))) for p, n in PINNED if len(re.findall(p, src)) != n]
    assert not moved, (
        "a dispatch threshold of csrc/optim.hip changed -- update the size / alignment matrix of "
        f"tests/test_gpu_optimiser_contract.py so that every path is still reached, then this list: {moved}")
