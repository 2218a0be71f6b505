// dist_host.h -- what the host side of the distributional learners' entry points shares, each written once: the shape bounds of the
// two mlp2 learners, the number of workgroups (= partial rows) of a gradient launch, and the launches of dist.hip.  Host code only.
#pragma once
#include "common.h"
#include "dist_device.h"

namespace rlhip {

// A list of bounds is a macro that hands each (condition, message) to B, so a learner states its bounds once: with B = RLHIP_REQUIRE
// the entry points fail on the first bound that does not hold, with its message and its condition; with B = DIST_BOUND_HOLDS a
// bool function returns false on it and sets no error (rlhip_*_workspace_bytes returns -1 then).
#define DIST_BOUND_HOLDS(cond, msg) \
    if (!(cond)) return false

// mlp2(ns, h, na * K) of the C51 and QR-DQN kernels; the learner's list adds K's bound
#define DIST_MLP2_BOUNDS(B)                                                              \
    B(ns >= 2 && ns <= 16, "obs dim must be 2..16");                                     \
    B(h >= 4 && h <= DIST_HMAX && h % 4 == 0, "hidden must be a multiple of 4, <= 256"); \
    B(na >= 1 && na <= MAXO, "na must be 1..4")

#define DIST_REQUIRE_ACT() RLHIP_REQUIRE(act == 0 || act == 1, "act must be 0 (relu) or 1 (tanh)")

// workgroups = partial rows of a gradient launch on tiles of `tile` samples: one per tile, at most 256 (one workgroup per CU; a larger
// batch gives its workgroups further tiles) and at most 16 MiB of rows (a row is up to 280 KB: 59 rows at the largest mlp2 shape)
static inline int64_t dist_num_blocks(int64_t np, int64_t batch, int64_t tile) {
    const int64_t tiles = (batch + tile - 1) / tile;
    int64_t cap = ((int64_t)16 << 20) / (np * (int64_t)sizeof(float));
    cap = cap < 1 ? 1 : (cap > 256 ? 256 : cap);
    return tiles < cap ? tiles : cap;
}

// ---- dist.hip
// grad[p] and loss[0] = (the partial rows / losses of workgroups 0 .. nb - 1 in ascending order, from +0) [/ fb]
int32_t dist_reduce_launch(const float* partials, const float* loss_partials, int64_t nb, int64_t np, float* grad, float* loss, float fb,
                           hipStream_t st);
// the debug build (RLHIP_BOUNDS_CHECK): an action outside 0 .. na - 1 is an error instead of a sample without a gradient; one int of
// `workspace` is the counter; the error names the caller's file and line.  Nothing in the default build.
int32_t dist_check_actions(const int32_t* a, int64_t batch, int64_t na, void* workspace, hipStream_t st, const char* file, int line);

}  // namespace rlhip
