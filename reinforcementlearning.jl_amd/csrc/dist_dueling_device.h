// dist_dueling_device.h -- the dueling combine of a distributional head, written once: the parameter-domain folds of csrc/dist_dueling.hip,
// the fused noisy folds and the output-domain combine of the per-env plan kernel (csrc/noisy.hip) all call these three functions.
// include/rlhip.h (the dueling distributional section) states the lines; the order is csrc/dueling.hip's, so a numpy Float32
// restatement is bit-exact (-ffp-contract=off is the build contract).
#pragma once
#include "mlp_device.h"  // MAXO

namespace rlhip {

// x[0 .. na) -> the left-folded sum ((x0 + x1) + x2) + x3
__device__ __forceinline__ float dist_duel_sum(const float x[MAXO], int na) {
    float s = x[0];
#pragma unroll
    for (int o = 1; o < MAXO; ++o)
        if (o < na) s = s + x[o];
    return s;
}

// the advantage values x[o] of one atom and its value v -> x[o] = (v + x[o]) - mean, mean = s / (float)na (a true division)
__device__ __forceinline__ void dist_duel_combine(float v, float x[MAXO], int na) {
    const float mean = dist_duel_sum(x, na) / (float)na;
#pragma unroll
    for (int o = 0; o < MAXO; ++o)
        if (o < na) x[o] = (v + x[o]) - mean;
}

// the chain rule of the combine: the gradients x[o] of one atom's effective values -> x[o] = x[o] - s / (float)na, returns s (the
// value row's gradient)
__device__ __forceinline__ float dist_duel_uncombine(float x[MAXO], int na) {
    const float s = dist_duel_sum(x, na);
    const float mean = s / (float)na;
#pragma unroll
    for (int o = 0; o < MAXO; ++o)
        if (o < na) x[o] = x[o] - mean;
    return s;
}

// the bounds of a dueling distributional net, stated once (dist_host.h: a list of bounds hands each one to B); K_MIN is the learner's
// (1 for quantiles, 2 for atoms)
#define DIST_DUEL_BOUNDS(B, K_MIN)                                                                                   \
    B(ns >= 2 && ns <= 16, "obs dim must be 2..16");                                                                 \
    B(h >= 4 && h <= DIST_HMAX && h % 4 == 0, "hidden must be a multiple of 4, <= 256");                             \
    B(na >= 1 && na <= MAXO, "na must be 1..4");                                                                     \
    B(K >= (K_MIN) && K <= DIST_MAXK, "atoms / quantiles per action beyond the learner's range (at most 64)");       \
    B((1 + na) * K <= DIST_MAXM, "a dueling distributional head has at most 256 rows: (1 + na) * K <= 256")

}  // namespace rlhip
