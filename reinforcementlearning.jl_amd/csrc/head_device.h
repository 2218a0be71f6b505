// head_device.h -- what the forward kernels (heads.hip) and the pullbacks (heads_grad.hip) of the diagonal Gaussian heads share: the
// bound on the action dimension, the reference's clamp and NNlib's softplus.
#pragma once
#include "ppo_sample_device.h"

namespace rlhip {

constexpr int HEAD_MAX_D = 64;

__device__ __forceinline__ float clampj(float x, float lo, float hi) { return x > hi ? hi : (x < lo ? lo : x); }
// NNlib.softplus (un-vendored): log1p(exp(-abs(x))) + relu(x)
__device__ __forceinline__ float softplus_nnlib(float x) { return log1pf(expf(-fabsf(x))) + (x > 0.0f ? x : 0.0f); }

// normal_draw(seed, id, step, q) and normal_draw(seed, id, step, q + 1) for an EVEN q: the two halves of one Philox block and one
// Box-Muller transform, the same Float64 operations as ppo_sample_device.h's normal_draw and therefore the same bits
__device__ __forceinline__ void normal_draw_pair(uint64_t seed, uint32_t id, uint32_t step, int q, float& even, float& odd) {
    u32x4 w = philox4x32_10(seed, id, (uint32_t)(q >> 1), step, TAG_NORMAL);
    double u1 = (double)((w.x >> 8) + 1u) * 0x1p-24;
    double u2 = (double)(w.y >> 8) * 0x1p-24;
    double r = ::sqrt(-2.0 * ::log(u1));
    double a = 6.283185307179586 * u2;
    even = (float)(r * ::cos(a));
    odd = (float)(r * ::sin(a));
}

}  // namespace rlhip
