// ring_nstep.hip -- n-step transitions gathered from FRAME rings (UInt8 images, Float32 observations wider than four components):
// the NStepBatchSampler of RLTrajectories 0.4 for the layouts that have no 64-byte records (record rings: rlhip_ring_fold_nstep,
// ring.hip).  One launch per batch, for every route the 1-step gathers of ring.hip take:
//   gather_small_nstep_kernel<E>    component-major SoA output, any n_env          (twin of gather_small_kernel<E>)
//   gather_frames_nstep_kernel      n_env == 1, frames >= 1 KB: frame-major output  (twin of gather_frames_kernel)
//   gather_stacked_nstep_kernel     stack-at-sample, n_env == 1                     (twin of gather_stacked_kernel)
//
// The window of start (li, e) is li .. li + ns - 1, ns = min(n_step, k + 1 of the first terminal step k, len_rt - li); the sample is
// {s = frame li, a[li], ret, term = terminal[li + ns - 1], s' = frame li + ns}, ret = discount_rewards_reduced over the window
// (gain = r[li + k] + gamma * gain from the window's end, Float32, no contraction, one lane: fold_window's order, fold_device.h).
// An n-step sample reads the same two frames as a 1-step sample; what it adds is ONE scalar round trip on the way to the second
// frame's address: lanes k < n_step of the first wavefront request reward / terminal of step li + k together, a 64-bit ballot of
// "the window ends here" gives ns, the rewards wait in LDS for the one lane that folds them.  The state frame does not depend on
// ns, so the frame-major kernel requests its first trip of state chunks BEFORE the barrier that publishes the next frame's offset.
// The small route keeps one lane per sample with an early-exit walk (its steps are strided by n_env: no shared line to fetch).
// Store policy as measured for the 1-step kernels: non-temporal 16-byte loads, ordinary stores.  All offsets are int64.
#include "ring_nstep_device.h"

namespace rlhip {

// The bodies "from the start index on" live in ring_nstep_device.h (shared with the prioritized launches of per_frames_nstep.hip);
// here the index comes from the caller's vector.

// small observations, component-major output: the index tile is staged in LDS as in gather_small_kernel; the lane that stages
// sample b also walks its window
template <typename E>
__global__ __launch_bounds__(NSTEP_TILE) void gather_small_nstep_kernel(NstepRing rb, const int64_t* __restrict__ idx, int64_t batch,
                                                                        int n_step, float gamma, E* __restrict__ s, NstepOut o,
                                                                        E* __restrict__ sn) {
    __shared__ int64_t l_ps[NSTEP_TILE], l_pn[NSTEP_TILE];
    __shared__ float l_rew[FOLD_MAX_NSTEP][NSTEP_TILE];
    const int64_t b0 = (int64_t)blockIdx.x * NSTEP_TILE;
    const int tile = (int)((batch - b0 < NSTEP_TILE) ? (batch - b0) : NSTEP_TILE);
    const int tid = threadIdx.x;
    if (tid < tile) gather_small_nstep_stage(rb, idx[b0 + tid], b0 + tid, tid, n_step, gamma, o, l_ps, l_pn, l_rew);
    __syncthreads();
    gather_small_nstep_copy<E>(rb, batch, b0, tile, tid, l_ps, l_pn, s, sn);
}

// large contiguous frames (n_env == 1): one workgroup per sample, frame-major output
__global__ __launch_bounds__(256) void gather_frames_nstep_kernel(NstepRing rb, const int64_t* __restrict__ idx, int64_t frame_bytes,
                                                                  int n_step, float gamma, uint8_t* __restrict__ s, NstepOut o,
                                                                  uint8_t* __restrict__ sn) {
    __shared__ float l_rew[FOLD_MAX_NSTEP];
    __shared__ int64_t l_next[2];  // byte offset of frame li + ns; ns
    const int64_t b = blockIdx.x;
    // (idx[b] is uniform: every wave computes the state frame's address itself)
    gather_frames_nstep_body(rb, idx[b], b, frame_bytes, n_step, gamma, s, o, sn, l_rew, l_next);
}

// stack-at-sample: state = stack(li), next state = stack(li + ns), stack(f) = frames f - n_stack + 1 .. f oldest first, a member
// all zeros when its frame index is negative or a terminal transition lies among the transitions from that frame up to f - 1 (the
// rule of gather_stacked_kernel).  The two stacks share n_stack - ns frames when ns < n_stack; the SOURCE list holds every frame of
// their union once -- the n_stack frames of the state stack, then the min(ns, n_stack) newest frames of the next stack -- and every
// member of either stack is written by exactly one source entry.
__global__ __launch_bounds__(256) void gather_stacked_nstep_kernel(NstepRing rb, const int64_t* __restrict__ idx, int64_t frame_bytes,
                                                                   int n_stack, int n_step, float gamma, uint8_t* __restrict__ s,
                                                                   NstepOut o, uint8_t* __restrict__ sn) {
    __shared__ float l_rew[FOLD_MAX_NSTEP];
    __shared__ int64_t l_off[2 * NSTEP_MAX_STACK + 2];  // byte offset per source frame; [16] = ns ([17] keeps the size a multiple of 16)
    __shared__ int l_ks[2 * NSTEP_MAX_STACK], l_kn[2 * NSTEP_MAX_STACK];  // member of the state / next stack: -1 none, k data, k | 16 zeros
    const int64_t b = blockIdx.x;
    gather_stacked_nstep_body(rb, idx[b], b, frame_bytes, n_stack, n_step, gamma, s, o, sn, l_rew, l_off, l_ks, l_kn);
}

}  // namespace rlhip

using namespace rlhip;

// what both entry points refuse before anything else
#define RLHIP_NSTEP_REQUIRE_COMMON(rb, idx, batch, n_step, s, a, ret, term, s_next)                                                      \
    RLHIP_REQUIRE(rb && idx && s && a && ret && term && s_next && batch >= 0, "bad arguments");                                          \
    RLHIP_REQUIRE(n_step >= 1 && n_step <= FOLD_MAX_NSTEP, "n_step must be in 1..32");                                                    \
    RLHIP_REQUIRE(rb->layout == RLHIP_RING_FRAMES,                                                                                        \
                  "the n-step gathers serve frame rings; a record ring (Float32 observations, obs_dim <= 4) folds its windows with "     \
                  "rlhip_ring_fold_nstep");                                                                                              \
    RLHIP_REQUIRE(rb->len_rt >= 1, "cannot sample from an empty trajectory")

extern "C" int32_t rlhip_ring_gather_nstep(const rlhip_ring* rb, const int64_t* idx, int64_t batch, int32_t n_step, float gamma, void* s,
                                           int32_t* a, float* ret, uint8_t* term, void* s_next, int32_t* n_used, rlhip_stream_t stream) {
    RLHIP_NSTEP_REQUIRE_COMMON(rb, idx, batch, n_step, s, a, ret, term, s_next);
    const bool big = rlhip_ring_gather_is_frame_major(rb) != 0;
    if (big)
        RLHIP_REQUIRE(((((uintptr_t)rb->state | (uintptr_t)s | (uintptr_t)s_next) & 15) == 0),
                      "frame-major gather needs 16-byte aligned buffers");
    if (batch == 0) return RLHIP_OK;
    RLHIP_CHECK_GATHER_INDICES(rb, idx, batch, stream);
    hipStream_t st = as_stream(stream);
    const NstepRing v = nstep_view(rb);
    const NstepOut o = {a, ret, term, n_used};
    if (big) {
        hipLaunchKernelGGL(gather_frames_nstep_kernel, dim3((int)batch), dim3(256), 0, st, v, idx, rb->obs_dim * (int64_t)rb->elem_bytes,
                           (int)n_step, gamma, (uint8_t*)s, o, (uint8_t*)s_next);
    } else {
        const dim3 grid((unsigned)((batch + NSTEP_TILE - 1) / NSTEP_TILE));
        if (rb->elem_bytes == 4)
            hipLaunchKernelGGL((gather_small_nstep_kernel<float>), grid, dim3(NSTEP_TILE), 0, st, v, idx, batch, (int)n_step, gamma,
                               (float*)s, o, (float*)s_next);
        else
            hipLaunchKernelGGL((gather_small_nstep_kernel<uint8_t>), grid, dim3(NSTEP_TILE), 0, st, v, idx, batch, (int)n_step, gamma,
                               (uint8_t*)s, o, (uint8_t*)s_next);
    }
    RLHIP_LAUNCH_CHECK();
    return RLHIP_OK;
}

extern "C" int32_t rlhip_ring_gather_stacked_nstep(const rlhip_ring* rb, const int64_t* idx, int64_t batch, int32_t n_stack, int32_t n_step,
                                                   float gamma, void* s, int32_t* a, float* ret, uint8_t* term, void* s_next,
                                                   int32_t* n_used, rlhip_stream_t stream) {
    RLHIP_NSTEP_REQUIRE_COMMON(rb, idx, batch, n_step, s, a, ret, term, s_next);
    RLHIP_REQUIRE(n_stack >= 1 && n_stack <= NSTEP_MAX_STACK, "n_stack must be in 1..8");
    RLHIP_REQUIRE(rb->n_env == 1, "stack-at-sample gather is defined for single-env frame rings");
    const int64_t frame_bytes = rb->obs_dim * (int64_t)rb->elem_bytes;
    RLHIP_REQUIRE(frame_bytes % 16 == 0, "frame size must be a multiple of 16 bytes");
    RLHIP_REQUIRE(((((uintptr_t)rb->state | (uintptr_t)s | (uintptr_t)s_next) & 15) == 0), "buffers must be 16-byte aligned");
    if (batch == 0) return RLHIP_OK;
    RLHIP_CHECK_GATHER_INDICES(rb, idx, batch, stream);
    hipLaunchKernelGGL(gather_stacked_nstep_kernel, dim3((int)batch), dim3(256), 0, as_stream(stream), nstep_view(rb), idx, frame_bytes,
                       (int)n_stack, (int)n_step, gamma, (uint8_t*)s, NstepOut{a, ret, term, n_used}, (uint8_t*)s_next);
    RLHIP_LAUNCH_CHECK();
    return RLHIP_OK;
}
