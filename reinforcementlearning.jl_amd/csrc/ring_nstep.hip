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
#include "common.h"
#include "fold_device.h"

namespace rlhip {

struct NstepRing {  // the ring as the kernels see it (RingView of ring.hip plus the length the window must not pass)
    int64_t capacity, n_env, obs_dim, head_sa, head_rt, len_rt;
    const void* state;
    const int32_t* action;
    const float* reward;
    const uint8_t* terminal;
};

struct NstepOut {
    int32_t* a;
    float* ret;
    uint8_t* term;
    int32_t* n_used;  // nullable
};

constexpr int NSTEP_TILE = 256;      // samples per workgroup of the small route
constexpr int NSTEP_MAX_STACK = 8;   // rlhip_ring_gather_stacked's bound

// Lanes k < n_step of ONE wavefront (called by all 64 lanes, uniform control flow): reward / terminal of step li + k in one round
// trip, rewards to l_rew[k].  Returns ns in every lane; `tlast` = the flag of step li + ns - 1 (every lane).
__device__ __forceinline__ int window_wave(const NstepRing& rb, int64_t li, int n_step, float* l_rew, uint32_t& tlast) {
    const int k = (int)threadIdx.x & 63;
    const bool stored = k < n_step && li + k < rb.len_rt;  // a window never reads past the newest stored transition
    float r = 0.0f;
    uint32_t t = 0u;
    if (stored) {
        const int64_t pt = (rb.head_rt + li + k) % rb.capacity;
        r = rb.reward[pt];
        t = rb.terminal[pt];
    }
    if (k < n_step) l_rew[k] = r;
    const bool last = k == n_step - 1 || li + k + 1 >= rb.len_rt;
    const unsigned long long ends = __ballot(k < n_step && (t != 0u || last));  // never empty: lane n_step - 1 is in it
    const int ns = __ffsll(ends);                                               // first lane that ends the window, plus one
    tlast = (__ballot(t != 0u) >> (ns - 1)) & 1ull ? 1u : 0u;
    return ns;
}

// gain = r[k] + gamma * gain from the window's end: one lane, this order (the contract of the return; no tree reduction)
__device__ __forceinline__ float fold_rewards(const float* l_rew, int ns, float gamma) {
    float gain = 0.0f;
    for (int k = ns - 1; k >= 0; --k) gain = l_rew[k] + gamma * gain;
    return gain;
}

// small observations, component-major output: the index tile is staged in LDS as in gather_small_kernel; the lane that stages
// sample b also walks its window (each further step one dependent read, issued only once the step before is known not to be
// terminal) with the rewards in its own LDS column l_rew[.][lane] -- consecutive dwords per step, no barrier needed for them.
template <typename E>
__global__ __launch_bounds__(NSTEP_TILE) void gather_small_nstep_kernel(NstepRing rb, const int64_t* __restrict__ idx, int64_t batch,
                                                                        int n_step, float gamma, E* __restrict__ s, NstepOut o,
                                                                        E* __restrict__ sn) {
    __shared__ int64_t l_ps[NSTEP_TILE], l_pn[NSTEP_TILE];
    __shared__ float l_rew[FOLD_MAX_NSTEP][NSTEP_TILE];
    const int64_t b0 = (int64_t)blockIdx.x * NSTEP_TILE;
    const int tile = (int)((batch - b0 < NSTEP_TILE) ? (batch - b0) : NSTEP_TILE);
    const int tid = threadIdx.x;
    if (tid < tile) {
        const int64_t j = idx[b0 + tid];
        const int64_t li = j / rb.n_env, e = j - li * rb.n_env;
        int64_t at = ((rb.head_rt + li) % rb.capacity) * rb.n_env + e;
        o.a[b0 + tid] = rb.action[at];
        l_rew[0][tid] = rb.reward[at];
        uint32_t term = rb.terminal[at];
        int ns = 1;
        for (int k = 1; k < n_step && !term && li + k < rb.len_rt; ++k) {
            at = ((rb.head_rt + li + k) % rb.capacity) * rb.n_env + e;
            l_rew[k][tid] = rb.reward[at];
            term = rb.terminal[at];
            ns = k + 1;
        }
        float gain = 0.0f;
        for (int k = ns - 1; k >= 0; --k) gain = l_rew[k][tid] + gamma * gain;
        o.ret[b0 + tid] = gain;
        o.term[b0 + tid] = term ? 1 : 0;
        if (o.n_used) o.n_used[b0 + tid] = ns;
        l_ps[tid] = ((rb.head_sa + li) % (rb.capacity + 1)) * rb.obs_dim * rb.n_env + e;
        l_pn[tid] = ((rb.head_sa + li + ns) % (rb.capacity + 1)) * rb.obs_dim * rb.n_env + e;
    }
    __syncthreads();
    const E* st = (const E*)rb.state;
    const int64_t work = (int64_t)tile * rb.obs_dim;
    for (int64_t w = tid; w < work; w += NSTEP_TILE) {
        const int64_t k = w / tile;
        const int bl = (int)(w - k * tile);  // consecutive lanes -> consecutive samples: coalesced writes
        s[k * batch + b0 + bl] = st[l_ps[bl] + k * rb.n_env];
        sn[k * batch + b0 + bl] = st[l_pn[bl] + k * rb.n_env];
    }
}

// large contiguous frames (n_env == 1): one workgroup per sample, frame-major output
__global__ __launch_bounds__(256) void gather_frames_nstep_kernel(NstepRing rb, const int64_t* __restrict__ idx, int64_t frame_bytes,
                                                                  int n_step, float gamma, uint8_t* __restrict__ s, NstepOut o,
                                                                  uint8_t* __restrict__ sn) {
    __shared__ float l_rew[FOLD_MAX_NSTEP];
    __shared__ int64_t l_next[2];  // byte offset of frame li + ns; ns
    const int64_t b = blockIdx.x;
    const int64_t li = idx[b];  // (uniform: every wave computes the state frame's address itself)
    const int tid = threadIdx.x;
    const int64_t n16 = frame_bytes / 16;
    const uint4* src0 = (const uint4*)((const uint8_t*)rb.state + ((rb.head_sa + li) % (rb.capacity + 1)) * frame_bytes);
    constexpr int U = 2;  // chunk pairs in flight per thread and trip, as in gather_frames_kernel
    nt_u32x4 x[U], y[U];
    if (tid < 64) {  // (uniform per wave) the window: one scalar round trip, in flight together with the state chunks below
        int32_t a0 = 0;
        if (tid == 0) a0 = rb.action[(rb.head_rt + li) % rb.capacity];
        uint32_t tlast;
        const int ns = window_wave(rb, li, n_step, l_rew, tlast);
        if (tid == 0) {
            l_next[0] = ((rb.head_sa + li + ns) % (rb.capacity + 1)) * frame_bytes;
            l_next[1] = ns;
            o.a[b] = a0;
            o.term[b] = (uint8_t)tlast;
            if (o.n_used) o.n_used[b] = ns;
        }
    }
#pragma unroll
    for (int u = 0; u < U; ++u)
        if (tid + 256 * u < n16) x[u] = nt_load16(src0 + tid + 256 * u);
    __syncthreads();
    const uint4* src1 = (const uint4*)((const uint8_t*)rb.state + l_next[0]);
    uint4* d0 = (uint4*)(s + b * frame_bytes);
    uint4* d1 = (uint4*)(sn + b * frame_bytes);
    for (int64_t i0 = tid; i0 < n16; i0 += 256 * U) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t i = i0 + 256 * u;
            if (i < n16) {
                if (i0 != tid) x[u] = nt_load16(src0 + i);  // (the first trip's are in flight since before the barrier)
                y[u] = nt_load16(src1 + i);
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t i = i0 + 256 * u;
            if (i < n16) {  // ordinary stores: the outputs are pure write streams (profiles/r03_store_policy.md)
                *reinterpret_cast<nt_u32x4*>(d0 + i) = x[u];
                *reinterpret_cast<nt_u32x4*>(d1 + i) = y[u];
            }
        }
    }
    if (tid == 0) o.ret[b] = fold_rewards(l_rew, (int)l_next[1], gamma);  // behind the copies: nothing waits for it
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
    const int64_t li = idx[b];
    const int tid = threadIdx.x;
    if (tid < 64) {  // (uniform per wave) window flags on lanes 0 .. n_step - 1, history flags on lanes 32 .. 32 + n_stack - 2: one round trip
        int32_t a0 = 0;
        if (tid == 0) a0 = rb.action[(rb.head_rt + li) % rb.capacity];
        // going back from frame li: bit i - 1 = "transition li - i is terminal, or frame li - i does not exist"
        const int i = tid - 31;
        bool bound = false;
        if (i >= 1 && i < n_stack) bound = li - i < 0 || rb.terminal[(rb.head_rt + li - i) % rb.capacity] != 0;
        uint32_t tlast;
        const int ns = window_wave(rb, li, n_step, l_rew, tlast);
        const unsigned long long hist = __ballot(bound) >> 32;
        // ... and back from frame li + ns: the window's last step, its ns - 1 non-terminal steps, then the history
        const unsigned long long nhist = (unsigned long long)tlast | (hist << ns);
        const int m = ns < n_stack ? ns : n_stack, nf = n_stack + m;
        if (tid < nf) {
            const int64_t f = tid < n_stack ? li - n_stack + 1 + tid : li + ns - m + 1 + (tid - n_stack);
            const int ks = tid < n_stack ? tid : -1;
            const int kn = (int)(f - (li + ns - n_stack + 1));  // < 0: older than the next stack
            const int back_s = n_stack - 1 - ks, back_n = n_stack - 1 - kn;
            const bool vs = ks >= 0 && (hist & ((1ull << back_s) - 1)) == 0;
            const bool vn = kn >= 0 && (nhist & ((1ull << back_n) - 1)) == 0;
            l_off[tid] = f >= 0 ? ((rb.head_sa + f) % (rb.capacity + 1)) * frame_bytes : 0;
            l_ks[tid] = ks < 0 ? -1 : (vs ? ks : ks | 16);
            l_kn[tid] = kn < 0 ? -1 : (vn ? kn : kn | 16);
        }
        if (tid == 0) {
            l_off[2 * NSTEP_MAX_STACK] = ns;
            o.a[b] = a0;
            o.term[b] = (uint8_t)tlast;
            if (o.n_used) o.n_used[b] = ns;
        }
    }
    __syncthreads();
    const int ns = (int)l_off[2 * NSTEP_MAX_STACK];
    const uint32_t n16 = (uint32_t)(frame_bytes / 16);
    const uint32_t total = n16 * (uint32_t)(n_stack + (ns < n_stack ? ns : n_stack));
    const nt_u32x4 zero = {0u, 0u, 0u, 0u};
    uint8_t* ds = s + b * n_stack * frame_bytes;
    uint8_t* dn = sn + b * n_stack * frame_bytes;
    // the flat (frame, chunk) space of gather_stacked_kernel: every trip but the last is full.  Each source chunk is read once
    // (non-temporal) and written with ordinary stores to the stack(s) it belongs to.
    for (uint32_t q = tid; q < total; q += 256) {
        const uint32_t j = q / n16, i = q - j * n16;
        const int ks = l_ks[j], kn = l_kn[j];
        nt_u32x4 v = zero;
        if ((ks >= 0 && ks < 16) || (kn >= 0 && kn < 16)) v = nt_load16((const uint4*)((const uint8_t*)rb.state + l_off[j]) + i);
        if (ks >= 0) *reinterpret_cast<nt_u32x4*>((uint4*)(ds + (int64_t)(ks & 15) * frame_bytes) + i) = ks < 16 ? v : zero;
        if (kn >= 0) *reinterpret_cast<nt_u32x4*>((uint4*)(dn + (int64_t)(kn & 15) * frame_bytes) + i) = kn < 16 ? v : zero;
    }
    if (tid == 0) o.ret[b] = fold_rewards(l_rew, ns, gamma);
}

static NstepRing nstep_view(const rlhip_ring* rb) {
    return {rb->capacity, rb->n_env, rb->obs_dim, rb->head_sa, rb->head_rt, rb->len_rt, rb->state, rb->action, rb->reward, rb->terminal};
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
