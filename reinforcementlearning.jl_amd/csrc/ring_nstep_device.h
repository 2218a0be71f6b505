// ring_nstep_device.h -- the n-step gathers of a FRAME ring as device functions "from the start index on", shared by the launches
// that take the index from the caller (ring_nstep.hip) and by those that draw it from the sum-tree first (per_frames_nstep.hip).
// A body is everything its kernel does once the flat logical start index is known; the kernel owns the LDS arrays and says where
// the index comes from.  ring_nstep.hip's header has the design (window, return, source list of the stacked form, store policy).
//
// Memory safety for ANY start with 0 <= li < capacity, 0 <= e < n_env (a drawn index is not validated by anyone): the traces are
// read at (head_rt + li [+ k]) mod capacity and only for li + k < len_rt, the state at (head_sa + f) mod (capacity + 1) with
// 0 <= f <= li + ns <= capacity.  A start at or past len_rt reads no window step: ns = 1.
#pragma once
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

// ---- small observations, component-major output ----
// The lane that stages sample b0 + tid of its tile, from the flat start index j on: walks its window (each further step one
// dependent read, issued only once the step before is known not to be terminal) with the rewards in its own LDS column
// l_rew[.][tid] -- consecutive dwords per step, no barrier needed for them -- and leaves the two state offsets in l_ps / l_pn.
__device__ __forceinline__ void gather_small_nstep_stage(const NstepRing& rb, int64_t j, int64_t b, int tid, int n_step, float gamma,
                                                         const NstepOut& o, int64_t* l_ps, int64_t* l_pn,
                                                         float (*l_rew)[NSTEP_TILE]) {
    const int64_t li = j / rb.n_env, e = j - li * rb.n_env;
    int64_t at = ((rb.head_rt + li) % rb.capacity) * rb.n_env + e;
    o.a[b] = rb.action[at];
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
    o.ret[b] = gain;
    o.term[b] = term ? 1 : 0;
    if (o.n_used) o.n_used[b] = ns;
    l_ps[tid] = ((rb.head_sa + li) % (rb.capacity + 1)) * rb.obs_dim * rb.n_env + e;
    l_pn[tid] = ((rb.head_sa + li + ns) % (rb.capacity + 1)) * rb.obs_dim * rb.n_env + e;
}

// ... and the tile's two state blocks, behind the barrier that publishes l_ps / l_pn
template <typename E>
__device__ __forceinline__ void gather_small_nstep_copy(const NstepRing& rb, int64_t batch, int64_t b0, int tile, int tid,
                                                        const int64_t* l_ps, const int64_t* l_pn, E* __restrict__ s,
                                                        E* __restrict__ sn) {
    const E* st = (const E*)rb.state;
    const int64_t work = (int64_t)tile * rb.obs_dim;
    for (int64_t w = tid; w < work; w += NSTEP_TILE) {
        const int64_t k = w / tile;
        const int bl = (int)(w - k * tile);  // consecutive lanes -> consecutive samples: coalesced writes
        s[k * batch + b0 + bl] = st[l_ps[bl] + k * rb.n_env];
        sn[k * batch + b0 + bl] = st[l_pn[bl] + k * rb.n_env];
    }
}

// ---- large contiguous frames (n_env == 1): one workgroup per sample, frame-major output ----
// Called by the whole workgroup with the start index li uniform in it.  l_next: byte offset of frame li + ns; ns.
__device__ __forceinline__ void gather_frames_nstep_body(const NstepRing& rb, int64_t li, int64_t b, int64_t frame_bytes, int n_step,
                                                         float gamma, uint8_t* __restrict__ s, const NstepOut& o,
                                                         uint8_t* __restrict__ sn, float* l_rew, int64_t* l_next) {
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

// ---- stack-at-sample (n_env == 1): one workgroup per sample ----
// l_off: byte offset per source frame, [2 * NSTEP_MAX_STACK] = ns; l_ks / l_kn: member of the state / next stack per source frame,
// -1 none, k data, k | 16 zeros.
__device__ __forceinline__ void gather_stacked_nstep_body(const NstepRing& rb, int64_t li, int64_t b, int64_t frame_bytes, int n_stack,
                                                          int n_step, float gamma, uint8_t* __restrict__ s, const NstepOut& o,
                                                          uint8_t* __restrict__ sn, float* l_rew, int64_t* l_off, int* l_ks,
                                                          int* l_kn) {
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

static inline NstepRing nstep_view(const rlhip_ring* rb) {
    return {rb->capacity, rb->n_env, rb->obs_dim, rb->head_sa, rb->head_rt, rb->len_rt, rb->state, rb->action, rb->reward, rb->terminal};
}

}  // namespace rlhip
