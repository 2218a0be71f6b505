// per_frames_nstep.hip -- prioritized n-step replay on FRAME rings (UInt8 images, Float32 observations wider than four components):
// the prioritized draw (rlhip_ring_sample_prioritized) and the n-step gather of its batch (rlhip_ring_gather_nstep /
// rlhip_ring_gather_stacked_nstep, ring_nstep.hip) in ONE launch, for every route the gathers take.  What rlhip_per_sample_fold_nstep_f32
// (per_nstep.hip) is for record rings; the mask that makes every drawn start a complete window is the tree's
// (rlhip_ring_push_priority_nstep_frames, per_nstep.hip) and this file neither knows nor needs it.
//   sample_gather_small_nstep_kernel<E>    the lane that stages sample b draws it (sumtree_draw: the sampler's own), then walks its window
//   sample_gather_frames_nstep_kernel      wave 0 draws with a four-levels-per-round-trip descent and publishes the start index; behind
//                                          that barrier the launch is gather_frames_nstep_kernel's body: every wave requests its first
//                                          trip of state chunks while wave 0 fetches the window, a second barrier publishes frame
//                                          li + ns (TWO barriers; the one-barrier schedule, draw + window before a single barrier and no
//                                          prefetch overlap, is profiles/attic/per_frames_nstep_one_barrier.patch; measurements of both:
//                                          profiles/per_frames_nstep.md)
//   sample_gather_stacked_nstep_kernel     wave 0 draws and goes on to the source table it alone builds: the one barrier of
//                                          gather_stacked_nstep_kernel stays the only one.  Launched for batches up to
//                                          STACKED_FUSED_MAX_BATCH; larger ones are served by the two launches (same bytes), because
//                                          there the fused form measured slower
// The gather bodies are ring_nstep_device.h's, shared with ring_nstep.hip, so the batch is that of the two launches by construction;
// idx / key / priority are those of sumtree_sample_kernel<true> (same Philox word, same comparisons on the same values in the same
// order: tests/test_gpu_per_frames_nstep.py holds both byte for byte).
//
// Memory safety: a drawn key is clamped below capacity * n_env, so 0 <= li < capacity and 0 <= e < n_env for ANY tree contents, which
// is the precondition under which the bodies stay inside the ring's allocations (ring_nstep_device.h); every tree read is at a heap
// position below 2 P; the child pairs are read as 8-byte loads, so the tree must be 8-byte aligned (refused otherwise; what
// rlhip_sumtree_nodes sizes and any device allocator returns is).  A leaf outside the logical range (li >= length: only a tree that
// was not written by the push ABI holds mass there) gives a one-step window.  No atomics, no spin-waits, nothing crosses a workgroup, no Float64, no dynamically indexed
// register array.
#include "ring_device.h"
#include "ring_nstep_device.h"
#include "sumtree_device.h"

namespace rlhip {

struct TreeDraw {
    const float* tree;
    int64_t P, n_leaves;
    int levels;  // log2(P): levels below the root
    uint64_t seed;
    uint32_t draw_ctr;
    int64_t* idx_out;
    int64_t* key_out;  // nullable
    float* prio_out;   // nullable
};

// leaf key -> flat logical start index (the convention of rlhip_ring_gather), as sumtree_sample_kernel<true> maps it
__device__ __forceinline__ int64_t key_to_flat(const NstepRing& rb, int64_t leaf) {
    int64_t pt, e;
    ring_split_index(leaf, rb.n_env, pt, e);
    int64_t li = pt - rb.head_rt;
    if (li < 0) li += rb.capacity;
    return li * rb.n_env + e;
}

// what one lane writes behind the draw of sample b -> the flat start index
__device__ __forceinline__ int64_t draw_publish(const TreeDraw& d, const NstepRing& rb, int64_t b, int64_t leaf) {
    if (d.key_out) d.key_out[b] = leaf;
    if (d.prio_out) d.prio_out[b] = d.tree[d.P + leaf];
    const int64_t flat = key_to_flat(rb, leaf);
    d.idx_out[b] = flat;
    return flat;
}

// a value every lane of the wavefront holds, moved to scalar registers (the ring arithmetic behind it then runs once per wave)
__device__ __forceinline__ int64_t wave_uniform(int64_t x) {
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)x), hi = __builtin_amdgcn_readfirstlane((uint32_t)((uint64_t)x >> 32));
    return (int64_t)(((uint64_t)hi << 32) | lo);
}

// sumtree_draw by a whole wavefront (all 64 lanes, uniform control flow), FOUR tree levels per memory round trip: lanes 0 .. 14
// request the 15 child pairs of the depth-4 subtree below the current node at once (the pair of relative node i on sub-level a sits
// in lane 2^a - 1 + i), then the four decisions of sumtree_descend are taken from those registers -- the same comparisons on the same
// values in the same order, hence the same leaf; the last trip takes the levels that remain (d.levels is no multiple of four for most
// rings).  The cooperative descent of ring.hip's fused 1-step launch, restated over plain loads: nothing in this launch writes the
// tree.  Returns the clamped leaf key in every lane.
__device__ __forceinline__ int64_t draw_wave(const TreeDraw& d, int64_t b) {
    const int lane = (int)threadIdx.x & 63;
    const u32x4 w = philox4x32_10(d.seed, (uint32_t)b, 0, d.draw_ctr, TAG_SAMPLER);
    float v = u01_f32(w.z) * d.tree[1];
    int64_t node = 1;
    for (int rem = d.levels; rem > 0;) {
        const int L = rem < 4 ? rem : 4;
        float cx = 0.0f, cy = 0.0f;
        if (lane < (1 << L) - 1) {
            const int a = 31 - __clz(lane + 1), i = lane + 1 - (1 << a);
            const float2 c = *reinterpret_cast<const float2*>(d.tree + 2 * ((node << a) + i));
            cx = c.x;
            cy = c.y;
        }
        int i = 0;
        for (int a = 0; a < L; ++a) {
            const int src = (1 << a) - 1 + i;
            const float lx = __shfl(cx, src, 64), ly = __shfl(cy, src, 64);
            const bool right = (v > lx && ly > 0.0f) || lx == 0.0f;
            if (right) v -= lx;
            i = 2 * i + (right ? 1 : 0);
        }
        node = (node << L) + i;
        rem -= L;
    }
    const int64_t leaf = node - d.P;
    return wave_uniform(leaf < d.n_leaves ? leaf : d.n_leaves - 1);  // (the clamp: a rounding walk into the zero padding of the last level)
}

template <typename E>
__global__ __launch_bounds__(NSTEP_TILE) void sample_gather_small_nstep_kernel(NstepRing rb, TreeDraw d, int64_t batch, int n_step,
                                                                               float gamma, E* __restrict__ s, NstepOut o,
                                                                               E* __restrict__ sn) {
    __shared__ int64_t l_ps[NSTEP_TILE], l_pn[NSTEP_TILE];
    __shared__ float l_rew[FOLD_MAX_NSTEP][NSTEP_TILE];
    const int64_t b0 = (int64_t)blockIdx.x * NSTEP_TILE;
    const int tile = (int)((batch - b0 < NSTEP_TILE) ? (batch - b0) : NSTEP_TILE);
    const int tid = threadIdx.x;
    if (tid < tile) {
        const int64_t b = b0 + tid;
        const int64_t j = draw_publish(d, rb, b, sumtree_draw(d.tree, d.P, d.n_leaves, d.seed, b, d.draw_ctr));
        gather_small_nstep_stage(rb, j, b, tid, n_step, gamma, o, l_ps, l_pn, l_rew);
    }
    __syncthreads();
    gather_small_nstep_copy<E>(rb, batch, b0, tile, tid, l_ps, l_pn, s, sn);
}

__global__ __launch_bounds__(256) void sample_gather_frames_nstep_kernel(NstepRing rb, TreeDraw d, int64_t frame_bytes, int n_step,
                                                                         float gamma, uint8_t* __restrict__ s, NstepOut o,
                                                                         uint8_t* __restrict__ sn) {
    __shared__ float l_rew[FOLD_MAX_NSTEP];
    __shared__ int64_t l_next[2];  // byte offset of frame li + ns; ns
    __shared__ int64_t l_li[1];    // the drawn start index
    const int64_t b = blockIdx.x;
    if (threadIdx.x < 64) {  // (uniform per wave)
        const int64_t leaf = draw_wave(d, b);
        if (threadIdx.x == 0) l_li[0] = draw_publish(d, rb, b, leaf);  // (n_env == 1 on this route: the flat index is li)
    }
    __syncthreads();
    gather_frames_nstep_body(rb, wave_uniform(l_li[0]), b, frame_bytes, n_step, gamma, s, o, sn, l_rew, l_next);
}

__global__ __launch_bounds__(256) void sample_gather_stacked_nstep_kernel(NstepRing rb, TreeDraw d, int64_t frame_bytes, int n_stack,
                                                                          int n_step, float gamma, uint8_t* __restrict__ s, NstepOut o,
                                                                          uint8_t* __restrict__ sn) {
    __shared__ float l_rew[FOLD_MAX_NSTEP];
    __shared__ int64_t l_off[2 * NSTEP_MAX_STACK + 2];  // byte offset per source frame; [16] = ns ([17] keeps the size a multiple of 16)
    __shared__ int l_ks[2 * NSTEP_MAX_STACK], l_kn[2 * NSTEP_MAX_STACK];  // member of the state / next stack: -1 none, k data, k | 16 zeros
    const int64_t b = blockIdx.x;
    int64_t li = 0;  // only wave 0 uses it: the body reads the index before its barrier alone
    if (threadIdx.x < 64) {
        const int64_t leaf = draw_wave(d, b);
        li = key_to_flat(rb, leaf);  // (n_env == 1)
        if (threadIdx.x == 0) draw_publish(d, rb, b, leaf);
    }
    gather_stacked_nstep_body(rb, li, b, frame_bytes, n_stack, n_step, gamma, s, o, sn, l_rew, l_off, l_ks, l_kn);
}

// The stacked route is fused up to this batch size and served by its two launches beyond it.  A stacked workgroup copies up to
// 2 n_stack frames behind its draw and nothing of it overlaps the descent; once one launch fills every workgroup slot of the device
// (256 CUs x 8 workgroups = 2048) the workgroups run in lockstep and the descent's round trips are exposed instead of hidden behind
// the copies of their neighbours (an explanation read off the kernel, not measured further).  Measured for ONE shape only
// (profiles/per_frames_nstep.md: n_stack 4, n_step 3, 7056-byte frames, 256 CUs): fused / two launches 0.85 - 0.87 for batch
// 32 .. 1536, 1.16 at 2048, 0.94 at 3072, 1.10 at 4096.  1536 is the largest size measured to win at n_stack 4; n_stack 1 and 8,
// where the ratio of copy to descent differs most, were not timed and take the same rule.
constexpr int64_t STACKED_FUSED_MAX_BATCH = 1536;

}  // namespace rlhip

using namespace rlhip;

// the union of what rlhip_ring_sample_prioritized and the two n-step gathers refuse, plus the draw's own pointers; the ring's
// counters are checked because every address of the launch is formed from them and from a key nobody else validates
#define RLHIP_PFN_REQUIRE_COMMON(rb, tree, batch, n_step, idx_out, s, a, ret, term, s_next)                                              \
    RLHIP_REQUIRE(rb && tree && idx_out && s && a && ret && term && s_next && batch >= 0, "bad arguments");                              \
    RLHIP_REQUIRE(((uintptr_t)tree & 7) == 0, "the tree must be 8-byte aligned (its child pairs are read as one 8-byte load)");          \
    RLHIP_REQUIRE(n_step >= 1 && n_step <= FOLD_MAX_NSTEP, "n_step must be in 1..32");                                                    \
    RLHIP_REQUIRE(rb->layout == RLHIP_RING_FRAMES,                                                                                        \
                  "the prioritized n-step gathers serve frame rings; a record ring (Float32 observations, obs_dim <= 4) draws and "      \
                  "folds its windows with rlhip_per_sample_fold_nstep_f32");                                                             \
    RLHIP_REQUIRE(rb->len_rt >= 1, "cannot sample from an empty trajectory");                                                            \
    RLHIP_REQUIRE(rb->capacity >= 1 && rb->n_env >= 1 && rb->len_rt <= rb->capacity && rb->head_sa >= 0 && rb->head_sa <= rb->capacity && \
                      rb->head_rt >= 0 && rb->head_rt < rb->capacity,                                                                    \
                  "ring counters out of range")

static TreeDraw tree_draw(const rlhip_ring* rb, const float* tree, uint64_t seed, uint32_t draw_ctr, int64_t* idx_out, int64_t* key_out,
                          float* prio_out) {
    TreeDraw d;
    d.tree = tree;
    d.n_leaves = rb->capacity * rb->n_env;
    d.P = pow2_ge(d.n_leaves);
    d.levels = 0;
    for (int64_t t = 1; t < d.P; t <<= 1) ++d.levels;
    d.seed = seed;
    d.draw_ctr = draw_ctr;
    d.idx_out = idx_out;
    d.key_out = key_out;
    d.prio_out = prio_out;
    return d;
}

extern "C" int32_t rlhip_ring_sample_gather_nstep_prioritized(const rlhip_ring* rb, const float* tree, int64_t batch, int32_t n_step,
                                                              float gamma, uint64_t seed, uint32_t draw_ctr, int64_t* idx_out,
                                                              int64_t* key_out, float* prio_out, void* s, int32_t* a, float* ret,
                                                              uint8_t* term, void* s_next, int32_t* n_used, rlhip_stream_t stream) {
    RLHIP_PFN_REQUIRE_COMMON(rb, tree, batch, n_step, idx_out, s, a, ret, term, s_next);
    const bool big = rlhip_ring_gather_is_frame_major(rb) != 0;
    if (big)
        RLHIP_REQUIRE(((((uintptr_t)rb->state | (uintptr_t)s | (uintptr_t)s_next) & 15) == 0),
                      "frame-major gather needs 16-byte aligned buffers");
    if (batch == 0) return RLHIP_OK;
    // (nothing for the bounds-checked build to validate: the indices are the launch's own)
    hipStream_t st = as_stream(stream);
    const NstepRing v = nstep_view(rb);
    const TreeDraw d = tree_draw(rb, tree, seed, draw_ctr, idx_out, key_out, prio_out);
    const NstepOut o = {a, ret, term, n_used};
    const int64_t groups = big ? batch : (batch + NSTEP_TILE - 1) / NSTEP_TILE;
    RLHIP_REQUIRE(groups <= INT32_MAX, "batch too large");
    if (big)
        hipLaunchKernelGGL(sample_gather_frames_nstep_kernel, dim3((int)groups), dim3(256), 0, st, v, d, rb->obs_dim * (int64_t)rb->elem_bytes,
                           (int)n_step, gamma, (uint8_t*)s, o, (uint8_t*)s_next);
    else if (rb->elem_bytes == 4)
        hipLaunchKernelGGL((sample_gather_small_nstep_kernel<float>), dim3((int)groups), dim3(NSTEP_TILE), 0, st, v, d, batch, (int)n_step,
                           gamma, (float*)s, o, (float*)s_next);
    else
        hipLaunchKernelGGL((sample_gather_small_nstep_kernel<uint8_t>), dim3((int)groups), dim3(NSTEP_TILE), 0, st, v, d, batch, (int)n_step,
                           gamma, (uint8_t*)s, o, (uint8_t*)s_next);
    RLHIP_LAUNCH_CHECK();
    return RLHIP_OK;
}

extern "C" int32_t rlhip_ring_sample_gather_stacked_nstep_prioritized(const rlhip_ring* rb, const float* tree, int64_t batch,
                                                                      int32_t n_stack, int32_t n_step, float gamma, uint64_t seed,
                                                                      uint32_t draw_ctr, int64_t* idx_out, int64_t* key_out,
                                                                      float* prio_out, void* s, int32_t* a, float* ret, uint8_t* term,
                                                                      void* s_next, int32_t* n_used, rlhip_stream_t stream) {
    RLHIP_PFN_REQUIRE_COMMON(rb, tree, batch, n_step, idx_out, s, a, ret, term, s_next);
    RLHIP_REQUIRE(n_stack >= 1 && n_stack <= NSTEP_MAX_STACK, "n_stack must be in 1..8");
    RLHIP_REQUIRE(rb->n_env == 1, "stack-at-sample gather is defined for single-env frame rings");
    const int64_t frame_bytes = rb->obs_dim * (int64_t)rb->elem_bytes;
    RLHIP_REQUIRE(frame_bytes % 16 == 0, "frame size must be a multiple of 16 bytes");
    RLHIP_REQUIRE(((((uintptr_t)rb->state | (uintptr_t)s | (uintptr_t)s_next) & 15) == 0), "buffers must be 16-byte aligned");
    if (batch == 0) return RLHIP_OK;
    RLHIP_REQUIRE(batch <= INT32_MAX, "batch too large");
    if (batch > STACKED_FUSED_MAX_BATCH) {  // the two launches this call stands for: same bytes (see STACKED_FUSED_MAX_BATCH)
        const int32_t rc = rlhip_ring_sample_prioritized(rb, tree, batch, seed, draw_ctr, idx_out, key_out, prio_out, stream);
        if (rc) return rc;
        return rlhip_ring_gather_stacked_nstep(rb, idx_out, batch, n_stack, n_step, gamma, s, a, ret, term, s_next, n_used, stream);
    }
    hipLaunchKernelGGL(sample_gather_stacked_nstep_kernel, dim3((int)batch), dim3(256), 0, as_stream(stream), nstep_view(rb),
                       tree_draw(rb, tree, seed, draw_ctr, idx_out, key_out, prio_out), frame_bytes, (int)n_stack, (int)n_step, gamma,
                       (uint8_t*)s, NstepOut{a, ret, term, n_used}, (uint8_t*)s_next);
    RLHIP_LAUNCH_CHECK();
    return RLHIP_OK;
}
