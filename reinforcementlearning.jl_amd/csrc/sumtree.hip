// sumtree.hip -- device-resident priority sum-tree for prioritized replay (BASELINE config 5:
// "1M-slot CircularArraySARTTraces ... prioritized sampling gather").
//
// Replaces, for rings that live in HBM:
//   CircularArrayBuffers.SumTree (compat 0.1.12, RLCore/Project.toml:30) -- `setindex!`, `get`, `rand(rng, t, n)`
//   ReinforcementLearningTrajectories 0.4 `CircularPrioritizedTraces` + the prioritized `BatchSampler` method
//   (`inds, priorities = rand(rng, sumtree, batchsize)`; `trajectory[:priority, keys] = p`)
// Both packages are un-vendored: PARITY UNPINNED, the published algorithm is restated.  Two
// deliberate differences, both documented in DESIGN.md:
//   * internal nodes are RE-COMPUTED as left + right from their children (one f32 add, fixed operand order)
//     instead of the reference's running `tree[parent] += change` delta walk: the tree is then a pure
//     function of the leaf values (no floating-point drift, no dependence on the update order), which is what
//     makes a parallel update bit-reproducible;
//   * the descent never enters a zero-sum subtree while the sibling has mass (the reference can return a
//     zero-priority leaf when u = 0 or on a rounding edge).
//
// Layout: implicit heap, float tree[2P], P = next power of two >= n_leaves; node 1 = root, children of i are
// 2i and 2i+1, leaf k lives at P + k (same positions as the reference's `nparents + k`, nparents = P - 1).
// Leaves are addressed by the PHYSICAL transition slot of the ring (slot * n_env + env), so a push overwrites
// the leaf of the transition it overwrites.  1M leaves = 8 MB: L2 / Infinity-Cache resident.
//
// Kernels (all HBM/L2-latency bound, tiny next to the frame gather they feed):
//   sumtree_level_kernel     one grid per level for bulk range fills (>= 2048 nodes on the level)
//   sumtree_range_kernel     one 1024-thread workgroup finishes the remaining levels of a contiguous range
//   sumtree_update_kernel    (sumtree_update.h) leaf writes with "last occurrence wins" for duplicate keys (the sequential reference
//                            semantics), then the ancestors: sparse levels split over workgroups by subtree, the
//                            top 13 levels recomputed whole in LDS by the last-arriving workgroup
//   sumtree_sample_kernel    one lane per draw, log2(P) dependent 8-byte loads
#include "common.h"
#include "sumtree_device.h"
#include "sumtree_update.h"

namespace rlhip {

__global__ __launch_bounds__(256) void sumtree_fill_leaves_kernel(float* __restrict__ tree, int64_t first,
                                                                  int64_t count, float value) {
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += stride) tree[first + i] = value;
}

__global__ __launch_bounds__(256) void sumtree_level_kernel(float* __restrict__ tree, int64_t lo, int64_t hi) {
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t node = lo + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; node <= hi; node += stride) {
        float2 c = *reinterpret_cast<const float2*>(tree + 2 * node);
        tree[node] = c.x + c.y;
    }
}

// remaining levels l = l0 .. logP of the contiguous leaf range [a, b] (heap positions), one workgroup
__global__ __launch_bounds__(1024) void sumtree_range_kernel(float* tree, int64_t a, int64_t b, int l0, int logP) {
    for (int l = l0; l <= logP; ++l) {
        int64_t lo = a >> l, hi = b >> l;
        for (int64_t node = lo + threadIdx.x; node <= hi; node += 1024) {
            float2 c = *reinterpret_cast<const float2*>(tree + 2 * node);
            tree[node] = c.x + c.y;
        }
        __syncthreads();  // workgroup-scope release/acquire: the next level reads what this one wrote
    }
}

// PrioritizedDQN write-back: p = (|td| + eps)^alpha; the power is evaluated in Float64 and rounded once
__global__ __launch_bounds__(256) void per_priority_kernel(const float* __restrict__ td, int64_t n, float eps,
                                                           float alpha, float* __restrict__ out) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    out[i] = per_priority_value(td[i], eps, alpha);
}

// Importance-sampling weights of prioritized replay (Schaul et al. 2016; the removed Zoo's PrioritizedDQN, from memory --
// PARITY UNPINNED like the rest of the prioritized path):  w = 1 ./ ((priorities .+ 1f-10) .^ beta);  w ./= maximum(w).
// (N and the total priority of the textbook form (N P(i))^-beta cancel in the normalisation by the maximum.)
// One workgroup: the powers in Float64, rounded once; the maximum over the batch behind one barrier.
__global__ __launch_bounds__(1024) void per_is_weights_kernel(const float* __restrict__ prio, int64_t n, float beta,
                                                              float* __restrict__ out) {
    __shared__ float l_m[16];
    float mx = 0.0f;
    for (int64_t i = threadIdx.x; i < n; i += 1024) {
        const float w = (float)(1.0 / pow((double)(prio[i] + 1e-10f), (double)beta));
        out[i] = w;
        mx = fmaxf(mx, w);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
    if ((threadIdx.x & 63) == 0) l_m[threadIdx.x >> 6] = mx;
    __syncthreads();
    mx = l_m[0];
#pragma unroll
    for (int w = 1; w < 16; ++w) mx = fmaxf(mx, l_m[w]);
    for (int64_t i = threadIdx.x; i < n; i += 1024) out[i] = out[i] / mx;  // each thread re-reads what it wrote itself
}

struct RingGeom {
    int64_t capacity, n_env, head_rt;
};

template <bool RING>
__global__ __launch_bounds__(256) void sumtree_sample_kernel(const float* __restrict__ tree, int64_t P,
                                                             int64_t n_leaves, int64_t batch, uint64_t seed,
                                                             uint32_t draw_ctr, RingGeom rg,
                                                             int64_t* __restrict__ idx_out,
                                                             int64_t* __restrict__ key_out,
                                                             float* __restrict__ prio_out) {
    int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= batch) return;
    const int64_t leaf = sumtree_draw(tree, P, n_leaves, seed, b, draw_ctr);
    if (key_out) key_out[b] = leaf;
    if (prio_out) prio_out[b] = tree[P + leaf];
    if (RING) {
        int64_t pt = leaf / rg.n_env, e = leaf - pt * rg.n_env;
        int64_t li = pt - rg.head_rt;
        if (li < 0) li += rg.capacity;
        idx_out[b] = li * rg.n_env + e;  // logical flat index, the convention of rlhip_ring_gather
    }
}

static int32_t fill_range(float* tree, int64_t n_leaves, int64_t start, int64_t count, float value, hipStream_t s) {
    RLHIP_REQUIRE(n_leaves >= 1 && start >= 0 && count >= 0 && start + count <= n_leaves, "leaf range out of bounds");
    RLHIP_REQUIRE(value >= 0.0f, "priorities must be non-negative");
    if (count == 0) return RLHIP_OK;
    RLHIP_REQUIRE(tree != nullptr, "NULL tree");
    const int64_t P = pow2_ge(n_leaves);
    const int logP = log2_of(P);
    const int64_t a = P + start, b = P + start + count - 1;
    hipLaunchKernelGGL(sumtree_fill_leaves_kernel, dim3(grid_for(count, 256)), dim3(256), 0, s, tree, a, count, value);
    int l = 1;
    for (; l <= logP; ++l) {
        int64_t lo = a >> l, hi = b >> l;
        if (hi - lo + 1 <= 2048) break;
        hipLaunchKernelGGL(sumtree_level_kernel, dim3(grid_for(hi - lo + 1, 256)), dim3(256), 0, s, tree, lo, hi);
    }
    if (l <= logP) hipLaunchKernelGGL(sumtree_range_kernel, dim3(1), dim3(1024), 0, s, tree, a, b, l, logP);
    RLHIP_LAUNCH_CHECK();
    return RLHIP_OK;
}

}  // namespace rlhip

using namespace rlhip;

extern "C" {

int64_t rlhip_sumtree_nodes(int64_t n_leaves) { return n_leaves < 1 ? 0 : 2 * pow2_ge(n_leaves); }

int32_t rlhip_sumtree_fill_range(float* tree, int64_t n_leaves, int64_t start, int64_t count, float value,
                                 rlhip_stream_t stream) {
    return fill_range(tree, n_leaves, start, count, value, as_stream(stream));
}

int32_t rlhip_sumtree_update(float* tree, int64_t n_leaves, const int64_t* leaf, const float* prio, int64_t n,
                             rlhip_stream_t stream) {
    RLHIP_REQUIRE(n_leaves >= 1 && n >= 0, "bad sizes");
    if (n == 0) return RLHIP_OK;
    RLHIP_REQUIRE(tree && leaf && prio, "NULL array");
    RLHIP_REQUIRE(n < (1ll << 31), "too many keys in one update");
    return sumtree_update_launch(tree, n_leaves, leaf, PrioLoad{prio}, n, as_stream(stream));
}

int32_t rlhip_sumtree_sample(const float* tree, int64_t n_leaves, int64_t batch, uint64_t seed, uint32_t draw_ctr,
                             int64_t* leaf_out, float* prio_out, rlhip_stream_t stream) {
    RLHIP_REQUIRE(n_leaves >= 1 && batch >= 0, "bad sizes");
    if (batch == 0) return RLHIP_OK;
    RLHIP_REQUIRE(tree && leaf_out, "NULL array");
    RingGeom rg = {0, 1, 0};
    hipLaunchKernelGGL((sumtree_sample_kernel<false>), dim3((int)((batch + 255) / 256)), dim3(256), 0, as_stream(stream),
                       tree, pow2_ge(n_leaves), n_leaves, batch, seed, draw_ctr, rg, (int64_t*)nullptr, leaf_out,
                       prio_out);
    RLHIP_LAUNCH_CHECK();
    return RLHIP_OK;
}

int32_t rlhip_per_priority_f32(const float* td, int64_t n, float eps, float alpha, float* out,
                               rlhip_stream_t stream) {
    RLHIP_REQUIRE(n >= 0 && eps >= 0.0f && alpha >= 0.0f, "bad arguments");
    if (n == 0) return RLHIP_OK;
    RLHIP_REQUIRE(td && out, "NULL array");
    hipLaunchKernelGGL(per_priority_kernel, dim3((int)((n + 255) / 256)), dim3(256), 0, as_stream(stream), td, n, eps,
                       alpha, out);
    RLHIP_LAUNCH_CHECK();
    return RLHIP_OK;
}

int32_t rlhip_per_is_weights_f32(const float* prio, int64_t n, float beta, float* w_out, rlhip_stream_t stream) {
    RLHIP_REQUIRE(n >= 0 && beta >= 0.0f, "bad arguments");
    if (n == 0) return RLHIP_OK;
    RLHIP_REQUIRE(prio && w_out, "NULL array");
    hipLaunchKernelGGL(per_is_weights_kernel, dim3(1), dim3(1024), 0, as_stream(stream), prio, n, beta, w_out);
    RLHIP_LAUNCH_CHECK();
    return RLHIP_OK;
}

int32_t rlhip_ring_push_priority(const rlhip_ring* rb, float* tree, float priority, rlhip_stream_t stream) {
    RLHIP_REQUIRE(rb && tree, "bad arguments");
    RLHIP_REQUIRE(rb->len_rt >= 1, "no transition has been pushed yet");
    int64_t newest = (rb->head_rt + rb->len_rt - 1) % rb->capacity;
    return fill_range(tree, rb->capacity * rb->n_env, newest * rb->n_env, rb->n_env, priority, as_stream(stream));
}

int32_t rlhip_ring_sample_prioritized(const rlhip_ring* rb, const float* tree, int64_t batch, uint64_t seed,
                                      uint32_t draw_ctr, int64_t* idx_out, int64_t* key_out, float* prio_out,
                                      rlhip_stream_t stream) {
    RLHIP_REQUIRE(rb && batch >= 0, "bad arguments");
    RLHIP_REQUIRE(rb->len_rt >= 1, "cannot sample from an empty trajectory");
    if (batch == 0) return RLHIP_OK;
    RLHIP_REQUIRE(tree && idx_out, "NULL array");
    const int64_t n_leaves = rb->capacity * rb->n_env;
    RingGeom rg = {rb->capacity, rb->n_env, rb->head_rt};
    hipLaunchKernelGGL((sumtree_sample_kernel<true>), dim3((int)((batch + 255) / 256)), dim3(256), 0, as_stream(stream),
                       tree, pow2_ge(n_leaves), n_leaves, batch, seed, draw_ctr, rg, idx_out, key_out, prio_out);
    RLHIP_LAUNCH_CHECK();
    return RLHIP_OK;
}

}  // extern "C"
