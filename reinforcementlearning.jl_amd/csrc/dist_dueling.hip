// dist_dueling.hip -- DuelingNetwork heads for the distributional learners (C51, QR-DQN) as an on-device parameter fold: the sibling of
// dueling.hip for a head whose value and advantage streams carry K atoms / quantiles each.  include/rlhip.h (the dueling distributional
// section) is the specification; tests/dist_dueling_ref.py replays it in numpy Float32.
//
// The reference's combine, per atom k:  l[k, o] = v[k] + a[k, o] - mean_o'(a[k, o']).  It is linear in the head, so with
//
//     W2e[k + K o, :] = Wval[k, :] + Wadv[k + K o, :] - mean_o'(Wadv[k + K o', :]),     b2e likewise
//
// a plain Dense(h, na K) head computes the dueling logits / quantiles, and every C51 / QR-DQN kernel serves the net UNCHANGED on the
// effective vector.  The scalar fold of dueling.hip cannot do this: its mean runs over every head row, this one over the na rows of
// ONE atom (rows K apart).
//
// Dueling vector: a plain mlp2(ns, h, M' = (1 + na) K) vector; rows m < na K of its head are the advantage rows in C51's order
// (m = k + K o), rows na K + k the value rows.  Effective vector: mlp2(ns, h, M = na K).  Both heads are column-major with the bias as
// one more column, so column j (j = h: the bias) starts at j M' in one layout and j M in the other, and one thread owns one (k, j):
// its 1 + na loads and na stores are coalesced along k in both strides.  W1 | b1 sit at the same offset in both layouts: a 16-byte
// copy with a scalar tail by the workgroups in front.  blockIdx.y selects the net of the two-net fold.  No LDS, no atomics, no
// Float64, vector stores only.
#include "dist_host.h"
#include "dist_dueling_device.h"

namespace rlhip {

constexpr int DD_THREADS = 256;

struct DistDuelArgs {
    const float* src[2];  // fold: the dueling vectors;  unfold: the gradient of the effective vector
    float* dst[2];        // fold: the effective vectors; unfold: the gradient of the dueling vector
    int nbase;            // floats in front of the head, h ns + h (the same offset in both layouts)
    int h, na, K;
    int copy_blocks;      // workgroups [0, copy_blocks) copy W1 | b1, the rest own the head
    int vec[2];           // both pointers of the net 16-byte aligned: float4 copies
};

// W1 | b1: quad q of the grid per thread; the last, partial quad (and everything, when unaligned) goes element by element
__device__ __forceinline__ void dd_copy_base(const float* __restrict__ src, float* __restrict__ dst, int nbase, int vec) {
    const int i = 4 * ((int)blockIdx.x * DD_THREADS + (int)threadIdx.x);
    if (i >= nbase) return;
    if (vec && i + 3 < nbase) {
        *reinterpret_cast<float4*>(dst + i) = *reinterpret_cast<const float4*>(src + i);
    } else {
        const int e = i + 4 < nbase ? i + 4 : nbase;
        for (int k = i; k < e; ++k) dst[k] = src[k];
    }
}

// the (k, j) of this thread among the (h + 1) K of the head; false beyond them
__device__ __forceinline__ bool dd_head_item(const DistDuelArgs& g, int& k, int& j) {
    const int t = ((int)blockIdx.x - g.copy_blocks) * DD_THREADS + (int)threadIdx.x;
    j = t / g.K, k = t - j * g.K;
    return j <= g.h;
}

// duel = [W1 | b1 | W2 ((1 + na) K x h) | b2] -> eff = [W1 | b1 | W2e (na K x h) | b2e]
__global__ __launch_bounds__(DD_THREADS) void dist_dueling_fold_kernel(DistDuelArgs g) {
    const int net = blockIdx.y;
    const float* __restrict__ src = g.src[net];
    float* __restrict__ dst = g.dst[net];
    if ((int)blockIdx.x < g.copy_blocks) {
        dd_copy_base(src, dst, g.nbase, g.vec[net]);
        return;
    }
    int k, j;
    if (!dd_head_item(g, k, j)) return;
    const int na = g.na, K = g.K, M = na * K;
    const float* in = src + g.nbase + j * (M + K);  // column j of the dueling head: na K advantage rows, then K value rows
    float* out = dst + g.nbase + j * M;
    float x[MAXO] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int o = 0; o < MAXO; ++o)
        if (o < na) x[o] = in[k + K * o];
    dist_duel_combine(in[M + k], x, na);
#pragma unroll
    for (int o = 0; o < MAXO; ++o)
        if (o < na) out[k + K * o] = x[o];
}

// grad_eff = [gW1 | gb1 | dW2e | db2e] -> grad_duel = [gW1 | gb1 | dW2 | db2]: dWval[k, j] = s, dWadv[k + K o, j] = dW2e - s / na
__global__ __launch_bounds__(DD_THREADS) void dist_dueling_unfold_kernel(DistDuelArgs g) {
    const float* __restrict__ src = g.src[0];
    float* __restrict__ dst = g.dst[0];
    if ((int)blockIdx.x < g.copy_blocks) {
        dd_copy_base(src, dst, g.nbase, g.vec[0]);
        return;
    }
    int k, j;
    if (!dd_head_item(g, k, j)) return;
    const int na = g.na, K = g.K, M = na * K;
    const float* ge = src + g.nbase + j * M;
    float* gd = dst + g.nbase + j * (M + K);
    float x[MAXO] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int o = 0; o < MAXO; ++o)
        if (o < na) x[o] = ge[k + K * o];
    const float s = dist_duel_uncombine(x, na);
#pragma unroll
    for (int o = 0; o < MAXO; ++o)
        if (o < na) gd[k + K * o] = x[o];
    gd[M + k] = s;
}

static bool dist_dueling_ok(int64_t ns, int64_t h, int64_t na, int64_t K) {
    DIST_DUEL_BOUNDS(DIST_BOUND_HOLDS, 1);
    return true;
}

static inline int dd_aligned16(const void* a, const void* b) { return ((((uintptr_t)a) | ((uintptr_t)b)) & 15) == 0; }
static inline bool dd_overlap(const float* a, int64_t na, const float* b, int64_t nb) {
    return (uintptr_t)a < (uintptr_t)(b + nb) && (uintptr_t)b < (uintptr_t)(a + na);
}

static void dist_dueling_grid(DistDuelArgs& g, int64_t ns, int64_t h, int64_t na, int64_t K, int* blocks) {
    g.nbase = (int)(h * ns + h);
    g.h = (int)h, g.na = (int)na, g.K = (int)K;
    g.copy_blocks = ((g.nbase + 3) / 4 + DD_THREADS - 1) / DD_THREADS;
    *blocks = g.copy_blocks + (int)(((h + 1) * K + DD_THREADS - 1) / DD_THREADS);
}

}  // namespace rlhip

using namespace rlhip;

extern "C" {

int64_t rlhip_dist_dueling_nparams(int64_t ns, int64_t h, int64_t na, int64_t K) {
    return dist_dueling_ok(ns, h, na, K) ? mlp2_nparams(ns, h, (1 + na) * K) : -1;
}

int32_t rlhip_dist_dueling_fold_f32(const float* duel, float* eff, const float* duel2, float* eff2, int64_t ns, int64_t h, int64_t na,
                                    int64_t K, rlhip_stream_t stream) {
    DIST_DUEL_BOUNDS(RLHIP_REQUIRE, 1);
    RLHIP_REQUIRE(duel && eff, "NULL argument");
    RLHIP_REQUIRE((duel2 == nullptr) == (eff2 == nullptr), "the second net is a pair: both duel2 and eff2, or neither");
    const int64_t nd = mlp2_nparams(ns, h, (1 + na) * K), ne = mlp2_nparams(ns, h, na * K);
    RLHIP_REQUIRE(!dd_overlap(eff, ne, duel, nd), "eff must not overlap the dueling vector");
    RLHIP_REQUIRE(!duel2 || (!dd_overlap(eff2, ne, duel2, nd) && !dd_overlap(eff2, ne, eff, ne) && !dd_overlap(eff2, ne, duel, nd) &&
                             !dd_overlap(eff, ne, duel2, nd)),
                  "the second pair must not overlap the first pair's output or its own input");
    DistDuelArgs g;
    int blocks;
    dist_dueling_grid(g, ns, h, na, K, &blocks);
    g.src[0] = duel, g.dst[0] = eff, g.vec[0] = dd_aligned16(duel, eff);
    g.src[1] = duel2, g.dst[1] = eff2, g.vec[1] = duel2 ? dd_aligned16(duel2, eff2) : 0;
    hipLaunchKernelGGL(dist_dueling_fold_kernel, dim3(blocks, duel2 ? 2 : 1), dim3(DD_THREADS), 0, as_stream(stream), g);
    RLHIP_LAUNCH_CHECK();
    return RLHIP_OK;
}

int32_t rlhip_dist_dueling_unfold_grad_f32(const float* grad_eff, float* grad_duel, int64_t ns, int64_t h, int64_t na, int64_t K,
                                           rlhip_stream_t stream) {
    DIST_DUEL_BOUNDS(RLHIP_REQUIRE, 1);
    RLHIP_REQUIRE(grad_eff && grad_duel, "NULL argument");
    RLHIP_REQUIRE(!dd_overlap(grad_duel, mlp2_nparams(ns, h, (1 + na) * K), grad_eff, mlp2_nparams(ns, h, na * K)),
                  "grad_duel must not overlap grad_eff");
    DistDuelArgs g;
    int blocks;
    dist_dueling_grid(g, ns, h, na, K, &blocks);
    g.src[0] = grad_eff, g.dst[0] = grad_duel, g.vec[0] = dd_aligned16(grad_eff, grad_duel);
    g.src[1] = nullptr, g.dst[1] = nullptr, g.vec[1] = 0;
    hipLaunchKernelGGL(dist_dueling_unfold_kernel, dim3(blocks), dim3(DD_THREADS), 0, as_stream(stream), g);
    RLHIP_LAUNCH_CHECK();
    return RLHIP_OK;
}

}  // extern "C"
