// dueling.hip -- DuelingNetwork(base, val, adv) Q-networks as an on-device parameter fold (RLCore/src/utils/networks.jl:510-522:
// Q = val .+ adv .- mean(adv, dims = 1)).
//
// The dueling combine is linear in the head.  With
//
//     W2e[a, :] = Wval + Wadv[a, :] - mean_a'(Wadv[a', :]),     b2e[a] = bval + badv[a] - mean_a'(badv[a'])
//
// a plain Dense(h, na) head computes the dueling Q, so every shipped kernel (plan, act, gradient, Double DQN fold) serves a dueling
// net UNCHANGED on the effective plain vector.  dL/dh = sum_a W2e[a, :] dQ_a is the same expression in both forms, so the plain
// gradient kernels give dW1, db1 and the hidden-layer gradients as they stand; the head gradient maps back by the chain rule:
//
//     dWval = sum_a dW2e[a, :],     dWadv[a, :] = dW2e[a, :] - mean_a'(dW2e[a', :]),     the biases likewise.
//
// Flat dueling vector: [ plain layout of the same net with (Wadv, badv) as its last Dense | Wval (h) | bval (1) ], length = plain
// nparams + h + 1; the last Dense is W (na x h, column-major: element (a, j) at j * na + a) followed by b (na).
//
// Arithmetic, fixed so that a numpy Float32 restatement is bit-exact (tests/dueling_ref.py; -ffp-contract=off is the build contract):
// per hidden unit j the left-folded sum s = ((x0 + x1) + x2) + x3 over the na rows, mean = s / float(na) (a true division),
// W2e[a, j] = (Wval[j] + Wadv[a, j]) - mean -- the reference's `val .+ adv .- mean` order; the unfold: dWval[j] = s over the dW2e
// rows, dWadv[a, j] = dW2e[a, j] - s / float(na).  No Float64, no atomics, nothing crosses a workgroup, vector stores only.
//
// Two launch-bound copies (<= ~270 KB at hidden 256, three layers): one launch each.  Workgroups [0, copy_blocks) copy everything in
// front of the head (16-byte accesses when both pointers are 16-byte aligned, a scalar tail), the workgroups behind them give the head
// one thread per hidden unit j (plus one thread for the biases): no LDS.  blockIdx.y selects the net of the two-net fold.
#include "common.h"

extern "C" int64_t rlhip_mlp2_nparams(int64_t n_in, int64_t h, int64_t n_out);
extern "C" int64_t rlhip_mlp3_nparams(int64_t ns, int64_t h, int64_t na);

namespace rlhip {

constexpr int DU_THREADS = 256;
constexpr int DU_MAXO = 4;

struct DuelArgs {
    const float* src[2];  // fold: the dueling vectors;  unfold: the plain (effective) gradient
    float* dst[2];        // fold: the effective vectors; unfold: the dueling gradient
    int64_t nbase;        // floats in front of the head (the same offset in both layouts)
    int h, na;
    int copy_blocks;      // workgroups [0, copy_blocks) copy the base, the rest own the head
    int vec[2];           // both pointers of the net 16-byte aligned: float4 copies
};

// base[0 .. nbase): quad q of the grid per thread; the last, partial quad (and everything, when unaligned) goes element by element
__device__ __forceinline__ void copy_base(const float* __restrict__ src, float* __restrict__ dst, int64_t nbase, int vec) {
    const int64_t q = (int64_t)blockIdx.x * DU_THREADS + threadIdx.x;
    const int64_t i = q * 4;
    if (i >= nbase) return;
    if (vec && i + 3 < nbase) {
        *reinterpret_cast<float4*>(dst + i) = *reinterpret_cast<const float4*>(src + i);
    } else {
        const int64_t e = i + 4 < nbase ? i + 4 : nbase;
        for (int64_t k = i; k < e; ++k) dst[k] = src[k];
    }
}

// x[0 .. na) -> the left-folded sum ((x0 + x1) + x2) + x3
__device__ __forceinline__ float fold_sum(const float* x, int na) {
    float s = x[0];
#pragma unroll
    for (int a = 1; a < DU_MAXO; ++a)
        if (a < na) s = s + x[a];
    return s;
}

// duel = [base | Wadv | badv | Wval | bval] -> eff = [base | W2e | b2e]
__global__ __launch_bounds__(DU_THREADS) void dueling_fold_kernel(DuelArgs g) {
    const int net = blockIdx.y;
    const float* __restrict__ src = g.src[net];
    float* __restrict__ dst = g.dst[net];
    if ((int)blockIdx.x < g.copy_blocks) {
        copy_base(src, dst, g.nbase, g.vec[net]);
        return;
    }
    const int h = g.h, na = g.na;
    const int j = ((int)blockIdx.x - g.copy_blocks) * DU_THREADS + threadIdx.x;
    if (j > h) return;
    const float* adv = src + g.nbase;                        // Wadv (na x h) | badv (na)
    const float* val = src + g.nbase + (int64_t)na * h + na;  // Wval (h) | bval (1)
    float* out = dst + g.nbase;
    // thread j < h: column j of the head; thread j == h: the biases (the same expressions on badv / bval)
    const int64_t o = (int64_t)na * j;
    float x[DU_MAXO] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int a = 0; a < DU_MAXO; ++a)
        if (a < na) x[a] = adv[o + a];
    const float v = val[j];
    const float mean = fold_sum(x, na) / (float)na;
#pragma unroll
    for (int a = 0; a < DU_MAXO; ++a)
        if (a < na) out[o + a] = (v + x[a]) - mean;
}

// grad_eff = [gbase | dW2e | db2e] -> grad_duel = [gbase | dWadv | dbadv | dWval | dbval]
__global__ __launch_bounds__(DU_THREADS) void dueling_unfold_kernel(DuelArgs g) {
    const float* __restrict__ src = g.src[0];
    float* __restrict__ dst = g.dst[0];
    if ((int)blockIdx.x < g.copy_blocks) {
        copy_base(src, dst, g.nbase, g.vec[0]);
        return;
    }
    const int h = g.h, na = g.na;
    const int j = ((int)blockIdx.x - g.copy_blocks) * DU_THREADS + threadIdx.x;
    if (j > h) return;
    const float* ge = src + g.nbase;  // dW2e (na x h) | db2e (na)
    float* gadv = dst + g.nbase;
    float* gval = dst + g.nbase + (int64_t)na * h + na;
    const int64_t o = (int64_t)na * j;
    float x[DU_MAXO] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int a = 0; a < DU_MAXO; ++a)
        if (a < na) x[a] = ge[o + a];
    const float s = fold_sum(x, na);
    const float mean = s / (float)na;
#pragma unroll
    for (int a = 0; a < DU_MAXO; ++a)
        if (a < na) gadv[o + a] = x[a] - mean;
    gval[j] = s;
}

static inline int64_t plain_nparams(int64_t ns, int64_t h, int64_t na, int32_t layers) {
    return layers == 2 ? rlhip_mlp2_nparams(ns, h, na) : rlhip_mlp3_nparams(ns, h, na);
}

static int32_t dueling_check(int64_t ns, int64_t h, int64_t na, int32_t layers) {
    RLHIP_REQUIRE(layers == 2 || layers == 3, "layers must be 2 or 3");
    RLHIP_REQUIRE(na >= 1 && na <= DU_MAXO, "na must be 1..4");
    RLHIP_REQUIRE(ns >= 1 && h >= 1, "ns and h must be >= 1");
    RLHIP_REQUIRE(plain_nparams(ns, h, na, layers) + h + 1 <= INT32_MAX, "network too large");
    return RLHIP_OK;
}

static inline int aligned16(const void* a, const void* b) { return ((((uintptr_t)a) | ((uintptr_t)b)) & 15) == 0; }

static void dueling_grid(DuelArgs& g, int64_t ns, int64_t h, int64_t na, int32_t layers, int* blocks) {
    g.nbase = plain_nparams(ns, h, na, layers) - na * h - na;
    g.h = (int)h;
    g.na = (int)na;
    g.copy_blocks = (int)(((g.nbase + 3) / 4 + DU_THREADS - 1) / DU_THREADS);
    *blocks = g.copy_blocks + (int)((h + 1 + DU_THREADS - 1) / DU_THREADS);
}

}  // namespace rlhip

using namespace rlhip;

extern "C" {

int64_t rlhip_dueling_nparams(int64_t ns, int64_t h, int64_t na, int32_t layers) {
    if (ns < 1 || h < 1 || na < 1 || (layers != 2 && layers != 3)) return -1;
    return plain_nparams(ns, h, na, layers) + h + 1;
}

int32_t rlhip_dueling_fold_f32(const float* duel, float* eff, const float* duel2, float* eff2, int64_t ns, int64_t h, int64_t na,
                               int32_t layers, rlhip_stream_t stream) {
    int32_t rc = dueling_check(ns, h, na, layers);
    if (rc) return rc;
    RLHIP_REQUIRE(duel && eff, "NULL argument");
    RLHIP_REQUIRE((const float*)eff != duel, "eff must not be the dueling vector (the layouts differ behind the head)");
    RLHIP_REQUIRE((duel2 == nullptr) == (eff2 == nullptr), "the second net is a pair: both duel2 and eff2, or neither");
    RLHIP_REQUIRE(!duel2 || ((const float*)eff2 != duel2 && eff2 != eff && (const float*)eff2 != duel && (const float*)eff != duel2),
                  "the second pair must not alias the first pair's output or its own input");
    DuelArgs g;
    int blocks;
    dueling_grid(g, ns, h, na, layers, &blocks);
    g.src[0] = duel, g.dst[0] = eff, g.vec[0] = aligned16(duel, eff);
    g.src[1] = duel2, g.dst[1] = eff2, g.vec[1] = duel2 ? aligned16(duel2, eff2) : 0;
    hipLaunchKernelGGL(dueling_fold_kernel, dim3(blocks, duel2 ? 2 : 1), dim3(DU_THREADS), 0, as_stream(stream), g);
    RLHIP_LAUNCH_CHECK();
    return RLHIP_OK;
}

int32_t rlhip_dueling_unfold_grad_f32(const float* grad_eff, float* grad_duel, int64_t ns, int64_t h, int64_t na, int32_t layers,
                                      rlhip_stream_t stream) {
    int32_t rc = dueling_check(ns, h, na, layers);
    if (rc) return rc;
    RLHIP_REQUIRE(grad_eff && grad_duel, "NULL argument");
    RLHIP_REQUIRE((const float*)grad_duel != grad_eff, "grad_duel must not be grad_eff (the layouts differ behind the head)");
    DuelArgs g;
    int blocks;
    dueling_grid(g, ns, h, na, layers, &blocks);
    g.src[0] = grad_eff, g.dst[0] = grad_duel, g.vec[0] = aligned16(grad_eff, grad_duel);
    g.src[1] = nullptr, g.dst[1] = nullptr, g.vec[1] = 0;
    hipLaunchKernelGGL(dueling_unfold_kernel, dim3(blocks), dim3(DU_THREADS), 0, as_stream(stream), g);
    RLHIP_LAUNCH_CHECK();
    return RLHIP_OK;
}

}  // extern "C"
