// td3_mlp3_device.h -- the tile passes of the three-layer off-policy learners, shared by csrc/td3_mlp3.hip (TD3 / DDPG: one actor
// output) and csrc/sac_mlp3.hip (SAC: two actor outputs, mu and rho): the network slots, the record gather, the forward pass, the
// back-propagation, the accumulators a workgroup carries across its tiles, the partial-row store, the critic gradient launch's body,
// the LDS sizing and the launch macros.  The header of csrc/td3_mlp3.hip describes the design; include/rlhip.h ("TD3 and DDPG with
// two hidden layers", "SAC with two hidden layers") states every chain and order.
//
// NO is the number of output rows of the network a pass runs, 1 or 2 (W3[o, j] at o + NO j, b3[o] behind it).  Every `if (NO == ..)`
// is a compile-time branch: the instantiation at NO = 1 is the code csrc/td3_mlp3.hip held before the passes moved here.
// No __global__ lives here: each object defines its own kernels around these passes.
#pragma once
#include "head_device.h"
#include "mfma_common.h"
#include "mlp_device.h"
#include "ring_device.h"

namespace rlhip {

constexpr int M3T = 32;        // samples per tile (the M of the MFMA)
constexpr int M3NT = 512;      // threads
constexpr int M3HMAX = 256;
constexpr int M3XS = 8;        // floats per row of the input image
constexpr int M3STATS = 2;     // partial sums per workgroup beside its gradient row
constexpr int M3MAXB = 256;    // partial rows at most ...
constexpr int64_t M3ROWBYTES = 16 << 20;  // ... and at most 16 MiB of them

__host__ __device__ __forceinline__ int64_t td3m_nparams(int64_t ni, int64_t h, int64_t no = 1) {
    return h * ni + h + h * h + h + no * h + no;
}

struct Td3mArgs {
    RingRecs ring;
    const int64_t* idx;
    const float* actor;    // target launch: the actor TARGET
    const float* critics;
    const float* targets;  // target launch only
    float* partials;
    float* stat_partials;
    float* ybuf;           // the TD targets: written by the target launch, read by the critic gradient launch
    int64_t batch;
    int ns, h, num_tiles, np;
    float gamma, lo, hi, scale, fb, target_noise, noise_clip;
    uint64_t seed;
    uint32_t step;
    float* y_out;      // nullable
    float* noise_out;  // nullable
};

// a network whose small tensors sit in an LDS slot (W1 | b1 | b2 | W3) and whose W2 stays in global memory
struct Td3mNet {
    const float *W1, *b1, *b2, *W3, *W2;
    float b3[2];
    int ni;
};
__host__ __device__ __forceinline__ int td3m_slot_floats(int h) { return h * 8 + 4; }  // ni <= 5: h ni + h + 2 h + 1; ni <= 4, NO = 2: 8 h
template <int NO = 1>
__device__ __forceinline__ Td3mNet td3m_stage(const float* __restrict__ P, int ni, int h, float* slot) {
    const int n1 = h * ni + h, n2 = (1 + NO) * h;
    const float* P2 = P + n1 + h * h;
    for (int q = threadIdx.x; q < n1; q += M3NT) slot[q] = P[q];
    for (int q = threadIdx.x; q < n2; q += M3NT) slot[n1 + q] = P2[q];
    Td3mNet v;
    v.W1 = slot, v.b1 = slot + h * ni, v.b2 = slot + n1, v.W3 = v.b2 + h, v.W2 = P + n1, v.b3[0] = P2[n2], v.ni = ni;
    v.b3[1] = NO == 2 ? P2[n2 + 1] : 0.0f;
    return v;
}
// (the view of a one-output network that td3m_stage has already copied into `slot`)
__device__ __forceinline__ Td3mNet td3m_view(const float* __restrict__ P, int ni, int h, const float* slot) {
    const int n1 = h * ni + h;
    Td3mNet v;
    v.W1 = slot, v.b1 = slot + h * ni, v.b2 = slot + n1, v.W3 = v.b2 + h, v.W2 = P + n1, v.b3[0] = P[n1 + h * h + 2 * h], v.b3[1] = 0.0f, v.ni = ni;
    return v;
}

// the tile's records and per-sample values.  x is the input image of the next forward pass: columns 0 .. ns - 1 the state, column
// ns the action.  A position past the batch holds the record of position 0: finite operands everywhere, zero gradient factors
struct Td3mTile {
    float x[M3T][M3XS], sn[M3T][4], r[M3T], cont[M3T], e[M3T], a[M3T], g[M3T], l[M3T], out[3][M3T];
};
__device__ __forceinline__ void td3m_gather(const Td3mArgs& g, int tile, bool next, Td3mTile& t) {
    const int tid = threadIdx.x;
    if (tid < M3T) {
        const int64_t b = (int64_t)tile * M3T + tid;
        const RingTransition rt = ring_load_transition(g.ring, g.idx[b < g.batch ? b : 0]);
#pragma unroll
        for (int k = 0; k < 4; ++k) t.x[tid][k] = next ? rt.sn[k] : rt.s[k], t.sn[tid][k] = rt.sn[k];
        if (!next) t.x[tid][g.ns] = __int_as_float(rt.a);  // the action word holds the bits of a Float32
        t.r[tid] = rt.r;
        t.cont[tid] = rt.t ? 0.0f : 1.0f;
    }
}

__device__ __forceinline__ float td3m_row_sum_down(float v) {  // the 16 lanes of a DPP row into its lane 0: += [i + 8], 4, 2, 1
    v = dpp_add<0x108>(v);
    v = dpp_add<0x104>(v);
    v = dpp_add<0x102>(v);
    return dpp_add<0x101>(v);
}

// out[o][m] = mlp3(ni, h, NO)(x[m]) for the tile's 32 rows (l_out: NO rows of M3T floats); leaves a1 and a2 of the tile in LDS, rows
// h + 1 floats apart.  Opens with a barrier (the caller's writes of x and of the staged slots) and closes with one (l_out)
template <int ACT, bool CHAIN3, int NO = 1>
__device__ __forceinline__ void td3m_forward(const Td3mNet& N, int h, const float (*l_x)[M3XS], float* l_a1, float* l_a2, float* l_out) {
    const int tid = threadIdx.x, P = h + 1;
    __syncthreads();
    for (int q = tid; q < M3T * h; q += M3NT) {
        const int m = q / h, j = q - m * h;
        float z = N.b1[j];
        for (int k = 0; k < N.ni; ++k) z = fmaf(N.W1[j + h * k], l_x[m][k], z);
        l_a1[m * P + j] = act_fwd_t<ACT>(z);
    }
    __syncthreads();
    const int lane = tid & 63, wave = tid >> 6, c = lane & 31, kb = lane >> 5;
    if (wave * 32 < h) {  // A[m = row c][k = unit e of layer 1], B[k = e][n = unit j], e = 2 ks + kb
        const int j = wave * 32 + c;
        const float b = N.b2[j];
        f32x16 acc;
#pragma unroll
        for (int q = 0; q < 16; ++q) acc[q] = b;
        const float* ap = l_a1 + c * P + kb;
        const float* bp = N.W2 + j + (int64_t)h * kb;
#pragma unroll 4
        for (int ks = 0; ks < h / 2; ++ks) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[2 * ks], bp[(int64_t)2 * ks * h], acc, 0, 0, 0);
#pragma unroll
        for (int q = 0; q < 16; ++q) l_a2[mfma_row(q, kb) * P + j] = act_fwd_t<ACT>(acc[q]);
    }
    __syncthreads();
    if (NO == 1) {
        if (CHAIN3) {
            if (tid < M3T) {
                float o = N.b3[0];
                for (int j = 0; j < h; ++j) o = fmaf(N.W3[j], l_a2[tid * P + j], o);
                l_out[tid] = o;
            }
        } else {
            const int r = tid >> 4, p = tid & 15;
            float part = 0.0f;
            for (int j = p; j < h; j += 16) part = fmaf(N.W3[j], l_a2[r * P + j], part);
            part = td3m_row_sum_down(part);
            if (p == 0) l_out[r] = part + N.b3[0];
        }
    } else if (CHAIN3) {  // thread = (output o, env m): ONE ascending chain each
        if (tid < 2 * M3T) {
            const int o = tid >> 5, m = tid & 31;
            float v = o ? N.b3[1] : N.b3[0];
            for (int j = 0; j < h; ++j) v = fmaf(N.W3[o + 2 * j], l_a2[m * P + j], v);
            l_out[o * M3T + m] = v;
        }
    } else {  // one 16-lane row per (sample, output): the 32 rows of the workgroup take output 0, then output 1
        const int r = tid >> 4, p = tid & 15;
#pragma unroll
        for (int o = 0; o < 2; ++o) {
            float part = 0.0f;
            for (int j = p; j < h; j += 16) part = fmaf(N.W3[o + 2 * j], l_a2[r * P + j], part);
            part = td3m_row_sum_down(part);
            if (p == 0) l_out[o * M3T + r] = part + N.b3[o];
        }
    }
    __syncthreads();
}

// what a workgroup carries across its tiles: thread j < h the chains of unit j, thread 0 the scalars, every wave its dW2 blocks
template <int NBW, int NO = 1>
struct Td3mAcc {
    float gw1[5], gb1, gb2, gw3[NO], gb3[NO], s0, s1;
    f32x16 dw2[NBW];
};
template <int NBW, int NO>
__device__ __forceinline__ void td3m_zero(Td3mAcc<NBW, NO>& A) {
#pragma unroll
    for (int k = 0; k < 5; ++k) A.gw1[k] = 0.f;
    A.gb1 = A.gb2 = A.s0 = A.s1 = 0.f;
#pragma unroll
    for (int o = 0; o < NO; ++o) A.gw3[o] = A.gb3[o] = 0.f;
#pragma unroll
    for (int i = 0; i < NBW; ++i)
#pragma unroll
        for (int q = 0; q < 16; ++q) A.dw2[i][q] = 0.f;
}

// back-propagation of l_g[o][m] (NO rows of M3T floats, zero past the batch) through the network whose a1 / a2 the forward pass left
// in LDS.  FULL: every parameter gradient into A (an accumulator of NO output rows); otherwise only dz1 (left in place of a1), for
// the pull-back to the action input, and A -- of any shape -- is not touched.  Needs a barrier before its first statement only if
// l_g was written after the forward pass's last one; ends WITHOUT a barrier
template <int ACT, int NBW, bool FULL, int NO = 1, class ACC>
__device__ __forceinline__ void td3m_backward(const Td3mNet& N, int h, const float (*l_x)[M3XS], const float* l_g, float* l_a1, float* l_a2,
                                              float* l_wt, ACC& A) {
    const int tid = threadIdx.x, P = h + 1, HB = h / 32;
    const int lane = tid & 63, wave = tid >> 6, c = lane & 31, kb = lane >> 5;
    if (tid < h) {  // dz2[m][j] in place of a2[m][j]; dW3[o, j] and db2[j] over m ascending
        if constexpr (NO == 1) {
            const float w3 = N.W3[tid];
#pragma unroll 4
            for (int m = 0; m < M3T; ++m) {
                const float hv = l_a2[m * P + tid], g = l_g[m];
                const float dz = (g * w3) * act_bwd_t<ACT>(hv, hv);
                if (FULL) A.gw3[0] = fmaf(g, hv, A.gw3[0]), A.gb2 += dz;
                l_a2[m * P + tid] = dz;
            }
        } else {
            const float w30 = N.W3[2 * tid], w31 = N.W3[2 * tid + 1];
#pragma unroll 4
            for (int m = 0; m < M3T; ++m) {
                const float hv = l_a2[m * P + tid], g0 = l_g[m], g1 = l_g[M3T + m];
                const float dz = fmaf(g1, w31, fmaf(g0, w30, 0.0f)) * act_bwd_t<ACT>(hv, hv);
                if (FULL) A.gw3[0] = fmaf(g0, hv, A.gw3[0]), A.gw3[1] = fmaf(g1, hv, A.gw3[1]), A.gb2 += dz;
                l_a2[m * P + tid] = dz;
            }
        }
    }
    if (FULL && tid == 0)
        for (int m = 0; m < M3T; ++m) {
            A.gb3[0] += l_g[m];
            if constexpr (NO == 2) A.gb3[1] += l_g[M3T + m];
        }
    __syncthreads();
    __builtin_amdgcn_sched_barrier(0);  // (no operand of another phase in flight across the dW2 accumulators)
    if (FULL) {  // dW2 block (jb, kk): A[row = unit j][k = sample m] = dz2[m][j], B[k = m][n = unit k'] = a1[m][k'], m = 2 ks + kb
#pragma unroll
        for (int i = 0; i < NBW; ++i) {
            const int blk = wave + 8 * (i * (int)gridDim.z + (int)blockIdx.z);
            if (blk < HB * HB) {
                const int jb = blk / HB, kk = blk - jb * HB;
                const float* ap = l_a2 + kb * P + jb * 32 + c;
                const float* bp = l_a1 + kb * P + kk * 32 + c;
#pragma unroll 4
                for (int ks = 0; ks < M3T / 2; ++ks) A.dw2[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[2 * ks * P], bp[2 * ks * P], A.dw2[i], 0, 0, 0);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    // da1[m][k'] = sum over j ascending of dz2[m][j] W2[j, k']: wave w owns the block k' = 32 w + c; W2 rows 32 sl .. + 31 -> l_wt[jl][k']
    f32x16 d;
#pragma unroll
    for (int q = 0; q < 16; ++q) d[q] = 0.f;
    for (int sl = 0; sl < HB; ++sl) {
        for (int q = tid; q < 32 * h; q += M3NT) {
            const int jl = q & 31, k2 = q >> 5;
            l_wt[jl * P + k2] = N.W2[32 * sl + jl + (int64_t)h * k2];
        }
        __syncthreads();
        if (wave < HB) {
            const float* ap = l_a2 + c * P + 32 * sl + kb;
            const float* bp = l_wt + kb * P + wave * 32 + c;
#pragma unroll 4
            for (int ks = 0; ks < 16; ++ks) d = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[2 * ks], bp[2 * ks * P], d, 0, 0, 0);
        }
        __syncthreads();  // (the last one: every wave is done with a1 as the B operand of dW2)
    }
    if (wave < HB) {
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            float* p = l_a1 + mfma_row(q, kb) * P + wave * 32 + c;
            const float hv = *p;
            *p = d[q] * act_bwd_t<ACT>(hv, hv);
        }
    }
    __syncthreads();
    if (FULL && tid < h) {  // dW1[j, k] and db1[j] over m ascending
#pragma unroll 4
        for (int m = 0; m < M3T; ++m) {
            const float dz = l_a1[m * P + tid];
            A.gb1 += dz;
#pragma unroll
            for (int k = 0; k < 5; ++k)
                if (k < N.ni) A.gw1[k] = fmaf(dz, l_x[m][k], A.gw1[k]);
        }
    }
}

// the workgroup's partial row of the network (ni, h, NO): the flat layout of the network itself
template <int NBW, int NO>
__device__ __forceinline__ void td3m_store_row(const Td3mAcc<NBW, NO>& A, int ni, int h, float* out) {
    const int tid = threadIdx.x, HB = h / 32;
    const int lane = tid & 63, wave = tid >> 6, c = lane & 31, kb = lane >> 5;
    const int ob1 = h * ni, oW2 = ob1 + h, ob2 = oW2 + h * h, oW3 = ob2 + h;
    if (tid < h && blockIdx.z == 0) {
#pragma unroll
        for (int k = 0; k < 5; ++k)
            if (k < ni) out[tid + h * k] = A.gw1[k];
        out[ob1 + tid] = A.gb1, out[ob2 + tid] = A.gb2;
#pragma unroll
        for (int o = 0; o < NO; ++o) out[oW3 + o + NO * tid] = A.gw3[o];
        if (tid == 0) {
#pragma unroll
            for (int o = 0; o < NO; ++o) out[oW3 + NO * h + o] = A.gb3[o];
        }
    }
#pragma unroll
    for (int i = 0; i < NBW; ++i) {
        const int blk = wave + 8 * (i * (int)gridDim.z + (int)blockIdx.z);
        if (blk < HB * HB) {
            const int jb = blk / HB, kk = blk - jb * HB;
#pragma unroll
            for (int q = 0; q < 16; ++q) out[oW2 + jb * 32 + mfma_row(q, kb) + h * (kk * 32 + c)] = A.dw2[i][q];
        }
    }
}

// the dynamic LDS: `slots` network slots, then `nbuf` tiles of 32 x (h + 1)
__host__ __device__ __forceinline__ size_t td3m_lds_bytes(int h, int slots, int nbuf) {
    return sizeof(float) * ((size_t)slots * td3m_slot_floats(h) + (size_t)nbuf * M3T * (h + 1));
}

// the body of the critic gradient launch: workgroup (x, y, z) = (tile group, critic, half of the dW2 blocks above h = 128); reads the
// TD targets the target launch left in g.ybuf.  One __global__ per object wraps it (td3m_critic_grad_kernel, sacm_critic_grad_kernel)
template <int ACT, int NBW>
__device__ __forceinline__ void td3m_critic_grad_body(const Td3mArgs g, float* m3_dyn, Td3mTile& t) {
    const int tid = threadIdx.x, h = g.h, ni = g.ns + 1, crit = blockIdx.y;
    const int64_t npq = td3m_nparams(ni, h);
    float* l_a1 = m3_dyn + td3m_slot_floats(h);
    float* l_a2 = l_a1 + M3T * (h + 1);
    float* l_wt = l_a2 + M3T * (h + 1);
    const Td3mNet Q = td3m_stage(g.critics + crit * npq, ni, h, m3_dyn);
    Td3mAcc<NBW> A;
    td3m_zero(A);
    for (int tile = blockIdx.x; tile < g.num_tiles; tile += gridDim.x) {
        const int64_t b0 = (int64_t)tile * M3T;
        const int cnt = (int)(g.batch - b0 < M3T ? g.batch - b0 : M3T);
        td3m_gather(g, tile, false, t);
        td3m_forward<ACT, false>(Q, h, t.x, l_a1, l_a2, t.out[0]);
        if (tid < M3T) {
            const float d = t.out[0][tid] - g.ybuf[tid < cnt ? b0 + tid : b0];
            t.l[tid] = d * d;
            t.g[tid] = tid < cnt ? (2.0f * d) / g.fb : 0.0f;
        }
        __syncthreads();
        if (tid == 0)
            for (int m = 0; m < cnt; ++m) A.s0 += t.l[m];
        td3m_backward<ACT, NBW, true>(Q, h, t.x, t.g, l_a1, l_a2, l_wt, A);
        __syncthreads();
    }
    td3m_store_row(A, ni, h, g.partials + (int64_t)blockIdx.x * g.np + crit * npq);
    if (tid == 0 && blockIdx.z == 0) g.stat_partials[blockIdx.x * M3STATS + crit] = A.s0;
}

// partial rows of np floats each: one per tile, at most 256, at most 16 MiB
static int td3m_blocks(int64_t batch, int64_t np) {
    const int64_t tiles = (batch + M3T - 1) / M3T, cap = M3ROWBYTES / (np * (int64_t)sizeof(float));
    const int64_t nb = tiles < M3MAXB ? tiles : M3MAXB;
    return (int)(nb < cap ? nb : cap);
}

// (one static word per kernel instantiation: the opt-in is for the largest net of the envelope)
#define TD3M_LAUNCH(KERNEL, grid, slots, nbuf, st, ...)                                                   \
    do {                                                                                                  \
        static unsigned long long done = 0;                                                               \
        const int32_t rc_ = allow_big_lds(KERNEL, td3m_lds_bytes(M3HMAX, slots, nbuf), &done);            \
        if (rc_) return rc_;                                                                              \
        hipLaunchKernelGGL(KERNEL, grid, dim3(M3NT), td3m_lds_bytes((int)h, slots, nbuf), st, __VA_ARGS__); \
    } while (0)

// the dW2 accumulator blocks per wave: (h / 32)^2 over eight waves is up to 2 at h <= 128 and up to 8 above.  Eight blocks (128
// accumulator registers) beside the rest of the tile's state spilled 39 .. 55 registers to scratch at 512 threads, so above h = 128
// TWO workgroups (grid z) share a partial row: both run the whole tile pass, each carries every second group of eight blocks (4 per
// wave), z = 0 stores everything that is not dW2.  No chain changes
#define TD3M_DISPATCH_GRAD(KERNEL, gx, gy, slots, st, g)                                              \
    do {                                                                                              \
        if (act == 0) {                                                                               \
            if (h <= 128) TD3M_LAUNCH((KERNEL<0, 2>), dim3(gx, gy, 1), slots, 3, st, g);              \
            else TD3M_LAUNCH((KERNEL<0, 4>), dim3(gx, gy, 2), slots, 3, st, g);                       \
        } else {                                                                                      \
            if (h <= 128) TD3M_LAUNCH((KERNEL<1, 2>), dim3(gx, gy, 1), slots, 3, st, g);              \
            else TD3M_LAUNCH((KERNEL<1, 4>), dim3(gx, gy, 2), slots, 3, st, g);                       \
        }                                                                                             \
    } while (0)

#define TD3M_REQUIRE_NET(ns, h, act)                                                                                                  \
    RLHIP_REQUIRE((ns) >= 2 && (ns) <= 4, "obs_dim must be 2..4 (frame rings and obs_dim > 4 are out of scope)");                     \
    RLHIP_REQUIRE((h) >= 32 && (h) <= M3HMAX && (h) % 32 == 0, "hidden must be a multiple of 32 in 32..256 (unit blocks of the "      \
                                                               "32x32x2 MFMA)");                                                       \
    RLHIP_REQUIRE((act) == 0 || (act) == 1, "act must be 0 (relu) or 1 (tanh)")

}  // namespace rlhip
