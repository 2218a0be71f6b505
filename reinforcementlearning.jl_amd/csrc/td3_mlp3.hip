// td3_mlp3.hip -- TD3 and DDPG with TWO hidden layers (256-256 in the TD3 paper's code, 400-300 in the DDPG paper): plan! and the two
// gradients of an update for actor = mlp3(ns, h, 1) and critics = [Q1 | Q2], each mlp3(ns + 1, h, 1) on vcat(s, u), flat as
// rlhip_mlp3_nparams / rlhip_mlp3_init_f32 lay them out (W1 | b1 | W2 (h x h, column-major) | b2 | W3 | b3), Float32 throughout.
// The update is the one of csrc/td3.hip; include/rlhip.h ("TD3 and DDPG with two hidden layers") states every chain and order, and
// tests/td3_mlp3_ref.py is its Float64 model.
//
// With a hidden x hidden layer a matrix instruction fits.  A tile is 32 samples (the M of v_mfma_f32_32x32x2_f32), a workgroup 512
// threads (eight waves):
//   layer 1    VALU: thread = (sample, unit), z1 = b1[j], fmaf(W1[j, k], x[k], .) over k ascending; a1 -> LDS [sample][h + 1] (the A image)
//   layer 2    MFMA: wave w owns the unit block w (h / 32 <= 8 blocks), b2[j] is the accumulator's initial value, h / 2 k-steps; A from the
//              LDS image, B = W2[j + h k] STRAIGHT FROM GLOBAL MEMORY: one coalesced 128-byte row per half-wave and k-step, L2-resident
//              after the first workgroup (W2 at h = 256 is 256 KB and does not fit the LDS beside the tiles; streaming it through LDS
//              slabs would put two barriers per slab on the chain for an operand every lane reads exactly once)
//   layer 3    VALU: gradient launches: one 16-lane DPP row per sample, lane p the units p, p + 16, .., a shift-down tree, + b3;
//              plan!: ONE ascending chain per env
//   backward   dz2 (in place of a2), dW3, db2 per unit over the tile's samples ascending; dW2[j, k] = sum_m dz2[m][j] a1[m][k] on the
//              MFMA with the SAMPLE as the k dimension, the (h / 32)^2 accumulator blocks dealt round-robin over the eight waves and
//              carried in registers across the workgroup's tiles (above h = 128 two workgroups share a row, 64 accumulator registers per
//              lane each: see TD3M_DISPATCH_GRAD); da1 = dz2 W2 on the
//              MFMA, the transposed read of W2 staged through an LDS slab of 32 rows (coalesced in global memory, conflict-free in
//              LDS); dz1 in place of a1; dW1 / db1 per unit over the samples ascending
// One workgroup cannot carry both critics' dW2, so the critic update is THREE launches on the stream: td3m_target_kernel (forward only:
// actor target, Qt1, Qt2 -> e, u', y into the workspace), td3m_critic_grad_kernel on a (tile group, critic) grid, td3m_reduce_kernel.
// The actor launch forwards the actor, forwards Q1, pulls -1/fb back through Q1 to the action input (no dW product), forwards the
// actor AGAIN (bit for bit; five activation tiles of h = 256 do not fit 160 KB) and back-propagates dmu through it.
// No float atomics anywhere: two calls on the same inputs give the same bytes.
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

__host__ __device__ __forceinline__ int64_t td3m_nparams(int64_t ni, int64_t h) { return h * ni + h + h * h + h + h + 1; }

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
    float b3;
    int ni;
};
__host__ __device__ __forceinline__ int td3m_slot_floats(int h) { return h * 8 + 4; }  // ni <= 5: h ni + h + 2 h + 1
__device__ __forceinline__ Td3mNet td3m_stage(const float* __restrict__ P, int ni, int h, float* slot) {
    const int n1 = h * ni + h, n2 = 2 * h;
    const float* P2 = P + n1 + h * h;
    for (int q = threadIdx.x; q < n1; q += M3NT) slot[q] = P[q];
    for (int q = threadIdx.x; q < n2; q += M3NT) slot[n1 + q] = P2[q];
    Td3mNet v;
    v.W1 = slot, v.b1 = slot + h * ni, v.b2 = slot + n1, v.W3 = v.b2 + h, v.W2 = P + n1, v.b3 = P2[n2], v.ni = ni;
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

// out[m] = mlp3(ni, h, 1)(x[m]) for the tile's 32 rows; leaves a1 and a2 of the tile in LDS, rows h + 1 floats apart.  Opens with a
// barrier (the caller's writes of x and of the staged slots) and closes with one (l_out)
template <int ACT, bool CHAIN3>
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
    if (CHAIN3) {
        if (tid < M3T) {
            float o = N.b3;
            for (int j = 0; j < h; ++j) o = fmaf(N.W3[j], l_a2[tid * P + j], o);
            l_out[tid] = o;
        }
    } else {
        const int r = tid >> 4, p = tid & 15;
        float part = 0.0f;
        for (int j = p; j < h; j += 16) part = fmaf(N.W3[j], l_a2[r * P + j], part);
        part = td3m_row_sum_down(part);
        if (p == 0) l_out[r] = part + N.b3;
    }
    __syncthreads();
}

// what a workgroup carries across its tiles: thread j < h the chains of unit j, thread 0 the scalars, every wave its dW2 blocks
template <int NBW>
struct Td3mAcc {
    float gw1[5], gb1, gb2, gw3, gb3, s0, s1;
    f32x16 dw2[NBW];
};
template <int NBW>
__device__ __forceinline__ void td3m_zero(Td3mAcc<NBW>& A) {
#pragma unroll
    for (int k = 0; k < 5; ++k) A.gw1[k] = 0.f;
    A.gb1 = A.gb2 = A.gw3 = A.gb3 = A.s0 = A.s1 = 0.f;
#pragma unroll
    for (int i = 0; i < NBW; ++i)
#pragma unroll
        for (int q = 0; q < 16; ++q) A.dw2[i][q] = 0.f;
}

// back-propagation of l_g[m] (zero past the batch) through the network whose a1 / a2 the forward pass left in LDS.  FULL: every
// parameter gradient into A; otherwise only dz1 (left in place of a1), for the pull-back to the action input.  Needs a barrier
// before its first statement only if l_g was written after the forward pass's last one; ends WITHOUT a barrier
template <int ACT, int NBW, bool FULL>
__device__ __forceinline__ void td3m_backward(const Td3mNet& N, int h, const float (*l_x)[M3XS], const float* l_g, float* l_a1, float* l_a2,
                                              float* l_wt, Td3mAcc<NBW>& A) {
    const int tid = threadIdx.x, P = h + 1, HB = h / 32;
    const int lane = tid & 63, wave = tid >> 6, c = lane & 31, kb = lane >> 5;
    if (tid < h) {  // dz2[m][j] in place of a2[m][j]; dW3[j] and db2[j] over m ascending
        const float w3 = N.W3[tid];
#pragma unroll 4
        for (int m = 0; m < M3T; ++m) {
            const float hv = l_a2[m * P + tid], g = l_g[m];
            const float dz = (g * w3) * act_bwd_t<ACT>(hv, hv);
            if (FULL) A.gw3 = fmaf(g, hv, A.gw3), A.gb2 += dz;
            l_a2[m * P + tid] = dz;
        }
    }
    if (FULL && tid == 0)
        for (int m = 0; m < M3T; ++m) A.gb3 += l_g[m];
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

// the workgroup's partial row of the network (ni, h): the flat layout of the network itself
template <int NBW>
__device__ __forceinline__ void td3m_store_row(const Td3mAcc<NBW>& A, int ni, int h, float* out) {
    const int tid = threadIdx.x, HB = h / 32;
    const int lane = tid & 63, wave = tid >> 6, c = lane & 31, kb = lane >> 5;
    const int ob1 = h * ni, oW2 = ob1 + h, ob2 = oW2 + h * h, oW3 = ob2 + h;
    if (tid < h && blockIdx.z == 0) {
#pragma unroll
        for (int k = 0; k < 5; ++k)
            if (k < ni) out[tid + h * k] = A.gw1[k];
        out[ob1 + tid] = A.gb1, out[ob2 + tid] = A.gb2, out[oW3 + tid] = A.gw3;
        if (tid == 0) out[oW3 + h] = A.gb3;
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

// ---- launch 1 of the critic update: e, u' and y of every sample, forward only
template <int ACT, int NC>
__global__ __launch_bounds__(M3NT) void td3m_target_kernel(Td3mArgs g) {
    extern __shared__ __attribute__((aligned(16))) float m3_dyn[];
    __shared__ Td3mTile t;
    const int tid = threadIdx.x, h = g.h, ns = g.ns, sf = td3m_slot_floats(h);
    float* l_a1 = m3_dyn + (1 + NC) * sf;
    float* l_a2 = l_a1 + M3T * (h + 1);
    const Td3mNet actor = td3m_stage(g.actor, ns, h, m3_dyn);
    Td3mNet qt[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) qt[c] = td3m_stage(g.targets + c * td3m_nparams(ns + 1, h), ns + 1, h, m3_dyn + (1 + c) * sf);
    for (int tile = blockIdx.x; tile < g.num_tiles; tile += gridDim.x) {
        const int64_t b0 = (int64_t)tile * M3T;
        const int cnt = (int)(g.batch - b0 < M3T ? g.batch - b0 : M3T);
        td3m_gather(g, tile, true, t);
        if (tid >= 64 && tid < 64 + M3T) {  // wave 1: the clipped target noise of batch position b0 + smp
            const int smp = tid - 64;
            float e = 0.0f;
            if (g.target_noise != 0.0f)
                e = clampj(g.target_noise * normal_draw(g.seed, (uint32_t)(b0 + smp), g.step, 0), -g.noise_clip, g.noise_clip);
            t.e[smp] = e;
            if (g.noise_out && smp < cnt) g.noise_out[b0 + smp] = e;
        }
        td3m_forward<ACT, false>(actor, h, t.x, l_a1, l_a2, t.out[0]);
        if (tid < M3T) t.x[tid][ns] = clampj(g.scale * tanhf(t.out[0][tid]) + t.e[tid], g.lo, g.hi);
#pragma unroll
        for (int c = 0; c < NC; ++c) td3m_forward<ACT, false>(qt[c], h, t.x, l_a1, l_a2, t.out[1 + c]);
        if (tid < cnt) {
            float q = t.out[1][tid];
            if (NC == 2) {
                const float q2 = t.out[2][tid];
                q = q2 < q ? q2 : q;
            }
            const float y = t.r[tid] + (g.gamma * t.cont[tid]) * q;
            g.ybuf[b0 + tid] = y;
            if (g.y_out) g.y_out[b0 + tid] = y;
        }
        __syncthreads();  // the next tile rewrites the tile's arrays
    }
}

// ---- launch 2: workgroup (x, y, z) = (tile group, critic, half of the dW2 blocks above h = 128)
template <int ACT, int NBW>
__global__ __launch_bounds__(M3NT) void td3m_critic_grad_kernel(Td3mArgs g) {
    extern __shared__ __attribute__((aligned(16))) float m3_dyn[];
    __shared__ Td3mTile t;
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

template <int ACT, int NBW>
__global__ __launch_bounds__(M3NT) void td3m_actor_grad_kernel(Td3mArgs g) {
    extern __shared__ __attribute__((aligned(16))) float m3_dyn[];
    __shared__ Td3mTile t;
    const int tid = threadIdx.x, h = g.h, ns = g.ns, sf = td3m_slot_floats(h);
    float* l_a1 = m3_dyn + 2 * sf;
    float* l_a2 = l_a1 + M3T * (h + 1);
    float* l_wt = l_a2 + M3T * (h + 1);
    const Td3mNet actor = td3m_stage(g.actor, ns, h, m3_dyn);
    const Td3mNet Q = td3m_stage(g.critics, ns + 1, h, m3_dyn + sf);
    const float dq = -1.0f / g.fb;
    Td3mAcc<NBW> A;
    td3m_zero(A);
    for (int tile = blockIdx.x; tile < g.num_tiles; tile += gridDim.x) {
        const int64_t b0 = (int64_t)tile * M3T;
        const int cnt = (int)(g.batch - b0 < M3T ? g.batch - b0 : M3T);
        td3m_gather(g, tile, false, t);
        td3m_forward<ACT, false>(actor, h, t.x, l_a1, l_a2, t.out[0]);
        if (tid < M3T) {
            const float a = tanhf(t.out[0][tid]);
            t.a[tid] = a;
            t.x[tid][ns] = g.scale * a;
            t.g[tid] = tid < cnt ? dq : 0.0f;
        }
        td3m_forward<ACT, false>(Q, h, t.x, l_a1, l_a2, t.out[1]);
        if (tid == 0)
            for (int m = 0; m < cnt; ++m) A.s0 += -t.out[1][m], A.s1 += t.out[1][m];
        td3m_backward<ACT, NBW, false>(Q, h, t.x, t.g, l_a1, l_a2, l_wt, A);  // -> dz1 of Q1 in place of its a1
        __syncthreads();
        {  // du = dz1 . W1[:, ns] by the unit slices of a 16-lane row and the tree; dmu in the row's lane 0
            const int r = tid >> 4, p = tid & 15;
            float part = 0.0f;
            for (int j = p; j < h; j += 16) part = fmaf(l_a1[r * (h + 1) + j], Q.W1[j + h * ns], part);
            part = td3m_row_sum_down(part);
            if (p == 0) t.l[r] = r < cnt ? (g.scale * part) * (1.0f - t.a[r] * t.a[r]) : 0.0f;
        }
        td3m_forward<ACT, false>(actor, h, t.x, l_a1, l_a2, t.out[0]);  // (again: the same bits)
        td3m_backward<ACT, NBW, true>(actor, h, t.x, t.l, l_a1, l_a2, l_wt, A);
        __syncthreads();
    }
    td3m_store_row(A, ns, h, g.partials + (int64_t)blockIdx.x * g.np);
    if (tid == 0 && blockIdx.z == 0) g.stat_partials[blockIdx.x * M3STATS + 0] = A.s0, g.stat_partials[blockIdx.x * M3STATS + 1] = A.s1;
}

// the fold of csrc/td3.hip's reduce: gradient element p = four groups of partial rows, ascending inside a group, then
// ((g0 + g1) + g2) + g3; statistic q (wave q + 1 of workgroup 0) = its partial sums lane-strided, a shift-down tree, / batch
__global__ __launch_bounds__(256) void td3m_reduce_kernel(const float* __restrict__ partials, const float* __restrict__ stat_partials, int nb,
                                                          int np, int nstat, float* __restrict__ grad, float* __restrict__ stats, float fb) {
    __shared__ float l_g[4][64];
    const int lane = threadIdx.x & 63, grp = threadIdx.x >> 6;
    const int p = blockIdx.x * 64 + lane;
    const int per = (nb + 3) / 4;
    const int r0 = grp * per, r1 = min(nb, r0 + per);
    float acc = 0.f;
    if (p < np) {
#pragma unroll 8
        for (int b = r0; b < r1; ++b) acc += partials[(int64_t)b * np + p];
    }
    l_g[grp][lane] = acc;
    __syncthreads();
    if (grp == 0 && p < np) grad[p] = ((l_g[0][lane] + l_g[1][lane]) + l_g[2][lane]) + l_g[3][lane];
    if (blockIdx.x == 0 && grp >= 1 && grp - 1 < nstat) {
        const int q = grp - 1;
        float a = 0.f;
        for (int b = lane; b < nb; b += 64) a += stat_partials[b * M3STATS + q];
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) a += __shfl_down(a, off, 64);
        if (lane == 0) stats[q] = a / fb;
    }
}

// plan!: a tile of 32 envs per workgroup
template <int ACT>
__global__ __launch_bounds__(M3NT) void td3m_plan_kernel(const float* __restrict__ actor, int ns, int h, const float* __restrict__ obs, int64_t n,
                                                         float scale, float act_noise, float lo, float hi, int deterministic, uint64_t seed,
                                                         uint32_t env_id_base, uint32_t step, float* __restrict__ action_out,
                                                         float* __restrict__ mu_out) {
    extern __shared__ __attribute__((aligned(16))) float m3_dyn[];
    __shared__ float l_x[M3T][M3XS], l_mu[M3T];
    const int tid = threadIdx.x;
    float* l_a1 = m3_dyn + td3m_slot_floats(h);
    float* l_a2 = l_a1 + M3T * (h + 1);
    const Td3mNet N = td3m_stage(actor, ns, h, m3_dyn);
    const int64_t env = (int64_t)blockIdx.x * M3T + tid;
    if (tid < M3T)
        for (int k = 0; k < ns; ++k) l_x[tid][k] = env < n ? obs[(int64_t)k * n + env] : 0.0f;
    td3m_forward<ACT, true>(N, h, l_x, l_a1, l_a2, l_mu);
    if (tid < M3T && env < n) {
        const float mu = l_mu[tid];
        if (mu_out) mu_out[env] = mu;
        float u = scale * tanhf(mu);
        if (!deterministic) u = u + act_noise * normal_draw(seed, env_id_base + (uint32_t)env, step, 0);
        action_out[env] = clampj(u, lo, hi);
    }
}

static bool td3m_shape_ok(int64_t ns, int64_t h, int64_t nc) {
    return ns >= 2 && ns <= 4 && h >= 32 && h <= M3HMAX && h % 32 == 0 && (nc == 1 || nc == 2);
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

}  // namespace rlhip

using namespace rlhip;

#define TD3M_REQUIRE_NET(ns, h, act)                                                                                                  \
    RLHIP_REQUIRE((ns) >= 2 && (ns) <= 4, "obs_dim must be 2..4 (frame rings and obs_dim > 4 are out of scope)");                     \
    RLHIP_REQUIRE((h) >= 32 && (h) <= M3HMAX && (h) % 32 == 0, "hidden must be a multiple of 32 in 32..256 (unit blocks of the "      \
                                                               "32x32x2 MFMA)");                                                       \
    RLHIP_REQUIRE((act) == 0 || (act) == 1, "act must be 0 (relu) or 1 (tanh)")

#define TD3M_REQUIRE_RING_AND_NET(rb, h, act, batch)                                                                                  \
    RLHIP_REQUIRE((rb) != nullptr, "NULL argument");                                                                                  \
    RLHIP_REQUIRE((rb)->layout == RLHIP_RING_RECORDS, "the TD3 / DDPG learner reads a record ring (Float32 observations, obs_dim "    \
                                                      "2..4); frame rings and obs_dim > 4 are out of scope");                         \
    TD3M_REQUIRE_NET((rb)->obs_dim, h, act);                                                                                          \
    RLHIP_REQUIRE((batch) >= 1, "empty batch");                                                                                       \
    RLHIP_REQUIRE((rb)->len_rt >= 1, "cannot sample from an empty trajectory")

extern "C" {

int64_t rlhip_td3_mlp3_workspace_bytes(int64_t ns, int64_t h, int64_t n_critics, int64_t batch) {
    if (!td3m_shape_ok(ns, h, n_critics) || batch < 1) return -1;
    const int64_t npa = td3m_nparams(ns, h), npq = n_critics * td3m_nparams(ns + 1, h);
    const int64_t ra = td3m_blocks(batch, npa) * (npa + M3STATS), rq = td3m_blocks(batch, npq) * (npq + M3STATS);
    return ((ra > rq ? ra : rq) + batch) * (int64_t)sizeof(float);  // partial rows | partial sums | the TD targets
}

int32_t rlhip_td3_mlp3_plan_f32(const float* actor, int64_t ns, int64_t h, int32_t act, const float* obs, int64_t n, float action_scale,
                                float act_noise, float action_lo, float action_hi, int32_t deterministic, uint64_t seed,
                                uint32_t env_id_base, uint32_t step, float* action_out, float* mu_out, rlhip_stream_t stream) {
    RLHIP_REQUIRE(actor && obs && action_out, "NULL argument");
    TD3M_REQUIRE_NET(ns, h, act);
    RLHIP_REQUIRE(n >= 0, "negative env count");
    if (n == 0) return RLHIP_OK;
    hipStream_t st = as_stream(stream);
    const dim3 grid((unsigned)((n + M3T - 1) / M3T));
    if (act == 0)
        TD3M_LAUNCH((td3m_plan_kernel<0>), grid, 1, 2, st, actor, (int)ns, (int)h, obs, n, action_scale, act_noise, action_lo, action_hi,
                    deterministic ? 1 : 0, seed, env_id_base, step, action_out, mu_out);
    else
        TD3M_LAUNCH((td3m_plan_kernel<1>), grid, 1, 2, st, actor, (int)ns, (int)h, obs, n, action_scale, act_noise, action_lo, action_hi,
                    deterministic ? 1 : 0, seed, env_id_base, step, action_out, mu_out);
    RLHIP_LAUNCH_CHECK();
    return RLHIP_OK;
}

int32_t rlhip_td3_mlp3_critic_grad_f32(const rlhip_ring* rb, int64_t h, int32_t act, int32_t n_critics, const float* actor_target,
                                       const float* critics, const float* critic_targets, int64_t batch, const int64_t* idx, float gamma,
                                       float action_scale, float target_noise, float noise_clip, float action_lo, float action_hi,
                                       uint64_t seed, uint32_t step, void* workspace, float* grad_out, float* loss_out, float* y_out,
                                       float* noise_out, rlhip_stream_t stream) {
    TD3M_REQUIRE_RING_AND_NET(rb, h, act, batch);
    RLHIP_REQUIRE(n_critics == 1 || n_critics == 2, "n_critics must be 1 (DDPG) or 2 (TD3)");
    RLHIP_REQUIRE(actor_target && critics && critic_targets && idx && workspace && grad_out && loss_out, "NULL argument");
    RLHIP_CHECK_GATHER_INDICES(rb, idx, batch, stream);
    hipStream_t st = as_stream(stream);
    const int ns = (int)rb->obs_dim;
    const int np = n_critics * (int)td3m_nparams(ns + 1, h), nb = td3m_blocks(batch, np);
    Td3mArgs g{};
    g.ring = {(const uint8_t*)rb->state, rb->capacity, rb->n_env, rb->head_sa};
    g.idx = idx, g.actor = actor_target, g.critics = critics, g.targets = critic_targets;
    g.partials = (float*)workspace;
    g.stat_partials = g.partials + (int64_t)nb * np;
    g.ybuf = g.stat_partials + (int64_t)nb * M3STATS;
    g.batch = batch, g.ns = ns, g.h = (int)h, g.num_tiles = (int)((batch + M3T - 1) / M3T), g.np = np;
    g.gamma = gamma, g.lo = action_lo, g.hi = action_hi, g.scale = action_scale, g.fb = (float)batch;
    g.target_noise = target_noise, g.noise_clip = noise_clip;
    g.seed = seed, g.step = step, g.y_out = y_out, g.noise_out = noise_out;
    const dim3 tgrid((unsigned)(g.num_tiles < M3MAXB ? g.num_tiles : M3MAXB));
    if (n_critics == 2) {
        if (act == 0) TD3M_LAUNCH((td3m_target_kernel<0, 2>), tgrid, 3, 2, st, g);
        else TD3M_LAUNCH((td3m_target_kernel<1, 2>), tgrid, 3, 2, st, g);
    } else {
        if (act == 0) TD3M_LAUNCH((td3m_target_kernel<0, 1>), tgrid, 2, 2, st, g);
        else TD3M_LAUNCH((td3m_target_kernel<1, 1>), tgrid, 2, 2, st, g);
    }
    RLHIP_LAUNCH_CHECK();
    TD3M_DISPATCH_GRAD(td3m_critic_grad_kernel, nb, n_critics, 1, st, g);
    RLHIP_LAUNCH_CHECK();
    hipLaunchKernelGGL(td3m_reduce_kernel, dim3((np + 63) / 64), dim3(256), 0, st, g.partials, g.stat_partials, nb, np, (int)n_critics,
                       grad_out, loss_out, g.fb);
    RLHIP_LAUNCH_CHECK();
    return RLHIP_OK;
}

int32_t rlhip_td3_mlp3_actor_grad_f32(const rlhip_ring* rb, int64_t h, int32_t act, const float* actor, const float* critics, int64_t batch,
                                      const int64_t* idx, float action_scale, void* workspace, float* grad_out, float* stats_out,
                                      rlhip_stream_t stream) {
    TD3M_REQUIRE_RING_AND_NET(rb, h, act, batch);
    RLHIP_REQUIRE(actor && critics && idx && workspace && grad_out && stats_out, "NULL argument");
    RLHIP_CHECK_GATHER_INDICES(rb, idx, batch, stream);
    hipStream_t st = as_stream(stream);
    const int ns = (int)rb->obs_dim;
    const int np = (int)td3m_nparams(ns, h), nb = td3m_blocks(batch, np);
    Td3mArgs g{};
    g.ring = {(const uint8_t*)rb->state, rb->capacity, rb->n_env, rb->head_sa};
    g.idx = idx, g.actor = actor, g.critics = critics;
    g.partials = (float*)workspace;
    g.stat_partials = g.partials + (int64_t)nb * np;
    g.batch = batch, g.ns = ns, g.h = (int)h, g.num_tiles = (int)((batch + M3T - 1) / M3T), g.np = np;
    g.scale = action_scale, g.fb = (float)batch;
    TD3M_DISPATCH_GRAD(td3m_actor_grad_kernel, nb, 1, 2, st, g);
    RLHIP_LAUNCH_CHECK();
    hipLaunchKernelGGL(td3m_reduce_kernel, dim3((np + 63) / 64), dim3(256), 0, st, g.partials, g.stat_partials, nb, np, 2, grad_out,
                       stats_out, g.fb);
    RLHIP_LAUNCH_CHECK();
    return RLHIP_OK;
}

}  // extern "C"
