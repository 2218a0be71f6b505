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
#include "td3_mlp3_device.h"

namespace rlhip {

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

// ---- launch 2: workgroup (x, y, z) = (tile group, critic, half of the dW2 blocks above h = 128): td3m_critic_grad_body
template <int ACT, int NBW>
__global__ __launch_bounds__(M3NT) void td3m_critic_grad_kernel(Td3mArgs g) {
    extern __shared__ __attribute__((aligned(16))) float m3_dyn[];
    __shared__ Td3mTile t;
    td3m_critic_grad_body<ACT, NBW>(g, m3_dyn, t);
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

}  // namespace rlhip

using namespace rlhip;

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
