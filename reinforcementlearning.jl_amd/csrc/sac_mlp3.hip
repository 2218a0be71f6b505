// sac_mlp3.hip -- Soft Actor-Critic with TWO hidden layers (256-256 in the SAC paper and in every common implementation): plan! and the
// two gradients of an update for actor = mlp3(ns, h, 2) (output row 0 mu, row 1 rho = the pre-softplus sigma) and critics = [Q1 | Q2],
// each mlp3(ns + 1, h, 1) on vcat(s, u), flat as rlhip_mlp3_nparams / rlhip_mlp3_init_f32 lay them out, Float32 throughout.  The
// per-sample mathematics is that of csrc/sac.hip, the tile passes are those of csrc/td3_mlp3.hip (csrc/td3_mlp3_device.h, here also
// at TWO output rows); include/rlhip.h ("SAC with two hidden layers") states every chain and order, tests/sac_mlp3_ref.py is its
// Float64 model.
//
// A tile is 32 samples, a workgroup 512 threads.  At two outputs layer 3 is one 16-lane DPP row per (sample, output) in the gradient
// launches and ONE ascending chain per (env, output) in plan!; the backward enters layer 2 with
// dz2 = fmaf(drho, W3[1, j], fmaf(dmu, W3[0, j], 0)) * act' and carries dW3[o, j] / db3[o] as one chain per output.
//   sacm_plan_kernel          a tile of 32 envs: the actor forward, then the SoftGaussian head in one lane per env
//   sacm_target_kernel        forward only: the actor at s', the head on draw 0, Qt1, Qt2 -> y into the workspace
//   sacm_critic_grad_kernel   the (tile group, critic, dW2 half) launch of the TD3 learner (td3m_critic_grad_body) against that y
//   sacm_actor_grad_kernel    per tile: actor forward and the head on draw 1; Q1 forward and the pull-back of dq to its action input;
//                             the same for Q2 IN THE SAME LDS TILES; only then sel = Q2 < Q1 and du = sel == 2 ? du2 : du1 (a select:
//                             the samples of one tile go through different critics, and the activations of both do not fit the LDS at
//                             h = 256, so every sample is pulled back through both and no critic is forwarded a third time); the
//                             head's reparameterised pullback, one lane per sample; the actor forward AGAIN (bit for bit, as the TD3
//                             launch does for lack of LDS) and the full two-cotangent backward.  Three network slots and three tiles
//                             of 32 x (h + 1): 120.4 KB of dynamic LDS at h = 256
//   sacm_reduce_kernel        the fixed-order fold, three statistics and the alpha step
// No float atomics anywhere: two calls on the same inputs give the same bytes.
#include "td3_mlp3_device.h"

namespace rlhip {

constexpr int SM3STATS = 4;  // partial sums per workgroup of the actor launch (loss, q, logp)

struct SacmArgs {
    Td3mArgs b;          // ring, idx, networks, workspace, batch, shape, gamma, scale, fb, seed, step, y_out
    const float* alpha;  // device f32[1]
    float min_sigma, max_sigma;
    int32_t* sel_out;    // actor launch, nullable
    float* logp_out;     // actor launch, nullable
};

// the SoftGaussianNetwork head at d = 1 (heads.hip HeadLogp<1>), from the actor's two outputs and one draw: csrc/sac.hip's SacHead
struct SacmHead {
    float raw, sg, z, a, logp;
    bool pass;
    __device__ __forceinline__ SacmHead(float mu, float rho, float eps, float lo, float hi) {
        raw = softplus_nnlib(rho);
        sg = clampj(raw, lo, hi);
        pass = !(raw > hi) && !(raw < lo);
        z = mu + sg * eps;
        a = tanhf(z);
        logp = normlogpdf1(mu, sg, z) - 2.0f * ((0.6931472f - z) - softplus_nnlib(-2.0f * z));
    }
};

// ---- launch 1 of the critic update: u', logp' and y of every sample, forward only
template <int ACT>
__global__ __launch_bounds__(M3NT) void sacm_target_kernel(SacmArgs sa) {
    extern __shared__ __attribute__((aligned(16))) float m3_dyn[];
    __shared__ Td3mTile t;
    const Td3mArgs& g = sa.b;
    const int tid = threadIdx.x, h = g.h, ns = g.ns, sf = td3m_slot_floats(h);
    float* l_a1 = m3_dyn + 3 * sf;
    float* l_a2 = l_a1 + M3T * (h + 1);
    const Td3mNet actor = td3m_stage<2>(g.actor, ns, h, m3_dyn);
    Td3mNet qt[2];
#pragma unroll
    for (int c = 0; c < 2; ++c) qt[c] = td3m_stage(g.targets + c * td3m_nparams(ns + 1, h), ns + 1, h, m3_dyn + (1 + c) * sf);
    const float alpha = sa.alpha[0];
    for (int tile = blockIdx.x; tile < g.num_tiles; tile += gridDim.x) {
        const int64_t b0 = (int64_t)tile * M3T;
        const int cnt = (int)(g.batch - b0 < M3T ? g.batch - b0 : M3T);
        td3m_gather(g, tile, true, t);
        td3m_forward<ACT, false, 2>(actor, h, t.x, l_a1, l_a2, t.out[0]);  // mu -> out[0], rho -> out[1]
        if (tid < M3T) {  // the head at s' on draw 0 of batch position b0 + tid
            const SacmHead hd(t.out[0][tid], t.out[1][tid], normal_draw(g.seed, (uint32_t)(b0 + tid), g.step, 0), sa.min_sigma, sa.max_sigma);
            t.x[tid][ns] = g.scale * hd.a;
            t.e[tid] = hd.logp;
        }
#pragma unroll
        for (int c = 0; c < 2; ++c) td3m_forward<ACT, false>(qt[c], h, t.x, l_a1, l_a2, t.out[1 + c]);
        if (tid < cnt) {
            const float q1 = t.out[1][tid], q2 = t.out[2][tid];
            const float qt_min = q2 < q1 ? q2 : q1;
            const float y = t.r[tid] + (g.gamma * t.cont[tid]) * (qt_min - alpha * t.e[tid]);
            g.ybuf[b0 + tid] = y;
            if (g.y_out) g.y_out[b0 + tid] = y;
        }
        __syncthreads();  // the next tile rewrites the tile's arrays
    }
}

// ---- launch 2: the critic gradient launch of the TD3 learner, against launch 1's y
template <int ACT, int NBW>
__global__ __launch_bounds__(M3NT) void sacm_critic_grad_kernel(Td3mArgs g) {
    extern __shared__ __attribute__((aligned(16))) float m3_dyn[];
    __shared__ Td3mTile t;
    td3m_critic_grad_body<ACT, NBW>(g, m3_dyn, t);
}

// what the actor launch keeps of every sample of the tile beside Td3mTile
struct SacmTile {
    float mu[M3T], rho[M3T], z[M3T], sg[M3T], eps[M3T], lp[M3T], du[2][M3T], d[2][M3T], st[3][M3T];
    int pass[M3T];
};

// Two dW2 accumulator blocks per wave at every h: with four (the TD3 split above h = 128) the launch spilled 13 .. 23 registers to
// scratch -- the head's draw (Float64 log / sin / cos) sits on top of the carried accumulators -- so above h = 128 FOUR workgroups
// (grid z) share a partial row, each carrying every fourth group of eight blocks.  No chain changes
template <int ACT>
__global__ __launch_bounds__(M3NT) void sacm_actor_grad_kernel(SacmArgs sa) {
    constexpr int NBW = 2;
    extern __shared__ __attribute__((aligned(16))) float m3_dyn[];
    __shared__ Td3mTile t;
    __shared__ SacmTile u;
    const Td3mArgs& g = sa.b;
    const int tid = threadIdx.x, h = g.h, ns = g.ns, sf = td3m_slot_floats(h);
    float* l_a1 = m3_dyn + 3 * sf;
    float* l_a2 = l_a1 + M3T * (h + 1);
    float* l_wt = l_a2 + M3T * (h + 1);
    const Td3mNet actor = td3m_stage<2>(g.actor, ns, h, m3_dyn);
    const int64_t npq = td3m_nparams(ns + 1, h);
    td3m_stage(g.critics, ns + 1, h, m3_dyn + sf);
    td3m_stage(g.critics + npq, ns + 1, h, m3_dyn + 2 * sf);
    const float alpha = sa.alpha[0];
    const float dlogp = alpha / g.fb, dq = -1.0f / g.fb;
    Td3mAcc<NBW, 2> A;
    td3m_zero(A);
    float s2 = 0.f;  // (the third statistic, beside A.s0 and A.s1)
    for (int tile = blockIdx.x; tile < g.num_tiles; tile += gridDim.x) {
        const int64_t b0 = (int64_t)tile * M3T;
        const int cnt = (int)(g.batch - b0 < M3T ? g.batch - b0 : M3T);
        td3m_gather(g, tile, false, t);
        td3m_forward<ACT, false, 2>(actor, h, t.x, l_a1, l_a2, t.out[0]);  // mu -> out[0], rho -> out[1]
        if (tid < M3T) {  // the head at s on draw 1 of batch position b0 + tid
            const float eps = normal_draw(g.seed, (uint32_t)(b0 + tid), g.step, 1);
            const float mu = t.out[0][tid], rho = t.out[1][tid];  // (the critics' outputs land in out[1] and out[2])
            const SacmHead hd(mu, rho, eps, sa.min_sigma, sa.max_sigma);
            u.mu[tid] = mu, u.rho[tid] = rho, u.z[tid] = hd.z, u.sg[tid] = hd.sg, u.eps[tid] = eps, u.lp[tid] = hd.logp, u.pass[tid] = hd.pass ? 1 : 0;
            t.a[tid] = hd.a;
            t.x[tid][ns] = g.scale * hd.a;
            t.g[tid] = tid < cnt ? dq : 0.0f;
        }
#pragma unroll 1  // (ONE copy of the pass in the code: ten registers fewer than two)
        for (int c = 0; c < 2; ++c) {  // Q_c(x) -> out[1 + c]; dq back to the action input of EVERY sample -> du[c]
            const Td3mNet Q = td3m_view(g.critics + c * npq, ns + 1, h, m3_dyn + (1 + c) * sf);
            td3m_forward<ACT, false>(Q, h, t.x, l_a1, l_a2, t.out[1 + c]);
            td3m_backward<ACT, NBW, false>(Q, h, t.x, t.g, l_a1, l_a2, l_wt, A);  // -> dz1 of Q_c in place of its a1
            __syncthreads();
            const int r = tid >> 4, p = tid & 15;
            float part = 0.0f;
            for (int j = p; j < h; j += 16) part = fmaf(l_a1[r * (h + 1) + j], Q.W1[j + h * ns], part);
            part = td3m_row_sum_down(part);
            if (p == 0) u.du[c][r] = part;
        }
        __syncthreads();
        if (tid < M3T) {  // the smaller critic, the loss line and the head's pullback (heads_grad.hip, soft = 1, d = 1, K = 1)
            const float q1 = t.out[1][tid], q2 = t.out[2][tid];
            const bool second = q2 < q1;
            const float q = second ? q2 : q1, du = second ? u.du[1][tid] : u.du[0][tid];
            const float dact = g.scale * du;
            const float mu = u.mu[tid], rho = u.rho[tid], eps = u.eps[tid], lp = u.lp[tid];
            const float s = u.sg[tid] + 1.0e-8f;
            const float zz = (u.z[tid] - mu) / s, w = zz / s, a = t.a[tid];
            float dz = dlogp * (2.0f * a - w);
            dz = dz + dact * (1.0f - a * a);
            const float dmu = dlogp * w + dz;
            const float dsg = dlogp * ((zz * zz - 1.0f) / s) + dz * eps;
            const float draw = u.pass[tid] ? dsg : 0.0f;
            const bool in = tid < cnt;
            u.d[0][tid] = in ? dmu : 0.0f;
            u.d[1][tid] = in ? draw * (1.0f / (1.0f + expf(-rho))) : 0.0f;
            u.st[0][tid] = alpha * lp - q;
            u.st[1][tid] = q;
            u.st[2][tid] = lp;
            if (in && blockIdx.z == 0) {
                if (sa.sel_out) sa.sel_out[b0 + tid] = second ? 2 : 1;
                if (sa.logp_out) sa.logp_out[b0 + tid] = lp;
            }
        }
        td3m_forward<ACT, false, 2>(actor, h, t.x, l_a1, l_a2, t.out[0]);  // (again: the same bits)
        if (tid == 0)
            for (int m = 0; m < cnt; ++m) A.s0 += u.st[0][m], A.s1 += u.st[1][m], s2 += u.st[2][m];
        td3m_backward<ACT, NBW, true, 2>(actor, h, t.x, u.d[0], l_a1, l_a2, l_wt, A);
        __syncthreads();
    }
    td3m_store_row(A, ns, h, g.partials + (int64_t)blockIdx.x * g.np);
    if (tid == 0 && blockIdx.z == 0) {
        float* sp = g.stat_partials + blockIdx.x * SM3STATS;
        sp[0] = A.s0, sp[1] = A.s1, sp[2] = s2;
    }
}

// the fold of csrc/sac.hip's reduce: gradient element p = four groups of partial rows, ascending inside a group, then
// ((g0 + g1) + g2) + g3; statistic q (wave q + 1 of workgroup 0) = its partial sums (`stride` apart) lane-strided, a shift-down tree,
// / batch.  The alpha step follows the mean log-probability in the lane that holds it
__global__ __launch_bounds__(256) void sacm_reduce_kernel(const float* __restrict__ partials, const float* __restrict__ stat_partials, int nb,
                                                          int np, int nstat, int stride, float* __restrict__ grad, float* __restrict__ stats,
                                                          float fb, const float* alpha, float alpha_lr, float target_entropy, float* alpha_out) {
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
        for (int b = lane; b < nb; b += 64) a += stat_partials[b * stride + q];
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) a += __shfl_down(a, off, 64);
        if (lane == 0) {
            const float m = a / fb;
            stats[q] = m;
            if (q == 2 && alpha_out != nullptr) alpha_out[0] = alpha[0] - alpha_lr * ((-m) - target_entropy);
        }
    }
}

// plan!: a tile of 32 envs per workgroup
template <int ACT>
__global__ __launch_bounds__(M3NT) void sacm_plan_kernel(const float* __restrict__ actor, int ns, int h, const float* __restrict__ obs, int64_t n,
                                                         float lo, float hi, float scale, int deterministic, uint64_t seed,
                                                         uint32_t env_id_base, uint32_t step, float* __restrict__ action_out,
                                                         float* __restrict__ logp_out, float* __restrict__ mu_out, float* __restrict__ rho_out,
                                                         float* __restrict__ raw_out) {
    extern __shared__ __attribute__((aligned(16))) float m3_dyn[];
    __shared__ float l_x[M3T][M3XS], l_o[2][M3T];
    const int tid = threadIdx.x;
    float* l_a1 = m3_dyn + td3m_slot_floats(h);
    float* l_a2 = l_a1 + M3T * (h + 1);
    const Td3mNet N = td3m_stage<2>(actor, ns, h, m3_dyn);
    const int64_t env = (int64_t)blockIdx.x * M3T + tid;
    if (tid < M3T)
        for (int k = 0; k < ns; ++k) l_x[tid][k] = env < n ? obs[(int64_t)k * n + env] : 0.0f;
    td3m_forward<ACT, true, 2>(N, h, l_x, l_a1, l_a2, l_o[0]);
    if (tid < M3T && env < n) {
        const float mu = l_o[0][tid], rho = l_o[1][tid];
        if (mu_out) mu_out[env] = mu;
        if (rho_out) rho_out[env] = rho;
        if (deterministic) {
            action_out[env] = scale * tanhf(mu);
            if (raw_out) raw_out[env] = softplus_nnlib(rho);
        } else {
            const SacmHead hd(mu, rho, normal_draw(seed, env_id_base + (uint32_t)env, step, 0), lo, hi);
            action_out[env] = scale * hd.a;
            if (logp_out) logp_out[env] = hd.logp;
            if (raw_out) raw_out[env] = hd.raw;
        }
    }
}

static bool sacm_shape_ok(int64_t ns, int64_t h) { return ns >= 2 && ns <= 4 && h >= 32 && h <= M3HMAX && h % 32 == 0; }

// the workspace: partial rows | partial sums | the TD targets
struct SacmLayout {
    int npa, npq, nba, nbq;
};
static SacmLayout sacm_layout(int64_t ns, int64_t h, int64_t batch) {
    SacmLayout L;
    L.npa = (int)td3m_nparams(ns, h, 2), L.npq = 2 * (int)td3m_nparams(ns + 1, h);
    L.nba = td3m_blocks(batch, L.npa), L.nbq = td3m_blocks(batch, L.npq);
    return L;
}

}  // namespace rlhip

using namespace rlhip;

#define SACM_REQUIRE_RING_AND_NET(rb, h, act, batch)                                                                                  \
    RLHIP_REQUIRE((rb) != nullptr, "NULL argument");                                                                                  \
    RLHIP_REQUIRE((rb)->layout == RLHIP_RING_RECORDS, "the SAC learner reads a record ring (Float32 observations, obs_dim 2..4); "   \
                                                      "frame rings and obs_dim > 4 are out of scope");                                \
    TD3M_REQUIRE_NET((rb)->obs_dim, h, act);                                                                                          \
    RLHIP_REQUIRE((batch) >= 1, "empty batch");                                                                                       \
    RLHIP_REQUIRE((rb)->len_rt >= 1, "cannot sample from an empty trajectory")

static SacmArgs sacm_args(const rlhip_ring* rb, int64_t h, const float* actor, const float* critics, const float* targets, int64_t batch,
                          const int64_t* idx, const float* alpha, float min_sigma, float max_sigma, float action_scale, uint64_t seed,
                          uint32_t step, void* workspace, int nb, int np, int stats) {
    SacmArgs sa{};
    Td3mArgs& g = sa.b;
    g.ring = {(const uint8_t*)rb->state, rb->capacity, rb->n_env, rb->head_sa};
    g.idx = idx, g.actor = actor, g.critics = critics, g.targets = targets;
    g.partials = (float*)workspace;
    g.stat_partials = g.partials + (int64_t)nb * np;
    g.ybuf = g.stat_partials + (int64_t)nb * stats;
    g.batch = batch, g.ns = (int)rb->obs_dim, g.h = (int)h, g.num_tiles = (int)((batch + M3T - 1) / M3T), g.np = np;
    g.scale = action_scale, g.fb = (float)batch, g.seed = seed, g.step = step;
    sa.alpha = alpha, sa.min_sigma = min_sigma, sa.max_sigma = max_sigma;
    return sa;
}

extern "C" {

int64_t rlhip_sac_mlp3_workspace_bytes(int64_t ns, int64_t h, int64_t batch) {
    if (!sacm_shape_ok(ns, h) || batch < 1) return -1;
    const SacmLayout L = sacm_layout(ns, h, batch);
    const int64_t ra = (int64_t)L.nba * (L.npa + SM3STATS), rq = (int64_t)L.nbq * (L.npq + M3STATS);
    return ((ra > rq ? ra : rq) + batch) * (int64_t)sizeof(float);
}

int32_t rlhip_sac_mlp3_plan_f32(const float* actor, int64_t ns, int64_t h, int32_t act, const float* obs, int64_t n, float min_sigma,
                                float max_sigma, float action_scale, int32_t deterministic, uint64_t seed, uint32_t env_id_base,
                                uint32_t step, float* action_out, float* logp_out, float* mu_out, float* rho_out, float* raw_sigma_out,
                                rlhip_stream_t stream) {
    RLHIP_REQUIRE(actor && obs && action_out, "NULL argument");
    TD3M_REQUIRE_NET(ns, h, act);
    RLHIP_REQUIRE(n >= 0, "negative env count");
    RLHIP_REQUIRE(!(deterministic && logp_out), "logp_out must be NULL with deterministic: no action is drawn");
    if (n == 0) return RLHIP_OK;
    hipStream_t st = as_stream(stream);
    const dim3 grid((unsigned)((n + M3T - 1) / M3T));
    if (act == 0)
        TD3M_LAUNCH((sacm_plan_kernel<0>), grid, 1, 2, st, actor, (int)ns, (int)h, obs, n, min_sigma, max_sigma, action_scale,
                    deterministic ? 1 : 0, seed, env_id_base, step, action_out, logp_out, mu_out, rho_out, raw_sigma_out);
    else
        TD3M_LAUNCH((sacm_plan_kernel<1>), grid, 1, 2, st, actor, (int)ns, (int)h, obs, n, min_sigma, max_sigma, action_scale,
                    deterministic ? 1 : 0, seed, env_id_base, step, action_out, logp_out, mu_out, rho_out, raw_sigma_out);
    RLHIP_LAUNCH_CHECK();
    return RLHIP_OK;
}

int32_t rlhip_sac_mlp3_critic_grad_f32(const rlhip_ring* rb, int64_t h, int32_t act, const float* actor, const float* critics,
                                       const float* targets, int64_t batch, const int64_t* idx, const float* alpha, float gamma,
                                       float min_sigma, float max_sigma, float action_scale, uint64_t seed, uint32_t step, void* workspace,
                                       float* grad_out, float* loss_out, float* y_out, rlhip_stream_t stream) {
    SACM_REQUIRE_RING_AND_NET(rb, h, act, batch);
    RLHIP_REQUIRE(actor && critics && targets && idx && alpha && workspace && grad_out && loss_out, "NULL argument");
    RLHIP_CHECK_GATHER_INDICES(rb, idx, batch, stream);
    hipStream_t st = as_stream(stream);
    const SacmLayout L = sacm_layout(rb->obs_dim, h, batch);
    const int np = L.npq, nb = L.nbq;
    SacmArgs sa = sacm_args(rb, h, actor, critics, targets, batch, idx, alpha, min_sigma, max_sigma, action_scale, seed, step, workspace, nb,
                            np, M3STATS);
    sa.b.gamma = gamma, sa.b.y_out = y_out;
    const dim3 tgrid((unsigned)(sa.b.num_tiles < M3MAXB ? sa.b.num_tiles : M3MAXB));
    if (act == 0) TD3M_LAUNCH((sacm_target_kernel<0>), tgrid, 3, 2, st, sa);
    else TD3M_LAUNCH((sacm_target_kernel<1>), tgrid, 3, 2, st, sa);
    RLHIP_LAUNCH_CHECK();
    const Td3mArgs g = sa.b;
    TD3M_DISPATCH_GRAD(sacm_critic_grad_kernel, nb, 2, 1, st, g);
    RLHIP_LAUNCH_CHECK();
    hipLaunchKernelGGL(sacm_reduce_kernel, dim3((np + 63) / 64), dim3(256), 0, st, g.partials, g.stat_partials, nb, np, 2, M3STATS, grad_out,
                       loss_out, g.fb, nullptr, 0.0f, 0.0f, nullptr);
    RLHIP_LAUNCH_CHECK();
    return RLHIP_OK;
}

int32_t rlhip_sac_mlp3_actor_grad_f32(const rlhip_ring* rb, int64_t h, int32_t act, const float* actor, const float* critics, int64_t batch,
                                      const int64_t* idx, const float* alpha, float min_sigma, float max_sigma, float action_scale,
                                      uint64_t seed, uint32_t step, float alpha_lr, float target_entropy, float* alpha_out, void* workspace,
                                      float* grad_out, float* stats_out, int32_t* sel_out, float* logp_out, rlhip_stream_t stream) {
    SACM_REQUIRE_RING_AND_NET(rb, h, act, batch);
    RLHIP_REQUIRE(actor && critics && idx && alpha && workspace && grad_out && stats_out, "NULL argument");
    RLHIP_CHECK_GATHER_INDICES(rb, idx, batch, stream);
    hipStream_t st = as_stream(stream);
    const SacmLayout L = sacm_layout(rb->obs_dim, h, batch);
    const int np = L.npa, nb = L.nba;
    SacmArgs sa = sacm_args(rb, h, actor, critics, nullptr, batch, idx, alpha, min_sigma, max_sigma, action_scale, seed, step, workspace, nb,
                            np, SM3STATS);
    sa.sel_out = sel_out, sa.logp_out = logp_out;
    const dim3 grid(nb, 1, h <= 128 ? 1 : 4);
    if (act == 0) TD3M_LAUNCH((sacm_actor_grad_kernel<0>), grid, 3, 3, st, sa);
    else TD3M_LAUNCH((sacm_actor_grad_kernel<1>), grid, 3, 3, st, sa);
    RLHIP_LAUNCH_CHECK();
    const bool step_alpha = alpha_lr > 0.0f && alpha_out != nullptr;
    hipLaunchKernelGGL(sacm_reduce_kernel, dim3((np + 63) / 64), dim3(256), 0, st, sa.b.partials, sa.b.stat_partials, nb, np, 3, SM3STATS,
                       grad_out, stats_out, sa.b.fb, alpha, alpha_lr, target_entropy, step_alpha ? alpha_out : nullptr);
    RLHIP_LAUNCH_CHECK();
    return RLHIP_OK;
}

}  // extern "C"
