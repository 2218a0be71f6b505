// sac.hip -- Soft Actor-Critic on the continuous vector envs (PendulumEnv, ContinuousMountainCarEnv, CartPoleEnv(continuous)): plan! as
// one launch, and the two gradients of an update -- both critics against the soft TD target, the actor against the stepped critics --
// each as one gradient launch plus a fixed-order fold.  include/rlhip.h states the formulas, the summation order and the stream
// separation; tests/sac_ref.py replays them.
//
// Reference: the SoftGaussianNetwork head is "mainly used for SAC" (RLCore/src/utils/networks.jl:127-128); the Zoo's SACPolicy is not in
// the tree, so the update is specified by the header's text.  Actor = mlp2(ns, h, 2) (row 0 mu, row 1 rho = the pre-softplus sigma),
// critics = [Q1 | Q2], each mlp2(ns + 1, h, 1) on vcat(s, u).  K = ns + 1 <= 5 inputs and one or two outputs: VALU work.
//
//   sac_plan_kernel<NS, ACT>          one lane per env, the actor staged in LDS (broadcast reads): the chain of mlp2_forward_kernel, then
//                                     the head of heads.hip's HeadLogp<1> at d = 1 in the same lane
//   sac_critic_grad_kernel<NS, ACT>   tiles of 64 samples, 512 threads:
//   sac_actor_grad_kernel<NS, ACT>
//       phase 0   every network the launch reads -> LDS (their flat layouts); the tile's records, one lane per sample, -> LDS
//       phase 1   thread = (sample, network): the WHOLE forward pass of one network on one sample in the order of
//                 rlhip_mlp2_forward_f32 (z = b1[j], fmaf over k ascending; out = b2, fmaf over j ascending) -- every lane of a wave reads
//                 the same weight (a broadcast), and no sum crosses lanes.  First the actor (one wave), then the critics side by
//                 side (four waves: Qt1, Qt2 at x', Q1, Q2 at x; two for the actor loss, which also carry dQ/du), then the TD / head
//                 line of each sample in one lane
//       phase 2   thread = (network, hidden unit j): recomputes z[j] of each sample of the tile by the same chain (five fmaf: cheaper than
//                 a 64 x h LDS hand-over, and bit for bit phase 1's z), and carries ONE fmaf / add chain per gradient element over the
//                 workgroup's samples in ascending order, in registers across its tiles
//   sac_reduce_kernel                 the partial rows, one per workgroup, and the partial loss sums in a fixed order; the alpha step
// No float atomics anywhere: two calls on the same inputs give the same bytes.
#include "head_device.h"
#include "ring_device.h"

namespace rlhip {

constexpr int STILE = 64;
constexpr int STHREADS = 512;
constexpr int SMAX_BLOCKS = 256;  // partial rows: a larger batch gives its workgroups further tiles
constexpr int SHMAX = 256;
constexpr int SSTATS = 4;  // partial sums per workgroup beside its gradient row (2 losses; loss, q, logp)
constexpr int SNPA_MAX = SHMAX * 4 + SHMAX + 2 * SHMAX + 2;  // mlp2(4, 256, 2)
constexpr int SNPQ_MAX = SHMAX * 5 + SHMAX + SHMAX + 1;      // mlp2(5, 256, 1)

struct SacArgs {
    RingRecs ring;
    const int64_t* idx;
    const float* actor;
    const float* critics;
    const float* targets;  // critic launch only
    const float* alpha;
    float* partials;
    float* stat_partials;
    int64_t batch;
    int h, num_tiles, np;
    float gamma, lo, hi, scale, fb;
    uint64_t seed;
    uint32_t step;
    float* y_out;       // critic launch, nullable
    int32_t* sel_out;   // actor launch, nullable
    float* logp_out;    // actor launch, nullable
};

// the SoftGaussianNetwork head at d = 1 (heads.hip HeadLogp<1>), from the actor's two outputs and one draw
struct SacHead {
    float raw, sg, z, a, logp;
    bool pass;
    __device__ __forceinline__ SacHead(float mu, float rho, float eps, float lo, float hi) {
        raw = softplus_nnlib(rho);
        sg = clampj(raw, lo, hi);
        pass = !(raw > hi) && !(raw < lo);
        z = mu + sg * eps;
        a = tanhf(z);
        logp = normlogpdf1(mu, sg, z) - 2.0f * ((0.6931472f - z) - softplus_nnlib(-2.0f * z));
    }
};

// out = mlp2(NI, h, NO)(x), the flat vector P in LDS, in the order of mlp2_forward_kernel (ppo.hip).  DU: also dQ/du of a critic
// (NO = 1) through layer 2, the activation's derivative and column NI - 1 of W1, scaled by dq, as one fmaf chain over j ascending
template <int NI, int ACT, int NO, bool DU>
__device__ __forceinline__ void sac_forward(const float* P, int h, const float (&x)[NI], float (&out)[NO], float dq, float& du) {
    const float* b1 = P + h * NI;
    const float* W2 = b1 + h;
    const float* b2 = W2 + NO * h;
#pragma unroll
    for (int o = 0; o < NO; ++o) out[o] = b2[o];
    du = 0.0f;
#pragma unroll 4
    for (int j = 0; j < h; ++j) {
        float z = b1[j];
#pragma unroll
        for (int k = 0; k < NI; ++k) z = fmaf(P[j + h * k], x[k], z);
        const float hv = act_fwd_t<ACT>(z);
#pragma unroll
        for (int o = 0; o < NO; ++o) out[o] = fmaf(W2[o + NO * j], hv, out[o]);
        if (DU) {
            const float dz = (dq * W2[j]) * (ACT == 0 ? (hv > 0.0f ? 1.0f : 0.0f) : (1.0f - hv * hv));
            du = fmaf(dz, P[j + h * (NI - 1)], du);
        }
    }
}

__device__ __forceinline__ void sac_stage(float* dst, const float* src, int n) {
    for (int q = threadIdx.x; q < n; q += STHREADS) dst[q] = src[q];
}

// the records of the tile's samples -> LDS, one lane per sample (one 64-byte record = one fabric request)
struct SacTile {
    float s[STILE][4], sn[STILE][4], a[STILE], r[STILE], cont[STILE];
};
__device__ __forceinline__ void sac_gather(const SacArgs& g, int tile, SacTile& t) {
    const int tid = threadIdx.x;
    if (tid < STILE) {
        const int64_t b = (int64_t)tile * STILE + tid;
        const int64_t fj = g.idx[b < g.batch ? b : 0];
        const RingTransition rt = ring_load_transition(g.ring, fj);
#pragma unroll
        for (int k = 0; k < 4; ++k) t.s[tid][k] = rt.s[k], t.sn[tid][k] = rt.sn[k];
        t.a[tid] = __int_as_float(rt.a);  // the action word holds the bits of a Float32
        t.r[tid] = rt.r;
        t.cont[tid] = rt.t ? 0.0f : 1.0f;
    }
}

template <int NS, int ACT>
__global__ __launch_bounds__(STHREADS) void sac_critic_grad_kernel(SacArgs g) {
    constexpr int NQ = NS + 1;
    __shared__ float l_actor[SNPA_MAX], l_q[4][SNPQ_MAX];  // Q1, Q2, Qt1, Qt2
    __shared__ SacTile l_t;
    __shared__ float l_un[STILE], l_lp[STILE], l_out[4][STILE], l_g[2][STILE], l_l[2][STILE];
    const int tid = threadIdx.x, h = g.h;
    const int npa = (int)mlp2_nparams(NS, h, 2), npq = (int)mlp2_nparams(NQ, h, 1);
    sac_stage(l_actor, g.actor, npa);
    sac_stage(l_q[0], g.critics, npq);
    sac_stage(l_q[1], g.critics + npq, npq);
    sac_stage(l_q[2], g.targets, npq);
    sac_stage(l_q[3], g.targets + npq, npq);
    const float alpha = g.alpha[0];

    // phase 2: this thread's (critic, unit)
    const bool p2 = tid < 2 * h;
    const int pc = p2 ? tid / h : 0, pj = p2 ? tid - pc * h : 0;
    float gw1[NQ], gb1 = 0.f, gw2 = 0.f, gb2 = 0.f, s_loss = 0.f;
#pragma unroll
    for (int k = 0; k < NQ; ++k) gw1[k] = 0.f;

    for (int tile = blockIdx.x; tile < g.num_tiles; tile += gridDim.x) {
        const int64_t b0 = (int64_t)tile * STILE;
        const int cnt = (int)(g.batch - b0 < STILE ? g.batch - b0 : STILE);
        sac_gather(g, tile, l_t);
        __syncthreads();  // (the first tile: the staged networks too)
        // ---- phase 1a: the actor and its head at s' (draw 0 of batch position b)
        if (tid < cnt) {
            float x[NS], o[2], du;
#pragma unroll
            for (int k = 0; k < NS; ++k) x[k] = l_t.sn[tid][k];
            sac_forward<NS, ACT, 2, false>(l_actor, h, x, o, 0.0f, du);
            const SacHead hd(o[0], o[1], normal_draw(g.seed, (uint32_t)(b0 + tid), g.step, 0), g.lo, g.hi);
            l_un[tid] = g.scale * hd.a;
            l_lp[tid] = hd.logp;
        }
        __syncthreads();
        // ---- phase 1b: Q1(x), Q2(x), Qt1(x'), Qt2(x'), one wave each
        if (tid < 4 * STILE) {
            const int net = tid >> 6, smp = tid & 63;
            if (smp < cnt) {
                float x[NQ], o[1], du;
#pragma unroll
                for (int k = 0; k < NS; ++k) x[k] = net < 2 ? l_t.s[smp][k] : l_t.sn[smp][k];
                x[NS] = net < 2 ? l_t.a[smp] : l_un[smp];
                sac_forward<NQ, ACT, 1, false>(l_q[net], h, x, o, 0.0f, du);
                l_out[net][smp] = o[0];
            }
        }
        __syncthreads();
        // ---- phase 1c: the soft TD target and both squared errors of the sample
        if (tid < cnt) {
            const float qt1 = l_out[2][tid], qt2 = l_out[3][tid];
            const float qt = qt2 < qt1 ? qt2 : qt1;
            const float y = l_t.r[tid] + (g.gamma * l_t.cont[tid]) * (qt - alpha * l_lp[tid]);
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const float d = l_out[c][tid] - y;
                l_l[c][tid] = d * d;
                l_g[c][tid] = (2.0f * d) / g.fb;
            }
            if (g.y_out) g.y_out[b0 + tid] = y;
        }
        __syncthreads();
        // ---- phase 2: unit pj of critic pc over the samples of the tile in ascending order
        if (p2) {
            const float* P = l_q[pc];
            float w1[NQ];
#pragma unroll
            for (int k = 0; k < NQ; ++k) w1[k] = P[pj + h * k];
            const float pb1 = P[h * NQ + pj], pw2 = P[h * NQ + h + pj];
            for (int i = 0; i < cnt; ++i) {
                float x[NQ];
#pragma unroll
                for (int k = 0; k < NS; ++k) x[k] = l_t.s[i][k];
                x[NS] = l_t.a[i];
                float z = pb1;
#pragma unroll
                for (int k = 0; k < NQ; ++k) z = fmaf(w1[k], x[k], z);
                const float hv = act_fwd_t<ACT>(z);
                const float gi = l_g[pc][i];
                gw2 = fmaf(gi, hv, gw2);
                const float dz = (gi * pw2) * (ACT == 0 ? (hv > 0.0f ? 1.0f : 0.0f) : (1.0f - hv * hv));
                gb1 += dz;
#pragma unroll
                for (int k = 0; k < NQ; ++k) gw1[k] = fmaf(dz, x[k], gw1[k]);
                if (pj == 0) {
                    gb2 += gi;
                    s_loss += l_l[pc][i];
                }
            }
        }
        __syncthreads();  // the next tile rewrites the tile's arrays
    }
    if (p2) {
        float* out = g.partials + (int64_t)blockIdx.x * g.np + pc * npq;
#pragma unroll
        for (int k = 0; k < NQ; ++k) out[pj + h * k] = gw1[k];
        out[h * NQ + pj] = gb1;
        out[h * NQ + h + pj] = gw2;
        if (pj == 0) {
            out[h * NQ + 2 * h] = gb2;
            g.stat_partials[blockIdx.x * SSTATS + pc] = s_loss;
        }
    }
}

template <int NS, int ACT>
__global__ __launch_bounds__(STHREADS) void sac_actor_grad_kernel(SacArgs g) {
    constexpr int NQ = NS + 1;
    __shared__ float l_actor[SNPA_MAX], l_q[2][SNPQ_MAX];
    __shared__ SacTile l_t;
    __shared__ float l_u[STILE], l_out[2][STILE], l_du[2][STILE], l_d[2][STILE], l_st[3][STILE];
    const int tid = threadIdx.x, h = g.h;
    const int npa = (int)mlp2_nparams(NS, h, 2), npq = (int)mlp2_nparams(NQ, h, 1);
    sac_stage(l_actor, g.actor, npa);
    sac_stage(l_q[0], g.critics, npq);
    sac_stage(l_q[1], g.critics + npq, npq);
    const float alpha = g.alpha[0];
    const float dlogp = alpha / g.fb, dq = -1.0f / g.fb;

    const bool p2 = tid < h;
    const int pj = p2 ? tid : 0;
    float gw1[NS], gb1 = 0.f, gw2[2] = {0.f, 0.f}, gb2[2] = {0.f, 0.f}, s_st[3] = {0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < NS; ++k) gw1[k] = 0.f;

    for (int tile = blockIdx.x; tile < g.num_tiles; tile += gridDim.x) {
        const int64_t b0 = (int64_t)tile * STILE;
        const int cnt = (int)(g.batch - b0 < STILE ? g.batch - b0 : STILE);
        sac_gather(g, tile, l_t);
        __syncthreads();
        // ---- phase 1a: the actor and its head at s (draw 1 of batch position b); the lane keeps the head for phase 1c
        float mu = 0.f, rho = 0.f, eps = 0.f;
        if (tid < cnt) {
            float x[NS], o[2], du;
#pragma unroll
            for (int k = 0; k < NS; ++k) x[k] = l_t.s[tid][k];
            sac_forward<NS, ACT, 2, false>(l_actor, h, x, o, 0.0f, du);
            mu = o[0], rho = o[1];
            eps = normal_draw(g.seed, (uint32_t)(b0 + tid), g.step, 1);
        }
        const SacHead hd(mu, rho, eps, g.lo, g.hi);
        if (tid < cnt) l_u[tid] = g.scale * hd.a;
        __syncthreads();
        // ---- phase 1b: Q1(x), Q2(x) and dq dQ/du of each, one wave per critic
        if (tid < 2 * STILE) {
            const int net = tid >> 6, smp = tid & 63;
            if (smp < cnt) {
                float x[NQ], o[1], du;
#pragma unroll
                for (int k = 0; k < NS; ++k) x[k] = l_t.s[smp][k];
                x[NS] = l_u[smp];
                sac_forward<NQ, ACT, 1, true>(l_q[net], h, x, o, dq, du);
                l_out[net][smp] = o[0];
                l_du[net][smp] = du;
            }
        }
        __syncthreads();
        // ---- phase 1c: the smaller critic, the loss line and the head's pullback (heads_grad.hip, soft = 1, d = 1, K = 1)
        if (tid < cnt) {
            const float q1 = l_out[0][tid], q2 = l_out[1][tid];
            const bool second = q2 < q1;
            const float q = second ? q2 : q1, du = second ? l_du[1][tid] : l_du[0][tid];
            const float dact = g.scale * du;
            const float s = hd.sg + 1.0e-8f;
            const float zz = (hd.z - mu) / s, w = zz / s, t = hd.a;
            float dz = dlogp * (2.0f * t - w);
            dz = dz + dact * (1.0f - t * t);
            const float dmu = dlogp * w + dz;
            const float dsg = dlogp * ((zz * zz - 1.0f) / s) + dz * eps;
            const float draw = hd.pass ? dsg : 0.0f;
            l_d[0][tid] = dmu;
            l_d[1][tid] = draw * (1.0f / (1.0f + expf(-rho)));
            l_st[0][tid] = alpha * hd.logp - q;
            l_st[1][tid] = q;
            l_st[2][tid] = hd.logp;
            if (g.sel_out) g.sel_out[b0 + tid] = second ? 2 : 1;
            if (g.logp_out) g.logp_out[b0 + tid] = hd.logp;
        }
        __syncthreads();
        // ---- phase 2: actor unit pj over the samples of the tile in ascending order
        if (p2) {
            float w1[NS];
#pragma unroll
            for (int k = 0; k < NS; ++k) w1[k] = l_actor[pj + h * k];
            const float pb1 = l_actor[h * NS + pj], pw20 = l_actor[h * NS + h + 2 * pj], pw21 = l_actor[h * NS + h + 2 * pj + 1];
            for (int i = 0; i < cnt; ++i) {
                float x[NS];
#pragma unroll
                for (int k = 0; k < NS; ++k) x[k] = l_t.s[i][k];
                float z = pb1;
#pragma unroll
                for (int k = 0; k < NS; ++k) z = fmaf(w1[k], x[k], z);
                const float hv = act_fwd_t<ACT>(z);
                const float d0 = l_d[0][i], d1 = l_d[1][i];
                gw2[0] = fmaf(d0, hv, gw2[0]);
                gw2[1] = fmaf(d1, hv, gw2[1]);
                float dh = fmaf(d0, pw20, 0.0f);
                dh = fmaf(d1, pw21, dh);
                const float dz = dh * (ACT == 0 ? (hv > 0.0f ? 1.0f : 0.0f) : (1.0f - hv * hv));
                gb1 += dz;
#pragma unroll
                for (int k = 0; k < NS; ++k) gw1[k] = fmaf(dz, x[k], gw1[k]);
                if (pj == 0) {
                    gb2[0] += d0;
                    gb2[1] += d1;
#pragma unroll
                    for (int q = 0; q < 3; ++q) s_st[q] += l_st[q][i];
                }
            }
        }
        __syncthreads();
    }
    if (p2) {
        float* out = g.partials + (int64_t)blockIdx.x * g.np;
#pragma unroll
        for (int k = 0; k < NS; ++k) out[pj + h * k] = gw1[k];
        out[h * NS + pj] = gb1;
        out[h * NS + h + 2 * pj] = gw2[0];
        out[h * NS + h + 2 * pj + 1] = gw2[1];
        if (pj == 0) {
            out[h * NS + 3 * h] = gb2[0];
            out[h * NS + 3 * h + 1] = gb2[1];
#pragma unroll
            for (int q = 0; q < 3; ++q) g.stat_partials[blockIdx.x * SSTATS + q] = s_st[q];
        }
    }
}

// gradient element p = four groups of partial rows, ascending inside a group, then ((g0 + g1) + g2) + g3 (the order of
// dqn_batch_reduce_kernel); statistic q (wave q + 1 of workgroup 0) = its partial sums lane-strided, a shift-down tree, divided by the
// batch.  The alpha step follows the mean log-probability in the lane that holds it.
__global__ __launch_bounds__(256) void sac_reduce_kernel(const float* __restrict__ partials, const float* __restrict__ stat_partials, int nb,
                                                         int np, int nstat, float* __restrict__ grad, float* __restrict__ stats, float fb,
                                                         const float* alpha, float alpha_lr, float target_entropy, float* alpha_out) {
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
        for (int b = lane; b < nb; b += 64) a += stat_partials[b * SSTATS + q];
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) a += __shfl_down(a, off, 64);
        if (lane == 0) {
            const float m = a / fb;
            stats[q] = m;
            if (q == 2 && alpha_out != nullptr) alpha_out[0] = alpha[0] - alpha_lr * ((-m) - target_entropy);
        }
    }
}

template <int NS, int ACT>
__global__ __launch_bounds__(64) void sac_plan_kernel(const float* __restrict__ actor, int h, const float* __restrict__ obs, int64_t n,
                                                      float lo, float hi, float scale, int deterministic, uint64_t seed, uint32_t env_id_base,
                                                      uint32_t step, float* __restrict__ action_out, float* __restrict__ logp_out,
                                                      float* __restrict__ mu_out, float* __restrict__ rho_out, float* __restrict__ raw_out) {
    __shared__ float l_actor[SNPA_MAX];
    const int npa = (int)mlp2_nparams(NS, h, 2);
    for (int q = threadIdx.x; q < npa; q += 64) l_actor[q] = actor[q];
    __syncthreads();
    const int64_t env = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (env >= n) return;
    float x[NS], o[2], du;
#pragma unroll
    for (int k = 0; k < NS; ++k) x[k] = obs[(int64_t)k * n + env];
    sac_forward<NS, ACT, 2, false>(l_actor, h, x, o, 0.0f, du);
    if (mu_out) mu_out[env] = o[0];
    if (rho_out) rho_out[env] = o[1];
    if (deterministic) {
        action_out[env] = scale * tanhf(o[0]);
        if (raw_out) raw_out[env] = softplus_nnlib(o[1]);
        return;
    }
    const SacHead hd(o[0], o[1], normal_draw(seed, env_id_base + (uint32_t)env, step, 0), lo, hi);
    action_out[env] = scale * hd.a;
    if (logp_out) logp_out[env] = hd.logp;
    if (raw_out) raw_out[env] = hd.raw;
}

static bool sac_shape_ok(int64_t ns, int64_t h) { return ns >= 2 && ns <= 4 && h >= 4 && h <= SHMAX && h % 4 == 0; }
static int sac_blocks(int64_t batch) {
    const int64_t tiles = (batch + STILE - 1) / STILE;
    return (int)(tiles < SMAX_BLOCKS ? tiles : SMAX_BLOCKS);
}

}  // namespace rlhip

using namespace rlhip;

#define SAC_REQUIRE_RING_AND_NET(rb, h, act, batch)                                                                                   \
    RLHIP_REQUIRE((rb) != nullptr, "NULL argument");                                                                                  \
    RLHIP_REQUIRE((rb)->layout == RLHIP_RING_RECORDS, "the SAC learner reads a record ring (Float32 observations, obs_dim 2..4); "   \
                                                      "frame rings and obs_dim > 4 are out of scope");                                \
    RLHIP_REQUIRE((rb)->obs_dim >= 2 && (rb)->obs_dim <= 4, "obs_dim must be 2..4");                                                  \
    RLHIP_REQUIRE((h) >= 4 && (h) <= SHMAX && (h) % 4 == 0, "hidden must be a multiple of 4, <= 256");                                \
    RLHIP_REQUIRE((act) == 0 || (act) == 1, "act must be 0 (relu) or 1 (tanh)");                                                      \
    RLHIP_REQUIRE((batch) >= 1, "empty batch");                                                                                       \
    RLHIP_REQUIRE((rb)->len_rt >= 1, "cannot sample from an empty trajectory")

#define SAC_DISPATCH(KERNEL, ns, act, ...)                                                              \
    do {                                                                                                \
        if ((ns) == 2) { if ((act) == 0) KERNEL(2, 0, __VA_ARGS__); else KERNEL(2, 1, __VA_ARGS__); }   \
        else if ((ns) == 3) { if ((act) == 0) KERNEL(3, 0, __VA_ARGS__); else KERNEL(3, 1, __VA_ARGS__); } \
        else { if ((act) == 0) KERNEL(4, 0, __VA_ARGS__); else KERNEL(4, 1, __VA_ARGS__); }             \
    } while (0)

extern "C" {

int64_t rlhip_sac_workspace_bytes(int64_t ns, int64_t h, int64_t batch) {
    if (!sac_shape_ok(ns, h) || batch < 1) return -1;
    const int64_t npa = mlp2_nparams(ns, h, 2), npq2 = 2 * mlp2_nparams(ns + 1, h, 1);
    return sac_blocks(batch) * ((npa > npq2 ? npa : npq2) + SSTATS) * (int64_t)sizeof(float);  // partial rows | partial sums
}

int32_t rlhip_sac_plan_f32(const float* actor, int64_t ns, int64_t h, int32_t act, const float* obs, int64_t n, float min_sigma,
                           float max_sigma, float action_scale, int32_t deterministic, uint64_t seed, uint32_t env_id_base,
                           uint32_t step, float* action_out, float* logp_out, float* mu_out, float* rho_out, float* raw_sigma_out,
                           rlhip_stream_t stream) {
    RLHIP_REQUIRE(actor && obs && action_out, "NULL argument");
    RLHIP_REQUIRE(ns >= 2 && ns <= 4, "obs dim must be 2..4 (frame rings and obs_dim > 4 are out of scope)");
    RLHIP_REQUIRE(h >= 4 && h <= SHMAX && h % 4 == 0, "hidden must be a multiple of 4, <= 256");
    RLHIP_REQUIRE(act == 0 || act == 1, "act must be 0 (relu) or 1 (tanh)");
    RLHIP_REQUIRE(n >= 0, "negative env count");
    RLHIP_REQUIRE(!(deterministic && logp_out), "logp_out must be NULL with deterministic: no action is drawn");
    if (n == 0) return RLHIP_OK;
    hipStream_t st = as_stream(stream);
#define LAUNCH_SAC_PLAN(NS_, ACT_, ...)                                                                                                  \
    hipLaunchKernelGGL((sac_plan_kernel<NS_, ACT_>), dim3((int)((n + 63) / 64)), dim3(64), 0, st, actor, (int)h, obs, n, min_sigma,      \
                       max_sigma, action_scale, deterministic ? 1 : 0, seed, env_id_base, step, action_out, logp_out, mu_out, rho_out,    \
                       raw_sigma_out)
    SAC_DISPATCH(LAUNCH_SAC_PLAN, ns, act, 0);
#undef LAUNCH_SAC_PLAN
    RLHIP_LAUNCH_CHECK();
    return RLHIP_OK;
}

int32_t rlhip_sac_critic_grad_f32(const rlhip_ring* rb, int64_t h, int32_t act, const float* actor, const float* critics,
                                  const float* targets, int64_t batch, const int64_t* idx, const float* alpha, float gamma,
                                  float min_sigma, float max_sigma, float action_scale, uint64_t seed, uint32_t step, void* workspace,
                                  float* grad_out, float* loss_out, float* y_out, rlhip_stream_t stream) {
    SAC_REQUIRE_RING_AND_NET(rb, h, act, batch);
    RLHIP_REQUIRE(actor && critics && targets && idx && alpha && workspace && grad_out && loss_out, "NULL argument");
    RLHIP_CHECK_GATHER_INDICES(rb, idx, batch, stream);
    hipStream_t st = as_stream(stream);
    const int ns = (int)rb->obs_dim, nb = sac_blocks(batch);
    const int np = 2 * (int)mlp2_nparams(ns + 1, h, 1);
    SacArgs g{};
    g.ring = {(const uint8_t*)rb->state, rb->capacity, rb->n_env, rb->head_sa};
    g.idx = idx, g.actor = actor, g.critics = critics, g.targets = targets, g.alpha = alpha;
    g.partials = (float*)workspace;
    g.stat_partials = g.partials + (int64_t)nb * np;
    g.batch = batch, g.h = (int)h, g.num_tiles = (int)((batch + STILE - 1) / STILE), g.np = np;
    g.gamma = gamma, g.lo = min_sigma, g.hi = max_sigma, g.scale = action_scale, g.fb = (float)batch;
    g.seed = seed, g.step = step, g.y_out = y_out;
#define LAUNCH_SAC_CRITIC(NS_, ACT_, ...) hipLaunchKernelGGL((sac_critic_grad_kernel<NS_, ACT_>), dim3(nb), dim3(STHREADS), 0, st, g)
    SAC_DISPATCH(LAUNCH_SAC_CRITIC, ns, act, 0);
#undef LAUNCH_SAC_CRITIC
    RLHIP_LAUNCH_CHECK();
    hipLaunchKernelGGL(sac_reduce_kernel, dim3((np + 63) / 64), dim3(256), 0, st, g.partials, g.stat_partials, nb, np, 2, grad_out,
                       loss_out, g.fb, nullptr, 0.0f, 0.0f, nullptr);
    RLHIP_LAUNCH_CHECK();
    return RLHIP_OK;
}

int32_t rlhip_sac_actor_grad_f32(const rlhip_ring* rb, int64_t h, int32_t act, const float* actor, const float* critics, int64_t batch,
                                 const int64_t* idx, const float* alpha, float min_sigma, float max_sigma, float action_scale,
                                 uint64_t seed, uint32_t step, float alpha_lr, float target_entropy, float* alpha_out, void* workspace,
                                 float* grad_out, float* stats_out, int32_t* sel_out, float* logp_out, rlhip_stream_t stream) {
    SAC_REQUIRE_RING_AND_NET(rb, h, act, batch);
    RLHIP_REQUIRE(actor && critics && idx && alpha && workspace && grad_out && stats_out, "NULL argument");
    RLHIP_CHECK_GATHER_INDICES(rb, idx, batch, stream);
    hipStream_t st = as_stream(stream);
    const int ns = (int)rb->obs_dim, nb = sac_blocks(batch);
    const int np = (int)mlp2_nparams(ns, h, 2);
    SacArgs g{};
    g.ring = {(const uint8_t*)rb->state, rb->capacity, rb->n_env, rb->head_sa};
    g.idx = idx, g.actor = actor, g.critics = critics, g.alpha = alpha;
    g.partials = (float*)workspace;
    g.stat_partials = g.partials + (int64_t)nb * np;
    g.batch = batch, g.h = (int)h, g.num_tiles = (int)((batch + STILE - 1) / STILE), g.np = np;
    g.lo = min_sigma, g.hi = max_sigma, g.scale = action_scale, g.fb = (float)batch;
    g.seed = seed, g.step = step, g.sel_out = sel_out, g.logp_out = logp_out;
#define LAUNCH_SAC_ACTOR(NS_, ACT_, ...) hipLaunchKernelGGL((sac_actor_grad_kernel<NS_, ACT_>), dim3(nb), dim3(STHREADS), 0, st, g)
    SAC_DISPATCH(LAUNCH_SAC_ACTOR, ns, act, 0);
#undef LAUNCH_SAC_ACTOR
    RLHIP_LAUNCH_CHECK();
    const bool step_alpha = alpha_lr > 0.0f && alpha_out != nullptr;
    hipLaunchKernelGGL(sac_reduce_kernel, dim3((np + 63) / 64), dim3(256), 0, st, g.partials, g.stat_partials, nb, np, 3, grad_out,
                       stats_out, g.fb, alpha, alpha_lr, target_entropy, step_alpha ? alpha_out : nullptr);
    RLHIP_LAUNCH_CHECK();
    return RLHIP_OK;
}

}  // extern "C"
