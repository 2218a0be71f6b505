// td3.hip -- TD3 and DDPG on the continuous vector envs (PendulumEnv, ContinuousMountainCarEnv, CartPoleEnv(continuous)): plan! as one
// launch, and the two gradients of an update -- the critics against the smoothed, clipped double-Q target, the deterministic actor
// against -Q1(s, pi(s)) -- each as one gradient launch plus a fixed-order fold.  include/rlhip.h states the formulas, the summation
// order and the stream separation; tests/td3_ref.py is their Float64 model.  DDPG is n_critics = 1 with target_noise = 0.
//
// Reference: the homepage lists DDPG among the algorithms and the docs build MADDPG on DDPGPolicy, but the Zoo's DDPGPolicy / TD3Policy
// are not in the tree, so the update is specified by the header's text.  actor = mlp2(ns, h, 1), critics = [Q1 | Q2] (or [Q1]), each
// mlp2(ns + 1, h, 1) on vcat(s, u).  At most 5 inputs and ONE output per network: VALU work, no matrix instruction fits (an MFMA
// tile wants K >= 4 real rows and N >= 4 real columns; here the second layer is a dot product).
//
// The design is the UNIT-SLICED forward.  csrc/sac.hip gives one lane the whole forward pass of one network on one sample: a dependent
// chain of h units, on five of its eight waves.  Here a (sample, network) pair belongs to one 16-lane DPP row:
//
//   td3_plan_kernel<NS, ACT>              one lane per env, the actor staged in LDS, the ONE-chain order of rlhip_mlp2_forward_f32 (mu_out
//                                         is its bytes), then the exploration noise and the clamp in the same lane
//   td3_critic_grad_kernel<NS, ACT, NC>   tiles of 64 samples, 512 threads:
//   td3_actor_grad_kernel<NS, ACT>
//       phase 0   every network the launch reads -> LDS in its flat layout (critic launch: actor target, Q_c, Qt_c -- 3 or 5 networks,
//                 34.8 KB at ns = 4, h = 256, so nothing had to be dropped or evaluated early; actor launch: actor, Q1); the tile's 64
//                 records, one lane per record and one 64-byte request each, -> LDS (wave 0), the tile's 64 clipped noise values
//                 (wave 1, beside the gather)
//       phase 1   row r = tid / 16 of the workgroup's 32 rows, lane p = tid % 16.  A pass over `nets` networks is 64 x nets pairs,
//                 32 at a time: in round `it` every row works on network it / 2 and sample 32 (it % 2) + r.  Lane p computes the units
//                 j = p, p + 16, .. ascending (z_j = b1[j], fmaf over k ascending), carries ONE partial fmaf(W2[j], act(z_j), .) from
//                 +0, the 16 partials meet in a shift-down tree of row-DPP moves (8, 4, 2, 1: four v_add with a DPP operand, no LDS),
//                 b2 is added last in lane 0.  Chain: h / 16 units + 4 moves instead of h units; all eight waves busy.  The four
//                 rows of a wave read the SAME weights for four samples (an LDS broadcast), the 16 lanes of a row 16 consecutive
//                 floats (conflict-free).  dQ1/du of the actor launch rides in the same pass as a second partial and a second tree.
//                 Then the TD line (critic launch) or the loss line (actor launch) of each sample in one lane.
//       phase 2   thread = (network, hidden unit j), as the SAC tile: recomputes z_j of each sample by the same chain (bit for bit
//                 phase 1's z_j) and carries ONE fmaf / add chain per gradient element over the workgroup's samples in ascending batch
//                 position, in registers across its tiles
//   td3_reduce_kernel                     the partial rows, one per workgroup, and the partial loss sums in a fixed order
// No float atomics anywhere: two calls on the same inputs give the same bytes.
#include "head_device.h"
#include "mlp_device.h"
#include "ring_device.h"

namespace rlhip {

constexpr int TTILE = 64;
constexpr int TTHREADS = 512;
constexpr int TROWS = TTHREADS / 16;  // 16-lane rows per workgroup
constexpr int TMAX_BLOCKS = 256;      // partial rows: a larger batch gives its workgroups further tiles
constexpr int THMAX = 256;
constexpr int TSTATS = 2;                               // partial sums per workgroup beside its gradient row (2 losses; loss, q)
constexpr int TNPA_MAX = THMAX * 4 + THMAX + THMAX + 1;  // mlp2(4, 256, 1)
constexpr int TNPQ_MAX = THMAX * 5 + THMAX + THMAX + 1;  // mlp2(5, 256, 1)

struct Td3Args {
    RingRecs ring;
    const int64_t* idx;
    const float* actor;    // critic launch: the actor TARGET
    const float* critics;
    const float* targets;  // critic launch only
    float* partials;
    float* stat_partials;
    int64_t batch;
    int h, num_tiles, np;
    float gamma, lo, hi, scale, fb, target_noise, noise_clip;
    uint64_t seed;
    uint32_t step;
    float* y_out;      // critic launch, nullable
    float* noise_out;  // critic launch, nullable
};

// the total of the 16 lanes of a DPP row in lane 0 of the row: v[i] += v[i + 8], += v[i + 4], += v[i + 2], += v[i + 1] (row_shl moves;
// a lane whose source lies outside the row adds +0 and holds no total)
__device__ __forceinline__ float td3_row_sum_down(float v) {
    v = dpp_add<0x108>(v);
    v = dpp_add<0x104>(v);
    v = dpp_add<0x102>(v);
    return dpp_add<0x101>(v);
}

// lane p's share of out = mlp2(NI, h, 1)(x), the flat vector P in LDS: the units j = p, p + 16, .. ascending.  Lane 0 of the row
// returns the output (the tree, then + b2).  DU: also dq dQ/du through layer 2, the activation's derivative and column NI - 1 of
// W1, by the same slicing and the same tree (lane 0 of the row)
template <int NI, int ACT, bool DU>
__device__ __forceinline__ float td3_forward_row(const float* P, int h, int p, const float (&x)[NI], float dq, float& du) {
    const float* b1 = P + h * NI;
    const float* W2 = b1 + h;
    float acc = 0.0f, dacc = 0.0f;
#pragma unroll 2
    for (int j = p; j < h; j += 16) {
        float z = b1[j];
#pragma unroll
        for (int k = 0; k < NI; ++k) z = fmaf(P[j + h * k], x[k], z);
        const float hv = act_fwd_t<ACT>(z);
        const float w2 = W2[j];
        acc = fmaf(w2, hv, acc);
        if (DU) {
            const float dz = (dq * w2) * (ACT == 0 ? (hv > 0.0f ? 1.0f : 0.0f) : (1.0f - hv * hv));
            dacc = fmaf(dz, P[j + h * (NI - 1)], dacc);
        }
    }
    if (DU) du = td3_row_sum_down(dacc);
    return td3_row_sum_down(acc) + W2[h];
}

__device__ __forceinline__ void td3_stage(float* dst, const float* src, int n) {
    for (int q = threadIdx.x; q < n; q += TTHREADS) dst[q] = src[q];
}

// the records of the tile's samples -> LDS, one lane per sample (one 64-byte record = one fabric request).  A position past the
// batch reads the record of position 0, so that every row of phase 1 has finite inputs and no lane of a row sits out
struct Td3Tile {
    float s[TTILE][4], sn[TTILE][4], a[TTILE], r[TTILE], cont[TTILE];
};
__device__ __forceinline__ void td3_gather(const Td3Args& g, int tile, Td3Tile& t) {
    const int tid = threadIdx.x;
    if (tid < TTILE) {
        const int64_t b = (int64_t)tile * TTILE + tid;
        const int64_t fj = g.idx[b < g.batch ? b : 0];
        const RingTransition rt = ring_load_transition(g.ring, fj);
#pragma unroll
        for (int k = 0; k < 4; ++k) t.s[tid][k] = rt.s[k], t.sn[tid][k] = rt.sn[k];
        t.a[tid] = __int_as_float(rt.a);  // the action word holds the bits of a Float32
        t.r[tid] = rt.r;
        t.cont[tid] = rt.t ? 0.0f : 1.0f;
    }
}

template <int NS, int ACT, int NC>
__global__ __launch_bounds__(TTHREADS) void td3_critic_grad_kernel(Td3Args g) {
    constexpr int NQ = NS + 1;
    __shared__ float l_actor[TNPA_MAX], l_q[2 * NC][TNPQ_MAX];  // Q_c, then Qt_c
    __shared__ Td3Tile l_t;
    __shared__ float l_e[TTILE], l_un[TTILE], l_out[2 * NC][TTILE], l_g[NC][TTILE], l_l[NC][TTILE];
    const int tid = threadIdx.x, h = g.h;
    const int row = tid >> 4, p = tid & 15;
    const int npa = (int)mlp2_nparams(NS, h, 1), npq = (int)mlp2_nparams(NQ, h, 1);
    td3_stage(l_actor, g.actor, npa);
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        td3_stage(l_q[c], g.critics + c * npq, npq);
        td3_stage(l_q[NC + c], g.targets + c * npq, npq);
    }

    // phase 2: this thread's (critic, unit)
    const bool p2 = tid < NC * h;
    const int pc = p2 ? tid / h : 0, pj = p2 ? tid - pc * h : 0;
    float gw1[NQ], gb1 = 0.f, gw2 = 0.f, gb2 = 0.f, s_loss = 0.f;
#pragma unroll
    for (int k = 0; k < NQ; ++k) gw1[k] = 0.f;

    for (int tile = blockIdx.x; tile < g.num_tiles; tile += gridDim.x) {
        const int64_t b0 = (int64_t)tile * TTILE;
        const int cnt = (int)(g.batch - b0 < TTILE ? g.batch - b0 : TTILE);
        td3_gather(g, tile, l_t);
        if (tid >= TTILE && tid < 2 * TTILE) {  // wave 1: the clipped target noise of batch position b0 + smp
            const int smp = tid - TTILE;
            float e = 0.0f;
            if (g.target_noise != 0.0f)
                e = clampj(g.target_noise * normal_draw(g.seed, (uint32_t)(b0 + smp), g.step, 0), -g.noise_clip, g.noise_clip);
            l_e[smp] = e;
            if (g.noise_out && smp < cnt) g.noise_out[b0 + smp] = e;
        }
        __syncthreads();  // (the first tile: the staged networks too)
        // ---- phase 1a: the target actor at s', one row per sample, and the smoothed target action
#pragma unroll
        for (int it = 0; it < TTILE / TROWS; ++it) {
            const int smp = it * TROWS + row;
            float x[NS], du;
#pragma unroll
            for (int k = 0; k < NS; ++k) x[k] = l_t.sn[smp][k];
            const float mu = td3_forward_row<NS, ACT, false>(l_actor, h, p, x, 0.0f, du);
            if (p == 0) l_un[smp] = clampj(g.scale * tanhf(mu) + l_e[smp], g.lo, g.hi);
        }
        __syncthreads();
        // ---- phase 1b: Q_c(x) and Qt_c(x'), one row per (sample, network)
        for (int it = 0; it < 2 * NC * (TTILE / TROWS); ++it) {
            const int net = it / (TTILE / TROWS), smp = (it % (TTILE / TROWS)) * TROWS + row;
            float x[NQ], du;
#pragma unroll
            for (int k = 0; k < NS; ++k) x[k] = net < NC ? l_t.s[smp][k] : l_t.sn[smp][k];
            x[NS] = net < NC ? l_t.a[smp] : l_un[smp];
            const float q = td3_forward_row<NQ, ACT, false>(l_q[net], h, p, x, 0.0f, du);
            if (p == 0) l_out[net][smp] = q;
        }
        __syncthreads();
        // ---- phase 1c: the TD target and the squared error(s) of the sample
        if (tid < cnt) {
            float qt = l_out[NC][tid];
            if (NC == 2) {
                const float qt2 = l_out[2 * NC - 1][tid];
                qt = qt2 < qt ? qt2 : qt;
            }
            const float y = l_t.r[tid] + (g.gamma * l_t.cont[tid]) * qt;
#pragma unroll
            for (int c = 0; c < NC; ++c) {
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
            g.stat_partials[blockIdx.x * TSTATS + pc] = s_loss;
        }
    }
}

template <int NS, int ACT>
__global__ __launch_bounds__(TTHREADS) void td3_actor_grad_kernel(Td3Args g) {
    constexpr int NQ = NS + 1;
    __shared__ float l_actor[TNPA_MAX], l_q[TNPQ_MAX];  // the actor, Q1
    __shared__ Td3Tile l_t;
    __shared__ float l_a[TTILE], l_d[TTILE], l_qv[TTILE];
    const int tid = threadIdx.x, h = g.h;
    const int row = tid >> 4, p = tid & 15;
    const int npa = (int)mlp2_nparams(NS, h, 1), npq = (int)mlp2_nparams(NQ, h, 1);
    td3_stage(l_actor, g.actor, npa);
    td3_stage(l_q, g.critics, npq);
    const float dq = -1.0f / g.fb;

    const bool p2 = tid < h;
    const int pj = p2 ? tid : 0;
    float gw1[NS], gb1 = 0.f, gw2 = 0.f, gb2 = 0.f, s_l = 0.f, s_q = 0.f;
#pragma unroll
    for (int k = 0; k < NS; ++k) gw1[k] = 0.f;

    for (int tile = blockIdx.x; tile < g.num_tiles; tile += gridDim.x) {
        const int64_t b0 = (int64_t)tile * TTILE;
        const int cnt = (int)(g.batch - b0 < TTILE ? g.batch - b0 : TTILE);
        td3_gather(g, tile, l_t);
        __syncthreads();
        // ---- phase 1a: a = tanhf(mu(s)), one row per sample
#pragma unroll
        for (int it = 0; it < TTILE / TROWS; ++it) {
            const int smp = it * TROWS + row;
            float x[NS], du;
#pragma unroll
            for (int k = 0; k < NS; ++k) x[k] = l_t.s[smp][k];
            const float mu = td3_forward_row<NS, ACT, false>(l_actor, h, p, x, 0.0f, du);
            if (p == 0) l_a[smp] = tanhf(mu);
        }
        __syncthreads();
        // ---- phase 1b: Q1(s, u) and dq dQ1/du, one row per sample; then dmu in the row's lane 0
#pragma unroll
        for (int it = 0; it < TTILE / TROWS; ++it) {
            const int smp = it * TROWS + row;
            float x[NQ], du = 0.0f;
#pragma unroll
            for (int k = 0; k < NS; ++k) x[k] = l_t.s[smp][k];
            const float a = l_a[smp];
            x[NS] = g.scale * a;
            const float q = td3_forward_row<NQ, ACT, true>(l_q, h, p, x, dq, du);
            if (p == 0) {
                l_qv[smp] = q;
                l_d[smp] = (g.scale * du) * (1.0f - a * a);
            }
        }
        __syncthreads();
        // ---- phase 2: actor unit pj over the samples of the tile in ascending order
        if (p2) {
            float w1[NS];
#pragma unroll
            for (int k = 0; k < NS; ++k) w1[k] = l_actor[pj + h * k];
            const float pb1 = l_actor[h * NS + pj], pw2 = l_actor[h * NS + h + pj];
            for (int i = 0; i < cnt; ++i) {
                float x[NS];
#pragma unroll
                for (int k = 0; k < NS; ++k) x[k] = l_t.s[i][k];
                float z = pb1;
#pragma unroll
                for (int k = 0; k < NS; ++k) z = fmaf(w1[k], x[k], z);
                const float hv = act_fwd_t<ACT>(z);
                const float d = l_d[i];
                gw2 = fmaf(d, hv, gw2);
                const float dz = (d * pw2) * (ACT == 0 ? (hv > 0.0f ? 1.0f : 0.0f) : (1.0f - hv * hv));
                gb1 += dz;
#pragma unroll
                for (int k = 0; k < NS; ++k) gw1[k] = fmaf(dz, x[k], gw1[k]);
                if (pj == 0) {
                    gb2 += d;
                    s_l += -l_qv[i];
                    s_q += l_qv[i];
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
        out[h * NS + h + pj] = gw2;
        if (pj == 0) {
            out[h * NS + 2 * h] = gb2;
            g.stat_partials[blockIdx.x * TSTATS + 0] = s_l;
            g.stat_partials[blockIdx.x * TSTATS + 1] = s_q;
        }
    }
}

// gradient element p = four groups of partial rows, ascending inside a group, then ((g0 + g1) + g2) + g3 (the order of
// dqn_batch_reduce_kernel); statistic q (wave q + 1 of workgroup 0) = its partial sums lane-strided, a shift-down tree, divided by the
// batch
__global__ __launch_bounds__(256) void td3_reduce_kernel(const float* __restrict__ partials, const float* __restrict__ stat_partials, int nb,
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
        for (int b = lane; b < nb; b += 64) a += stat_partials[b * TSTATS + q];
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) a += __shfl_down(a, off, 64);
        if (lane == 0) stats[q] = a / fb;
    }
}

template <int NS, int ACT>
__global__ __launch_bounds__(64) void td3_plan_kernel(const float* __restrict__ actor, int h, const float* __restrict__ obs, int64_t n,
                                                      float scale, float act_noise, float lo, float hi, int deterministic, uint64_t seed,
                                                      uint32_t env_id_base, uint32_t step, float* __restrict__ action_out,
                                                      float* __restrict__ mu_out) {
    __shared__ float l_actor[TNPA_MAX];
    const int npa = (int)mlp2_nparams(NS, h, 1);
    for (int q = threadIdx.x; q < npa; q += 64) l_actor[q] = actor[q];
    __syncthreads();
    const int64_t env = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (env >= n) return;
    float x[NS];
#pragma unroll
    for (int k = 0; k < NS; ++k) x[k] = obs[(int64_t)k * n + env];
    // the one chain of mlp2_forward_kernel (ppo.hip): mu = b2, fmaf over j ascending
    const float* b1 = l_actor + h * NS;
    const float* W2 = b1 + h;
    float mu = W2[h];
#pragma unroll 4
    for (int j = 0; j < h; ++j) {
        float z = b1[j];
#pragma unroll
        for (int k = 0; k < NS; ++k) z = fmaf(l_actor[j + h * k], x[k], z);
        mu = fmaf(W2[j], act_fwd_t<ACT>(z), mu);
    }
    if (mu_out) mu_out[env] = mu;
    float u = scale * tanhf(mu);
    if (!deterministic) u = u + act_noise * normal_draw(seed, env_id_base + (uint32_t)env, step, 0);
    action_out[env] = clampj(u, lo, hi);
}

static bool td3_shape_ok(int64_t ns, int64_t h, int64_t nc) {
    return ns >= 2 && ns <= 4 && h >= 16 && h <= THMAX && h % 16 == 0 && (nc == 1 || nc == 2);
}
static int td3_blocks(int64_t batch) {
    const int64_t tiles = (batch + TTILE - 1) / TTILE;
    return (int)(tiles < TMAX_BLOCKS ? tiles : TMAX_BLOCKS);
}

}  // namespace rlhip

using namespace rlhip;

#define TD3_REQUIRE_NET(ns, h, act)                                                                                                   \
    RLHIP_REQUIRE((ns) >= 2 && (ns) <= 4, "obs_dim must be 2..4 (frame rings and obs_dim > 4 are out of scope)");                     \
    RLHIP_REQUIRE((h) >= 16 && (h) <= THMAX && (h) % 16 == 0, "hidden must be a multiple of 16 in 16..256 (a unit slice per lane of " \
                                                              "a 16-lane row)");                                                       \
    RLHIP_REQUIRE((act) == 0 || (act) == 1, "act must be 0 (relu) or 1 (tanh)")

#define TD3_REQUIRE_RING_AND_NET(rb, h, act, batch)                                                                                   \
    RLHIP_REQUIRE((rb) != nullptr, "NULL argument");                                                                                  \
    RLHIP_REQUIRE((rb)->layout == RLHIP_RING_RECORDS, "the TD3 / DDPG learner reads a record ring (Float32 observations, obs_dim "    \
                                                      "2..4); frame rings and obs_dim > 4 are out of scope");                         \
    TD3_REQUIRE_NET((rb)->obs_dim, h, act);                                                                                           \
    RLHIP_REQUIRE((batch) >= 1, "empty batch");                                                                                       \
    RLHIP_REQUIRE((rb)->len_rt >= 1, "cannot sample from an empty trajectory")

#define TD3_DISPATCH(KERNEL, ns, act, ...)                                                              \
    do {                                                                                                \
        if ((ns) == 2) { if ((act) == 0) KERNEL(2, 0, __VA_ARGS__); else KERNEL(2, 1, __VA_ARGS__); }   \
        else if ((ns) == 3) { if ((act) == 0) KERNEL(3, 0, __VA_ARGS__); else KERNEL(3, 1, __VA_ARGS__); } \
        else { if ((act) == 0) KERNEL(4, 0, __VA_ARGS__); else KERNEL(4, 1, __VA_ARGS__); }             \
    } while (0)

extern "C" {

int64_t rlhip_td3_workspace_bytes(int64_t ns, int64_t h, int64_t n_critics, int64_t batch) {
    if (!td3_shape_ok(ns, h, n_critics) || batch < 1) return -1;
    const int64_t npa = mlp2_nparams(ns, h, 1), npq = n_critics * mlp2_nparams(ns + 1, h, 1);
    return td3_blocks(batch) * ((npa > npq ? npa : npq) + TSTATS) * (int64_t)sizeof(float);  // partial rows | partial sums
}

int32_t rlhip_td3_plan_f32(const float* actor, int64_t ns, int64_t h, int32_t act, const float* obs, int64_t n, float action_scale,
                           float act_noise, float action_lo, float action_hi, int32_t deterministic, uint64_t seed,
                           uint32_t env_id_base, uint32_t step, float* action_out, float* mu_out, rlhip_stream_t stream) {
    RLHIP_REQUIRE(actor && obs && action_out, "NULL argument");
    TD3_REQUIRE_NET(ns, h, act);
    RLHIP_REQUIRE(n >= 0, "negative env count");
    if (n == 0) return RLHIP_OK;
    hipStream_t st = as_stream(stream);
#define LAUNCH_TD3_PLAN(NS_, ACT_, ...)                                                                                                 \
    hipLaunchKernelGGL((td3_plan_kernel<NS_, ACT_>), dim3((int)((n + 63) / 64)), dim3(64), 0, st, actor, (int)h, obs, n, action_scale,  \
                       act_noise, action_lo, action_hi, deterministic ? 1 : 0, seed, env_id_base, step, action_out, mu_out)
    TD3_DISPATCH(LAUNCH_TD3_PLAN, ns, act, 0);
#undef LAUNCH_TD3_PLAN
    RLHIP_LAUNCH_CHECK();
    return RLHIP_OK;
}

int32_t rlhip_td3_critic_grad_f32(const rlhip_ring* rb, int64_t h, int32_t act, int32_t n_critics, const float* actor_target,
                                  const float* critics, const float* critic_targets, int64_t batch, const int64_t* idx, float gamma,
                                  float action_scale, float target_noise, float noise_clip, float action_lo, float action_hi,
                                  uint64_t seed, uint32_t step, void* workspace, float* grad_out, float* loss_out, float* y_out,
                                  float* noise_out, rlhip_stream_t stream) {
    TD3_REQUIRE_RING_AND_NET(rb, h, act, batch);
    RLHIP_REQUIRE(n_critics == 1 || n_critics == 2, "n_critics must be 1 (DDPG) or 2 (TD3)");
    RLHIP_REQUIRE(actor_target && critics && critic_targets && idx && workspace && grad_out && loss_out, "NULL argument");
    RLHIP_CHECK_GATHER_INDICES(rb, idx, batch, stream);
    hipStream_t st = as_stream(stream);
    const int ns = (int)rb->obs_dim, nb = td3_blocks(batch);
    const int np = n_critics * (int)mlp2_nparams(ns + 1, h, 1);
    Td3Args g{};
    g.ring = {(const uint8_t*)rb->state, rb->capacity, rb->n_env, rb->head_sa};
    g.idx = idx, g.actor = actor_target, g.critics = critics, g.targets = critic_targets;
    g.partials = (float*)workspace;
    g.stat_partials = g.partials + (int64_t)nb * np;
    g.batch = batch, g.h = (int)h, g.num_tiles = (int)((batch + TTILE - 1) / TTILE), g.np = np;
    g.gamma = gamma, g.lo = action_lo, g.hi = action_hi, g.scale = action_scale, g.fb = (float)batch;
    g.target_noise = target_noise, g.noise_clip = noise_clip;
    g.seed = seed, g.step = step, g.y_out = y_out, g.noise_out = noise_out;
#define LAUNCH_TD3_CRITIC(NS_, ACT_, ...)                                                                              \
    do {                                                                                                               \
        if (n_critics == 2) hipLaunchKernelGGL((td3_critic_grad_kernel<NS_, ACT_, 2>), dim3(nb), dim3(TTHREADS), 0, st, g); \
        else hipLaunchKernelGGL((td3_critic_grad_kernel<NS_, ACT_, 1>), dim3(nb), dim3(TTHREADS), 0, st, g);            \
    } while (0)
    TD3_DISPATCH(LAUNCH_TD3_CRITIC, ns, act, 0);
#undef LAUNCH_TD3_CRITIC
    RLHIP_LAUNCH_CHECK();
    hipLaunchKernelGGL(td3_reduce_kernel, dim3((np + 63) / 64), dim3(256), 0, st, g.partials, g.stat_partials, nb, np, (int)n_critics,
                       grad_out, loss_out, g.fb);
    RLHIP_LAUNCH_CHECK();
    return RLHIP_OK;
}

int32_t rlhip_td3_actor_grad_f32(const rlhip_ring* rb, int64_t h, int32_t act, const float* actor, const float* critics, int64_t batch,
                                 const int64_t* idx, float action_scale, void* workspace, float* grad_out, float* stats_out,
                                 rlhip_stream_t stream) {
    TD3_REQUIRE_RING_AND_NET(rb, h, act, batch);
    RLHIP_REQUIRE(actor && critics && idx && workspace && grad_out && stats_out, "NULL argument");
    RLHIP_CHECK_GATHER_INDICES(rb, idx, batch, stream);
    hipStream_t st = as_stream(stream);
    const int ns = (int)rb->obs_dim, nb = td3_blocks(batch);
    const int np = (int)mlp2_nparams(ns, h, 1);
    Td3Args g{};
    g.ring = {(const uint8_t*)rb->state, rb->capacity, rb->n_env, rb->head_sa};
    g.idx = idx, g.actor = actor, g.critics = critics;
    g.partials = (float*)workspace;
    g.stat_partials = g.partials + (int64_t)nb * np;
    g.batch = batch, g.h = (int)h, g.num_tiles = (int)((batch + TTILE - 1) / TTILE), g.np = np;
    g.scale = action_scale, g.fb = (float)batch;
#define LAUNCH_TD3_ACTOR(NS_, ACT_, ...) hipLaunchKernelGGL((td3_actor_grad_kernel<NS_, ACT_>), dim3(nb), dim3(TTHREADS), 0, st, g)
    TD3_DISPATCH(LAUNCH_TD3_ACTOR, ns, act, 0);
#undef LAUNCH_TD3_ACTOR
    RLHIP_LAUNCH_CHECK();
    hipLaunchKernelGGL(td3_reduce_kernel, dim3((np + 63) / 64), dim3(256), 0, st, g.partials, g.stat_partials, nb, np, 2, grad_out,
                       stats_out, g.fb);
    RLHIP_LAUNCH_CHECK();
    return RLHIP_OK;
}

}  // extern "C"
