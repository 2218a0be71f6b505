// dqn_sample_fold.hip -- the folded batch of a two-layer DQN learner in ONE launch: the sampler's draw, the n-step window fold and
// the Double DQN target, i.e. what the per-stage learner (DQNLearner.optimise_ / _optimise_double_) issues as
//
//     rlhip_ring_sample_indices[_nstep]  ->  rlhip_ring_fold_nstep (n_step > 1)  ->  rlhip_dqn_fold_double_f32 (double_dqn)
//
// Two of those launches do nothing but hand a tile's worth of indices and records to the next one through memory.  Here the lane
// that owns sample b draws its own index (the Philox draw of sample_indices_kernel, as dqn_grad_kernel does inline), walks its
// window (fold_nstep_kernel's walk and its right-to-left Float32 return, operation for operation) and leaves the folded transition
// in LDS, where the tile structure of dqn_fold_double_kernel (dqn_double.hip) takes it up unchanged: both nets staged as l_rec unit
// records while the first record's loads are in flight, row = sample, the 16 lanes of a DPP row walk the hidden units of both nets
// on s', group_sum_dpp<16>, first maximum wins, lanes 0..3 of the row store the record as one 64-byte line.  Results are byte for
// byte those of the composition (tests/test_gpu_fused_folds.py).
//
// Cost: a latency chain -- n_step dependent 64-byte record reads per sample (the next read is issued only once the step before is
// known not to be terminal), then the two forwards out of LDS on one CU per tile.  No Float64, no atomics, nothing crosses a
// workgroup, no MFMA.
#include "mlp_device.h"
#include "ring_device.h"

namespace rlhip {

constexpr int SF_TILE = 64;
constexpr int SF_THREADS = 1024;
constexpr int SF_MAX_BLOCKS = 512;
constexpr int SF_HMAX = 256;
constexpr int SF_MAX_NSTEP = 32;

struct SampleFoldArgs {
    RingRecs ring;
    int64_t len_rt;
    uint64_t total;  // (len_rt - n_step + 1) * n_env: the range of the draw
    uint64_t seed;
    uint32_t draw_ctr;
    const float* params;   // DBL only
    const float* tparams;  // DBL only
    int64_t batch;
    uint8_t* out;      // slot 0 of the folded ring: `batch` records
    int64_t* idx_out;  // nullable
    int64_t* iota;     // nullable
    int h, na, num_tiles, n_step;
    float gamma, gamma_eff;
};

// y = r + gamma * (1 - t) * Qt(s')[a*], a* = findmax(Q(s')): dqn_double.hip's target line, first maximum wins (strict >)
__device__ __forceinline__ float sf_double_target(float r, uint32_t term, float gamma, float q0, float q1, float q2, float q3, float t0,
                                                  float t1, float t2, float t3, int na) {
    float m = q0, v = t0;
    if (na > 1 && q1 > m) m = q1, v = t1;
    if (na > 2 && q2 > m) m = q2, v = t2;
    if (na > 3 && q3 > m) m = q3, v = t3;
    const float cont = term ? 0.f : 1.f;
    return r + gamma * cont * v;
}

template <int NS, int ACT, bool DBL>
__global__ __launch_bounds__(SF_THREADS) void dqn_sample_fold_kernel(SampleFoldArgs g) {
    // l_rec[net][j] = {W1[j, 0..3]}, {b1[j], W2[0..2, j]}, {W2[3, j], -, -, -}: dqn_fold_double_kernel's layout (not allocated without DBL)
    __shared__ float4 l_rec[DBL ? 2 : 1][DBL ? SF_HMAX : 1][3];
    __shared__ nt_u32x4 l_s[SF_TILE], l_w[SF_TILE], l_sn[SF_TILE];  // the three live quarters of each sample's FOLDED record
    __shared__ float l_rew[SF_MAX_NSTEP][SF_TILE];                  // the window's rewards, [step][sample]: conflict-free per step

    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int row = lane >> 4, c = lane & 15;
    const int h = g.h, na = g.na;
    const int smp = 4 * w + row;  // this row's sample of the tile
    bool staged = false;

    for (int tile = blockIdx.x; tile < g.num_tiles; tile += gridDim.x) {
        float bq[MAXO] = {0.f, 0.f, 0.f, 0.f}, btq[MAXO] = {0.f, 0.f, 0.f, 0.f};
        if (DBL) {  // output biases: requested first, in flight across the staging and the barrier
            const float* b2 = g.params + h * NS + h + na * h;
            const float* tb2 = g.tparams + h * NS + h + na * h;
#pragma unroll
            for (int o = 0; o < MAXO; ++o) {
                bq[o] = (o < na) ? b2[o] : 0.f;
                btq[o] = (o < na) ? tb2[o] : 0.f;
            }
        }
        nt_u32x4 rs = {0u, 0u, 0u, 0u}, rw = rs, rsn = rs;
        int64_t fj = 0;
        if (tid < SF_TILE) {
            const int64_t b = (int64_t)tile * SF_TILE + tid;
            const bool valid = b < g.batch;  // a lane past the batch repeats sample 0's draw: a valid window, nothing is written for it
            const u32x4 wd = philox4x32_10(g.seed, (uint32_t)(valid ? b : 0), 0, g.draw_ctr, TAG_SAMPLER);
            fj = (int64_t)__umul64hi(((uint64_t)wd.x << 32) | (uint64_t)wd.y, g.total);
            if (valid && g.idx_out) g.idx_out[b] = fj;
            const uint8_t* r0 = g.ring.rec + ring_record_offset(g.ring, fj);  // the window's first record: one fabric request
            rs = *reinterpret_cast<const nt_u32x4*>(r0);
            rw = *reinterpret_cast<const nt_u32x4*>(r0 + 16);
            rsn = *reinterpret_cast<const nt_u32x4*>(r0 + 32);
        }
        if (DBL && !staged) {  // both networks -> LDS once per workgroup, while the first record is in flight
            staged = true;
            for (int q = tid; q < 2 * h; q += SF_THREADS) {
                const int net = q >= h ? 1 : 0, u = q - net * h;
                const float* P = net ? g.tparams : g.params;
                float w1[4] = {0.f, 0.f, 0.f, 0.f}, w2[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int k = 0; k < NS; ++k) w1[k] = P[u + h * k];
#pragma unroll
                for (int o = 0; o < MAXO; ++o)
                    if (o < na) w2[o] = P[h * NS + h + o + na * u];
                l_rec[net][u][0] = make_float4(w1[0], w1[1], w1[2], w1[3]);
                l_rec[net][u][1] = make_float4(P[h * NS + u], w2[0], w2[1], w2[2]);
                l_rec[net][u][2] = make_float4(w2[3], 0.f, 0.f, 0.f);
            }
        }
        if (tid < SF_TILE) {
            // the window li .. li + ns - 1 of this sample's env (fold_nstep_kernel): up to and including the first terminal step
            uint32_t term = (rw[2] & 0xffu) ? 1u : 0u;
            float ret = __uint_as_float(rw[1]);  // n_step == 1: the stored reward as it stands
            if (g.n_step > 1) {
                int64_t li;
                if (((uint64_t)fj | (uint64_t)g.ring.n_env) >> 32) li = fj / g.ring.n_env;
                else li = (uint32_t)fj / (uint32_t)g.ring.n_env;
                l_rew[0][tid] = ret;
                int ns = 1;
                for (int k = 1; k < g.n_step && !term && li + k < g.len_rt; ++k) {  // (never past the newest stored transition)
                    const uint8_t* rk = g.ring.rec + ring_record_offset(g.ring, fj + (int64_t)k * g.ring.n_env);
                    const nt_u32x4 kw = *reinterpret_cast<const nt_u32x4*>(rk + 16);
                    rsn = *reinterpret_cast<const nt_u32x4*>(rk + 32);
                    l_rew[k][tid] = __uint_as_float(kw[1]);
                    term = (kw[2] & 0xffu) ? 1u : 0u;
                    ns = k + 1;
                }
                float gain = 0.0f;  // discount_rewards_reduced: gain = r[k] + gamma * gain from the window's end
                for (int k = ns - 1; k >= 0; --k) gain = l_rew[k][tid] + g.gamma * gain;
                ret = gain;
            }
            l_s[tid] = rs;
            l_w[tid] = nt_u32x4{rw[0], __float_as_uint(ret), term, 0u};
            l_sn[tid] = rsn;
        }
        __syncthreads();
        {
            const nt_u32x4 un = l_sn[smp], uw = l_w[smp];
            float y = __uint_as_float(uw[1]);
            uint32_t tout = uw[2];
            if (DBL) {
                const float xn[4] = {__uint_as_float(un[0]), __uint_as_float(un[1]), __uint_as_float(un[2]), __uint_as_float(un[3])};
                float acc[MAXO] = {0.f, 0.f, 0.f, 0.f}, acn[MAXO] = {0.f, 0.f, 0.f, 0.f};  // online / target net, both on s'
#pragma unroll 2
                for (int jj = c; jj < h; jj += 16) {
                    const float4 a0 = l_rec[0][jj][0], a1 = l_rec[0][jj][1], c0 = l_rec[DBL ? 1 : 0][jj][0], c1 = l_rec[DBL ? 1 : 0][jj][1];
                    const float wa[4] = {a0.x, a0.y, a0.z, a0.w}, wc[4] = {c0.x, c0.y, c0.z, c0.w};
                    float z = a1.x, zn = c1.x;
#pragma unroll
                    for (int k = 0; k < NS; ++k) {
                        z = fmaf(wa[k], xn[k], z);
                        zn = fmaf(wc[k], xn[k], zn);
                    }
                    const float hv = act_fwd_t<ACT>(z), hn = act_fwd_t<ACT>(zn);
                    acc[0] = fmaf(a1.y, hv, acc[0]);
                    acn[0] = fmaf(c1.y, hn, acn[0]);
                    acc[1] = fmaf(a1.z, hv, acc[1]);  // (rows o >= na are staged as zeros)
                    acn[1] = fmaf(c1.z, hn, acn[1]);
                    if (na > 2) {  // (uniform)
                        acc[2] = fmaf(a1.w, hv, acc[2]);
                        acn[2] = fmaf(c1.w, hn, acn[2]);
                    }
                    if (na == 4) {
                        acc[3] = fmaf(l_rec[0][jj][2].x, hv, acc[3]);
                        acn[3] = fmaf(l_rec[DBL ? 1 : 0][jj][2].x, hn, acn[3]);
                    }
                }
                float q[MAXO], qt[MAXO];
#pragma unroll
                for (int o = 0; o < MAXO; ++o) {
                    q[o] = 0.f, qt[o] = 0.f;
                    if (o < na) {  // (uniform)
                        q[o] = group_sum_dpp<16>(acc[o]) + bq[o];
                        qt[o] = group_sum_dpp<16>(acn[o]) + btq[o];
                    }
                }
                y = sf_double_target(y, tout, g.gamma_eff, q[0], q[1], q[2], q[3], qt[0], qt[1], qt[2], qt[3], na);
                tout = 1u;
            }
            const int64_t b = (int64_t)tile * SF_TILE + smp;
            if (b < g.batch && c < 4) {  // lanes 0..3 of the row: the four quarters of one 64-byte line, one store instruction
                nt_u32x4 o4 = {0u, 0u, 0u, 0u};
                if (c == 0) o4 = l_s[smp];
                else if (c == 1) o4 = nt_u32x4{uw[0], __float_as_uint(y), tout, 0u};
                else if (c == 2) o4 = un;
                *reinterpret_cast<nt_u32x4*>(g.out + b * RING_REC_BYTES + 16 * c) = o4;
                if (c == 0 && g.iota) g.iota[b] = b;
            }
        }
        __syncthreads();  // the next tile overwrites l_s / l_w / l_sn / l_rew
    }
}

}  // namespace rlhip

using namespace rlhip;

extern "C" int32_t rlhip_dqn_sample_fold_f32(const rlhip_ring* rb, int64_t batch, int32_t n_step, int32_t double_dqn, float gamma,
                                             uint64_t seed, uint32_t draw_ctr, int64_t h, int64_t na, int32_t act, const float* params,
                                             const float* target_params, rlhip_ring* folded, int64_t* idx_out, int64_t* iota_out,
                                             rlhip_stream_t stream) {
    RLHIP_REQUIRE(rb && folded && batch >= 1, "bad arguments");
    RLHIP_REQUIRE(n_step >= 1 && n_step <= SF_MAX_NSTEP, "n_step must be in 1..32");
    RLHIP_REQUIRE(rb->layout == RLHIP_RING_RECORDS && rb->elem_bytes == 4 && rb->state != nullptr,
                  "the sample + fold launch is defined for record rings (Float32 observations, obs_dim <= 4)");
    RLHIP_REQUIRE(rb->obs_dim >= 2 && rb->obs_dim <= 4, "the DQN learners take obs_dim 2..4");
    RLHIP_REQUIRE(h >= 4 && h <= SF_HMAX && h % 4 == 0, "hidden must be a multiple of 4, <= 256");
    RLHIP_REQUIRE(na >= 1 && na <= MAXO, "na must be <= 4");
    RLHIP_REQUIRE(act == 0 || act == 1, "act must be 0 (relu) or 1 (tanh)");
    RLHIP_REQUIRE(!double_dqn || (params && target_params), "double_dqn needs the online and the target parameters");
    RLHIP_REQUIRE(folded->layout == RLHIP_RING_RECORDS && folded->state != nullptr && folded->capacity >= 1 && folded->n_env == batch &&
                      folded->obs_dim == rb->obs_dim,
                  "`folded` must be a record ring initialised with rlhip_ring_init(capacity >= 1, n_env = batch, the source's obs_dim)");
    RLHIP_REQUIRE(folded->state != rb->state, "`folded` must not alias the source ring");
    RLHIP_REQUIRE(rb->len_rt >= 1, "cannot sample from an empty trajectory");
    RLHIP_REQUIRE(rb->len_rt >= n_step, "the trajectory holds fewer than n_step transitions");
    RLHIP_REQUIRE(rb->len_rt <= rb->capacity && rb->head_sa >= 0 && rb->head_sa <= rb->capacity, "ring counters out of range");
    // (nothing for the bounds-checked build to validate: the indices are the launch's own, < total by construction)
    SampleFoldArgs g;
    g.ring = {(const uint8_t*)rb->state, rb->capacity, rb->n_env, rb->head_sa};
    g.len_rt = rb->len_rt;
    g.total = (uint64_t)(rb->len_rt - n_step + 1) * (uint64_t)rb->n_env;
    g.seed = seed;
    g.draw_ctr = draw_ctr;
    g.params = params;
    g.tparams = target_params;
    g.batch = batch;
    g.out = (uint8_t*)folded->state;
    g.idx_out = idx_out;
    g.iota = iota_out;
    g.h = (int)h;
    g.na = (int)na;
    g.n_step = (int)n_step;
    const int64_t tiles = (batch + SF_TILE - 1) / SF_TILE;
    RLHIP_REQUIRE(tiles <= INT32_MAX, "batch too large");
    g.num_tiles = (int)tiles;
    g.gamma = gamma;
    g.gamma_eff = rlhip_gamma_pow(gamma, n_step);
    const int nb = g.num_tiles < SF_MAX_BLOCKS ? g.num_tiles : SF_MAX_BLOCKS;
    const int ns = (int)rb->obs_dim;
    hipStream_t s = as_stream(stream);
#define LAUNCH_SF2(NS_, ACT_)                                                                                                  \
    do {                                                                                                                       \
        if (double_dqn) hipLaunchKernelGGL((dqn_sample_fold_kernel<NS_, ACT_, true>), dim3(nb), dim3(SF_THREADS), 0, s, g);     \
        else hipLaunchKernelGGL((dqn_sample_fold_kernel<NS_, ACT_, false>), dim3(nb), dim3(SF_THREADS), 0, s, g);               \
    } while (0)
#define LAUNCH_SF(NS_)                    \
    do {                                  \
        if (act == 0) LAUNCH_SF2(NS_, 0); \
        else LAUNCH_SF2(NS_, 1);          \
    } while (0)
    if (ns == 4) LAUNCH_SF(4);
    else if (ns == 3) LAUNCH_SF(3);
    else LAUNCH_SF(2);
#undef LAUNCH_SF
#undef LAUNCH_SF2
    RLHIP_LAUNCH_CHECK();
    // slot 0 of `folded` now holds `batch` complete transitions: one stored vec-step of a `batch`-env ring
    folded->head_sa = 0;
    folded->len_sa = 2;
    folded->head_rt = 0;
    folded->len_rt = 1;
    return RLHIP_OK;
}
