// dqn_sample_fold.hip -- the folded batch of a two-layer DQN learner in ONE launch: the sampler's draw, the n-step window fold and
// the Double DQN target, i.e. what the per-stage learner (DQNLearner.optimise_ / _optimise_double_) issues as
//
//     rlhip_ring_sample_indices[_nstep]  ->  rlhip_ring_fold_nstep (n_step > 1)  ->  rlhip_dqn_fold_double_f32 (double_dqn)
//
// Two of those launches do nothing but hand a tile's worth of indices and records to the next one through memory.  Here the lane
// that owns sample b draws its own index (the Philox draw of sample_indices_kernel, as dqn_grad_kernel does inline), walks its
// window (fold_device.h's `fold_window`) and leaves the folded transition in LDS, where the tile structure of dqn_fold_double_kernel
// (dqn_double.hip) takes it up unchanged, made of the same stages of fold_device.h: both nets staged as l_rec unit records while the
// first record's loads are in flight, row = sample, the 16 lanes of a DPP row walk the hidden units of both nets on s', first
// maximum wins, lanes 0..3 of the row store the record as one 64-byte line.  Results are byte for byte those of the composition
// (tests/test_gpu_fused_folds.py), whose window walk is fold_nstep_kernel's own.
//
// Cost: a latency chain -- n_step dependent 64-byte record reads per sample (the next read is issued only once the step before is
// known not to be terminal), then the two forwards out of LDS on one CU per tile.  No Float64, no atomics, nothing crosses a
// workgroup, no MFMA.
#include "fold_device.h"
#include "fold_host.h"

namespace rlhip {

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

template <int NS, int ACT, bool DBL>
__global__ __launch_bounds__(FOLD_THREADS) void dqn_sample_fold_kernel(SampleFoldArgs g) {
    __shared__ float4 l_rec[DBL ? 2 : 1][DBL ? FOLD_HMAX : 1][3];             // FoldNets (not allocated without DBL)
    __shared__ nt_u32x4 l_s[FOLD_TILE], l_w[FOLD_TILE], l_sn[FOLD_TILE];     // the three live quarters of each sample's FOLDED record
    __shared__ float l_rew[FOLD_MAX_NSTEP][FOLD_TILE];                        // the window's rewards, [step][sample]

    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int row = lane >> 4, c = lane & 15;
    const int h = g.h, na = g.na;
    const int smp = 4 * w + row;  // this row's sample of the tile
    bool staged = false;

    for (int tile = blockIdx.x; tile < g.num_tiles; tile += gridDim.x) {
        float bq[MAXO] = {0.f, 0.f, 0.f, 0.f}, btq[MAXO] = {0.f, 0.f, 0.f, 0.f};
        if constexpr (DBL) fold_load_out_biases<NS>(g.params, g.tparams, h, na, bq, btq);
        nt_u32x4 rs = {0u, 0u, 0u, 0u}, rw = rs, rsn = rs;
        int64_t li = 0;
        RingCursor cur = ring_cursor(g.ring, 0, 0);
        if (tid < FOLD_TILE) {
            const int64_t b = (int64_t)tile * FOLD_TILE + tid;
            const bool valid = b < g.batch;  // a lane past the batch repeats sample 0's draw: a valid window, nothing is written for it
            const u32x4 wd = philox4x32_10(g.seed, (uint32_t)(valid ? b : 0), 0, g.draw_ctr, TAG_SAMPLER);
            const int64_t fj = (int64_t)__umul64hi(((uint64_t)wd.x << 32) | (uint64_t)wd.y, g.total);
            if (valid && g.idx_out) g.idx_out[b] = fj;
            int64_t e;
            ring_split_index(fj, g.ring.n_env, li, e);
            cur = ring_cursor(g.ring, li, e);
            const uint8_t* r0 = cur.record();  // the window's first record: one fabric request
            rs = *reinterpret_cast<const nt_u32x4*>(r0);
            rw = *reinterpret_cast<const nt_u32x4*>(r0 + 16);
            rsn = *reinterpret_cast<const nt_u32x4*>(r0 + 32);
        }
        if constexpr (DBL) {
            if (!staged) {  // once per workgroup, while the first record is in flight
                staged = true;
                fold_stage_two_nets<NS>(l_rec, g.params, g.tparams, h, na, tid);
            }
        }
        if (tid < FOLD_TILE) {
            uint32_t term = (rw[2] & 0xffu) ? 1u : 0u;
            float ret = __uint_as_float(rw[1]);  // n_step == 1: the stored reward as it stands
            if (g.n_step > 1) ret = fold_window(l_rew, tid, cur, li, g.len_rt, g.n_step, g.gamma, ret, term, rsn);
            l_s[tid] = rs;
            l_w[tid] = nt_u32x4{rw[0], __float_as_uint(ret), term, 0u};
            l_sn[tid] = rsn;
        }
        __syncthreads();
        {
            const nt_u32x4 un = l_sn[smp], uw = l_w[smp];
            float y = __uint_as_float(uw[1]);
            uint32_t tout = uw[2];
            if constexpr (DBL) {
                float q[MAXO], qt[MAXO];
                fold_two_net_q<NS, ACT>(l_rec, un, h, na, c, bq, btq, q, qt);
                y = double_target(y, tout, g.gamma_eff, q[0], q[1], q[2], q[3], qt[0], qt[1], qt[2], qt[3], na);
                tout = 1u;
            }
            const int64_t b = (int64_t)tile * FOLD_TILE + smp;
            if (b < g.batch && c < 4) fold_store_row(g.out, g.iota, b, c, l_s[smp], uw[0], y, tout, un);
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
    RLHIP_REQUIRE(n_step >= 1 && n_step <= FOLD_MAX_NSTEP, "n_step must be in 1..32");
    RLHIP_REQUIRE(rb->layout == RLHIP_RING_RECORDS && rb->elem_bytes == 4 && rb->state != nullptr,
                  "the sample + fold launch is defined for record rings (Float32 observations, obs_dim <= 4)");
    RLHIP_REQUIRE(rb->obs_dim >= 2 && rb->obs_dim <= 4, "the DQN learners take obs_dim 2..4");
    int32_t rc = check_mlp2_fold_net(h, na, act);
    if (rc) return rc;
    RLHIP_REQUIRE(!double_dqn || (params && target_params), "double_dqn needs the online and the target parameters");
    rc = check_folded_dest(rb, folded, batch);
    if (rc) return rc;
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
    const int64_t tiles = (batch + FOLD_TILE - 1) / FOLD_TILE;
    RLHIP_REQUIRE(tiles <= INT32_MAX, "batch too large");
    g.num_tiles = (int)tiles;
    g.gamma = gamma;
    g.gamma_eff = rlhip_gamma_pow(gamma, n_step);
    const int nb = g.num_tiles < FOLD_MAX_BLOCKS ? g.num_tiles : FOLD_MAX_BLOCKS;
    const int ns = (int)rb->obs_dim;
    hipStream_t s = as_stream(stream);
#define LAUNCH_SF2(NS_, ACT_)                                                                                                  \
    do {                                                                                                                       \
        if (double_dqn) hipLaunchKernelGGL((dqn_sample_fold_kernel<NS_, ACT_, true>), dim3(nb), dim3(FOLD_THREADS), 0, s, g);     \
        else hipLaunchKernelGGL((dqn_sample_fold_kernel<NS_, ACT_, false>), dim3(nb), dim3(FOLD_THREADS), 0, s, g);               \
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
    mark_folded(folded);
    return RLHIP_OK;
}
