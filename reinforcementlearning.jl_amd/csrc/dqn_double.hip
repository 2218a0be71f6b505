// dqn_double.hip -- Double DQN targets as an on-device batch fold (the removed DQNLearner's
// `is_enable_double_DQN`, on by default there).
//
// Double DQN replaces the bootstrap value max_a' Qt(s', a') by Qt(s', a*), a* = findmax(Q_online(s')) (first maximum wins,
// RLCore/src/utils/basic.jl:91-120).  Instead of a second copy of every tuned gradient kernel, the sampled batch is rewritten --
// like rlhip_ring_fold_nstep rewrites an n-step window -- into records the UNCHANGED kernels take:
//
//     {s, a, r, t, s'}  ->  {s, a, y = r + gamma_eff * (1 - t) * Qt(s')[a*], terminal = 1, s'}
//
// Exactness.  Every gradient kernel's target line is G = r + gamma * cont * mx with cont = 1 - terminal (dqn.hip, the MFMA learners
// and oracle/rlo_learn.c alike; -ffp-contract=off is the build contract).  With the record's reward = y and terminal = 1 that is
// G = y + gamma * 0 * mx = y + 0 = y bit for bit, for any finite Qt(s'): the kernel's own target forward becomes redundant work, its
// Huber / backward half is the Double DQN update.  The price is this one launch plus that redundant forward.
//
// Two-layer nets: ONE launch with the phase-0 / phase-1 structure of dqn_grad_kernel (dqn.hip) -- 64 lanes request their sample's
// 64-byte record (one fabric request per sample: the gather is bound by requests) while all lanes stage both
// networks into LDS; then row = sample, the 16 lanes of a DPP row walk the hidden units of BOTH nets on s' (the very accumulation
// order of the gradient kernel's Qt(s')), select, and lanes 0..3 of the row store the four 16-byte quarters of the new record as one
// 64-byte line.  No Float64, no atomics, nothing crosses a workgroup: a record is read and written by the same workgroup, so the fold
// may run IN PLACE on an already folded ring (n-step first, then double with gamma^n).
//
// Three-layer nets (bf16 MFMA forward): composition -- gather s' into the workspace, the shipped forward (rlhip_dqn3_plan_f32,
// actions = NULL) once per net, one select-and-write kernel.  No MFMA code lives in this file.
#include "fold_device.h"
#include "fold_host.h"

namespace rlhip {

struct FoldDoubleArgs {
    RingRecs ring;
    const float* params;
    const float* tparams;
    const int64_t* idx;
    int64_t batch;
    uint8_t* out;   // slot 0 of the folded ring: `batch` records
    int64_t* iota;  // nullable
    int h, na, num_tiles;
    float gamma;
};

template <int NS, int ACT>
__global__ __launch_bounds__(FOLD_THREADS) void dqn_fold_double_kernel(FoldDoubleArgs g) {
    __shared__ FoldNets l_rec;
    __shared__ nt_u32x4 l_s[FOLD_TILE], l_w[FOLD_TILE], l_sn[FOLD_TILE];  // the three live quarters of each sample's record

    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int row = lane >> 4, c = lane & 15;
    const int h = g.h, na = g.na;
    const int smp = 4 * w + row;  // this row's sample of the tile
    bool staged = false;

    for (int tile = blockIdx.x; tile < g.num_tiles; tile += gridDim.x) {
        float bq[MAXO], btq[MAXO];
        fold_load_out_biases<NS>(g.params, g.tparams, h, na, bq, btq);
        nt_u32x4 rs = {0u, 0u, 0u, 0u}, rw = rs, rsn = rs;
        if (tid < FOLD_TILE) {
            const int64_t b = (int64_t)tile * FOLD_TILE + tid;
            const int64_t fj = g.idx[b < g.batch ? b : 0];
            const uint8_t* r0 = g.ring.rec + ring_record_offset(g.ring, fj);  // one 64-byte record = one fabric request per sample
            rs = *reinterpret_cast<const nt_u32x4*>(r0);
            rw = *reinterpret_cast<const nt_u32x4*>(r0 + 16);
            rsn = *reinterpret_cast<const nt_u32x4*>(r0 + 32);
        }
        if (!staged) {  // once per workgroup, while the gather is in flight
            staged = true;
            fold_stage_two_nets<NS>(l_rec, g.params, g.tparams, h, na, tid);
        }
        if (tid < FOLD_TILE) {
            l_s[tid] = rs;
            l_w[tid] = rw;
            l_sn[tid] = rsn;
        }
        __syncthreads();
        {
            const nt_u32x4 un = l_sn[smp], uw = l_w[smp];
            float q[MAXO], qt[MAXO];
            fold_two_net_q<NS, ACT>(l_rec, un, h, na, c, bq, btq, q, qt);
            const float y = double_target(__uint_as_float(uw[1]), uw[2] & 0xffu, g.gamma, q[0], q[1], q[2], q[3], qt[0], qt[1], qt[2], qt[3], na);
            const int64_t b = (int64_t)tile * FOLD_TILE + smp;
            if (b < g.batch && c < 4) fold_store_row(g.out, g.iota, b, c, l_s[smp], uw[0], y, 1u, un);
        }
        __syncthreads();  // the next tile overwrites l_s / l_w / l_sn
    }
}

// ---- three-layer composition: s' of every sample as the (ns x batch) observation block the plan kernels read
__global__ __launch_bounds__(256) void fold_double_gather_next_kernel(RingRecs ring, const int64_t* __restrict__ idx, int64_t batch, int ns,
                                                                      float* __restrict__ obs) {
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= batch) return;
    RingChunk sn;
    sn.u = *reinterpret_cast<const nt_u32x4*>(ring.rec + ring_record_offset(ring, idx[b]) + 32);
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (k < ns) obs[(int64_t)k * batch + b] = sn.f[k];
}

// ... and, behind the two forwards, one lane per sample: read the record, select, write the folded record (the same lane reads and
// writes record b: in-place safe)
__global__ __launch_bounds__(256) void fold_double_select_kernel(RingRecs ring, const int64_t* __restrict__ idx, int64_t batch, int na,
                                                                 const float* __restrict__ q_on, const float* __restrict__ q_tg, float gamma,
                                                                 uint8_t* out, int64_t* __restrict__ iota) {  // (out may be the ring)
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= batch) return;
    const uint8_t* r0 = ring.rec + ring_record_offset(ring, idx[b]);
    const nt_u32x4 rs = *reinterpret_cast<const nt_u32x4*>(r0);
    const nt_u32x4 rw = *reinterpret_cast<const nt_u32x4*>(r0 + 16);
    const nt_u32x4 rsn = *reinterpret_cast<const nt_u32x4*>(r0 + 32);
    float q[MAXO] = {0.f, 0.f, 0.f, 0.f}, qt[MAXO] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int o = 0; o < MAXO; ++o)
        if (o < na) {
            q[o] = q_on[(int64_t)o * batch + b];
            qt[o] = q_tg[(int64_t)o * batch + b];
        }
    const float y = double_target(__uint_as_float(rw[1]), rw[2] & 0xffu, gamma, q[0], q[1], q[2], q[3], qt[0], qt[1], qt[2], qt[3], na);
    fold_store_record(out, iota, b, rs, rw[0], y, 1u, rsn);
}

static inline int64_t round256(int64_t n) { return (n + 255) / 256 * 256; }

// the checks both forms share; `folded` may be the source itself when that is an already folded ring (one stored vec-step of `batch`
// envs) and idx its iota: record b is then read and rewritten by one workgroup / lane
static int32_t fold_double_check(const rlhip_ring* rb, const int64_t* idx, int64_t batch, const rlhip_ring* folded) {
    RLHIP_REQUIRE(rb && idx && folded && batch >= 1, "bad arguments");
    RLHIP_REQUIRE(rb->layout == RLHIP_RING_RECORDS && rb->elem_bytes == 4,
                  "the Double DQN fold is defined for record rings (Float32 observations, obs_dim <= 4)");
    RLHIP_REQUIRE(rb->obs_dim >= 2 && rb->obs_dim <= 4, "the DQN learners take obs_dim 2..4");
    const int32_t rc = check_folded_dest(rb, folded, batch, /*may_alias=*/true);
    if (rc) return rc;
    RLHIP_REQUIRE(folded->state != rb->state || (rb->n_env == batch && rb->head_sa == 0 && rb->len_rt == 1),
                  "in place (`folded` = the source) only on an already folded ring: one stored vec-step of `batch` envs, idx = its iota");
    RLHIP_REQUIRE(rb->len_rt >= 1, "cannot sample from an empty trajectory");
    return RLHIP_OK;
}

}  // namespace rlhip

using namespace rlhip;

extern "C" {

int64_t rlhip_dqn_double_workspace_bytes(int64_t ns, int64_t h, int64_t na, int64_t batch, int32_t layers) {
    (void)h;
    if (ns < 1 || na < 1 || batch < 1 || (layers != 2 && layers != 3)) return -1;
    if (layers == 2) return 0;  // the two-layer fold is one launch without scratch
    return round256(ns * batch * (int64_t)sizeof(float)) + 2 * round256(na * batch * (int64_t)sizeof(float));  // s' | Q(s') | Qt(s')
}

int32_t rlhip_dqn_fold_double_f32(const rlhip_ring* rb, int64_t h, int64_t na, int32_t act, const float* params,
                                  const float* target_params, const int64_t* idx, int64_t batch, float gamma_eff, rlhip_ring* folded,
                                  int64_t* iota_out, void* workspace, rlhip_stream_t stream) {
    (void)workspace;
    int32_t rc = fold_double_check(rb, idx, batch, folded);
    if (rc) return rc;
    RLHIP_REQUIRE(params && target_params, "NULL argument");
    rc = check_mlp2_fold_net(h, na, act);
    if (rc) return rc;
    RLHIP_CHECK_GATHER_INDICES(rb, idx, batch, stream);
    FoldDoubleArgs g;
    g.ring = {(const uint8_t*)rb->state, rb->capacity, rb->n_env, rb->head_sa};
    g.params = params;
    g.tparams = target_params;
    g.idx = idx;
    g.batch = batch;
    g.out = (uint8_t*)folded->state;
    g.iota = iota_out;
    g.h = (int)h;
    g.na = (int)na;
    const int64_t tiles = (batch + FOLD_TILE - 1) / FOLD_TILE;
    RLHIP_REQUIRE(tiles <= INT32_MAX, "batch too large");
    g.num_tiles = (int)tiles;
    g.gamma = gamma_eff;
    const int nb = g.num_tiles < FOLD_MAX_BLOCKS ? g.num_tiles : FOLD_MAX_BLOCKS;
    const int ns = (int)rb->obs_dim;
    hipStream_t s = as_stream(stream);
#define LAUNCH_FD(NS_)                                                                                              \
    do {                                                                                                            \
        if (act == 0) hipLaunchKernelGGL((dqn_fold_double_kernel<NS_, 0>), dim3(nb), dim3(FOLD_THREADS), 0, s, g);    \
        else hipLaunchKernelGGL((dqn_fold_double_kernel<NS_, 1>), dim3(nb), dim3(FOLD_THREADS), 0, s, g);             \
    } while (0)
    if (ns == 4) LAUNCH_FD(4);
    else if (ns == 3) LAUNCH_FD(3);
    else LAUNCH_FD(2);
#undef LAUNCH_FD
    RLHIP_LAUNCH_CHECK();
    mark_folded(folded);
    return RLHIP_OK;
}

int32_t rlhip_dqn3_fold_double_f32(const rlhip_ring* rb, int64_t h, int64_t na, int32_t act, const float* params, const uint16_t* packed,
                                   const float* target_params, const uint16_t* target_packed, const int64_t* idx, int64_t batch,
                                   float gamma_eff, rlhip_ring* folded, int64_t* iota_out, void* workspace, rlhip_stream_t stream) {
    int32_t rc = fold_double_check(rb, idx, batch, folded);
    if (rc) return rc;
    RLHIP_REQUIRE(params && packed && target_params && target_packed && workspace, "NULL argument");
    RLHIP_REQUIRE(h == 128 || h == 256, "the MFMA Q-network path is built for hidden = 128 or 256");
    const int64_t ns = rb->obs_dim;
    RLHIP_REQUIRE((ns == 4 && na == 2) || (ns == 2 && na == 3) || (ns == 3 && na == 3),
                  "(obs dim, actions) must be (4, 2) CartPole, (2, 3) MountainCar or (3, 3) Pendulum");
    RLHIP_REQUIRE(act == 0 || act == 1, "act must be 0 (relu) or 1 (tanh)");
    RLHIP_REQUIRE((((uintptr_t)workspace) & 15) == 0, "the workspace must be 16-byte aligned");
    RLHIP_CHECK_GATHER_INDICES(rb, idx, batch, stream);
    const RingRecs ring = {(const uint8_t*)rb->state, rb->capacity, rb->n_env, rb->head_sa};
    float* obs = (float*)workspace;
    float* q_on = (float*)((uint8_t*)workspace + round256(ns * batch * (int64_t)sizeof(float)));
    float* q_tg = (float*)((uint8_t*)q_on + round256(na * batch * (int64_t)sizeof(float)));
    hipStream_t s = as_stream(stream);
    const dim3 grid((unsigned)((batch + 255) / 256));
    hipLaunchKernelGGL(fold_double_gather_next_kernel, grid, dim3(256), 0, s, ring, idx, batch, (int)ns, obs);
    RLHIP_LAUNCH_CHECK();
    rc = rlhip_dqn3_plan_f32(params, packed, ns, h, na, act, obs, batch, 0.0, 0, 0, 0, nullptr, q_on, stream);
    if (rc) return rc;
    rc = rlhip_dqn3_plan_f32(target_params, target_packed, ns, h, na, act, obs, batch, 0.0, 0, 0, 0, nullptr, q_tg, stream);
    if (rc) return rc;
    hipLaunchKernelGGL(fold_double_select_kernel, grid, dim3(256), 0, s, ring, idx, batch, (int)na, q_on, q_tg, gamma_eff,
                       (uint8_t*)folded->state, iota_out);
    RLHIP_LAUNCH_CHECK();
    mark_folded(folded);
    return RLHIP_OK;
}

}  // extern "C"
