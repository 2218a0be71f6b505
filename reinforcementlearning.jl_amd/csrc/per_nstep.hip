// per_nstep.hip -- prioritized n-step replay (RLTrajectories 0.4 `sample(::NStepBatchSampler, ::CircularPrioritizedTraces)`: the
// priorities are multiplied by a validity mask -- "n transitions lie at or after this start" -- and the draw is made from the
// product; un-vendored like the rest of the prioritized path, PARITY UNPINNED).
//
// The mask lives in the TREE: rlhip_ring_push_priority_nstep holds the leaves of the newest n_step - 1 transition frames at 0 and
// hands a frame its default priority only once n_step transitions lie at or after it.  The descent of the shipped sampler never
// enters a zero-sum subtree, so the UNCHANGED draw (rlhip_ring_sample_prioritized) returns only valid window starts, distributed as
// p * valid / sum(p * valid): no new sampling arithmetic.
//
// rlhip_per_sample_fold_nstep_f32 is that draw and the window fold (rlhip_ring_fold_nstep) in ONE launch, as dqn_sample_fold.hip is
// for the uniform sampler: the lane that owns sample b makes the Philox draw of sumtree_sample_kernel, descends (sumtree_descend,
// sumtree_device.h: the sampler's own), maps the leaf key to its logical index, walks its window -- fold_nstep_kernel's walk and its
// right-to-left Float32 return, operation for operation -- and writes the folded record as one whole 64-byte line.  Outputs are
// byte for byte those of the two launches (tests/test_gpu_per_nstep.py).
//
// Cost: one latency chain per sample -- log2(P) dependent 8-byte tree reads (L2 resident: 1M leaves = 8 MB), then up to n_step
// dependent 64-byte record reads (the next one is issued only once the step before is known not to be terminal).  One wavefront per
// workgroup, so that a batch of 512 spreads its chains over 8 CUs; the window's rewards wait in LDS, [step][lane]: consecutive
// dwords per step, conflict-free, and no dynamically indexed register array (no scratch).  No Float64, no atomics, nothing crosses
// a workgroup, no barrier, no MFMA.
#include "ring_device.h"
#include "sumtree_device.h"

namespace rlhip {

constexpr int PN_TILE = 64;  // samples per workgroup = one wavefront
constexpr int PN_MAX_NSTEP = 32;

struct PerNstepArgs {
    const float* tree;
    int64_t P, n_leaves;
    RingRecs ring;
    int64_t head_rt, len_rt;
    int64_t batch;
    uint64_t seed;
    uint32_t draw_ctr;
    int n_step;
    float gamma;
    uint8_t* out;       // slot 0 of the folded ring: `batch` records
    int64_t* idx_out;
    int64_t* key_out;   // nullable
    float* prio_out;    // nullable
    int64_t* iota;      // nullable
};

__global__ __launch_bounds__(PN_TILE) void per_sample_fold_nstep_kernel(PerNstepArgs g) {
    __shared__ float l_rew[PN_MAX_NSTEP][PN_TILE];  // the window's rewards, [step][lane]
    const int tid = threadIdx.x;
    const int64_t b = (int64_t)blockIdx.x * PN_TILE + tid;
    if (b >= g.batch) return;  // (no barrier below: a lane's LDS column is its own)
    // ---- the draw of sumtree_sample_kernel<true> ----
    const u32x4 w = philox4x32_10(g.seed, (uint32_t)b, 0, g.draw_ctr, TAG_SAMPLER);
    const float v = u01_f32(w.z) * g.tree[1];  // rand(rng, Float32) * t.tree[1]
    int64_t leaf = sumtree_descend(g.tree, g.P, v);
    if (leaf >= g.n_leaves) leaf = g.n_leaves - 1;
    if (g.key_out) g.key_out[b] = leaf;
    if (g.prio_out) g.prio_out[b] = g.tree[g.P + leaf];
    const int64_t n_env = g.ring.n_env;
    int64_t pt, e;  // physical transition frame, env (no 64-bit division where 32 bits do: ring_device.h)
    if (((uint64_t)leaf | (uint64_t)n_env) >> 32) {
        pt = leaf / n_env;
        e = leaf - pt * n_env;
    } else {
        const uint32_t q = (uint32_t)leaf / (uint32_t)n_env;
        pt = q;
        e = (uint32_t)leaf - q * (uint32_t)n_env;
    }
    int64_t li = pt - g.head_rt;
    if (li < 0) li += g.ring.capacity;
    const int64_t fj = li * n_env + e;  // logical flat index, the convention of rlhip_ring_gather
    g.idx_out[b] = fj;
    // ---- fold_nstep_kernel's walk: the window li .. li + ns - 1 of env e, up to and including the first terminal step.  The record
    // of logical step li + k sits in state slot (head_sa + li + k) mod (capacity + 1) (ring_record_offset without its division:
    // li + k < len_rt <= capacity, so the sum wraps at most once) ----
    int64_t ps = g.ring.head_sa + li;
    if (ps > g.ring.capacity) ps -= g.ring.capacity + 1;
    const uint8_t* r0 = g.ring.rec + (ps * n_env + e) * RING_REC_BYTES;
    const nt_u32x4 rs = *reinterpret_cast<const nt_u32x4*>(r0);
    const nt_u32x4 rw = *reinterpret_cast<const nt_u32x4*>(r0 + 16);
    nt_u32x4 rsn = *reinterpret_cast<const nt_u32x4*>(r0 + 32);
    uint32_t term = (rw[2] & 0xffu) ? 1u : 0u;
    l_rew[0][tid] = __uint_as_float(rw[1]);
    int ns = 1;
    for (int k = 1; k < g.n_step && !term && li + k < g.len_rt; ++k) {  // (never past the newest stored transition)
        ps = (ps == g.ring.capacity) ? 0 : ps + 1;
        const uint8_t* rk = g.ring.rec + (ps * n_env + e) * RING_REC_BYTES;
        const nt_u32x4 kw = *reinterpret_cast<const nt_u32x4*>(rk + 16);
        rsn = *reinterpret_cast<const nt_u32x4*>(rk + 32);
        l_rew[k][tid] = __uint_as_float(kw[1]);
        term = (kw[2] & 0xffu) ? 1u : 0u;
        ns = k + 1;
    }
    float gain = 0.0f;  // discount_rewards_reduced: gain = r[k] + gamma * gain from the window's end
    for (int k = ns - 1; k >= 0; --k) gain = l_rew[k][tid] + g.gamma * gain;
    // ---- the folded record: the lane's own 64-byte line, all four quarters ----
    uint8_t* o = g.out + b * RING_REC_BYTES;
    *reinterpret_cast<nt_u32x4*>(o) = rs;
    *reinterpret_cast<nt_u32x4*>(o + 16) = nt_u32x4{rw[0], __float_as_uint(gain), term, 0u};
    *reinterpret_cast<nt_u32x4*>(o + 32) = rsn;
    *reinterpret_cast<nt_u32x4*>(o + 48) = nt_u32x4{0u, 0u, 0u, 0u};
    if (g.iota) g.iota[b] = b;
}

static inline int64_t pn_pow2_ge(int64_t n) {
    int64_t p = 1;
    while (p < n) p <<= 1;
    return p;
}

}  // namespace rlhip

using namespace rlhip;

extern "C" int32_t rlhip_ring_push_priority_nstep(const rlhip_ring* rb, float* tree, float priority, int32_t n_step,
                                                  rlhip_stream_t stream) {
    RLHIP_REQUIRE(rb && tree, "bad arguments");
    RLHIP_REQUIRE(n_step >= 1 && n_step <= PN_MAX_NSTEP, "n_step must be in 1..32");
    RLHIP_REQUIRE(rb->layout == RLHIP_RING_RECORDS, "n-step priorities are defined for record rings (Float32 observations, obs_dim <= 4)");
    RLHIP_REQUIRE(n_step <= rb->capacity, "n_step exceeds the ring's capacity: no window would ever be complete");
    RLHIP_REQUIRE(priority >= 0.0f, "priorities must be non-negative");
    RLHIP_REQUIRE(rb->len_rt >= 1, "no transition has been pushed yet");
    RLHIP_REQUIRE(rb->len_rt <= rb->capacity && rb->head_rt >= 0 && rb->head_rt < rb->capacity, "ring counters out of range");
    const int64_t n_leaves = rb->capacity * rb->n_env;
    const int64_t newest = (rb->head_rt + rb->len_rt - 1) % rb->capacity;
    if (n_step > 1) {  // the newest frame starts no complete window (after a wrap its leaves still carry the overwritten transition's priority)
        const int32_t rc = rlhip_sumtree_fill_range(tree, n_leaves, newest * rb->n_env, rb->n_env, 0.0f, stream);
        if (rc != RLHIP_OK) return rc;
        if (rb->len_rt < n_step) return RLHIP_OK;
    }
    // logical frame len_rt - n_step: n_step transitions lie at or after it from now on (n_step = 1: the newest frame itself, the
    // one fill of rlhip_ring_push_priority -- the tree is a pure function of its leaves)
    const int64_t ready = (rb->head_rt + rb->len_rt - n_step) % rb->capacity;
    return rlhip_sumtree_fill_range(tree, n_leaves, ready * rb->n_env, rb->n_env, priority, stream);
}

extern "C" int32_t rlhip_per_sample_fold_nstep_f32(const rlhip_ring* rb, const float* tree, int64_t batch, int32_t n_step, float gamma,
                                                   uint64_t seed, uint32_t draw_ctr, int64_t* idx_out, int64_t* key_out,
                                                   float* prio_out, rlhip_ring* folded, int64_t* iota_out, rlhip_stream_t stream) {
    RLHIP_REQUIRE(rb && tree && folded && idx_out && batch >= 1, "bad arguments");
    RLHIP_REQUIRE(n_step >= 1 && n_step <= PN_MAX_NSTEP, "n_step must be in 1..32");
    RLHIP_REQUIRE(rb->layout == RLHIP_RING_RECORDS && rb->elem_bytes == 4 && rb->state != nullptr,
                  "the prioritized sample + fold launch is defined for record rings (Float32 observations, obs_dim <= 4)");
    RLHIP_REQUIRE(folded->layout == RLHIP_RING_RECORDS && folded->state != nullptr && folded->capacity >= 1 && folded->n_env == batch &&
                      folded->obs_dim == rb->obs_dim,
                  "`folded` must be a record ring initialised with rlhip_ring_init(capacity >= 1, n_env = batch, the source's obs_dim)");
    RLHIP_REQUIRE(folded->state != rb->state, "`folded` must not alias the source ring");
    RLHIP_REQUIRE(rb->len_rt >= 1, "cannot sample from an empty trajectory");
    RLHIP_REQUIRE(rb->len_rt >= n_step, "the trajectory holds fewer than n_step transitions: the masked tree has no mass");
    RLHIP_REQUIRE(rb->capacity >= 1 && rb->n_env >= 1 && rb->len_rt <= rb->capacity && rb->head_sa >= 0 && rb->head_sa <= rb->capacity &&
                      rb->head_rt >= 0 && rb->head_rt < rb->capacity,
                  "ring counters out of range");
    // (nothing for the bounds-checked build to validate: the indices are the launch's own -- a leaf key is clamped below
    // capacity * n_env, so every record read stays inside the ring's (capacity + 1) * n_env records)
    PerNstepArgs g;
    g.tree = tree;
    g.n_leaves = rb->capacity * rb->n_env;
    g.P = pn_pow2_ge(g.n_leaves);
    g.ring = {(const uint8_t*)rb->state, rb->capacity, rb->n_env, rb->head_sa};
    g.head_rt = rb->head_rt;
    g.len_rt = rb->len_rt;
    g.batch = batch;
    g.seed = seed;
    g.draw_ctr = draw_ctr;
    g.n_step = (int)n_step;
    g.gamma = gamma;
    g.out = (uint8_t*)folded->state;
    g.idx_out = idx_out;
    g.key_out = key_out;
    g.prio_out = prio_out;
    g.iota = iota_out;
    const int64_t tiles = (batch + PN_TILE - 1) / PN_TILE;
    RLHIP_REQUIRE(tiles <= INT32_MAX, "batch too large");
    hipLaunchKernelGGL(per_sample_fold_nstep_kernel, dim3((int)tiles), dim3(PN_TILE), 0, as_stream(stream), g);
    RLHIP_LAUNCH_CHECK();
    // slot 0 of `folded` now holds `batch` complete transitions: one stored vec-step of a `batch`-env ring
    folded->head_sa = 0;
    folded->len_sa = 2;
    folded->head_rt = 0;
    folded->len_rt = 1;
    return RLHIP_OK;
}
