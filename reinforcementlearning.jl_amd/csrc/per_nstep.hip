// per_nstep.hip -- prioritized n-step replay (RLTrajectories 0.4 `sample(::NStepBatchSampler, ::CircularPrioritizedTraces)`: the
// priorities are multiplied by a validity mask -- "n transitions lie at or after this start" -- and the draw is made from the
// product; un-vendored like the rest of the prioritized path, PARITY UNPINNED).
//
// The mask lives in the TREE: rlhip_ring_push_priority_nstep holds the leaves of the newest n_step - 1 transition frames at 0 and
// hands a frame its default priority only once n_step transitions lie at or after it.  The descent of the shipped sampler never
// enters a zero-sum subtree, so the UNCHANGED draw (rlhip_ring_sample_prioritized) returns only valid window starts, distributed as
// p * valid / sum(p * valid): no new sampling arithmetic.  rlhip_ring_push_priority_nstep_frames is the same rule for frame rings
// (one body: the keys are `physical rt frame * n_env + e` in both layouts); their draw + gather launch is per_frames_nstep.hip.
//
// rlhip_per_sample_fold_nstep_f32 is that draw and the window fold (rlhip_ring_fold_nstep) in ONE launch, as dqn_sample_fold.hip is
// for the uniform sampler: the lane that owns sample b makes the draw of sumtree_sample_kernel (sumtree_device.h's `sumtree_draw`:
// the sampler's own), maps the leaf key to its logical index, walks its window (fold_device.h's `fold_window`) and writes the folded
// record as one whole 64-byte line.  Outputs are byte for byte those of the two launches (tests/test_gpu_per_nstep.py), whose window
// walk is fold_nstep_kernel's own.
//
// Cost: one latency chain per sample -- log2(P) dependent 8-byte tree reads (L2 resident: 1M leaves = 8 MB), then up to n_step
// dependent 64-byte record reads (the next one is issued only once the step before is known not to be terminal).  One wavefront per
// workgroup, so that a batch of 512 spreads its chains over 8 CUs; the window's rewards wait in LDS, [step][lane]: consecutive
// dwords per step, conflict-free, and no dynamically indexed register array (no scratch).  No Float64, no atomics, nothing crosses
// a workgroup, no barrier, no MFMA.
#include "fold_device.h"
#include "fold_host.h"
#include "sumtree_device.h"

namespace rlhip {

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

__global__ __launch_bounds__(FOLD_TILE) void per_sample_fold_nstep_kernel(PerNstepArgs g) {  // one wavefront per workgroup
    __shared__ float l_rew[FOLD_MAX_NSTEP][FOLD_TILE];  // the window's rewards, [step][lane]
    const int tid = threadIdx.x;
    const int64_t b = (int64_t)blockIdx.x * FOLD_TILE + tid;
    if (b >= g.batch) return;  // (no barrier below: a lane's LDS column is its own)
    const int64_t leaf = sumtree_draw(g.tree, g.P, g.n_leaves, g.seed, b, g.draw_ctr);
    if (g.key_out) g.key_out[b] = leaf;
    if (g.prio_out) g.prio_out[b] = g.tree[g.P + leaf];
    int64_t pt, e;  // physical transition frame, env
    ring_split_index(leaf, g.ring.n_env, pt, e);
    int64_t li = pt - g.head_rt;
    if (li < 0) li += g.ring.capacity;
    g.idx_out[b] = li * g.ring.n_env + e;  // logical flat index, the convention of rlhip_ring_gather
    const RingCursor cur = ring_cursor(g.ring, li, e);
    const uint8_t* r0 = cur.record();
    const nt_u32x4 rs = *reinterpret_cast<const nt_u32x4*>(r0);
    const nt_u32x4 rw = *reinterpret_cast<const nt_u32x4*>(r0 + 16);
    nt_u32x4 rsn = *reinterpret_cast<const nt_u32x4*>(r0 + 32);
    uint32_t term = (rw[2] & 0xffu) ? 1u : 0u;
    const float gain = fold_window(l_rew, tid, cur, li, g.len_rt, g.n_step, g.gamma, __uint_as_float(rw[1]), term, rsn);
    fold_store_record(g.out, g.iota, b, rs, rw[0], gain, term, rsn);
}

}  // namespace rlhip

using namespace rlhip;

// the lagged push of both layouts: the sum-tree's keys are `physical rt frame * n_env + e` whatever holds the transitions, so the
// rule never looks at the storage; `layout` / `layout_message` say which rings the calling entry point serves
static int32_t push_priority_nstep(const rlhip_ring* rb, float* tree, float priority, int32_t n_step, rlhip_stream_t stream,
                                   int32_t layout, const char* layout_message) {
    RLHIP_REQUIRE(rb && tree, "bad arguments");
    RLHIP_REQUIRE(n_step >= 1 && n_step <= FOLD_MAX_NSTEP, "n_step must be in 1..32");
    RLHIP_REQUIRE(rb->layout == layout, layout_message);
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

extern "C" int32_t rlhip_ring_push_priority_nstep(const rlhip_ring* rb, float* tree, float priority, int32_t n_step,
                                                  rlhip_stream_t stream) {
    return push_priority_nstep(rb, tree, priority, n_step, stream, RLHIP_RING_RECORDS,
                               "n-step priorities are defined for record rings (Float32 observations, obs_dim <= 4)");
}

extern "C" int32_t rlhip_ring_push_priority_nstep_frames(const rlhip_ring* rb, float* tree, float priority, int32_t n_step,
                                                         rlhip_stream_t stream) {
    return push_priority_nstep(rb, tree, priority, n_step, stream, RLHIP_RING_FRAMES,
                               "this push serves frame rings; a record ring (Float32 observations, obs_dim <= 4) takes "
                               "rlhip_ring_push_priority_nstep");
}

extern "C" int32_t rlhip_per_sample_fold_nstep_f32(const rlhip_ring* rb, const float* tree, int64_t batch, int32_t n_step, float gamma,
                                                   uint64_t seed, uint32_t draw_ctr, int64_t* idx_out, int64_t* key_out,
                                                   float* prio_out, rlhip_ring* folded, int64_t* iota_out, rlhip_stream_t stream) {
    RLHIP_REQUIRE(rb && tree && folded && idx_out && batch >= 1, "bad arguments");
    RLHIP_REQUIRE(n_step >= 1 && n_step <= FOLD_MAX_NSTEP, "n_step must be in 1..32");
    RLHIP_REQUIRE(rb->layout == RLHIP_RING_RECORDS && rb->elem_bytes == 4 && rb->state != nullptr,
                  "the prioritized sample + fold launch is defined for record rings (Float32 observations, obs_dim <= 4)");
    const int32_t rc = check_folded_dest(rb, folded, batch);
    if (rc) return rc;
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
    g.P = pow2_ge(g.n_leaves);
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
    const int64_t tiles = (batch + FOLD_TILE - 1) / FOLD_TILE;
    RLHIP_REQUIRE(tiles <= INT32_MAX, "batch too large");
    hipLaunchKernelGGL(per_sample_fold_nstep_kernel, dim3((int)tiles), dim3(FOLD_TILE), 0, as_stream(stream), g);
    RLHIP_LAUNCH_CHECK();
    mark_folded(folded);
    return RLHIP_OK;
}
