// dqn_step_per.hip -- one whole vec-step of the DQN agent loop as ONE C-ABI call for a learner over PRIORITIZED replay
// (host-side composition in the style of dqn_step_fold.hip, whose act dispatch, tail and checks it shares through
// dqn_step_common.h; the one new kernel it drives is per_writeback.hip).
//
// What it replaces: one trip round the body of `_run` (RLCore/src/core/run.jl:52-70) for `Agent{QBasedPolicy{DQNLearner}}` whose
// trajectory is `CircularPrioritizedTraces` (RLTrajectories 0.4) sampled by the prioritized `BatchSampler` or, with n_step > 1, by
// `NStepBatchSampler` over the masked tree -- the removed Zoo's PrioritizedDQN, with or without importance-sampling weights, Double
// DQN targets and a DuelingNetwork.  The per-stage protocol issues about eleven calls per vec-step for such a learner:
//     plan! + act! + push!                    the three-way dispatch of rlhip_dqn_vec_step_f32
//     priority push                           rlhip_ring_push_priority[_nstep]          (CircularPrioritizedTraces.push!)
//     draw [+ window fold]                    rlhip_ring_sample_prioritized / rlhip_per_sample_fold_nstep_f32
//     importance-sampling weights (beta > 0)  rlhip_per_is_weights_f32
//     Double DQN fold                         rlhip_dqn[3]_fold_double_f32, in place on the n-step batch
//     gradient                                rlhip_dqn_grad_idx[_w]_f32 / rlhip_dqn3_grad[_w]_f32, td out
//     priority write-back                     rlhip_per_priority_f32 + rlhip_sumtree_update  ->  here rlhip_per_writeback_f32
//     clip + Adam [+ pack], target sync       the tail of rlhip_dqn_vec_step_fold_f32
// This entry point enqueues the same kernels in the same order with the same arguments; the write-back is the one launch that
// equals the two byte for byte.  Results are bit-identical to the per-stage loop (tests/test_gpu_fused_per.py).
#include "common.h"
#include "dqn_step_common.h"

using namespace rlhip;

namespace {

int32_t check_per_step(const rlhip_dqn_per_step_args* p, bool folds, bool dueling) {
    const rlhip_dqn_fold_step_args* f = &p->fold;
    const rlhip_dqn_step_args* a = &f->base;
    int32_t rc = check_fold_step(f, folds, dueling);
    if (rc) return rc;
    // what every gradient entry point of a prioritized learner asks of the trajectory and the net, asked in front of the push: of a
    // folded batch check_fold_step has asked it already
    if (!folds) {
        const int64_t ns = rlhip_env_obs_dim(a->kind);
        RLHIP_REQUIRE(a->ring->layout == RLHIP_RING_RECORDS && a->ring->elem_bytes == 4 && ns >= 2 && ns <= 4,
                      "the prioritized step is defined for record rings (Float32 observations, obs_dim 2..4)");
        if (a->layers == 2) {
            rc = check_mlp2_fold_net(a->h, a->na, a->act);
            if (rc) return rc;
        } else {
            RLHIP_REQUIRE(a->h == 128 || a->h == 256, "the MFMA Q-network path is built for hidden = 128 or 256");
            RLHIP_REQUIRE(a->act == 0 || a->act == 1, "act must be 0 (relu) or 1 (tanh)");
        }
    }
    RLHIP_REQUIRE(p->tree != nullptr, "NULL tree");
    RLHIP_REQUIRE(p->default_priority > 0.0f, "default_priority must be > 0");
    RLHIP_REQUIRE(p->per_eps >= 0.0f && p->per_alpha >= 0.0f && p->per_beta >= 0.0f, "per_eps, per_alpha and per_beta must be >= 0");
    RLHIP_REQUIRE(f->n_step <= a->ring->capacity, "n_step exceeds the ring's capacity: no window would ever be complete");
    RLHIP_REQUIRE(a->ring->capacity >= 1 && a->ring->len_rt >= 0 && a->ring->len_rt <= a->ring->capacity && a->ring->head_rt >= 0 &&
                      a->ring->head_rt < a->ring->capacity,
                  "ring counters out of range");
    if (!a->do_update) return RLHIP_OK;
    RLHIP_REQUIRE(f->idx && p->key && p->prio && f->td && p->priority_out, "idx / key / prio / td / priority_out missing");
    RLHIP_REQUIRE(!(p->per_beta > 0.0f) || p->is_weights, "per_beta > 0 needs is_weights");
    RLHIP_REQUIRE(a->batch < (1ll << 31), "batch too large");
    const uintptr_t t0 = reinterpret_cast<uintptr_t>(f->td), p0 = reinterpret_cast<uintptr_t>(p->priority_out);
    const uintptr_t bytes = (uintptr_t)a->batch * sizeof(float);
    RLHIP_REQUIRE(t0 + bytes <= p0 || p0 + bytes <= t0, "priority_out must not overlap fold.td");
    RLHIP_REQUIRE(a->ring->len_sa == a->ring->len_rt + 1, "push the first state (rlhip_ring_push_state) before the first vec-step");
    return RLHIP_OK;
}

}  // namespace

extern "C" int32_t rlhip_dqn_vec_step_per_f32(rlhip_dqn_per_step_args* p, rlhip_stream_t stream) {
    RLHIP_REQUIRE(p != nullptr, "args is NULL");
    rlhip_dqn_fold_step_args* f = &p->fold;
    rlhip_dqn_step_args* a = &f->base;
    const bool dueling = f->dueling_params || f->target_dueling || f->grad_dueling;
    const bool folds = f->n_step != 1 || f->double_dqn != 0;
    int32_t rc = check_per_step(p, folds, dueling);
    if (rc) return rc;
    const int64_t ns = rlhip_env_obs_dim(a->kind);
    rc = dqn_step_act(a, ns, stream);  // plan! + act! + push!
    if (rc) return rc;
    // CircularPrioritizedTraces.push!: the new frame enters the tree (n_step > 1: the validity mask of the n-step sampler moves on)
    if (f->n_step == 1) rc = rlhip_ring_push_priority(a->ring, p->tree, p->default_priority, stream);
    else rc = rlhip_ring_push_priority_nstep(a->ring, p->tree, p->default_priority, f->n_step, stream);
    if (rc) return rc;
    if (!a->do_update) return RLHIP_OK;
    // optimise!(learner, trajectory): the draw in proportion to the priorities [+ the window fold, one launch] ...
    const bool nstep = f->n_step > 1;
    if (!nstep) rc = rlhip_ring_sample_prioritized(a->ring, p->tree, a->batch, a->sampler_seed, a->draw_ctr, f->idx, p->key, p->prio, stream);
    else rc = rlhip_per_sample_fold_nstep_f32(a->ring, p->tree, a->batch, f->n_step, a->gamma, a->sampler_seed, a->draw_ctr, f->idx, p->key,
                                              p->prio, f->folded, f->iota, stream);
    if (rc) return rc;
    // ... the importance-sampling weights of the drawn priorities ...
    const bool weighted = p->per_beta > 0.0f;
    if (weighted) {
        rc = rlhip_per_is_weights_f32(p->prio, a->batch, p->per_beta, p->is_weights, stream);
        if (rc) return rc;
    }
    // ... the Double DQN target: in place on the n-step batch with its iota, or from the trajectory with the drawn indices ...
    const float gamma_eff = rlhip_gamma_pow(a->gamma, f->n_step);
    if (f->double_dqn) {
        const rlhip_ring* src = nstep ? f->folded : a->ring;
        const int64_t* src_idx = nstep ? f->iota : f->idx;
        if (a->layers == 2)
            rc = rlhip_dqn_fold_double_f32(src, a->h, a->na, a->act, a->params, a->target, src_idx, a->batch, gamma_eff, f->folded, f->iota,
                                           f->fold_workspace, stream);
        else
            rc = rlhip_dqn3_fold_double_f32(src, a->h, a->na, a->act, a->params, a->packed, a->target, a->target_packed, src_idx, a->batch,
                                            gamma_eff, f->folded, f->iota, f->fold_workspace, stream);
        if (rc) return rc;
    }
    // ... the unchanged gradient entry point: on the folded batch with gamma^n, or on the trajectory at the drawn indices ...
    const rlhip_ring* gring = folds ? f->folded : a->ring;
    const int64_t* gidx = folds ? f->iota : f->idx;
    const float ggamma = folds ? gamma_eff : a->gamma;
    if (a->layers == 2) {
        if (weighted)
            rc = rlhip_dqn_grad_idx_w_f32(gring, a->h, a->na, a->act, a->params, a->target, a->batch, gidx, p->is_weights, ggamma,
                                          a->huber_delta, a->workspace, a->grad, a->loss, f->td, stream);
        else
            rc = rlhip_dqn_grad_idx_f32(gring, a->h, a->na, a->act, a->params, a->target, a->batch, gidx, ggamma, a->huber_delta,
                                        a->workspace, a->grad, a->loss, f->td, stream);
    } else {
        if (weighted)
            rc = rlhip_dqn3_grad_w_f32(gring, a->h, a->na, a->act, a->params, a->packed, a->target, a->target_packed, a->batch, gidx,
                                       p->is_weights, ggamma, a->huber_delta, a->workspace, a->grad, a->loss, f->td, stream);
        else
            rc = rlhip_dqn3_grad_f32(gring, a->h, a->na, a->act, a->params, a->packed, a->target, a->target_packed, a->batch, gidx, ggamma,
                                     a->huber_delta, a->sampler_seed, a->draw_ctr, a->workspace, a->grad, a->loss, f->td, stream);
    }
    if (rc) return rc;
    // ... trajectory[:priority, keys] = (|td| + eps)^alpha under the drawn keys, power and write-back in one launch ...
    // The write-back is the one launch for every batch size.  Rule: the one-launch form wherever it is not slower than
    // rlhip_per_priority_f32 + rlhip_sumtree_update by more than the spread of a form against itself, the two launches for a key range
    // where it is.  Measured on an MI355X with HIP events on a 2^20-leaf tree, 300 alternations of 20-call blocks
    // (tools/per_step_time.py, profiles/per_fused_step.md), median us per write-back, one launch / two launches / same-form spread:
    //     32 keys  8.70 /  9.55 / 0.10      512 keys  13.41 / 14.58 / 0.09      4096 keys  18.88 / 20.49 / 0.08
    // -- faster at every size by 0.9 .. 1.6 us, ten times the spread: no key range composes the two launches, so there is no threshold.
    const int64_t n_leaves = a->ring->capacity * a->ring->n_env;
    rc = rlhip_per_writeback_f32(p->tree, n_leaves, p->key, f->td, a->batch, p->per_eps, p->per_alpha, p->priority_out, stream);
    if (rc) return rc;
    // ... and the tail: optimise!(approximator, grad), then TargetNetwork's sync
    return dqn_step_tail(f, ns, dueling, stream);
}
