// dqn_step_fold.hip -- one whole vec-step of the DQN agent loop as ONE C-ABI call for learners whose batches are FOLDED: n-step
// targets, Double DQN targets, a DuelingNetwork, or any combination (host-side composition in the style of dqn_step.hip; the one
// new kernel it drives is dqn_sample_fold.hip).
//
// What it replaces: one trip round the body of `_run` (RLCore/src/core/run.jl:52-70) for `Agent{QBasedPolicy{DQNLearner}}` on the
// vector env, where the learner samples with NStepBatchSampler (RLTrajectories 0.4), has `is_enable_double_DQN` set, or approximates
// Q with DuelingNetwork(base, val, adv) (RLCore/src/utils/networks.jl:510-522) --
//     action = plan!(policy, env)                      q_based_policy.jl:30-32 -> explorer :108-112
//     act!(env, action)                                CartPoleEnv.jl:112-140 (+ auto-reset, MultiThreadEnv protocol)
//     push!(agent, PostActStage(), env, action)        agent_base.jl:56-59
//     optimise!(agent, PostActStage())                 q_based_policy.jl:49 -> learner -> flux_approximator.jl:46,
//                                                      target_network.jl:70-88
// The per-stage protocol issues about ten calls per vec-step for such a learner.  This entry point enqueues the same kernels in the
// same order with the same arguments -- for two-layer nets the draw, the window fold and the Double DQN target as one launch that
// equals the three byte for byte -- so results are bit-identical to the per-stage loop (tests/test_gpu_fused_folds.py).
#include "common.h"
#include "dqn_step_common.h"

using namespace rlhip;

extern "C" int32_t rlhip_dqn_vec_step_fold_f32(rlhip_dqn_fold_step_args* f, rlhip_stream_t stream) {
    RLHIP_REQUIRE(f != nullptr, "args is NULL");
    rlhip_dqn_step_args* a = &f->base;
    const bool dueling = f->dueling_params || f->target_dueling || f->grad_dueling;
    const bool folds = f->n_step != 1 || f->double_dqn != 0;
    int32_t rc = check_fold_step(f, folds, dueling);
    if (rc) return rc;
    if (!folds && !dueling) return rlhip_dqn_vec_step_f32(a, stream);  // a plain learner: the shipped entry point as it stands
    const int64_t ns = rlhip_env_obs_dim(a->kind);
    rc = dqn_step_act(a, ns, stream);  // plan! + act! + push!
    if (rc) return rc;
    if (!a->do_update) return RLHIP_OK;
    // optimise!(learner, trajectory): the folded batch ...
    const float gamma_eff = rlhip_gamma_pow(a->gamma, f->n_step);
    if (folds && a->layers == 2) {  // draw + n-step window + Double DQN target: one launch (dqn_sample_fold.hip)
        rc = rlhip_dqn_sample_fold_f32(a->ring, a->batch, f->n_step, f->double_dqn, a->gamma, a->sampler_seed, a->draw_ctr, a->h, a->na,
                                       a->act, a->params, a->target, f->folded, f->idx, f->iota, stream);
        if (rc) return rc;
    } else if (folds) {  // three layers: the shipped calls, as DQNLearner and DoubleTargetFold.fold issue them
        if (f->n_step == 1) rc = rlhip_ring_sample_indices(a->ring, a->batch, a->sampler_seed, a->draw_ctr, f->idx, stream);
        else rc = rlhip_ring_sample_indices_nstep(a->ring, a->batch, f->n_step, a->sampler_seed, a->draw_ctr, f->idx, stream);
        if (rc) return rc;
        if (f->n_step > 1) {
            rc = rlhip_ring_fold_nstep(a->ring, f->idx, a->batch, f->n_step, a->gamma, f->folded, f->iota, stream);
            if (rc) return rc;
        }
        if (f->double_dqn) {  // in place on the n-step ring with its iota, or from the trajectory with the drawn indices
            const bool in_place = f->n_step > 1;
            rc = rlhip_dqn3_fold_double_f32(in_place ? f->folded : a->ring, a->h, a->na, a->act, a->params, a->packed, a->target,
                                            a->target_packed, in_place ? f->iota : f->idx, a->batch, gamma_eff, f->folded, f->iota,
                                            f->fold_workspace, stream);
            if (rc) return rc;
        }
    }
    // ... the unchanged gradient entry point on it (gamma^n as its discount) ...
    if (folds) {
        if (a->layers == 2)
            rc = rlhip_dqn_grad_idx_f32(f->folded, a->h, a->na, a->act, a->params, a->target, a->batch, f->iota, gamma_eff,
                                        a->huber_delta, a->workspace, a->grad, a->loss, f->td, stream);
        else
            rc = rlhip_dqn3_grad_f32(f->folded, a->h, a->na, a->act, a->params, a->packed, a->target, a->target_packed, a->batch,
                                     f->iota, gamma_eff, a->huber_delta, a->sampler_seed, a->draw_ctr, a->workspace, a->grad, a->loss,
                                     f->td, stream);
    } else {  // a dueling net with plain 1-step targets: the sampling gradient on the trajectory itself
        if (a->layers == 2)
            rc = rlhip_dqn_grad_f32(a->ring, a->h, a->na, a->act, a->params, a->target, a->batch, a->gamma, a->huber_delta,
                                    a->sampler_seed, a->draw_ctr, a->workspace, a->grad, a->loss, stream);
        else
            rc = rlhip_dqn3_grad_f32(a->ring, a->h, a->na, a->act, a->params, a->packed, a->target, a->target_packed, a->batch, nullptr,
                                     a->gamma, a->huber_delta, a->sampler_seed, a->draw_ctr, a->workspace, a->grad, a->loss, f->td,
                                     stream);
    }
    if (rc) return rc;
    // ... and the tail: optimise!(approximator, grad), then TargetNetwork's sync
    return dqn_step_tail(f, ns, dueling, stream);
}
