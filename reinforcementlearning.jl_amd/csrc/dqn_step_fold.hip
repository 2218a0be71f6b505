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

namespace {

// the largest obs_dim / na / h the composed calls take: checked here so that a refusal comes before the push
int32_t check_fold_step(const rlhip_dqn_fold_step_args* f, bool folds, bool dueling) {
    const rlhip_dqn_step_args* a = &f->base;
    RLHIP_REQUIRE(a->env_cfg && a->st && a->obs && a->ring && a->params && a->actions, "NULL argument");
    RLHIP_REQUIRE(a->layers == 2 || a->layers == 3, "layers must be 2 or 3");
    RLHIP_REQUIRE(a->layers == 2 || (a->packed && a->target_packed), "3-layer network needs the packed weights");
    RLHIP_REQUIRE(!a->do_update || (a->target && a->m && a->v && a->beta_pow && a->workspace && a->grad && a->loss),
                  "learner buffers missing");
    const int64_t ns = rlhip_env_obs_dim(a->kind);
    RLHIP_REQUIRE(ns == a->ring->obs_dim && a->n == a->ring->n_env, "ring geometry does not match the env");
    RLHIP_REQUIRE(f->n_step >= 1 && f->n_step <= 32, "n_step must be in 1..32");
    RLHIP_REQUIRE(f->double_dqn == 0 || f->double_dqn == 1, "double_dqn must be 0 or 1");
    RLHIP_REQUIRE((f->dueling_params != nullptr) == (f->target_dueling != nullptr) &&
                      (f->dueling_params != nullptr) == (f->grad_dueling != nullptr),
                  "dueling_params, target_dueling and grad_dueling must be all given or all NULL");
    RLHIP_REQUIRE(a->batch >= 1, "batch must be >= 1");
    if (dueling) RLHIP_REQUIRE(rlhip_dueling_nparams(ns, a->h, a->na, a->layers) > 0, "the dueling fold takes 1..4 actions, h >= 1");
    if (!folds) return RLHIP_OK;
    RLHIP_REQUIRE(a->ring->layout == RLHIP_RING_RECORDS && a->ring->elem_bytes == 4 && ns >= 2 && ns <= 4,
                  "folded batches are defined for record rings (Float32 observations, obs_dim 2..4)");
    RLHIP_REQUIRE(f->folded && f->idx && f->iota, "folded / idx / iota missing");
    RLHIP_REQUIRE(f->folded->layout == RLHIP_RING_RECORDS && f->folded->state != nullptr && f->folded->capacity >= 1 &&
                      f->folded->n_env == a->batch && f->folded->obs_dim == ns,
                  "`folded` must be a record ring initialised with rlhip_ring_init(capacity >= 1, n_env = batch, the env's obs_dim)");
    RLHIP_REQUIRE(f->folded->state != a->ring->state, "`folded` must not alias the trajectory");
    if (a->layers == 2) {
        RLHIP_REQUIRE(a->h >= 4 && a->h <= 256 && a->h % 4 == 0, "hidden must be a multiple of 4, <= 256");
        RLHIP_REQUIRE(a->na >= 1 && a->na <= 4, "na must be <= 4");
    } else {
        RLHIP_REQUIRE(a->h == 128 || a->h == 256, "the MFMA Q-network path is built for hidden = 128 or 256");
        RLHIP_REQUIRE(!f->double_dqn || !a->do_update || f->fold_workspace, "the 3-layer Double DQN fold needs fold_workspace");
    }
    RLHIP_REQUIRE(a->act == 0 || a->act == 1, "act must be 0 (relu) or 1 (tanh)");
    if (a->do_update) {  // the ring as it will be after this call's push
        const int64_t len_after = a->ring->len_rt < a->ring->capacity ? a->ring->len_rt + 1 : a->ring->capacity;
        RLHIP_REQUIRE(a->ring->len_sa == a->ring->len_rt + 1, "push the first state (rlhip_ring_push_state) before the first vec-step");
        RLHIP_REQUIRE(len_after >= f->n_step, "do_update with fewer than n_step stored steps");
    }
    return RLHIP_OK;
}

}  // namespace

extern "C" int32_t rlhip_dqn_vec_step_fold_f32(rlhip_dqn_fold_step_args* f, rlhip_stream_t stream) {
    RLHIP_REQUIRE(f != nullptr, "args is NULL");
    rlhip_dqn_step_args* a = &f->base;
    const bool dueling = f->dueling_params || f->target_dueling || f->grad_dueling;
    const bool folds = f->n_step != 1 || f->double_dqn != 0;
    int32_t rc = check_fold_step(f, folds, dueling);
    if (rc) return rc;
    if (!folds && !dueling) return rlhip_dqn_vec_step_f32(a, stream);  // a plain learner: the shipped entry point as it stands
    const int64_t ns = rlhip_env_obs_dim(a->kind);
    // plan! + act! + push!: the three-way dispatch of rlhip_dqn_vec_step_f32
    if (a->layers == 2 && rlhip_dqn_act_supported(a->kind, a->n, a->h)) {
        rc = rlhip_dqn_act_f32(a->kind, a->env_cfg, a->st, a->n, a->params, a->h, a->na, a->act, a->eps, a->explorer_seed,
                               a->explorer_step, a->env_seed, a->env_id_base, a->ring, a->actions, a->q, a->obs, a->last_obs, stream);
        if (rc) return rc;
    } else if (a->layers == 3 && rlhip_dqn3_act_supported(a->kind, a->n, a->h, a->na)) {
        rc = rlhip_dqn3_act_f32(a->kind, a->env_cfg, a->st, a->n, a->params, a->packed, a->h, a->na, a->act, a->eps, a->explorer_seed,
                                a->explorer_step, a->env_seed, a->env_id_base, a->ring, a->actions, a->q, a->obs, a->last_obs, stream);
        if (rc) return rc;
    } else {
        if (a->layers == 2)
            rc = rlhip_dqn_plan_f32(a->params, ns, a->h, a->na, a->act, a->obs, a->n, a->eps, a->explorer_seed, a->env_id_base,
                                    a->explorer_step, a->actions, a->q, stream);
        else
            rc = rlhip_dqn3_plan_f32(a->params, a->packed, ns, a->h, a->na, a->act, a->obs, a->n, a->eps, a->explorer_seed,
                                     a->env_id_base, a->explorer_step, a->actions, a->q, stream);
        if (rc) return rc;
        rc = rlhip_env_act_push_f32(a->kind, a->env_cfg, a->st, a->n, a->actions, a->env_seed, a->env_id_base, a->ring, a->obs,
                                    a->last_obs, stream);
        if (rc) return rc;
    }
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
    // ... and the tail: optimise!(approximator, grad), then TargetNetwork's sync (dest = rho * dest + (1 - rho) * src)
    if (!dueling) {
        const int64_t np = a->layers == 2 ? rlhip_mlp2_nparams(ns, a->h, a->na) : rlhip_mlp3_nparams(ns, a->h, a->na);
        rc = rlhip_clip_adam_f32(a->params, a->grad, a->m, a->v, a->beta_pow, np, a->grad_scale, a->max_grad_norm, a->lr, a->beta1,
                                 a->beta2, a->adam_eps, a->gn, stream);
        if (rc) return rc;
        if (a->layers == 3) {
            rc = rlhip_mlp3_pack_bf16(a->params, ns, a->h, a->na, a->packed, stream);
            if (rc) return rc;
        }
        if (a->do_sync) {
            rc = rlhip_polyak_f32(a->target, a->params, np, a->rho, stream);
            if (rc) return rc;
            if (a->layers == 3) rc = rlhip_mlp3_pack_bf16(a->target, ns, a->h, a->na, a->target_packed, stream);
        }
        return rc;
    }
    // DuelingApproximator.optimise_: the plain gradient back onto the dueling vector, clip + Adam there, fold again
    const int64_t nd = rlhip_dueling_nparams(ns, a->h, a->na, a->layers);
    rc = rlhip_dueling_unfold_grad_f32(a->grad, f->grad_dueling, ns, a->h, a->na, a->layers, stream);
    if (rc) return rc;
    rc = rlhip_clip_adam_f32(f->dueling_params, f->grad_dueling, a->m, a->v, a->beta_pow, nd, a->grad_scale, a->max_grad_norm, a->lr,
                             a->beta1, a->beta2, a->adam_eps, a->gn, stream);
    if (rc) return rc;
    rc = rlhip_dueling_fold_f32(f->dueling_params, a->params, nullptr, nullptr, ns, a->h, a->na, a->layers, stream);
    if (rc) return rc;
    if (a->layers == 3) {
        rc = rlhip_mlp3_pack_bf16(a->params, ns, a->h, a->na, a->packed, stream);
        if (rc) return rc;
    }
    if (a->do_sync) {  // TargetNetwork.optimise_ with a dueling net: Polyak on the dueling vectors, the effective target folded again
        rc = rlhip_polyak_f32(f->target_dueling, f->dueling_params, nd, a->rho, stream);
        if (rc) return rc;
        rc = rlhip_dueling_fold_f32(f->target_dueling, a->target, nullptr, nullptr, ns, a->h, a->na, a->layers, stream);
        if (rc) return rc;
        if (a->layers == 3) rc = rlhip_mlp3_pack_bf16(a->target, ns, a->h, a->na, a->target_packed, stream);
    }
    return rc;
}
