// dqn_step_common.h -- the stages that the composed DQN vec-steps share, each written once: the argument checks of a folded step,
// plan! + act! + push! (the three-way dispatch of rlhip_dqn_vec_step_f32) and the tail of an update (clip + Adam [+ pack], the
// target sync; for a DuelingNetwork through the dueling vectors).  Used by dqn_step_fold.hip (rlhip_dqn_vec_step_fold_f32) and
// dqn_step_per.hip (rlhip_dqn_vec_step_per_f32); host code only.
#pragma once
#include "common.h"
#include "fold_host.h"

namespace rlhip {

// the largest obs_dim / na / h the composed calls take: checked here so that a refusal comes before the push
static inline int32_t check_fold_step(const rlhip_dqn_fold_step_args* f, bool folds, bool dueling) {
    const rlhip_dqn_step_args* a = &f->base;
    RLHIP_REQUIRE(a->env_cfg && a->st && a->obs && a->ring && a->params && a->actions, "NULL argument");
    RLHIP_REQUIRE(a->layers == 2 || a->layers == 3, "layers must be 2 or 3");
    RLHIP_REQUIRE(a->layers == 2 || (a->packed && a->target_packed), "3-layer network needs the packed weights");
    RLHIP_REQUIRE(!a->do_update || (a->target && a->m && a->v && a->beta_pow && a->workspace && a->grad && a->loss),
                  "learner buffers missing");
    const int64_t ns = rlhip_env_obs_dim(a->kind);
    RLHIP_REQUIRE(ns == a->ring->obs_dim && a->n == a->ring->n_env, "ring geometry does not match the env");
    RLHIP_REQUIRE(f->n_step >= 1 && f->n_step <= FOLD_MAX_NSTEP, "n_step must be in 1..32");
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
        const int32_t rc = check_mlp2_fold_net(a->h, a->na, a->act);
        if (rc) return rc;
    } else {
        RLHIP_REQUIRE(a->h == 128 || a->h == 256, "the MFMA Q-network path is built for hidden = 128 or 256");
        RLHIP_REQUIRE(!f->double_dqn || !a->do_update || f->fold_workspace, "the 3-layer Double DQN fold needs fold_workspace");
        RLHIP_REQUIRE(a->act == 0 || a->act == 1, "act must be 0 (relu) or 1 (tanh)");
    }
    if (a->do_update) {  // the ring as it will be after this call's push
        const int64_t len_after = a->ring->len_rt < a->ring->capacity ? a->ring->len_rt + 1 : a->ring->capacity;
        RLHIP_REQUIRE(a->ring->len_sa == a->ring->len_rt + 1, "push the first state (rlhip_ring_push_state) before the first vec-step");
        RLHIP_REQUIRE(len_after >= f->n_step, "do_update with fewer than n_step stored steps");
    }
    return RLHIP_OK;
}

// plan! + act! + push!: the three-way dispatch of rlhip_dqn_vec_step_f32
static inline int32_t dqn_step_act(rlhip_dqn_step_args* a, int64_t ns, rlhip_stream_t stream) {
    if (a->layers == 2 && rlhip_dqn_act_supported(a->kind, a->n, a->h))
        return rlhip_dqn_act_f32(a->kind, a->env_cfg, a->st, a->n, a->params, a->h, a->na, a->act, a->eps, a->explorer_seed,
                                 a->explorer_step, a->env_seed, a->env_id_base, a->ring, a->actions, a->q, a->obs, a->last_obs, stream);
    if (a->layers == 3 && rlhip_dqn3_act_supported(a->kind, a->n, a->h, a->na))
        return rlhip_dqn3_act_f32(a->kind, a->env_cfg, a->st, a->n, a->params, a->packed, a->h, a->na, a->act, a->eps, a->explorer_seed,
                                  a->explorer_step, a->env_seed, a->env_id_base, a->ring, a->actions, a->q, a->obs, a->last_obs, stream);
    int32_t rc;
    if (a->layers == 2)
        rc = rlhip_dqn_plan_f32(a->params, ns, a->h, a->na, a->act, a->obs, a->n, a->eps, a->explorer_seed, a->env_id_base,
                                a->explorer_step, a->actions, a->q, stream);
    else
        rc = rlhip_dqn3_plan_f32(a->params, a->packed, ns, a->h, a->na, a->act, a->obs, a->n, a->eps, a->explorer_seed,
                                 a->env_id_base, a->explorer_step, a->actions, a->q, stream);
    if (rc) return rc;
    return rlhip_env_act_push_f32(a->kind, a->env_cfg, a->st, a->n, a->actions, a->env_seed, a->env_id_base, a->ring, a->obs,
                                  a->last_obs, stream);
}

// the tail of an update: optimise!(approximator, grad), then TargetNetwork's sync (dest = rho * dest + (1 - rho) * src)
static inline int32_t dqn_step_tail(rlhip_dqn_fold_step_args* f, int64_t ns, bool dueling, rlhip_stream_t stream) {
    rlhip_dqn_step_args* a = &f->base;
    int32_t rc;
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

}  // namespace rlhip
