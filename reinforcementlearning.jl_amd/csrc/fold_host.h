// fold_host.h -- what the host side of every fold entry point asks and leaves behind, each written once: the destination ring of
// a fold, the two-layer net a fold can stage (fold_device.h: FOLD_HMAX, MAXO) and the counters of a folded ring.  Messages that name
// their entry point stay with it.  Host code only.
#pragma once
#include "common.h"
#include "fold_device.h"

namespace rlhip {

// `folded` takes `batch` folded records of `rb`.  may_alias: the Double DQN folds, which state their own rule for running in place.
static inline int32_t check_folded_dest(const rlhip_ring* rb, const rlhip_ring* folded, int64_t batch, bool may_alias = false) {
    RLHIP_REQUIRE(folded->layout == RLHIP_RING_RECORDS && folded->state != nullptr && folded->capacity >= 1 && folded->n_env == batch &&
                      folded->obs_dim == rb->obs_dim,
                  "`folded` must be a record ring initialised with rlhip_ring_init(capacity >= 1, n_env = batch, the source's obs_dim)");
    RLHIP_REQUIRE(may_alias || folded->state != rb->state, "`folded` must not alias the source ring");
    return RLHIP_OK;
}

// the two-layer nets whose forward a fold kernel runs out of LDS
static inline int32_t check_mlp2_fold_net(int64_t h, int64_t na, int32_t act) {
    RLHIP_REQUIRE(h >= 4 && h <= FOLD_HMAX && h % 4 == 0, "hidden must be a multiple of 4, <= 256");
    RLHIP_REQUIRE(na >= 1 && na <= MAXO, "na must be <= 4");
    RLHIP_REQUIRE(act == 0 || act == 1, "act must be 0 (relu) or 1 (tanh)");
    return RLHIP_OK;
}

// slot 0 of `folded` now holds `batch` complete transitions: one stored vec-step of a `batch`-env ring
static inline void mark_folded(rlhip_ring* folded) {
    folded->head_sa = 0;
    folded->len_sa = 2;
    folded->head_rt = 0;
    folded->len_rt = 1;
}

}  // namespace rlhip
