// per_writeback.hip -- the priority write-back of a prioritized DQN update in ONE launch: p = (|td| + eps)^alpha and
// `trajectory[:priority, keys] = p` (ReinforcementLearningTrajectories 0.4 `CircularPrioritizedTraces`; the removed Zoo's
// PrioritizedDQN, PARITY UNPINNED like the rest of the prioritized path).
//
// What it replaces: rlhip_per_priority_f32 (an element-wise launch) immediately followed by rlhip_sumtree_update, which reads each
// priority exactly once.  Here the write-back kernels of sumtree_update.h are instantiated with the power of td[item] as their value
// source (PrioPower, sumtree_device.h) instead of a load: same election, same block recompute, same arrival counter in tree[0],
// same dispatch -- every path of the shipped update has its fused twin, and no workgroup waits for another.  The power is a pure
// function of td[i], so
//   * a leaf's winner evaluates it for its own item (whichever workgroup owns the key), and
//   * prio_out[i] is stored by ITEM NUMBER in a grid-stride pass that does not look at the keys (the one-wave path: lane i), so items
//     with out-of-range keys get their value too.
// Other workgroups read td while prio_out is being written: the two must not overlap (checked before the launch).
// The tree (every node) and prio_out are byte for byte those of the two shipped launches (tests/test_gpu_per_writeback.py).
#include "common.h"
#include "sumtree_device.h"
#include "sumtree_update.h"

using namespace rlhip;

extern "C" int32_t rlhip_per_writeback_f32(float* tree, int64_t n_leaves, const int64_t* key, const float* td, int64_t n, float eps,
                                           float alpha, float* prio_out, rlhip_stream_t stream) {
    RLHIP_REQUIRE(n_leaves >= 1 && n >= 0, "bad sizes");
    RLHIP_REQUIRE(eps >= 0.0f && alpha >= 0.0f, "bad arguments");
    if (n == 0) return RLHIP_OK;
    RLHIP_REQUIRE(tree && key && td && prio_out, "NULL array");
    RLHIP_REQUIRE(n < (1ll << 31), "too many keys in one update");
    const uintptr_t t0 = reinterpret_cast<uintptr_t>(td), p0 = reinterpret_cast<uintptr_t>(prio_out);
    const uintptr_t bytes = (uintptr_t)n * sizeof(float);
    RLHIP_REQUIRE(t0 + bytes <= p0 || p0 + bytes <= t0, "prio_out must not overlap td (other workgroups read td while it is written)");
    return sumtree_update_launch(tree, n_leaves, key, PrioPower{td, eps, alpha, prio_out}, n, as_stream(stream));
}
