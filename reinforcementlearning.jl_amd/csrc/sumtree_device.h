// sumtree_device.h -- the one-wavefront priority write-back (<= 64 keys) as a device function, shared by its own launch
// (sumtree.hip: rlhip_sumtree_update), by the prologue of the fused "update -> draw -> gather" launch (ring.hip, round 6) and by the
// fused power + write-back (per_writeback.hip); the value sources of a write-back; and one prioritized draw (sumtree_draw: sumtree_sample_kernel
// and the prioritized n-step launch of per_nstep.hip).
#pragma once
#include "common.h"

namespace rlhip {

constexpr int SMALL_UPDATE_MAX = 64;
constexpr int SMALL_MAXL = 32;  // levels (n_leaves < 2^31)

// PrioritizedDQN write-back value p = (|td| + eps)^alpha: the power in Float64, rounded once (per_priority_kernel's line, and the
// power source below: one definition, the same bits)
__device__ __forceinline__ float per_priority_value(float td, float eps, float alpha) {
    float x = fabsf(td) + eps;
    return (alpha == 1.0f) ? x : (float)pow((double)x, (double)alpha);
}

// Where a write-back takes the value of item i from.  PrioLoad: the caller's priority array (rlhip_sumtree_update).  PrioPower: the
// power of td[i] (rlhip_per_writeback_f32) -- a pure function of td[i], so whichever lane needs item i's value evaluates it again;
// `publish` leaves it in out[i], by item number, whatever the item's key is.
struct PrioLoad {
    static constexpr bool PUBLISHES = false;
    const float* __restrict__ prio;
    __device__ __forceinline__ float operator()(int64_t i) const { return prio[i]; }
    __device__ __forceinline__ void publish(int64_t, float) const {}
};
struct PrioPower {
    static constexpr bool PUBLISHES = true;
    const float* __restrict__ td;
    float eps, alpha;
    float* __restrict__ out;
    __device__ __forceinline__ float operator()(int64_t i) const { return per_priority_value(td[i], eps, alpha); }
    __device__ __forceinline__ void publish(int64_t i, float v) const { out[i] = v; }
};

// LDS of one call: 64 keys + 64 values + SMALL_MAXL x 64 siblings
struct SmallUpdateLds {
    uint32_t key[64];
    float val[64];
    float sib[SMALL_MAXL][64];
};

// rand(rng, t)'s descent for one draw, `v <= left ? left : (v -= left; right)`, never into a zero-sum subtree while the sibling has
// mass: log2(P) dependent 8-byte reads.  (The fused draw + gather of ring.hip restates it over its own loads: after an in-launch
// write-back those are device-scope.)
__device__ __forceinline__ int64_t sumtree_descend(const float* __restrict__ tree, int64_t P, float v) {
    int64_t node = 1;
    while (node < P) {
        float2 c = *reinterpret_cast<const float2*>(tree + 2 * node);
        bool right = (v > c.x && c.y > 0.0f) || c.x == 0.0f;
        if (right) v -= c.x;
        node = 2 * node + (right ? 1 : 0);
    }
    return node - P;
}

// the heap's leaf level starts at P = the smallest power of two >= n_leaves
static inline int64_t pow2_ge(int64_t n) {
    int64_t p = 1;
    while (p < n) p <<= 1;
    return p;
}

// One prioritized draw, sample b of draw `draw_ctr`: rand(rng, Float32) * t.tree[1] from the sample's Philox word, the descent, and
// the clamp below n_leaves (a rounding walk into the zero padding of the last level) -> the leaf key.
__device__ __forceinline__ int64_t sumtree_draw(const float* __restrict__ tree, int64_t P, int64_t n_leaves, uint64_t seed, int64_t b,
                                                uint32_t draw_ctr) {
    const u32x4 w = philox4x32_10(seed, (uint32_t)b, 0, draw_ctr, TAG_SAMPLER);
    const float v = u01_f32(w.z) * tree[1];
    const int64_t leaf = sumtree_descend(tree, P, v);
    return leaf < n_leaves ? leaf : n_leaves - 1;
}

// tree stores: plain when the kernel boundary publishes them (COHERENT = false: the stand-alone launch), device-scope write-through
// when workgroups of the SAME launch read the tree afterwards (COHERENT = true: the fused launch; common.h's hand-off contract)
template <bool COHERENT>
__device__ __forceinline__ void tree_store(float* p, float v) {
    if (COHERENT) store_wt(p, v);
    else *p = v;
}

// Called by ALL 64 lanes of ONE wavefront (uniform control flow); the wave's LDS accesses execute in order, so the exchanges through
// `sh` need no workgroup barrier (the caller may be one wave of a larger workgroup).  Steps: see sumtree.hip.
template <bool COHERENT, class Src>
__device__ __forceinline__ void sumtree_update_small_wave(float* tree, int64_t P, int logP, int64_t n_leaves,
                                                          const int64_t* __restrict__ leaf, const Src src, int n,
                                                          SmallUpdateLds& sh) {
    const int lane = (int)threadIdx.x & 63;
    // ---- 1. load; composite sort key = leaf * 64 + item number (invalid / out-of-range keys sort last) ----
    int64_t k = lane < n ? leaf[lane] : -1;
    float pv = lane < n ? src(lane) : 0.0f;
    if (lane < n) src.publish(lane, pv);
    const bool ok = k >= 0 && k < n_leaves;
    uint64_t ck = ok ? ((uint64_t)k << 6) | (uint64_t)lane : ~0ull;
    // ---- 2. bitonic sort over the 64 lanes (ascending) ----
#pragma unroll
    for (int sz = 2; sz <= 64; sz <<= 1) {
#pragma unroll
        for (int st = sz >> 1; st > 0; st >>= 1) {
            const uint32_t olo = __shfl_xor((uint32_t)ck, st, 64), ohi = __shfl_xor((uint32_t)(ck >> 32), st, 64);
            const float opv = __shfl_xor(pv, st, 64);
            const uint64_t ock = ((uint64_t)ohi << 32) | olo;
            const bool up = (lane & sz) == 0;           // direction of this lane's sub-sequence
            const bool lower = (lane & st) == 0;        // this lane keeps the smaller (up) / larger (down) element
            const bool take = (ock < ck) == (up == lower);
            if (ock != ck && take) {
                ck = ock;
                pv = opv;
            }
        }
    }
    const bool valid = ck != ~0ull;
    const uint32_t kk = (uint32_t)(ck >> 6);  // the leaf (n_leaves < 2^31)
    const uint32_t knext = __shfl_down(kk, 1, 64);
    const bool vnext = __shfl_down((int)valid, 1, 64) != 0;
    const bool win = valid && (lane == 63 || !vnext || knext != kk);  // last occurrence of its leaf
    const uint64_t wmask = __ballot(win);
    const int m = __popcll(wmask);
    const int rank = __popcll(wmask & ((1ull << lane) - 1ull));
    if (win) {
        sh.key[rank] = kk;
        sh.val[rank] = pv;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    bool active = lane < m;
    uint32_t cur = active ? (uint32_t)P + sh.key[lane] : 0u;  // heap positions fit 32 bits (n_leaves < 2^31)
    float val = active ? sh.val[lane] : 0.0f;
    // ---- 3. the leaf, and the siblings of the whole path (relaxed agent-scope loads: past this CU's L1).  The loads are issued
    // from an unrolled loop (all in flight together) and parked in LDS, [level][lane]: the walk below is a rolled loop ----
    {
        float sib[SMALL_MAXL];
#pragma unroll
        for (int l = 0; l < SMALL_MAXL; ++l) {
            sib[l] = 0.0f;
            if (active && l < logP) sib[l] = __hip_atomic_load(tree + ((cur >> l) ^ 1u), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        if (active) tree_store<COHERENT>(tree + cur, val);
#pragma unroll
        for (int l = 0; l < SMALL_MAXL; ++l) sh.sib[l][lane] = sib[l];
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    // ---- 4. walk up: neighbour links over the active lanes (prv / nxt; -1 = none) ----
    int prv = (active && lane > 0) ? lane - 1 : -1;
    int nxt = (active && lane + 1 < m) ? lane + 1 : -1;
    for (int l = 0; l < logP; ++l) {
        const int pl = prv >= 0 ? prv : lane, nl = nxt >= 0 ? nxt : lane;
        const uint32_t lcur = __shfl(cur, pl, 64), rcur = __shfl(cur, nl, 64);
        const float lval = __shfl(val, pl, 64), rval = __shfl(val, nl, 64);
        const float sv = sh.sib[l][lane];
        const bool is_right = (cur & 1u) != 0u;
        const bool sib_left = active && is_right && prv >= 0 && lcur == cur - 1u;   // the even sibling is the left neighbour
        const bool sib_right = active && !is_right && nxt >= 0 && rcur == cur + 1u;
        float parent;
        if (is_right) parent = (sib_left ? lval : sv) + val;   // left + right
        else parent = val + (sib_right ? rval : sv);
        const bool dies = sib_left;  // the pair merges into the left (even) lane
        // links: skip a neighbour that retires on this level (two neighbouring lanes never both retire)
        const int pd = __shfl((int)dies, pl, 64), nd = __shfl((int)dies, nl, 64);
        const int pp = __shfl(prv, pl, 64), nn = __shfl(nxt, nl, 64);
        if (active) {
            if (prv >= 0 && pd) prv = pp;
            if (nxt >= 0 && nd) nxt = nn;
            if (dies) active = false;
            else {
                cur >>= 1;
                val = parent;
                tree_store<COHERENT>(tree + cur, parent);
            }
        }
    }
}

template <bool COHERENT>
__device__ __forceinline__ void sumtree_update_small_wave(float* tree, int64_t P, int logP, int64_t n_leaves,
                                                          const int64_t* __restrict__ leaf, const float* __restrict__ prio, int n,
                                                          SmallUpdateLds& sh) {
    sumtree_update_small_wave<COHERENT>(tree, P, logP, n_leaves, leaf, PrioLoad{prio}, n, sh);
}

}  // namespace rlhip
