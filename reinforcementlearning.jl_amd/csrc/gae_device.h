// gae_device.h -- the GAE recurrence of one env instance over a time-major trajectory, for fusing into the tail of
// the rollout kernels (the stand-alone scan is scans.hip; both follow RLCore/src/utils/basic.jl:408-417 operation for
// operation, so the fused result is bit-identical to rlhip_gae_returns_f32 on the same arrays).
#pragma once
#include "common.h"

namespace rlhip {

template <typename T>
__device__ __forceinline__ T strong_zero_mul(T x, bool keep) {
    return keep ? x : (T)copysign((T)0, x);  // Julia: x * false == copysign(0, x), also for NaN / Inf
}

// adv / ret / r / term: (T, n) time-major, v: (T + 1, n); one lane scans env `i` backwards in chunks of 16 steps whose
// loads are all issued before the first dependent add (the lane reads back what it wrote during the rollout: L2 hits)
__device__ __forceinline__ void gae_scan_lane(float* __restrict__ adv, float* __restrict__ ret,
                                              const float* __restrict__ r, const float* __restrict__ v,
                                              const uint8_t* __restrict__ term, int64_t n, int T, int64_t i, float gamma,
                                              float lambda) {
    constexpr int CH = 16;
    float gae = 0.0f;                    // :409
    float vnext = v[(int64_t)T * n + i];  // V[T+1]
    const float gl = gamma * lambda;
    for (int hi = T; hi > 0; hi -= CH) {
        const int cnt = hi < CH ? hi : CH;
        float r_[CH], v_[CH];
        uint8_t t_[CH];
#pragma unroll
        for (int c = 0; c < CH; ++c) {
            const int64_t t = hi - 1 - c;
            if (c < cnt) {
                r_[c] = r[t * n + i];
                v_[c] = v[t * n + i];
                t_[c] = term[t * n + i];
            }
        }
#pragma unroll
        for (int c = 0; c < CH; ++c) {
            if (c < cnt) {
                const int64_t t = hi - 1 - c;
                const bool is_continue = !t_[c];                              // :411
                const float vi = v_[c];
                const float boot = strong_zero_mul(gamma * vnext, is_continue);
                const float delta = r_[c] + boot - vi;                        // :412
                const float glc = strong_zero_mul(gl, is_continue);
                gae = delta + glc * gae;                                      // :413
                adv[t * n + i] = gae;                                         // :414
                ret[t * n + i] = gae + vi;
                vnext = vi;
            }
        }
    }
}

// ---- the same scan with its operands on chip (csrc/ppo.hip rollout_split_kernel: the L lanes of a wavefront that share env
// `i` have seen value / reward / terminal of every step go by and kept them in LDS, T <= GAE_LDS_T).  One slot of four floats per
// step: {value, reward, terminal (0 / 1), -}.  gae_lds_terms: lane `sub` forms delta and the gamma-lambda factor of the steps
// t = sub, sub + L, ... -- they do not depend on the recurrence -- and leaves them in floats 2, 3 of the slot (nobody reads
// another step's floats 2, 3; float 0 of step t + 1 is only read), zeros in the steps up to the next multiple of L.
// gae_lds_chain: every lane walks the ONE sequential chain gae = delta + gl * gae from the top step down (the operations
// and their order are gae_scan_lane's, so the same bits; a leading step of zeros leaves gae = +0), lane `sub` keeps the
// value of step b + sub of each block of L steps and stores adv / ret of that step: T / L store instructions per array
// instead of T.  Between the two the caller orders the LDS accesses of the wavefront (fence + wave barrier).
constexpr int GAE_LDS_T = 32;

template <int L>
__device__ __forceinline__ void gae_lds_terms(float (*slot)[4], int T, int sub, float v_last, float gamma, float lambda) {
    const float gl = gamma * lambda;
    const int t_end = (T + L - 1) / L * L;
    for (int t = sub; t < t_end; t += L) {
        const float vi = slot[t][0], ri = slot[t][1], ti = slot[t][2];
        const float vn = slot[t + 1][0];  // (slot T exists: the array has GAE_LDS_T + 1 of them; not a value there)
        const bool is_continue = !(ti != 0.0f);                           // :411
        const float vnext = (t + 1 < T) ? vn : v_last;
        const float boot = strong_zero_mul(gamma * vnext, is_continue);
        const float delta = ri + boot - vi;                               // :412
        const float glc = strong_zero_mul(gl, is_continue);
        slot[t][2] = t < T ? delta : 0.0f;
        slot[t][3] = t < T ? glc : 0.0f;
    }
}

template <int L>
__device__ __forceinline__ void gae_lds_chain(float* __restrict__ adv, float* __restrict__ ret, const float (*slot)[4],
                                              int64_t n, int T, int64_t i, int sub, bool store) {
    static_assert(GAE_LDS_T % L == 0, "blocks of L steps");
    float gae = 0.0f;  // :409
    for (int b = (T - 1) / L * L; b >= 0; b -= L) {
        float d_[L], g_[L];
#pragma unroll
        for (int c = 0; c < L; ++c) {
            d_[c] = slot[b + c][2];
            g_[c] = slot[b + c][3];
        }
        float keep = 0.0f;
#pragma unroll
        for (int c = L - 1; c >= 0; --c) {
            gae = d_[c] + g_[c] * gae;  // :413
            keep = c == sub ? gae : keep;
        }
        const int t = b + sub;
        if (store && t < T) {
            adv[(int64_t)t * n + i] = keep;  // :414
            ret[(int64_t)t * n + i] = keep + slot[t][0];
        }
    }
}

}  // namespace rlhip
