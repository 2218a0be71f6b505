// dist_device.h -- the two forward chains the distributional learners share (csrc/c51.hip, csrc/qrdqn.hip): layer 1 of a tile into LDS
// and the output rows of mlp2(ns, h, M = na * N), "thread = output row".  include/rlhip.h (the C51 section) states both chains; the
// functions keep the names they had in c51.hip, from which they were moved unchanged.
#pragma once
#include "mlp_device.h"

namespace rlhip {

// layer 1 of `P` on the T columns of l_x ([k][T]) -> l_h ([j][T]): z = b1[j], fmaf over k ascending
template <int ACT, int T, int NT>
__device__ __forceinline__ void c51_layer1(const float* __restrict__ P, int ns, int h, const float* l_x, float* l_h) {
    for (int q = threadIdx.x; q < h * T; q += NT) {
        const int i = q % T, j = q / T;
        // branch-free, as in dqn_plan_obsn_kernel: a weight beyond ns is read from a clamped index and its fmaf dropped by a select, so
        // that the sixteen loads are in flight together instead of one round trip to L2 per input
        float w1[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) w1[k] = P[j + h * (k < ns ? k : 0)];
        float z = P[h * ns + j];
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const float t = fmaf(w1[k], l_x[k * T + i], z);
            z = (k < ns) ? t : z;
        }
        l_h[q] = act_fwd_t<ACT>(z);
    }
}

// logits of SPT consecutive samples starting at i0, row m: l = b2[m], fmaf(W2[m, j], h[j], .) over j ascending -> l_l[i][m]
template <int T, int SPT, int WCH>
__device__ __forceinline__ void c51_logits(const float* __restrict__ P, int ns, int h, int M, int m, int i0, const float* l_h, float* l_l,
                                           int ls) {
    static_assert(SPT % 4 == 0 && WCH % 4 == 0, "the hidden values of a thread's samples are read as float4; h is a multiple of 4");
    const float* W2 = P + h * ns + h;
    float acc[SPT];
    const float b = W2[M * h + m];
#pragma unroll
    for (int s = 0; s < SPT; ++s) acc[s] = b;
    // the row of W2 comes from L2 in chunks of WCH weights, the next chunk requested before the current one is used (a round trip per
    // weight would put h of them on the chain); weights beyond h are read from a clamped index and never used.  WCH = 16 where a thread
    // has 8 samples (the gradient tile), 4 where it has 16 and the FMAs cover the loads (plan)
    float cur[WCH], nxt[WCH];
#pragma unroll
    for (int u = 0; u < WCH; ++u) cur[u] = W2[m + M * (u < h ? u : h - 1)];
    for (int j0 = 0; j0 < h; j0 += WCH) {
#pragma unroll
        for (int u = 0; u < WCH; ++u) {
            const int jn = j0 + WCH + u;
            nxt[u] = W2[m + M * (jn < h ? jn : h - 1)];
        }
#pragma unroll
        for (int u = 0; u < WCH; ++u) {
            if (j0 + (u & ~3) < h) {  // (uniform; h is a multiple of 4)
                const float w = cur[u];
                const float4* hv = reinterpret_cast<const float4*>(l_h + (j0 + u) * T + i0);
#pragma unroll
                for (int v = 0; v < SPT / 4; ++v) {
                    const float4 t = hv[v];
                    acc[4 * v] = fmaf(w, t.x, acc[4 * v]);
                    acc[4 * v + 1] = fmaf(w, t.y, acc[4 * v + 1]);
                    acc[4 * v + 2] = fmaf(w, t.z, acc[4 * v + 2]);
                    acc[4 * v + 3] = fmaf(w, t.w, acc[4 * v + 3]);
                }
            }
        }
#pragma unroll
        for (int u = 0; u < WCH; ++u) cur[u] = nxt[u];
    }
#pragma unroll
    for (int s = 0; s < SPT; ++s) l_l[(i0 + s) * ls + m] = acc[s];
}

}  // namespace rlhip
