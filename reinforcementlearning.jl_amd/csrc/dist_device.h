// dist_device.h -- the stages the distributional learners' kernels are made of (csrc/c51.hip, csrc/qrdqn.hip, csrc/iqn.hip and the
// acting kernel of csrc/noisy.hip), each written once.  A kernel of those files reads as the list of its stages plus the section that
// is its own: the projection and the cross-entropy line (C51), the pairwise quantile-Huber term (QR-DQN), the MFMA row blocks (IQN),
// the factorised noise (NoisyDense).  include/rlhip.h (the C51 section) states the chains.  LDS arrays come in as pointers and every
// stride as a template parameter, so the addresses stay immediates.
//
//   tile constants          DIST_*: one set for the two mlp2 learners (IQN keeps its own where they differ)
//   dist_load_obs / dist_load_states   the plan's observations / the tile's s and s' -> [16][T]
//   dist_load_gpow          the gamma table from the kernel-argument segment
//   dist_tile_scalars       r, c = gamma^n_used * (1 - term), w and the action (-1 where it selects nothing) of the tile's samples
//   dist_layer1, dist_rows  the two forward chains of mlp2(ns, h, M = na * K), "thread = output row"
//   dist_select_action      a*, the first maximum wins
//   dist_backward           dW2 | db2, dh -> dz, dW1 | db1 with the carry through the workgroup's partial row (C51, QR-DQN)
//   dist_plan_tail          optional row stores, Q per (env, action) through the caller's rows -> Q function, eps_greedy_select1
//   c51_atom / c51_exp_sum / c51_probs_q   logits -> probabilities -> Q (c51.hip, noisy.hip)
// No stage asks which learner calls it.  The launches the learners share (the reduce kernel, the bad-action check) are in dist.hip.
#pragma once
#include "mlp_device.h"
#include "select_device.h"

namespace rlhip {

// ---- one set of tile constants for the two mlp2 learners
constexpr int DIST_MAXK = 64;         // atoms / quantiles per action
constexpr int DIST_MAXM = 256;        // output rows = na * K
constexpr int DIST_HMAX = 256;
constexpr int DIST_PT = 16;           // plan: envs per workgroup
constexpr int DIST_PTHREADS = 256;
constexpr int DIST_GT = 8;            // gradient: samples per tile
constexpr int DIST_GTHREADS = 256;
constexpr int DIST_GSPT = DIST_GT / (DIST_GTHREADS / DIST_MAXM);    // samples per thread of the rows pass (8)
constexpr int DIST_QO = MAXO * DIST_GT > 64 ? MAXO * DIST_GT : 64;  // first thread of the online net's (sample, action) pairs: another wave
constexpr int DIST_AS = DIST_MAXK + 1;  // per-sample atom / quantile rows in LDS are 65 floats apart
constexpr int DIST_GPOW = 33;         // gamma^n for n = 0..32 (IQN's table too)
constexpr int DIST_WCH = 16;          // weights of a W2 row requested together (the rows pass, dh)
// The per-atom / per-quantile loops of the gradient kernels run in chunks of DIST_CH: the chunk is read from LDS first, its expf /
// divisions / selects are independent of each other (one thread owns a whole chain: instruction-level parallelism is all it has), and
// the sums are then taken one by one in ascending order, so the chunking changes no rounding.  An element beyond the row is read from a
// clamped index and dropped by a select.  The plan kernels, whose workgroups each pass once through their code, keep the plain loops
// (chunks of 1: with the unrolled bodies the C51 plan measured 23.4 us at 4096 envs, with the loops 17.8 -- profiles/c51.md).
constexpr int DIST_CH = 8;

// ---- the plan's observations -> l_x [16][T]: coalesced along the envs, zero beyond ns and beyond the nv valid columns
template <int T>
__device__ __forceinline__ void dist_load_obs(const float* obs, int64_t n, int64_t e0, int nv, int ns, float* l_x) {
    const int tid = threadIdx.x;
    if (tid < 16 * T) {
        const int i = tid % T, k = tid / T;
        l_x[tid] = (k < ns && i < nv) ? obs[(int64_t)k * n + e0 + i] : 0.f;
    }
}

// ---- the tile's states s, s' -> l_x, l_xn [16][T]
template <int T>
__device__ __forceinline__ void dist_load_states(const float* s, const float* sn, int64_t batch, int64_t b0, int nv, int ns, float* l_x,
                                                 float* l_xn) {
    const int tid = threadIdx.x;
    if (tid < 16 * T) {
        const int i = tid % T, k = tid / T;
        const bool in = k < ns && i < nv;
        l_x[tid] = in ? s[(int64_t)k * batch + b0 + i] : 0.f;
        l_xn[tid] = in ? sn[(int64_t)k * batch + b0 + i] : 0.f;
    }
}

// ---- Args::gpow -> l_gp: the table is read from the kernel-argument segment with a per-lane index, so no scalar register holds it
template <class Args>
__device__ __forceinline__ void dist_load_gpow(float* l_gp) {
    if (threadIdx.x < DIST_GPOW) {
        const char* ka = (const char*)__builtin_amdgcn_kernarg_segment_ptr();
        l_gp[threadIdx.x] = reinterpret_cast<const float*>(ka + offsetof(Args, gpow))[threadIdx.x];
    }
}

// ---- the scalars of the tile's samples (threads 0 .. T - 1; l_gp is published by the caller's barrier).  g: any gradient argument
// struct (r, a, term, n_used, isw, gamma, na)
template <int T, class Args>
__device__ __forceinline__ void dist_tile_scalars(const Args& g, int64_t b0, int nv, const float* l_gp, float* l_r, float* l_c, float* l_w,
                                                  int* l_ai) {
    const int tid = threadIdx.x;
    if (tid < T) {
        float r = 0.f, c = 0.f, w = 1.0f;
        int a = -1;
        if (tid < nv) {
            const int64_t b = b0 + tid;
            r = g.r[b];
            a = g.a[b];
            if (a < 0 || a >= g.na) a = -1;  // the action is only ever COMPARED: one outside 0 .. na - 1 selects nothing
            const float cont = g.term[b] ? 0.f : 1.f;
            float disc = g.gamma;
            if (g.n_used) {
                int nu = g.n_used[b];
                nu = nu < 0 ? 0 : (nu > DIST_GPOW - 1 ? DIST_GPOW - 1 : nu);
                disc = l_gp[nu];
            }
            c = disc * cont;
            if (g.isw) w = g.isw[b];
        }
        l_r[tid] = r, l_c[tid] = c, l_w[tid] = w, l_ai[tid] = a;
    }
}

// ---- a* of the tile's samples from q [o][T] (threads 0 .. T - 1): the first maximum wins (strict >)
template <int T>
__device__ __forceinline__ void dist_select_action(const float* q, int na, int* l_as, int32_t* sel_out, int64_t b0, int nv) {
    const int tid = threadIdx.x;
    if (tid < T) {
        int as = 0;
        float mq = q[tid];
        for (int o = 1; o < na; ++o)
            if (q[o * T + tid] > mq) mq = q[o * T + tid], as = o;
        l_as[tid] = as;
        if (sel_out && tid < nv) sel_out[b0 + tid] = as;
    }
}

// ---- layer 1 of `P` on the T columns of l_x ([k][T]) -> l_h ([j][T]): z = b1[j], fmaf over k ascending
template <int ACT, int T, int NT>
__device__ __forceinline__ void dist_layer1(const float* __restrict__ P, int ns, int h, const float* l_x, float* l_h) {
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

// ---- output row m of SPT consecutive samples starting at i0: l = b2[m], fmaf(W2[m, j], h[j], .) over j ascending -> l_l[i][m]
template <int T, int SPT, int WCH>
__device__ __forceinline__ void dist_rows(const float* __restrict__ P, int ns, int h, int M, int m, int i0, const float* l_h, float* l_l,
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

// ---- the backward pass of a tile of mlp2(ns, h, M = na * K) whose output gradient is g_k = l_g[i][k] on the K rows of action l_ai[i]
// (nothing where it is -1): ONE chain per gradient element over the workgroup's samples in ascending order, carried from tile to tile
// through the workgroup's own partial row (`first`: the chains start from +0).  h(s) in l_h [h][T], s in l_x; dz goes to l_dz [T][HS1].
// W2: the online net's W2 | b2, a pointer the kernel forms ONCE ahead of its tile loop (formed here, behind the barrier, it cost the C51
// gradient launch 0.8 us of 93: profiles/dist_stages.md)
template <int ACT, int T, int NT, int AS, int HS1, int WCH>
__device__ __forceinline__ void dist_backward(const float* W2, float* row, bool first, int nv, int ns, int h, int M, int K,
                                              const int* l_ai, const float* l_g, const float* l_h, const float* l_x, float* l_dz) {
    const int tid = threadIdx.x;
    // dW2 and db2: element (m, j), one chain over the samples whose action owns row m
    {
        const int off = h * ns + h;
        const int ne = M * h + M;
        int ai[T];
#pragma unroll
        for (int i = 0; i < T; ++i) ai[i] = l_ai[i];
        for (int e0 = tid; e0 < ne; e0 += 4 * NT) {  // four elements per round: their running sums are requested together
            float acc[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) acc[u] = (first || e0 + u * NT >= ne) ? 0.f : row[off + e0 + u * NT];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int e = e0 + u * NT;
                if (e < ne) {
                    const bool bias = e >= M * h;
                    const int m = bias ? e - M * h : e % M, j = bias ? 0 : e / M;
                    const int o = m / K, k = m - o * K;
                    // all T sample slots, branch-free (a slot beyond nv holds a_i = -1): the reads of an element are in flight together
                    float a_ = acc[u], gv[T], hv[T];
#pragma unroll
                    for (int i = 0; i < T; ++i) gv[i] = l_g[i * AS + k], hv[i] = bias ? 1.0f : l_h[j * T + i];
#pragma unroll
                    for (int i = 0; i < T; ++i) {
                        const float t = bias ? a_ + gv[i] : fmaf(gv[i], hv[i], a_);
                        a_ = (ai[i] == o) ? t : a_;
                    }
                    acc[u] = a_;
                }
            }
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (e0 + u * NT < ne) row[off + e0 + u * NT] = acc[u];
        }
    }
    __syncthreads();  // h(s) is read for the last time below, by the thread that owns (i, j)
    for (int q = tid; q < h * T; q += NT) {
        const int i = q % T, j = q / T;
        const int a = l_ai[i];
        float dz = 0.f;
        if (a >= 0) {
            const float* w2 = W2 + a * K + M * j;
            const float* gi = l_g + i * AS;
            float dh = 0.f;
            for (int k0 = 0; k0 < K; k0 += WCH) {  // WCH weights in flight; the chain itself stays k ascending
                float wv[WCH];
#pragma unroll
                for (int u = 0; u < WCH; ++u) wv[u] = w2[k0 + u < K ? k0 + u : K - 1];
#pragma unroll
                for (int u = 0; u < WCH; ++u) {
                    const float t = fmaf(gi[k0 + u < K ? k0 + u : 0], wv[u], dh);
                    dh = (k0 + u < K) ? t : dh;
                }
            }
            const float hv = l_h[q];
            dz = dh * (ACT == 0 ? (hv > 0.0f ? 1.0f : 0.0f) : (1.0f - hv * hv));
        }
        l_dz[i * HS1 + j] = dz;
    }
    __syncthreads();
    // dW1 and db1
    for (int e = tid; e < h * ns + h; e += NT) {
        const bool bias = e >= h * ns;
        const int j = bias ? e - h * ns : e % h, k = bias ? 0 : e / h;
        float acc = first ? 0.f : row[e];
        float dzv[T], xv[T];
#pragma unroll
        for (int i = 0; i < T; ++i) dzv[i] = l_dz[i * HS1 + j], xv[i] = l_x[k * T + i];
#pragma unroll
        for (int i = 0; i < T; ++i) {
            const float t = bias ? acc + dzv[i] : fmaf(dzv[i], xv[i], acc);
            acc = (i < nv) ? t : acc;
        }
        row[e] = acc;
    }
}

// what a plan launch selects with and where it stores (every pointer nullable; rows_raw: the rows as the net gave them, for a learner
// whose rows_to_q rewrites them (RAW_ROWS), rows_out: as rows_to_q left them)
struct DistPlanOut {
    float *q_out, *rows_raw, *rows_out;
    int32_t* actions;
    int64_t n;
    double eps;
    uint64_t seed;
    uint32_t env_id_base, step;
};

// ---- the tail of a plan kernel: the rows of the tile's envs wait in l_l [T][LS].  One thread per (env, action): Q = rows_to_q(the K
// rows of the action), which may rewrite them in place; then the stores and eps_greedy_select1 per env
template <int T, int NT, int LS, bool RAW_ROWS, class RowsToQ>
__device__ __forceinline__ void dist_plan_tail(const DistPlanOut& g, int64_t e0, int nv, int na, int K, float* l_l, float* l_q,
                                               RowsToQ rows_to_q) {
    const int tid = threadIdx.x, M = na * K;
    if (RAW_ROWS && g.rows_raw) {
        for (int q = tid; q < M * T; q += NT) {
            const int i = q % T, m = q / T;
            if (i < nv) g.rows_raw[(int64_t)m * g.n + e0 + i] = l_l[i * LS + m];
        }
        __syncthreads();
    }
    if (tid < na * T) {
        const int i = tid % T, o = tid / T;
        l_q[o * T + i] = rows_to_q(l_l + i * LS + o * K);
    }
    __syncthreads();
    if (g.rows_out) {
        for (int q = tid; q < M * T; q += NT) {
            const int i = q % T, m = q / T;
            if (i < nv) g.rows_out[(int64_t)m * g.n + e0 + i] = l_l[i * LS + m];
        }
    }
    if (g.q_out && tid < na * T) {
        const int i = tid % T, o = tid / T;
        if (i < nv) g.q_out[(int64_t)o * g.n + e0 + i] = l_q[tid];
    }
    if (g.actions && tid < nv) {
        const int64_t env = e0 + tid;
        g.actions[env] = eps_greedy_select1(StridedValues{l_q + tid, T}, NoMask{}, na, g.eps, false, g.seed, g.env_id_base + (uint32_t)env,
                                            g.step);
    }
}

// ---- logits -> probabilities -> Q, shared by c51.hip and noisy.hip; the loops run in chunks of ACH atoms (DIST_CH above)
__device__ __forceinline__ float c51_atom(int k, float v_min, float delta) { return fmaf((float)k, delta, v_min); }

// e[k] = expf(l[k] - mx), S = sum_k e[k] in ascending k -> S (e may alias l)
template <int ACH>
__device__ __forceinline__ float c51_exp_sum(const float* l, float* e, int n_atoms, float& mx) {
    mx = l[0];
    for (int k0 = 0; k0 < n_atoms; k0 += ACH) {
        float v[ACH];
#pragma unroll
        for (int u = 0; u < ACH; ++u) v[u] = l[k0 + u < n_atoms ? k0 + u : 0];
#pragma unroll
        for (int u = 0; u < ACH; ++u) mx = v[u] > mx ? v[u] : mx;
    }
    float S = 0.f;
    for (int k0 = 0; k0 < n_atoms; k0 += ACH) {
        float v[ACH];
#pragma unroll
        for (int u = 0; u < ACH; ++u) v[u] = l[k0 + u < n_atoms ? k0 + u : n_atoms - 1];
#pragma unroll
        for (int u = 0; u < ACH; ++u) v[u] = expf(v[u] - mx);
#pragma unroll
        for (int u = 0; u < ACH; ++u) {
            if (k0 + u < n_atoms) e[k0 + u] = v[u];
            S = (k0 + u < n_atoms) ? S + v[u] : S;
        }
    }
    return S;
}

// logits of one action -> its probabilities (in place) and Q = sum_k z_k p_k, both in ascending k
template <int ACH>
__device__ __forceinline__ float c51_probs_q(float* l, int n_atoms, float v_min, float delta) {
    float mx;
    const float S = c51_exp_sum<ACH>(l, l, n_atoms, mx);
    float q = 0.f;
    for (int k0 = 0; k0 < n_atoms; k0 += ACH) {
        float v[ACH];
#pragma unroll
        for (int u = 0; u < ACH; ++u) v[u] = l[k0 + u < n_atoms ? k0 + u : n_atoms - 1];
#pragma unroll
        for (int u = 0; u < ACH; ++u) v[u] = v[u] / S;
#pragma unroll
        for (int u = 0; u < ACH; ++u) {
            if (k0 + u < n_atoms) l[k0 + u] = v[u];
            const float t = fmaf(c51_atom(k0 + u, v_min, delta), v[u], q);
            q = (k0 + u < n_atoms) ? t : q;
        }
    }
    return q;
}

}  // namespace rlhip
