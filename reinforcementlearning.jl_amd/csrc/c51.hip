// c51.hip -- the categorical (C51) distributional DQN learner: forward / plan! as one launch, and the loss / gradient of a two-layer
// network mlp2(ns, h, M = na * n_atoms) on a MATERIALISED batch (the SoA arrays rlhip_dqn_grad_batch_f32 takes).  include/rlhip.h is
// the specification (formulas, roundings, summation orders); tests/c51_ref.py replays it.
//
// Output row m = k + n_atoms * o is atom k of action o.  M is up to 256 rows: one lane cannot hold a sample's logits, so every forward
// pass is "thread = output row": the thread reads its W2 row from global memory once (coalesced along m, L2-resident) and carries one
// fmaf chain over j ascending per sample of the tile, the hidden vectors read as LDS broadcasts.  VALU work throughout: ns * h + M * h
// is at most 70k FMAs per sample, the launches are bound by their dependent chains, not by arithmetic.
//
//   c51_plan_kernel<ACT>   16 envs per workgroup of 256 threads: layer 1 -> LDS, logits (thread = row), then one thread per
//                          (env, action): softmax and Q = sum z_k p_k in ascending k (c51_probs_q, the one definition of logits -> Q
//                          for forward, plan and the gradient's target side), then eps_greedy_select1 per env.  rlhip_c51_forward_f32 is
//                          the same launch without the selection
//   c51_grad_kernel<ACT>   tiles of 8 samples, 256 threads (a batch of 32 already spreads over four CUs).  Per tile: target net on s'
//                          [, online net on s'] -> Q, a*; the dense projection m; online net on s -> cross-entropy and g; then ONE
//                          fmaf chain per gradient element over the workgroup's samples in ascending order, carried from tile to
//                          tile through the workgroup's own partial row
//   c51_reduce_kernel      the partial rows, one per workgroup, ascending
// No float atomics anywhere: two calls on the same inputs give the same bytes.
#include "dist_device.h"  // c51_layer1, c51_logits: the two forward chains, shared with qrdqn.hip
#include "select_device.h"

namespace rlhip {

constexpr int C51_MAXA = 64;         // atoms
constexpr int C51_MAXM = 256;        // output rows = na * n_atoms
constexpr int C51_HMAX = 256;
constexpr int C51_PT = 16;           // plan: envs per workgroup
constexpr int C51_PTHREADS = 256;
constexpr int C51_GT = 8;            // gradient: samples per tile
constexpr int C51_GTHREADS = 256;
constexpr int C51_GSPT = C51_GT / (C51_GTHREADS / C51_MAXM);  // samples per thread of the logits pass (8)
constexpr int C51_QO = MAXO * C51_GT > 64 ? MAXO * C51_GT : 64;  // first thread of the online net's (sample, action) pairs: another wave
constexpr int C51_MAX_BLOCKS = 256;  // partial rows (one workgroup per CU); a larger batch gives its workgroups further tiles
constexpr int64_t C51_MAX_PARTIAL_BYTES = 16 << 20;  // ... and at most 16 MiB of them (a row is up to 280 KB: 59 rows at the largest shape)
constexpr int C51_AS = C51_MAXA + 1; // per-sample atom rows in LDS are 65 floats apart
constexpr int C51_GPOW = 33;         // gamma^n for n = 0..32
constexpr int C51_WCH = 16;          // weights of a W2 row requested together (the logits pass, dh)

__device__ __forceinline__ float c51_atom(int k, float v_min, float delta) { return fmaf((float)k, delta, v_min); }

// The per-atom loops below run in chunks of C51_ACH atoms: the chunk is read from LDS first, its expf / divisions are independent of
// each other (one thread owns a whole distribution: instruction-level parallelism is all it has), and the sums are then taken atom by
// atom in ascending k, so the chunking changes no rounding.  An atom beyond n_atoms is read from a clamped index and dropped by a select.
// The gradient kernel uses chunks of 8; the plan kernel, whose workgroups each pass once through their code, keeps the plain loops
// (chunks of 1: with the unrolled bodies it measured 23.4 us at 4096 envs, with the loops 17.8 -- profiles/c51.md).
constexpr int C51_ACH = 8;

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

struct C51PlanArgs {
    const float* params;
    const float* obs;
    float* q_out;       // nullable
    float* probs_out;   // nullable
    float* logits_out;  // nullable
    int32_t* actions;   // nullable: forward
    int64_t n;
    int ns, h, na, n_atoms;
    float v_min, delta;
    double eps;
    uint64_t seed;
    uint32_t env_id_base, step;
};

template <int ACT>
__global__ __launch_bounds__(C51_PTHREADS) void c51_plan_kernel(C51PlanArgs g) {
    constexpr int T = C51_PT, LS = C51_MAXM + 1;
    __shared__ float l_x[16 * T];
    __shared__ __attribute__((aligned(16))) float l_h[C51_HMAX * T];
    __shared__ float l_l[T * LS];
    __shared__ float l_q[MAXO * T];
    const int tid = threadIdx.x;
    const int ns = g.ns, h = g.h, na = g.na, n_atoms = g.n_atoms, M = na * n_atoms;
    const int64_t e0 = (int64_t)blockIdx.x * T;
    const int nv = (int)(g.n - e0 < T ? g.n - e0 : T);
    if (tid < 16 * T) {
        const int i = tid % T, k = tid / T;
        l_x[tid] = (k < ns && i < nv) ? g.obs[(int64_t)k * g.n + e0 + i] : 0.f;
    }
    __syncthreads();
    c51_layer1<ACT, T, C51_PTHREADS>(g.params, ns, h, l_x, l_h);
    __syncthreads();
    if (tid < M) c51_logits<T, T, 4>(g.params, ns, h, M, tid, 0, l_h, l_l, LS);
    __syncthreads();
    if (g.logits_out) {
        for (int q = tid; q < M * T; q += C51_PTHREADS) {
            const int i = q % T, m = q / T;
            if (i < nv) g.logits_out[(int64_t)m * g.n + e0 + i] = l_l[i * LS + m];
        }
        __syncthreads();
    }
    if (tid < na * T) {
        const int i = tid % T, o = tid / T;
        l_q[o * T + i] = c51_probs_q<1>(l_l + i * LS + o * n_atoms, n_atoms, g.v_min, g.delta);
    }
    __syncthreads();
    if (g.probs_out) {
        for (int q = tid; q < M * T; q += C51_PTHREADS) {
            const int i = q % T, m = q / T;
            if (i < nv) g.probs_out[(int64_t)m * g.n + e0 + i] = l_l[i * LS + m];
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

struct C51GradArgs {
    const float* params;
    const float* tparams;
    const float* s;
    const int32_t* a;
    const float* r;
    const uint8_t* term;
    const float* sn;
    const int32_t* n_used;  // nullable
    const float* isw;       // nullable
    float* partials;
    float* loss_partials;
    float* ce_out;     // nullable
    float* proj_out;   // nullable
    int32_t* sel_out;  // nullable
    int64_t batch;
    int ns, h, na, n_atoms, np, num_tiles, double_dqn;
    float gamma, v_min, v_max, delta, fb;
    float gpow[C51_GPOW];
};

template <int ACT>
// (the second bound: two waves per SIMD, i.e. at most 256 registers -- the chunks of weights in flight live in them -- and two
// workgroups per CU; a launch has at most 256 workgroups)
__global__ __launch_bounds__(C51_GTHREADS, 2) void c51_grad_kernel(C51GradArgs g) {
    constexpr int T = C51_GT, NT = C51_GTHREADS, AS = C51_AS;
    static_assert(16 * T <= NT && C51_QO + MAXO * T <= NT && C51_QO % T == 0 && (16 * T) % 4 == 0, "thread maps of the tile");
    // LDS: static, sized for h = 256 and 256 rows (33 KB), so that every address is an immediate
    constexpr int LS = C51_MAXM + 1;   // logit rows are 257 floats apart (odd); the dz rows [T][h + 1 <= 257] reuse the first buffer
    constexpr int HS1 = C51_HMAX + 1;
    __shared__ __attribute__((aligned(16))) float l_h[C51_HMAX * T];  // [h][T]
    __shared__ float l_x[16 * T], l_xn[16 * T];                       // [16][T]
    __shared__ float l_lt[T * LS];                                    // target logits / probabilities of s'; later dz
    __shared__ float l_lo[T * LS];                                    // online logits of s', then of s
    __shared__ float l_qt[MAXO * T], l_qo[MAXO * T];
    __shared__ float l_tz[T * AS], l_m[T * AS];
    __shared__ float l_g[T * AS];                                     // e_k of the cross-entropy line, then g_k
    __shared__ float l_r[T], l_c[T], l_w[T], l_loss[T], l_gp[C51_GPOW];
    __shared__ int l_ai[T];                                           // the sample's action, -1 where it selects nothing
    __shared__ int l_as[T];                                           // a*
    const int ns = g.ns, h = g.h, na = g.na, n_atoms = g.n_atoms, M = na * n_atoms;

    const int tid = threadIdx.x;
    const int lm = tid % C51_MAXM, li0 = (tid / C51_MAXM) * C51_GSPT;  // the logits pass: row lm, samples li0 .. li0 + 7
    const float* W2 = g.params + h * ns + h;
    float s_loss = 0.f;  // thread 0: the workgroup's loss chain
    float* row = g.partials + (int64_t)blockIdx.x * g.np;
    if (tid < C51_GPOW) {  // the table is read from the kernel-argument segment with a per-lane index: no scalar register holds it
        const char* ka = (const char*)__builtin_amdgcn_kernarg_segment_ptr();
        l_gp[tid] = reinterpret_cast<const float*>(ka + offsetof(C51GradArgs, gpow))[tid];
    }

    for (int tile = blockIdx.x; tile < g.num_tiles; tile += gridDim.x) {
        const bool first = tile == (int)blockIdx.x;
        const int64_t b0 = (int64_t)tile * T;
        const int nv = (int)(g.batch - b0 < T ? g.batch - b0 : T);
        // ---- the tile's states (coalesced along the batch) and scalars
        if (tid < 16 * T) {
            const int i = tid % T, k = tid / T;
            const bool in = k < ns && i < nv;
            l_x[tid] = in ? g.s[(int64_t)k * g.batch + b0 + i] : 0.f;
            l_xn[tid] = in ? g.sn[(int64_t)k * g.batch + b0 + i] : 0.f;
        }
        __syncthreads();  // (also: l_gp is written, the previous tile's readers of l_h / l_lt are done)
        if (tid < T) {
            float r = 0.f, c = 0.f, w = 1.0f;
            int a = -1;
            if (tid < nv) {
                const int64_t b = b0 + tid;
                r = g.r[b];
                a = g.a[b];
                if (a < 0 || a >= na) a = -1;  // the action is only ever COMPARED: one outside 0 .. na - 1 selects nothing
                const float cont = g.term[b] ? 0.f : 1.f;
                float disc = g.gamma;
                if (g.n_used) {
                    int nu = g.n_used[b];
                    nu = nu < 0 ? 0 : (nu > C51_GPOW - 1 ? C51_GPOW - 1 : nu);
                    disc = l_gp[nu];
                }
                c = disc * cont;
                if (g.isw) w = g.isw[b];
            }
            l_r[tid] = r, l_c[tid] = c, l_w[tid] = w, l_ai[tid] = a;
        }
        // ---- target net on s' [, online net on s']
        c51_layer1<ACT, T, NT>(g.tparams, ns, h, l_xn, l_h);
        __syncthreads();
        if (lm < M) c51_logits<T, C51_GSPT, C51_WCH>(g.tparams, ns, h, M, lm, li0, l_h, l_lt, LS);
        __syncthreads();
        if (g.double_dqn) {  // (uniform)
            c51_layer1<ACT, T, NT>(g.params, ns, h, l_xn, l_h);
            __syncthreads();
            if (lm < M) c51_logits<T, C51_GSPT, C51_WCH>(g.params, ns, h, M, lm, li0, l_h, l_lo, LS);
            __syncthreads();
        }
        // ---- Q of both: one thread per (sample, action); the online net's pairs sit in other waves
        if (tid < na * T) {
            const int i = tid % T, o = tid / T;
            l_qt[o * T + i] = c51_probs_q<C51_ACH>(l_lt + i * LS + o * n_atoms, n_atoms, g.v_min, g.delta);
        } else if (g.double_dqn && tid >= C51_QO && tid < C51_QO + na * T) {
            const int i = tid % T, o = (tid - C51_QO) / T;
            l_qo[o * T + i] = c51_probs_q<C51_ACH>(l_lo + i * LS + o * n_atoms, n_atoms, g.v_min, g.delta);
        }
        __syncthreads();
        if (tid < T) {  // a*: the first maximum wins (strict >)
            const float* q = g.double_dqn ? l_qo : l_qt;
            int as = 0;
            float mq = q[tid];
            for (int o = 1; o < na; ++o)
                if (q[o * T + tid] > mq) mq = q[o * T + tid], as = o;
            l_as[tid] = as;
            if (g.sel_out && tid < nv) g.sel_out[b0 + tid] = as;
        }
        for (int q = tid; q < n_atoms * T; q += NT) {  // Tz_j = clamp(r + c z_j)
            const int i = q % T, j = q / T;
            const float t = l_r[i] + l_c[i] * c51_atom(j, g.v_min, g.delta);
            l_tz[i * AS + j] = fminf(fmaxf(t, g.v_min), g.v_max);
        }
        __syncthreads();
        // ---- the dense projection: m_k = sum_j clamp(1 - |Tz_j - z_k| / delta, 0, 1) pt_j, j ascending
        for (int q = tid; q < n_atoms * T; q += NT) {
            const int i = q % T, k = q / T;
            const float zk = c51_atom(k, g.v_min, g.delta);
            const float* pt = l_lt + i * LS + l_as[i] * n_atoms;
            const float* tz = l_tz + i * AS;
            float m = 0.f;
            for (int j0 = 0; j0 < n_atoms; j0 += C51_ACH) {  // the divisions of a chunk are independent; the chain stays j ascending
                float wgt[C51_ACH], pj[C51_ACH];
#pragma unroll
                for (int u = 0; u < C51_ACH; ++u) {
                    const int j = j0 + u < n_atoms ? j0 + u : n_atoms - 1;
                    wgt[u] = tz[j], pj[u] = pt[j];
                }
#pragma unroll
                for (int u = 0; u < C51_ACH; ++u) wgt[u] = fminf(fmaxf(1.0f - fabsf(wgt[u] - zk) / g.delta, 0.f), 1.0f);
#pragma unroll
                for (int u = 0; u < C51_ACH; ++u) {
                    const float t = fmaf(wgt[u], pj[u], m);
                    m = (j0 + u < n_atoms) ? t : m;
                }
            }
            l_m[i * AS + k] = m;
            if (g.proj_out && i < nv) g.proj_out[(int64_t)k * g.batch + b0 + i] = m;
        }
        // ---- online net on s; h(s) stays in l_h for the backward pass
        c51_layer1<ACT, T, NT>(g.params, ns, h, l_x, l_h);
        __syncthreads();
        if (lm < M) c51_logits<T, C51_GSPT, C51_WCH>(g.params, ns, h, M, lm, li0, l_h, l_lo, LS);
        __syncthreads();
        if (tid < T) {  // the cross-entropy line of sample `tid`
            const int a = l_ai[tid];
            float L = 0.f;
            if (a >= 0) {
                const float* l = l_lo + tid * LS + a * n_atoms;
                float* e = l_g + tid * AS;
                const float* m = l_m + tid * AS;
                float mx;
                const float S = c51_exp_sum<C51_ACH>(l, e, n_atoms, mx);
                const float logS = logf(S);
                float acc = 0.f, Sm = 0.f;
                for (int k = 0; k < n_atoms; ++k) {
                    const float lp = (l[k] - mx) - logS;
                    acc = fmaf(m[k], lp, acc);
                    Sm += m[k];
                }
                L = -acc;
                const float w = l_w[tid];
                for (int k = 0; k < n_atoms; ++k) {
                    float gk = ((e[k] / S) * Sm - m[k]) / g.fb;
                    if (g.isw) gk *= w;
                    e[k] = gk;
                }
                if (g.ce_out) g.ce_out[b0 + tid] = L;
                if (g.isw) L *= w;
            } else if (tid < nv && g.ce_out) {
                g.ce_out[b0 + tid] = 0.f;
            }
            l_loss[tid] = L;
        }
        __syncthreads();
        if (tid == 0)
            for (int i = 0; i < nv; ++i) s_loss += l_loss[i];
        // ---- dW2 and db2: element (m, j), one chain over the samples whose action owns row m
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
                        const int o = m / n_atoms, k = m - o * n_atoms;
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
        __syncthreads();  // h(s) is read for the last time below, by the thread that owns (i, j); dz goes to l_lt
        for (int q = tid; q < h * T; q += NT) {
            const int i = q % T, j = q / T;
            const int a = l_ai[i];
            float dz = 0.f;
            if (a >= 0) {
                const float* w2 = W2 + a * n_atoms + M * j;
                const float* gi = l_g + i * AS;
                float dh = 0.f;
                for (int k0 = 0; k0 < n_atoms; k0 += C51_WCH) {  // sixteen weights in flight; the chain itself stays k ascending
                    float wv[C51_WCH];
#pragma unroll
                    for (int u = 0; u < C51_WCH; ++u) wv[u] = w2[k0 + u < n_atoms ? k0 + u : n_atoms - 1];
#pragma unroll
                    for (int u = 0; u < C51_WCH; ++u) {
                        const float t = fmaf(gi[k0 + u < n_atoms ? k0 + u : 0], wv[u], dh);
                        dh = (k0 + u < n_atoms) ? t : dh;
                    }
                }
                const float hv = l_h[q];
                dz = dh * (ACT == 0 ? (hv > 0.0f ? 1.0f : 0.0f) : (1.0f - hv * hv));
            }
            l_lt[i * HS1 + j] = dz;
        }
        __syncthreads();
        // ---- dW1 and db1
        for (int e = tid; e < h * ns + h; e += NT) {
            const bool bias = e >= h * ns;
            const int j = bias ? e - h * ns : e % h, k = bias ? 0 : e / h;
            float acc = first ? 0.f : row[e];
            float dzv[T], xv[T];
#pragma unroll
            for (int i = 0; i < T; ++i) dzv[i] = l_lt[i * HS1 + j], xv[i] = l_x[k * T + i];
#pragma unroll
            for (int i = 0; i < T; ++i) {
                const float t = bias ? acc + dzv[i] : fmaf(dzv[i], xv[i], acc);
                acc = (i < nv) ? t : acc;
            }
            row[e] = acc;
        }
        __syncthreads();  // the next tile rewrites every buffer
    }
    if (tid == 0) g.loss_partials[blockIdx.x] = s_loss;
}

// gradient element p and the loss: the partial rows / losses of workgroups 0, 1, .. in ascending order, from +0
__global__ __launch_bounds__(256) void c51_reduce_kernel(const float* __restrict__ partials, const float* __restrict__ loss_partials, int nb,
                                                         int np, float* __restrict__ grad, float* __restrict__ loss, float fb) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p < np) {
        float acc = 0.f;
#pragma unroll 8
        for (int b = 0; b < nb; ++b) acc += partials[(int64_t)b * np + p];
        grad[p] = acc;
    }
    if (p == 0) {
        float a = 0.f;
        for (int b = 0; b < nb; ++b) a += loss_partials[b];
        loss[0] = a / fb;
    }
}

#ifdef RLHIP_BOUNDS_CHECK
__global__ __launch_bounds__(256) void c51_count_bad_actions_kernel(const int32_t* __restrict__ a, int64_t batch, int na, int* __restrict__ n_bad) {
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b < batch && (a[b] < 0 || a[b] >= na)) atomicAdd(n_bad, 1);
}
#endif

template <int ACT>
static int32_t c51_launch_grad(const C51GradArgs& g, int nb, hipStream_t s) {
    hipLaunchKernelGGL((c51_grad_kernel<ACT>), dim3(nb), dim3(C51_GTHREADS), 0, s, g);
    return RLHIP_OK;
}

// workgroups = partial rows: one per tile up to C51_MAX_BLOCKS and C51_MAX_PARTIAL_BYTES of rows
static int64_t c51_num_blocks(int64_t np, int64_t batch) {
    const int64_t tiles = (batch + C51_GT - 1) / C51_GT;
    int64_t cap = C51_MAX_PARTIAL_BYTES / (np * (int64_t)sizeof(float));
    cap = cap < 1 ? 1 : (cap > C51_MAX_BLOCKS ? C51_MAX_BLOCKS : cap);
    return tiles < cap ? tiles : cap;
}

static bool c51_shape_ok(int64_t ns, int64_t h, int64_t na, int64_t n_atoms) {
    return ns >= 2 && ns <= 16 && h >= 4 && h <= C51_HMAX && h % 4 == 0 && na >= 1 && na <= MAXO && n_atoms >= 2 && n_atoms <= C51_MAXA;
}

static bool c51_support_ok(float v_min, float v_max) { return std::isfinite(v_min) && std::isfinite(v_max) && v_min < v_max; }

}  // namespace rlhip

using namespace rlhip;

#define C51_REQUIRE_SHAPE()                                                                                          \
    RLHIP_REQUIRE(ns >= 2 && ns <= 16, "obs dim must be 2..16");                                                     \
    RLHIP_REQUIRE(h >= 4 && h <= C51_HMAX && h % 4 == 0, "hidden must be a multiple of 4, <= 256");                  \
    RLHIP_REQUIRE(na >= 1 && na <= MAXO, "na must be 1..4");                                                         \
    RLHIP_REQUIRE(n_atoms >= 2 && n_atoms <= C51_MAXA, "n_atoms must be 2..64");                                     \
    RLHIP_REQUIRE(act == 0 || act == 1, "act must be 0 (relu) or 1 (tanh)");                                         \
    RLHIP_REQUIRE(c51_support_ok(v_min, v_max), "the support needs finite v_min < v_max")

static int32_t c51_plan_launch(const float* params, int64_t ns, int64_t h, int64_t na, int64_t n_atoms, int32_t act, float v_min,
                               float v_max, const float* obs, int64_t n, double eps, uint64_t seed, uint32_t env_id_base, uint32_t step,
                               int32_t* actions, float* q_out, float* probs_out, float* logits_out, rlhip_stream_t stream) {
    C51PlanArgs g;
    g.params = params, g.obs = obs, g.q_out = q_out, g.probs_out = probs_out, g.logits_out = logits_out, g.actions = actions;
    g.n = n, g.ns = (int)ns, g.h = (int)h, g.na = (int)na, g.n_atoms = (int)n_atoms;
    g.v_min = v_min, g.delta = (v_max - v_min) / (float)(n_atoms - 1);
    g.eps = eps, g.seed = seed, g.env_id_base = env_id_base, g.step = step;
    const dim3 grid((unsigned)((n + C51_PT - 1) / C51_PT));
    // the instantiation set: ACT in {0, 1}
    if (act == 0) hipLaunchKernelGGL((c51_plan_kernel<0>), grid, dim3(C51_PTHREADS), 0, as_stream(stream), g);
    else hipLaunchKernelGGL((c51_plan_kernel<1>), grid, dim3(C51_PTHREADS), 0, as_stream(stream), g);
    RLHIP_LAUNCH_CHECK();
    return RLHIP_OK;
}

extern "C" {

int32_t rlhip_c51_forward_f32(const float* params, int64_t ns, int64_t h, int64_t na, int64_t n_atoms, int32_t act, float v_min,
                              float v_max, const float* obs, int64_t n, float* q_out, float* probs_out, float* logits_out,
                              rlhip_stream_t stream) {
    C51_REQUIRE_SHAPE();
    RLHIP_REQUIRE(n >= 0 && n <= 0x7fffffffLL, "env count must be 0 .. 2^31 - 1");
    RLHIP_REQUIRE(params && obs && q_out, "NULL argument");
    if (n == 0) return RLHIP_OK;
    return c51_plan_launch(params, ns, h, na, n_atoms, act, v_min, v_max, obs, n, 0.0, 0, 0, 0, nullptr, q_out, probs_out, logits_out,
                           stream);
}

int32_t rlhip_c51_plan_f32(const float* params, int64_t ns, int64_t h, int64_t na, int64_t n_atoms, int32_t act, float v_min, float v_max,
                           const float* obs, int64_t n, double eps, uint64_t seed, uint32_t env_id_base, uint32_t step, int32_t* actions,
                           float* q_out, rlhip_stream_t stream) {
    C51_REQUIRE_SHAPE();
    RLHIP_REQUIRE(n >= 0 && n <= 0x7fffffffLL, "env count must be 0 .. 2^31 - 1");
    RLHIP_REQUIRE(params && obs && actions, "NULL argument");
    if (n == 0) return RLHIP_OK;
    return c51_plan_launch(params, ns, h, na, n_atoms, act, v_min, v_max, obs, n, eps, seed, env_id_base, step, actions, q_out, nullptr,
                           nullptr, stream);
}

int64_t rlhip_c51_workspace_bytes(int64_t ns, int64_t h, int64_t na, int64_t n_atoms, int64_t batch) {
    if (!c51_shape_ok(ns, h, na, n_atoms) || batch < 1) return -1;
    const int64_t np = mlp2_nparams(ns, h, na * n_atoms);
    return c51_num_blocks(np, batch) * (np + 1) * (int64_t)sizeof(float);  // partial rows | partial losses
}

int32_t rlhip_c51_grad_batch_f32(int64_t ns, int64_t h, int64_t na, int64_t n_atoms, int32_t act, float v_min, float v_max,
                                 const float* params, const float* target_params, const float* s, const int32_t* a, const float* r,
                                 const uint8_t* term, const float* s_next, int64_t batch, float gamma, const int32_t* n_used,
                                 const float* weights, int32_t double_dqn, void* workspace, float* grad_out, float* loss_out,
                                 float* ce_out, float* proj_out, int32_t* sel_out, rlhip_stream_t stream) {
    C51_REQUIRE_SHAPE();
    RLHIP_REQUIRE(batch >= 1 && batch <= 0x7fffffffLL, "batch must be 1 .. 2^31 - 1");
    RLHIP_REQUIRE(params && target_params && s && a && r && term && s_next && workspace && grad_out && loss_out, "NULL argument");
    hipStream_t st = as_stream(stream);
#ifdef RLHIP_BOUNDS_CHECK
    {  // the debug build: an action outside 0 .. na - 1 is an error instead of a sample without a gradient
        int* cnt = (int*)workspace;
        int n_bad = 0;
        RLHIP_CHECK_HIP(hipMemsetAsync(cnt, 0, sizeof(int), st));
        hipLaunchKernelGGL(c51_count_bad_actions_kernel, dim3((int)((batch + 255) / 256)), dim3(256), 0, st, a, batch, (int)na, cnt);
        RLHIP_LAUNCH_CHECK();
        RLHIP_CHECK_HIP(hipMemcpyAsync(&n_bad, cnt, sizeof(int), hipMemcpyDeviceToHost, st));
        RLHIP_CHECK_HIP(hipStreamSynchronize(st));
        if (n_bad) {
            ::rlhip::set_error("%s:%d: %d of %lld actions are outside 0 .. %lld", __FILE__, __LINE__, n_bad, (long long)batch, (long long)na - 1);
            return RLHIP_EINVAL;
        }
    }
#endif
    const int64_t np = mlp2_nparams(ns, h, na * n_atoms);
    C51GradArgs g;
    g.params = params, g.tparams = target_params;
    g.s = s, g.a = a, g.r = r, g.term = term, g.sn = s_next;
    g.n_used = n_used, g.isw = weights, g.ce_out = ce_out, g.proj_out = proj_out, g.sel_out = sel_out;
    g.batch = batch;
    g.ns = (int)ns, g.h = (int)h, g.na = (int)na, g.n_atoms = (int)n_atoms, g.np = (int)np;
    g.num_tiles = (int)((batch + C51_GT - 1) / C51_GT);
    g.double_dqn = double_dqn ? 1 : 0;
    g.gamma = gamma, g.v_min = v_min, g.v_max = v_max, g.delta = (v_max - v_min) / (float)(n_atoms - 1), g.fb = (float)batch;
    for (int n = 0; n < C51_GPOW; ++n) g.gpow[n] = rlhip_gamma_pow(gamma, n);
    const int nb = (int)c51_num_blocks(np, batch);
    g.partials = (float*)workspace;
    g.loss_partials = g.partials + (int64_t)nb * np;
    // the instantiation set: ACT in {0, 1}
    const int32_t rc = act == 0 ? c51_launch_grad<0>(g, nb, st) : c51_launch_grad<1>(g, nb, st);
    if (rc) return rc;
    RLHIP_LAUNCH_CHECK();
    hipLaunchKernelGGL(c51_reduce_kernel, dim3((int)((np + 255) / 256)), dim3(256), 0, st, g.partials, g.loss_partials, nb, (int)np, grad_out,
                       loss_out, g.fb);
    RLHIP_LAUNCH_CHECK();
    return RLHIP_OK;
}

}  // extern "C"
