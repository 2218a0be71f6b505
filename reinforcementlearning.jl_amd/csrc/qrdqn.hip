// qrdqn.hip -- the quantile-regression (QR-DQN) distributional DQN learner: forward / plan! as one launch, and the quantile-Huber loss /
// gradient of a two-layer network mlp2(ns, h, M = na * N) on a MATERIALISED batch (the SoA arrays rlhip_dqn_grad_batch_f32 takes).
// include/rlhip.h is the specification (formulas, roundings, summation orders); tests/qrdqn_ref.py replays it.
//
// Output row m = k + N * o is quantile k of action o.  The two forward chains (layer 1 into LDS, "thread = output row" for the M rows)
// are the C51 learner's, shared through dist_device.h; what differs is everything behind the rows: no softmax, Q = the mean of an
// action's quantiles, and the loss is the N x N pairwise quantile-Huber term.
//
//   qrdqn_plan_kernel<ACT>   16 envs per workgroup of 256 threads: layer 1 -> LDS, rows (thread = row), then one thread per
//                            (env, action): Q = (sum_k th_k) / N in ascending k (qr_mean, the one definition of rows -> Q for forward,
//                            plan and the gradient's selection), then eps_greedy_select1 per env.  rlhip_qrdqn_forward_f32 is the same
//                            launch without the selection
//   qrdqn_grad_kernel<ACT>   tiles of 8 samples, 256 threads.  Per tile: target net on s' [, online net on s'] -> Q, a*; T_j; online
//                            net on s; then one thread per (sample, k): the two fmaf chains rho_k and d_k over j ascending, T_j and
//                            th_k read from LDS; then ONE fmaf chain per gradient element over the workgroup's samples in ascending
//                            order, carried from tile to tile through the workgroup's own partial row (the C51 kernel's structure)
//   qrdqn_reduce_kernel      the partial rows, one per workgroup, ascending
// No float atomics anywhere: two calls on the same inputs give the same bytes.
#include "dist_device.h"
#include "select_device.h"

namespace rlhip {

constexpr int QR_MAXN = 64;         // quantiles
constexpr int QR_MAXM = 256;        // output rows = na * N
constexpr int QR_HMAX = 256;
constexpr int QR_PT = 16;           // plan: envs per workgroup
constexpr int QR_PTHREADS = 256;
constexpr int QR_GT = 8;            // gradient: samples per tile
constexpr int QR_GTHREADS = 256;
constexpr int QR_GSPT = QR_GT / (QR_GTHREADS / QR_MAXM);  // samples per thread of the rows pass (8)
constexpr int QR_QO = MAXO * QR_GT > 64 ? MAXO * QR_GT : 64;  // first thread of the online net's (sample, action) pairs: another wave
constexpr int QR_MAX_BLOCKS = 256;  // partial rows (one workgroup per CU); a larger batch gives its workgroups further tiles
constexpr int64_t QR_MAX_PARTIAL_BYTES = 16 << 20;  // ... and at most 16 MiB of them
constexpr int QR_AS = QR_MAXN + 1;  // per-sample quantile rows in LDS are 65 floats apart
constexpr int QR_GPOW = 33;         // gamma^n for n = 0..32
constexpr int QR_WCH = 16;          // weights of a W2 row requested together (the rows pass, dh)
// The per-quantile loops of the gradient kernel run in chunks of QR_CH: the chunk is read from LDS first, its divisions and selects are
// independent of each other (one thread owns a whole chain: instruction-level parallelism is all it has), and the sums are then taken
// one by one in ascending order, so the chunking changes no rounding.  The plan kernel keeps the plain loop (chunks of 1), as the C51
// plan kernel does.
constexpr int QR_CH = 8;

// Q of one action: (sum_k th[k], k ascending, from +0) / (float)N
template <int CH>
__device__ __forceinline__ float qr_mean(const float* th, int N, float fN) {
    float q = 0.f;
    for (int k0 = 0; k0 < N; k0 += CH) {
        float v[CH];
#pragma unroll
        for (int u = 0; u < CH; ++u) v[u] = th[k0 + u < N ? k0 + u : N - 1];
#pragma unroll
        for (int u = 0; u < CH; ++u) q = (k0 + u < N) ? q + v[u] : q;
    }
    return q / fN;
}

struct QRPlanArgs {
    const float* params;
    const float* obs;
    float* q_out;          // nullable
    float* quantiles_out;  // nullable
    int32_t* actions;      // nullable: forward
    int64_t n;
    int ns, h, na, N;
    double eps;
    uint64_t seed;
    uint32_t env_id_base, step;
};

template <int ACT>
__global__ __launch_bounds__(QR_PTHREADS) void qrdqn_plan_kernel(QRPlanArgs g) {
    constexpr int T = QR_PT, LS = QR_MAXM + 1;
    __shared__ float l_x[16 * T];
    __shared__ __attribute__((aligned(16))) float l_h[QR_HMAX * T];
    __shared__ float l_l[T * LS];
    __shared__ float l_q[MAXO * T];
    const int tid = threadIdx.x;
    const int ns = g.ns, h = g.h, na = g.na, N = g.N, M = na * N;
    const int64_t e0 = (int64_t)blockIdx.x * T;
    const int nv = (int)(g.n - e0 < T ? g.n - e0 : T);
    if (tid < 16 * T) {
        const int i = tid % T, k = tid / T;
        l_x[tid] = (k < ns && i < nv) ? g.obs[(int64_t)k * g.n + e0 + i] : 0.f;
    }
    __syncthreads();
    c51_layer1<ACT, T, QR_PTHREADS>(g.params, ns, h, l_x, l_h);
    __syncthreads();
    if (tid < M) c51_logits<T, T, 4>(g.params, ns, h, M, tid, 0, l_h, l_l, LS);
    __syncthreads();
    if (g.quantiles_out) {
        for (int q = tid; q < M * T; q += QR_PTHREADS) {
            const int i = q % T, m = q / T;
            if (i < nv) g.quantiles_out[(int64_t)m * g.n + e0 + i] = l_l[i * LS + m];
        }
    }
    if (tid < na * T) {
        const int i = tid % T, o = tid / T;
        l_q[o * T + i] = qr_mean<1>(l_l + i * LS + o * N, N, (float)N);
    }
    __syncthreads();
    if (g.q_out && tid < na * T) {
        const int i = tid % T;
        if (i < nv) g.q_out[(int64_t)(tid / T) * g.n + e0 + i] = l_q[tid];
    }
    if (g.actions && tid < nv) {
        const int64_t env = e0 + tid;
        g.actions[env] = eps_greedy_select1(StridedValues{l_q + tid, T}, NoMask{}, na, g.eps, false, g.seed, g.env_id_base + (uint32_t)env,
                                            g.step);
    }
}

struct QRGradArgs {
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
    float* ql_out;      // nullable
    float* target_out;  // nullable
    int32_t* sel_out;   // nullable
    int64_t batch;
    int ns, h, na, N, np, num_tiles, double_dqn;
    float gamma, kappa, fN, fNB, fb;  // fNB = (float)N * (float)batch, one Float32 product
    float gpow[QR_GPOW];
};

template <int ACT>
// (two waves per SIMD, i.e. at most 256 registers -- the chunks of weights in flight live in them -- and two workgroups per CU)
__global__ __launch_bounds__(QR_GTHREADS, 2) void qrdqn_grad_kernel(QRGradArgs g) {
    constexpr int T = QR_GT, NT = QR_GTHREADS, AS = QR_AS;
    static_assert(16 * T <= NT && QR_QO + MAXO * T <= NT && QR_QO % T == 0 && (16 * T) % 4 == 0, "thread maps of the tile");
    // LDS: static, sized for h = 256 and 256 rows, so that every address is an immediate
    constexpr int LS = QR_MAXM + 1;   // rows of a sample are 257 floats apart (odd); the dz rows [T][h + 1 <= 257] reuse the first buffer
    constexpr int HS1 = QR_HMAX + 1;
    __shared__ __attribute__((aligned(16))) float l_h[QR_HMAX * T];  // [h][T]
    __shared__ float l_x[16 * T], l_xn[16 * T];                      // [16][T]
    __shared__ float l_lt[T * LS];                                   // target quantiles of s'; later dz
    __shared__ float l_lo[T * LS];                                   // online quantiles of s', then of s
    __shared__ float l_qt[MAXO * T], l_qo[MAXO * T];
    __shared__ float l_T[T * AS];                                    // T_j
    __shared__ float l_rho[T * AS];                                  // rho_k
    __shared__ float l_g[T * AS];                                    // g_k
    __shared__ float l_r[T], l_c[T], l_w[T], l_loss[T], l_gp[QR_GPOW];
    __shared__ int l_ai[T];                                          // the sample's action, -1 where it selects nothing
    __shared__ int l_as[T];                                          // a*
    const int ns = g.ns, h = g.h, na = g.na, N = g.N, M = na * N;

    const int tid = threadIdx.x;
    const int lm = tid % QR_MAXM, li0 = (tid / QR_MAXM) * QR_GSPT;  // the rows pass: row lm, samples li0 .. li0 + 7
    const float* W2 = g.params + h * ns + h;
    const float kappa = g.kappa;
    float s_loss = 0.f;  // thread 0: the workgroup's loss chain
    float* row = g.partials + (int64_t)blockIdx.x * g.np;
    if (tid < QR_GPOW) {  // the table is read from the kernel-argument segment with a per-lane index: no scalar register holds it
        const char* ka = (const char*)__builtin_amdgcn_kernarg_segment_ptr();
        l_gp[tid] = reinterpret_cast<const float*>(ka + offsetof(QRGradArgs, gpow))[tid];
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
                    nu = nu < 0 ? 0 : (nu > QR_GPOW - 1 ? QR_GPOW - 1 : nu);
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
        if (lm < M) c51_logits<T, QR_GSPT, QR_WCH>(g.tparams, ns, h, M, lm, li0, l_h, l_lt, LS);
        __syncthreads();
        if (g.double_dqn) {  // (uniform)
            c51_layer1<ACT, T, NT>(g.params, ns, h, l_xn, l_h);
            __syncthreads();
            if (lm < M) c51_logits<T, QR_GSPT, QR_WCH>(g.params, ns, h, M, lm, li0, l_h, l_lo, LS);
            __syncthreads();
        }
        // ---- Q of both: one thread per (sample, action); the online net's pairs sit in other waves
        if (tid < na * T) {
            const int i = tid % T, o = tid / T;
            l_qt[o * T + i] = qr_mean<QR_CH>(l_lt + i * LS + o * N, N, g.fN);
        } else if (g.double_dqn && tid >= QR_QO && tid < QR_QO + na * T) {
            const int i = tid % T, o = (tid - QR_QO) / T;
            l_qo[o * T + i] = qr_mean<QR_CH>(l_lo + i * LS + o * N, N, g.fN);
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
        __syncthreads();
        for (int q = tid; q < N * T; q += NT) {  // T_j = fmaf(c, th_t(s')[j, a*], r)
            const int i = q % T, j = q / T;
            const float t = fmaf(l_c[i], l_lt[i * LS + l_as[i] * N + j], l_r[i]);
            l_T[i * AS + j] = t;
            if (g.target_out && i < nv) g.target_out[(int64_t)j * g.batch + b0 + i] = t;
        }
        // ---- online net on s; h(s) stays in l_h for the backward pass
        c51_layer1<ACT, T, NT>(g.params, ns, h, l_x, l_h);
        __syncthreads();
        if (lm < M) c51_logits<T, QR_GSPT, QR_WCH>(g.params, ns, h, M, lm, li0, l_h, l_lo, LS);
        __syncthreads();
        // ---- the pairwise term: thread = chain (i, k); rho_k and d_k over j ascending
        for (int q = tid; q < N * T; q += NT) {
            const int i = q % T, k = q / T;
            const int a = l_ai[i];
            const float thk = l_lo[i * LS + (a < 0 ? 0 : a) * N + k];
            const float tau = (float)(2 * k + 1) / (float)(2 * N);
            const float* tj = l_T + i * AS;
            float rho = 0.f, d = 0.f;
            for (int j0 = 0; j0 < N; j0 += QR_CH) {  // the divisions and selects of a chunk are independent; the chains stay j ascending
                float u[QR_CH], hub[QR_CH], dhub[QR_CH], w[QR_CH];
#pragma unroll
                for (int v = 0; v < QR_CH; ++v) u[v] = tj[j0 + v < N ? j0 + v : N - 1] - thk;
#pragma unroll
                for (int v = 0; v < QR_CH; ++v) {
                    const float au = fabsf(u[v]);
                    hub[v] = (au <= kappa ? 0.5f * u[v] * u[v] : kappa * (au - 0.5f * kappa)) / kappa;
                    dhub[v] = fminf(fmaxf(u[v], -kappa), kappa) / kappa;
                    w[v] = u[v] < 0.f ? 1.0f - tau : tau;
                }
#pragma unroll
                for (int v = 0; v < QR_CH; ++v) {
                    const float tr = fmaf(w[v], hub[v], rho), td = fmaf(w[v], dhub[v], d);
                    rho = (j0 + v < N) ? tr : rho;
                    d = (j0 + v < N) ? td : d;
                }
            }
            float gk = -d / g.fNB;
            if (g.isw) gk *= l_w[i];
            l_rho[i * AS + k] = a < 0 ? 0.f : rho;
            l_g[i * AS + k] = a < 0 ? 0.f : gk;
        }
        __syncthreads();
        if (tid < T) {  // L_i of sample `tid`
            float L = 0.f;
            if (l_ai[tid] >= 0) {
                L = qr_mean<QR_CH>(l_rho + tid * AS, N, g.fN);
                if (g.ql_out) g.ql_out[b0 + tid] = L;
                if (g.isw) L *= l_w[tid];
            } else if (tid < nv && g.ql_out) {
                g.ql_out[b0 + tid] = 0.f;
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
                        const int o = m / N, k = m - o * N;
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
                const float* w2 = W2 + a * N + M * j;
                const float* gi = l_g + i * AS;
                float dh = 0.f;
                for (int k0 = 0; k0 < N; k0 += QR_WCH) {  // sixteen weights in flight; the chain itself stays k ascending
                    float wv[QR_WCH];
#pragma unroll
                    for (int u = 0; u < QR_WCH; ++u) wv[u] = w2[k0 + u < N ? k0 + u : N - 1];
#pragma unroll
                    for (int u = 0; u < QR_WCH; ++u) {
                        const float t = fmaf(gi[k0 + u < N ? k0 + u : 0], wv[u], dh);
                        dh = (k0 + u < N) ? t : dh;
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
__global__ __launch_bounds__(256) void qrdqn_reduce_kernel(const float* __restrict__ partials, const float* __restrict__ loss_partials, int nb,
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
__global__ __launch_bounds__(256) void qrdqn_count_bad_actions_kernel(const int32_t* __restrict__ a, int64_t batch, int na, int* __restrict__ n_bad) {
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b < batch && (a[b] < 0 || a[b] >= na)) atomicAdd(n_bad, 1);
}
#endif

template <int ACT>
static int32_t qrdqn_launch_grad(const QRGradArgs& g, int nb, hipStream_t s) {
    hipLaunchKernelGGL((qrdqn_grad_kernel<ACT>), dim3(nb), dim3(QR_GTHREADS), 0, s, g);
    return RLHIP_OK;
}

// workgroups = partial rows: one per tile up to QR_MAX_BLOCKS and QR_MAX_PARTIAL_BYTES of rows
static int64_t qrdqn_num_blocks(int64_t np, int64_t batch) {
    const int64_t tiles = (batch + QR_GT - 1) / QR_GT;
    int64_t cap = QR_MAX_PARTIAL_BYTES / (np * (int64_t)sizeof(float));
    cap = cap < 1 ? 1 : (cap > QR_MAX_BLOCKS ? QR_MAX_BLOCKS : cap);
    return tiles < cap ? tiles : cap;
}

static bool qrdqn_shape_ok(int64_t ns, int64_t h, int64_t na, int64_t N) {
    return ns >= 2 && ns <= 16 && h >= 4 && h <= QR_HMAX && h % 4 == 0 && na >= 1 && na <= MAXO && N >= 1 && N <= QR_MAXN;
}

}  // namespace rlhip

using namespace rlhip;

#define QR_REQUIRE_SHAPE()                                                                                          \
    RLHIP_REQUIRE(ns >= 2 && ns <= 16, "obs dim must be 2..16");                                                    \
    RLHIP_REQUIRE(h >= 4 && h <= QR_HMAX && h % 4 == 0, "hidden must be a multiple of 4, <= 256");                  \
    RLHIP_REQUIRE(na >= 1 && na <= MAXO, "na must be 1..4");                                                        \
    RLHIP_REQUIRE(n_quantiles >= 1 && n_quantiles <= QR_MAXN, "n_quantiles must be 1..64");                         \
    RLHIP_REQUIRE(act == 0 || act == 1, "act must be 0 (relu) or 1 (tanh)")

static int32_t qrdqn_plan_launch(const float* params, int64_t ns, int64_t h, int64_t na, int64_t n_quantiles, int32_t act, const float* obs,
                                 int64_t n, double eps, uint64_t seed, uint32_t env_id_base, uint32_t step, int32_t* actions, float* q_out,
                                 float* quantiles_out, rlhip_stream_t stream) {
    QRPlanArgs g;
    g.params = params, g.obs = obs, g.q_out = q_out, g.quantiles_out = quantiles_out, g.actions = actions;
    g.n = n, g.ns = (int)ns, g.h = (int)h, g.na = (int)na, g.N = (int)n_quantiles;
    g.eps = eps, g.seed = seed, g.env_id_base = env_id_base, g.step = step;
    const dim3 grid((unsigned)((n + QR_PT - 1) / QR_PT));
    // the instantiation set: ACT in {0, 1}
    if (act == 0) hipLaunchKernelGGL((qrdqn_plan_kernel<0>), grid, dim3(QR_PTHREADS), 0, as_stream(stream), g);
    else hipLaunchKernelGGL((qrdqn_plan_kernel<1>), grid, dim3(QR_PTHREADS), 0, as_stream(stream), g);
    RLHIP_LAUNCH_CHECK();
    return RLHIP_OK;
}

extern "C" {

int32_t rlhip_qrdqn_forward_f32(const float* params, int64_t ns, int64_t h, int64_t na, int64_t n_quantiles, int32_t act, const float* obs,
                                int64_t n, float* q_out, float* quantiles_out, rlhip_stream_t stream) {
    QR_REQUIRE_SHAPE();
    RLHIP_REQUIRE(n >= 0 && n <= 0x7fffffffLL, "env count must be 0 .. 2^31 - 1");
    RLHIP_REQUIRE(params && obs && q_out, "NULL argument");
    if (n == 0) return RLHIP_OK;
    return qrdqn_plan_launch(params, ns, h, na, n_quantiles, act, obs, n, 0.0, 0, 0, 0, nullptr, q_out, quantiles_out, stream);
}

int32_t rlhip_qrdqn_plan_f32(const float* params, int64_t ns, int64_t h, int64_t na, int64_t n_quantiles, int32_t act, const float* obs,
                             int64_t n, double eps, uint64_t seed, uint32_t env_id_base, uint32_t step, int32_t* actions, float* q_out,
                             rlhip_stream_t stream) {
    QR_REQUIRE_SHAPE();
    RLHIP_REQUIRE(n >= 0 && n <= 0x7fffffffLL, "env count must be 0 .. 2^31 - 1");
    RLHIP_REQUIRE(params && obs && actions, "NULL argument");
    if (n == 0) return RLHIP_OK;
    return qrdqn_plan_launch(params, ns, h, na, n_quantiles, act, obs, n, eps, seed, env_id_base, step, actions, q_out, nullptr, stream);
}

int64_t rlhip_qrdqn_workspace_bytes(int64_t ns, int64_t h, int64_t na, int64_t n_quantiles, int64_t batch) {
    if (!qrdqn_shape_ok(ns, h, na, n_quantiles) || batch < 1) return -1;
    const int64_t np = mlp2_nparams(ns, h, na * n_quantiles);
    return qrdqn_num_blocks(np, batch) * (np + 1) * (int64_t)sizeof(float);  // partial rows | partial losses
}

int32_t rlhip_qrdqn_grad_batch_f32(int64_t ns, int64_t h, int64_t na, int64_t n_quantiles, int32_t act, float kappa, const float* params,
                                   const float* target_params, const float* s, const int32_t* a, const float* r, const uint8_t* term,
                                   const float* s_next, int64_t batch, float gamma, const int32_t* n_used, const float* weights,
                                   int32_t double_dqn, void* workspace, float* grad_out, float* loss_out, float* ql_out, float* target_out,
                                   int32_t* sel_out, rlhip_stream_t stream) {
    QR_REQUIRE_SHAPE();
    RLHIP_REQUIRE(std::isfinite(kappa) && kappa > 0.f, "kappa must be finite and > 0");
    RLHIP_REQUIRE(batch >= 1 && batch <= 0x7fffffffLL, "batch must be 1 .. 2^31 - 1");
    RLHIP_REQUIRE(params && target_params && s && a && r && term && s_next && workspace && grad_out && loss_out, "NULL argument");
    hipStream_t st = as_stream(stream);
#ifdef RLHIP_BOUNDS_CHECK
    {  // the debug build: an action outside 0 .. na - 1 is an error instead of a sample without a gradient
        int* cnt = (int*)workspace;
        int n_bad = 0;
        RLHIP_CHECK_HIP(hipMemsetAsync(cnt, 0, sizeof(int), st));
        hipLaunchKernelGGL(qrdqn_count_bad_actions_kernel, dim3((int)((batch + 255) / 256)), dim3(256), 0, st, a, batch, (int)na, cnt);
        RLHIP_LAUNCH_CHECK();
        RLHIP_CHECK_HIP(hipMemcpyAsync(&n_bad, cnt, sizeof(int), hipMemcpyDeviceToHost, st));
        RLHIP_CHECK_HIP(hipStreamSynchronize(st));
        if (n_bad) {
            ::rlhip::set_error("%s:%d: %d of %lld actions are outside 0 .. %lld", __FILE__, __LINE__, n_bad, (long long)batch, (long long)na - 1);
            return RLHIP_EINVAL;
        }
    }
#endif
    const int64_t np = mlp2_nparams(ns, h, na * n_quantiles);
    QRGradArgs g;
    g.params = params, g.tparams = target_params;
    g.s = s, g.a = a, g.r = r, g.term = term, g.sn = s_next;
    g.n_used = n_used, g.isw = weights, g.ql_out = ql_out, g.target_out = target_out, g.sel_out = sel_out;
    g.batch = batch;
    g.ns = (int)ns, g.h = (int)h, g.na = (int)na, g.N = (int)n_quantiles, g.np = (int)np;
    g.num_tiles = (int)((batch + QR_GT - 1) / QR_GT);
    g.double_dqn = double_dqn ? 1 : 0;
    g.gamma = gamma, g.kappa = kappa, g.fN = (float)n_quantiles, g.fb = (float)batch, g.fNB = g.fN * g.fb;
    for (int n = 0; n < QR_GPOW; ++n) g.gpow[n] = rlhip_gamma_pow(gamma, n);
    const int nb = (int)qrdqn_num_blocks(np, batch);
    g.partials = (float*)workspace;
    g.loss_partials = g.partials + (int64_t)nb * np;
    // the instantiation set: ACT in {0, 1}
    const int32_t rc = act == 0 ? qrdqn_launch_grad<0>(g, nb, st) : qrdqn_launch_grad<1>(g, nb, st);
    if (rc) return rc;
    RLHIP_LAUNCH_CHECK();
    hipLaunchKernelGGL(qrdqn_reduce_kernel, dim3((int)((np + 255) / 256)), dim3(256), 0, st, g.partials, g.loss_partials, nb, (int)np, grad_out,
                       loss_out, g.fb);
    RLHIP_LAUNCH_CHECK();
    return RLHIP_OK;
}

}  // extern "C"
