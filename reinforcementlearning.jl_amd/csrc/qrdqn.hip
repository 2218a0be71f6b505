// qrdqn.hip -- the quantile-regression (QR-DQN) distributional DQN learner: forward / plan! as one launch, and the quantile-Huber loss /
// gradient of a two-layer network mlp2(ns, h, M = na * N) on a MATERIALISED batch (the SoA arrays rlhip_dqn_grad_batch_f32 takes).
// include/rlhip.h is the specification (formulas, roundings, summation orders); tests/qrdqn_ref.py replays it.
//
// Output row m = k + N * o is quantile k of action o.  The kernels are the stages of dist_device.h, shared with c51.hip (tile loads,
// the two forward chains, a*, the backward pass with its carry, the plan's tail); what is written here is what sits behind the rows: no
// softmax, Q = the mean of an action's quantiles, and the loss is the N x N pairwise quantile-Huber term.
//
//   qrdqn_plan_kernel<ACT>   16 envs per workgroup of 256 threads: layer 1 -> LDS, rows (thread = row), then one thread per
//                            (env, action): Q = (sum_k th_k) / N in ascending k (qr_mean, the one definition of rows -> Q for forward,
//                            plan and the gradient's selection), then eps_greedy_select1 per env.  rlhip_qrdqn_forward_f32 is the same
//                            launch without the selection
//   qrdqn_grad_kernel<ACT>   tiles of 8 samples, 256 threads.  Per tile: target net on s' [, online net on s'] -> Q, a*; T_j; online
//                            net on s; then one thread per (sample, k): the two fmaf chains rho_k and d_k over j ascending, T_j and
//                            th_k read from LDS; then ONE fmaf chain per gradient element over the workgroup's samples in ascending
//                            order, carried from tile to tile through the workgroup's own partial row (dist_backward)
//   dist_reduce_kernel       (dist.hip) the partial rows, one per workgroup, ascending
// No float atomics anywhere: two calls on the same inputs give the same bytes.
#include "dist_host.h"

namespace rlhip {

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
    DistPlanOut out;  // rows_out: the quantiles (qr_mean leaves the rows as they are)
    int ns, h, na, N;
};

template <int ACT>
__global__ __launch_bounds__(DIST_PTHREADS) void qrdqn_plan_kernel(QRPlanArgs g) {
    constexpr int T = DIST_PT, LS = DIST_MAXM + 1;
    __shared__ float l_x[16 * T];
    __shared__ __attribute__((aligned(16))) float l_h[DIST_HMAX * T];
    __shared__ float l_l[T * LS];
    __shared__ float l_q[MAXO * T];
    const int tid = threadIdx.x;
    const int ns = g.ns, h = g.h, na = g.na, N = g.N, M = na * N;
    const int64_t e0 = (int64_t)blockIdx.x * T;
    const int nv = (int)(g.out.n - e0 < T ? g.out.n - e0 : T);
    dist_load_obs<T>(g.obs, g.out.n, e0, nv, ns, l_x);
    __syncthreads();
    dist_layer1<ACT, T, DIST_PTHREADS>(g.params, ns, h, l_x, l_h);
    __syncthreads();
    if (tid < M) dist_rows<T, T, 4>(g.params, ns, h, M, tid, 0, l_h, l_l, LS);
    __syncthreads();
    dist_plan_tail<T, DIST_PTHREADS, LS, false>(g.out, e0, nv, na, N, l_l, l_q, [&](float* th) { return qr_mean<1>(th, N, (float)N); });
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
    float gpow[DIST_GPOW];
};

template <int ACT>
// (two waves per SIMD, i.e. at most 256 registers -- the chunks of weights in flight live in them -- and two workgroups per CU)
__global__ __launch_bounds__(DIST_GTHREADS, 2) void qrdqn_grad_kernel(QRGradArgs g) {
    constexpr int T = DIST_GT, NT = DIST_GTHREADS, AS = DIST_AS;
    static_assert(16 * T <= NT && DIST_QO + MAXO * T <= NT && DIST_QO % T == 0 && (16 * T) % 4 == 0, "thread maps of the tile");
    // LDS: static, sized for h = 256 and 256 rows, so that every address is an immediate
    constexpr int LS = DIST_MAXM + 1;   // rows of a sample are 257 floats apart (odd); the dz rows [T][h + 1 <= 257] reuse the first buffer
    constexpr int HS1 = DIST_HMAX + 1;
    __shared__ __attribute__((aligned(16))) float l_h[DIST_HMAX * T];  // [h][T]
    __shared__ float l_x[16 * T], l_xn[16 * T];                      // [16][T]
    __shared__ float l_lt[T * LS];                                   // target quantiles of s'; later dz
    __shared__ float l_lo[T * LS];                                   // online quantiles of s', then of s
    __shared__ float l_qt[MAXO * T], l_qo[MAXO * T];
    __shared__ float l_T[T * AS];                                    // T_j
    __shared__ float l_rho[T * AS];                                  // rho_k
    __shared__ float l_g[T * AS];                                    // g_k
    __shared__ float l_r[T], l_c[T], l_w[T], l_loss[T], l_gp[DIST_GPOW];
    __shared__ int l_ai[T];                                          // the sample's action, -1 where it selects nothing
    __shared__ int l_as[T];                                          // a*
    const int ns = g.ns, h = g.h, na = g.na, N = g.N, M = na * N;

    const int tid = threadIdx.x;
    const int lm = tid % DIST_MAXM, li0 = (tid / DIST_MAXM) * DIST_GSPT;  // the rows pass: row lm, samples li0 .. li0 + 7
    const float kappa = g.kappa;
    const float* W2 = g.params + h * ns + h;
    float s_loss = 0.f;  // thread 0: the workgroup's loss chain
    float* row = g.partials + (int64_t)blockIdx.x * g.np;
    dist_load_gpow<QRGradArgs>(l_gp);

    for (int tile = blockIdx.x; tile < g.num_tiles; tile += gridDim.x) {
        const bool first = tile == (int)blockIdx.x;
        const int64_t b0 = (int64_t)tile * T;
        const int nv = (int)(g.batch - b0 < T ? g.batch - b0 : T);
        // ---- the tile's states (coalesced along the batch) and scalars
        dist_load_states<T>(g.s, g.sn, g.batch, b0, nv, ns, l_x, l_xn);
        __syncthreads();  // (also: l_gp is written, the previous tile's readers of l_h / l_lt are done)
        dist_tile_scalars<T>(g, b0, nv, l_gp, l_r, l_c, l_w, l_ai);
        // ---- target net on s' [, online net on s']
        dist_layer1<ACT, T, NT>(g.tparams, ns, h, l_xn, l_h);
        __syncthreads();
        if (lm < M) dist_rows<T, DIST_GSPT, DIST_WCH>(g.tparams, ns, h, M, lm, li0, l_h, l_lt, LS);
        __syncthreads();
        if (g.double_dqn) {  // (uniform)
            dist_layer1<ACT, T, NT>(g.params, ns, h, l_xn, l_h);
            __syncthreads();
            if (lm < M) dist_rows<T, DIST_GSPT, DIST_WCH>(g.params, ns, h, M, lm, li0, l_h, l_lo, LS);
            __syncthreads();
        }
        // ---- Q of both: one thread per (sample, action); the online net's pairs sit in other waves
        if (tid < na * T) {
            const int i = tid % T, o = tid / T;
            l_qt[o * T + i] = qr_mean<DIST_CH>(l_lt + i * LS + o * N, N, g.fN);
        } else if (g.double_dqn && tid >= DIST_QO && tid < DIST_QO + na * T) {
            const int i = tid % T, o = (tid - DIST_QO) / T;
            l_qo[o * T + i] = qr_mean<DIST_CH>(l_lo + i * LS + o * N, N, g.fN);
        }
        __syncthreads();
        dist_select_action<T>(g.double_dqn ? l_qo : l_qt, na, l_as, g.sel_out, b0, nv);
        __syncthreads();
        for (int q = tid; q < N * T; q += NT) {  // T_j = fmaf(c, th_t(s')[j, a*], r)
            const int i = q % T, j = q / T;
            const float t = fmaf(l_c[i], l_lt[i * LS + l_as[i] * N + j], l_r[i]);
            l_T[i * AS + j] = t;
            if (g.target_out && i < nv) g.target_out[(int64_t)j * g.batch + b0 + i] = t;
        }
        // ---- online net on s; h(s) stays in l_h for the backward pass
        dist_layer1<ACT, T, NT>(g.params, ns, h, l_x, l_h);
        __syncthreads();
        if (lm < M) dist_rows<T, DIST_GSPT, DIST_WCH>(g.params, ns, h, M, lm, li0, l_h, l_lo, LS);
        __syncthreads();
        // ---- the pairwise term: thread = chain (i, k); rho_k and d_k over j ascending
        for (int q = tid; q < N * T; q += NT) {
            const int i = q % T, k = q / T;
            const int a = l_ai[i];
            const float thk = l_lo[i * LS + (a < 0 ? 0 : a) * N + k];
            const float tau = (float)(2 * k + 1) / (float)(2 * N);
            const float* tj = l_T + i * AS;
            float rho = 0.f, d = 0.f;
            for (int j0 = 0; j0 < N; j0 += DIST_CH) {  // the divisions and selects of a chunk are independent; the chains stay j ascending
                float u[DIST_CH], hub[DIST_CH], dhub[DIST_CH], w[DIST_CH];
#pragma unroll
                for (int v = 0; v < DIST_CH; ++v) u[v] = tj[j0 + v < N ? j0 + v : N - 1] - thk;
#pragma unroll
                for (int v = 0; v < DIST_CH; ++v) {
                    const float au = fabsf(u[v]);
                    hub[v] = (au <= kappa ? 0.5f * u[v] * u[v] : kappa * (au - 0.5f * kappa)) / kappa;
                    dhub[v] = fminf(fmaxf(u[v], -kappa), kappa) / kappa;
                    w[v] = u[v] < 0.f ? 1.0f - tau : tau;
                }
#pragma unroll
                for (int v = 0; v < DIST_CH; ++v) {
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
                L = qr_mean<DIST_CH>(l_rho + tid * AS, N, g.fN);
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
        // ---- dW2 | db2, dh -> dz (into l_lt), dW1 | db1
        dist_backward<ACT, T, NT, AS, HS1, DIST_WCH>(W2, row, first, nv, ns, h, M, N, l_ai, l_g, l_h, l_x, l_lt);
        __syncthreads();  // the next tile rewrites every buffer
    }
    if (tid == 0) g.loss_partials[blockIdx.x] = s_loss;
}

template <int ACT>
static int32_t qrdqn_launch_grad(const QRGradArgs& g, int nb, hipStream_t s) {
    hipLaunchKernelGGL((qrdqn_grad_kernel<ACT>), dim3(nb), dim3(DIST_GTHREADS), 0, s, g);
    return RLHIP_OK;
}

#define QR_SHAPE_BOUNDS(B) \
    DIST_MLP2_BOUNDS(B);   \
    B(n_quantiles >= 1 && n_quantiles <= DIST_MAXK, "n_quantiles must be 1..64")

static bool qrdqn_shape_ok(int64_t ns, int64_t h, int64_t na, int64_t n_quantiles) {
    QR_SHAPE_BOUNDS(DIST_BOUND_HOLDS);
    return true;
}

}  // namespace rlhip

using namespace rlhip;

#define QR_REQUIRE_SHAPE()         \
    QR_SHAPE_BOUNDS(RLHIP_REQUIRE); \
    DIST_REQUIRE_ACT()

static int32_t qrdqn_plan_launch(const float* params, int64_t ns, int64_t h, int64_t na, int64_t n_quantiles, int32_t act, const float* obs,
                                 int64_t n, double eps, uint64_t seed, uint32_t env_id_base, uint32_t step, int32_t* actions, float* q_out,
                                 float* quantiles_out, rlhip_stream_t stream) {
    QRPlanArgs g;
    g.params = params, g.obs = obs, g.out = DistPlanOut{q_out, nullptr, quantiles_out, actions, n, eps, seed, env_id_base, step};
    g.ns = (int)ns, g.h = (int)h, g.na = (int)na, g.N = (int)n_quantiles;
    const dim3 grid((unsigned)((n + DIST_PT - 1) / DIST_PT));
    // the instantiation set: ACT in {0, 1}
    if (act == 0) hipLaunchKernelGGL((qrdqn_plan_kernel<0>), grid, dim3(DIST_PTHREADS), 0, as_stream(stream), g);
    else hipLaunchKernelGGL((qrdqn_plan_kernel<1>), grid, dim3(DIST_PTHREADS), 0, as_stream(stream), g);
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
    return dist_num_blocks(np, batch, DIST_GT) * (np + 1) * (int64_t)sizeof(float);  // partial rows | partial losses
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
    {
        const int32_t rc = dist_check_actions(a, batch, na, workspace, st, __FILE__, __LINE__);
        if (rc) return rc;
    }
    const int64_t np = mlp2_nparams(ns, h, na * n_quantiles);
    QRGradArgs g;
    g.params = params, g.tparams = target_params;
    g.s = s, g.a = a, g.r = r, g.term = term, g.sn = s_next;
    g.n_used = n_used, g.isw = weights, g.ql_out = ql_out, g.target_out = target_out, g.sel_out = sel_out;
    g.batch = batch;
    g.ns = (int)ns, g.h = (int)h, g.na = (int)na, g.N = (int)n_quantiles, g.np = (int)np;
    g.num_tiles = (int)((batch + DIST_GT - 1) / DIST_GT);
    g.double_dqn = double_dqn ? 1 : 0;
    g.gamma = gamma, g.kappa = kappa, g.fN = (float)n_quantiles, g.fb = (float)batch, g.fNB = g.fN * g.fb;
    for (int n = 0; n < DIST_GPOW; ++n) g.gpow[n] = rlhip_gamma_pow(gamma, n);
    const int nb = (int)dist_num_blocks(np, batch, DIST_GT);
    g.partials = (float*)workspace;
    g.loss_partials = g.partials + (int64_t)nb * np;
    // the instantiation set: ACT in {0, 1}
    const int32_t rc = act == 0 ? qrdqn_launch_grad<0>(g, nb, st) : qrdqn_launch_grad<1>(g, nb, st);
    if (rc) return rc;
    RLHIP_LAUNCH_CHECK();
    return dist_reduce_launch(g.partials, g.loss_partials, nb, np, grad_out, loss_out, g.fb, st);
}

}  // extern "C"
