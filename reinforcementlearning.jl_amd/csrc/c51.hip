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
//   dist_reduce_kernel     (dist.hip) the partial rows, one per workgroup, ascending
// Everything but the projection and the cross-entropy line is a stage of dist_device.h, shared with qrdqn.hip (and iqn.hip, noisy.hip).
// No float atomics anywhere: two calls on the same inputs give the same bytes.
#include "dist_host.h"

namespace rlhip {

struct C51PlanArgs {
    const float* params;
    const float* obs;
    DistPlanOut out;  // rows_raw: logits, rows_out: probabilities
    int ns, h, na, n_atoms;
    float v_min, delta;
};

template <int ACT>
__global__ __launch_bounds__(DIST_PTHREADS) void c51_plan_kernel(C51PlanArgs g) {
    constexpr int T = DIST_PT, LS = DIST_MAXM + 1;
    __shared__ float l_x[16 * T];
    __shared__ __attribute__((aligned(16))) float l_h[DIST_HMAX * T];
    __shared__ float l_l[T * LS];
    __shared__ float l_q[MAXO * T];
    const int tid = threadIdx.x;
    const int ns = g.ns, h = g.h, na = g.na, n_atoms = g.n_atoms, M = na * n_atoms;
    const int64_t e0 = (int64_t)blockIdx.x * T;
    const int nv = (int)(g.out.n - e0 < T ? g.out.n - e0 : T);
    dist_load_obs<T>(g.obs, g.out.n, e0, nv, ns, l_x);
    __syncthreads();
    dist_layer1<ACT, T, DIST_PTHREADS>(g.params, ns, h, l_x, l_h);
    __syncthreads();
    if (tid < M) dist_rows<T, T, 4>(g.params, ns, h, M, tid, 0, l_h, l_l, LS);
    __syncthreads();
    // c51_probs_q: the one definition of logits -> Q for forward, plan and the gradient's target side
    dist_plan_tail<T, DIST_PTHREADS, LS, true>(g.out, e0, nv, na, n_atoms, l_l, l_q,
                                         [&](float* l) { return c51_probs_q<1>(l, n_atoms, g.v_min, g.delta); });
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
    float gpow[DIST_GPOW];
};

template <int ACT>
// (the second bound: two waves per SIMD, i.e. at most 256 registers -- the chunks of weights in flight live in them -- and two
// workgroups per CU; a launch has at most 256 workgroups)
__global__ __launch_bounds__(DIST_GTHREADS, 2) void c51_grad_kernel(C51GradArgs g) {
    constexpr int T = DIST_GT, NT = DIST_GTHREADS, AS = DIST_AS;
    static_assert(16 * T <= NT && DIST_QO + MAXO * T <= NT && DIST_QO % T == 0 && (16 * T) % 4 == 0, "thread maps of the tile");
    // LDS: static, sized for h = 256 and 256 rows (33 KB), so that every address is an immediate
    constexpr int LS = DIST_MAXM + 1;   // logit rows are 257 floats apart (odd); the dz rows [T][h + 1 <= 257] reuse the first buffer
    constexpr int HS1 = DIST_HMAX + 1;
    __shared__ __attribute__((aligned(16))) float l_h[DIST_HMAX * T];  // [h][T]
    __shared__ float l_x[16 * T], l_xn[16 * T];                       // [16][T]
    __shared__ float l_lt[T * LS];                                    // target logits / probabilities of s'; later dz
    __shared__ float l_lo[T * LS];                                    // online logits of s', then of s
    __shared__ float l_qt[MAXO * T], l_qo[MAXO * T];
    __shared__ float l_tz[T * AS], l_m[T * AS];
    __shared__ float l_g[T * AS];                                     // e_k of the cross-entropy line, then g_k
    __shared__ float l_r[T], l_c[T], l_w[T], l_loss[T], l_gp[DIST_GPOW];
    __shared__ int l_ai[T];                                           // the sample's action, -1 where it selects nothing
    __shared__ int l_as[T];                                           // a*
    const int ns = g.ns, h = g.h, na = g.na, n_atoms = g.n_atoms, M = na * n_atoms;

    const int tid = threadIdx.x;
    const int lm = tid % DIST_MAXM, li0 = (tid / DIST_MAXM) * DIST_GSPT;  // the logits pass: row lm, samples li0 .. li0 + 7
    const float* W2 = g.params + h * ns + h;
    float s_loss = 0.f;  // thread 0: the workgroup's loss chain
    float* row = g.partials + (int64_t)blockIdx.x * g.np;
    dist_load_gpow<C51GradArgs>(l_gp);

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
            l_qt[o * T + i] = c51_probs_q<DIST_CH>(l_lt + i * LS + o * n_atoms, n_atoms, g.v_min, g.delta);
        } else if (g.double_dqn && tid >= DIST_QO && tid < DIST_QO + na * T) {
            const int i = tid % T, o = (tid - DIST_QO) / T;
            l_qo[o * T + i] = c51_probs_q<DIST_CH>(l_lo + i * LS + o * n_atoms, n_atoms, g.v_min, g.delta);
        }
        __syncthreads();
        dist_select_action<T>(g.double_dqn ? l_qo : l_qt, na, l_as, g.sel_out, b0, nv);
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
            for (int j0 = 0; j0 < n_atoms; j0 += DIST_CH) {  // the divisions of a chunk are independent; the chain stays j ascending
                float wgt[DIST_CH], pj[DIST_CH];
#pragma unroll
                for (int u = 0; u < DIST_CH; ++u) {
                    const int j = j0 + u < n_atoms ? j0 + u : n_atoms - 1;
                    wgt[u] = tz[j], pj[u] = pt[j];
                }
#pragma unroll
                for (int u = 0; u < DIST_CH; ++u) wgt[u] = fminf(fmaxf(1.0f - fabsf(wgt[u] - zk) / g.delta, 0.f), 1.0f);
#pragma unroll
                for (int u = 0; u < DIST_CH; ++u) {
                    const float t = fmaf(wgt[u], pj[u], m);
                    m = (j0 + u < n_atoms) ? t : m;
                }
            }
            l_m[i * AS + k] = m;
            if (g.proj_out && i < nv) g.proj_out[(int64_t)k * g.batch + b0 + i] = m;
        }
        // ---- online net on s; h(s) stays in l_h for the backward pass
        dist_layer1<ACT, T, NT>(g.params, ns, h, l_x, l_h);
        __syncthreads();
        if (lm < M) dist_rows<T, DIST_GSPT, DIST_WCH>(g.params, ns, h, M, lm, li0, l_h, l_lo, LS);
        __syncthreads();
        if (tid < T) {  // the cross-entropy line of sample `tid`
            const int a = l_ai[tid];
            float L = 0.f;
            if (a >= 0) {
                const float* l = l_lo + tid * LS + a * n_atoms;
                float* e = l_g + tid * AS;
                const float* m = l_m + tid * AS;
                float mx;
                const float S = c51_exp_sum<DIST_CH>(l, e, n_atoms, mx);
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
        // ---- dW2 | db2, dh -> dz (into l_lt), dW1 | db1
        dist_backward<ACT, T, NT, AS, HS1, DIST_WCH>(W2, row, first, nv, ns, h, M, n_atoms, l_ai, l_g, l_h, l_x, l_lt);
        __syncthreads();  // the next tile rewrites every buffer
    }
    if (tid == 0) g.loss_partials[blockIdx.x] = s_loss;
}

template <int ACT>
static int32_t c51_launch_grad(const C51GradArgs& g, int nb, hipStream_t s) {
    hipLaunchKernelGGL((c51_grad_kernel<ACT>), dim3(nb), dim3(DIST_GTHREADS), 0, s, g);
    return RLHIP_OK;
}

#define C51_SHAPE_BOUNDS(B) \
    DIST_MLP2_BOUNDS(B);    \
    B(n_atoms >= 2 && n_atoms <= DIST_MAXK, "n_atoms must be 2..64")

static bool c51_shape_ok(int64_t ns, int64_t h, int64_t na, int64_t n_atoms) {
    C51_SHAPE_BOUNDS(DIST_BOUND_HOLDS);
    return true;
}

static bool c51_support_ok(float v_min, float v_max) { return std::isfinite(v_min) && std::isfinite(v_max) && v_min < v_max; }

}  // namespace rlhip

using namespace rlhip;

#define C51_REQUIRE_SHAPE()             \
    C51_SHAPE_BOUNDS(RLHIP_REQUIRE);    \
    DIST_REQUIRE_ACT();                 \
    RLHIP_REQUIRE(c51_support_ok(v_min, v_max), "the support needs finite v_min < v_max")

static int32_t c51_plan_launch(const float* params, int64_t ns, int64_t h, int64_t na, int64_t n_atoms, int32_t act, float v_min,
                               float v_max, const float* obs, int64_t n, double eps, uint64_t seed, uint32_t env_id_base, uint32_t step,
                               int32_t* actions, float* q_out, float* probs_out, float* logits_out, rlhip_stream_t stream) {
    C51PlanArgs g;
    g.params = params, g.obs = obs, g.out = DistPlanOut{q_out, logits_out, probs_out, actions, n, eps, seed, env_id_base, step};
    g.ns = (int)ns, g.h = (int)h, g.na = (int)na, g.n_atoms = (int)n_atoms;
    g.v_min = v_min, g.delta = (v_max - v_min) / (float)(n_atoms - 1);
    const dim3 grid((unsigned)((n + DIST_PT - 1) / DIST_PT));
    // the instantiation set: ACT in {0, 1}
    if (act == 0) hipLaunchKernelGGL((c51_plan_kernel<0>), grid, dim3(DIST_PTHREADS), 0, as_stream(stream), g);
    else hipLaunchKernelGGL((c51_plan_kernel<1>), grid, dim3(DIST_PTHREADS), 0, as_stream(stream), g);
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
    return dist_num_blocks(np, batch, DIST_GT) * (np + 1) * (int64_t)sizeof(float);  // partial rows | partial losses
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
    {
        const int32_t rc = dist_check_actions(a, batch, na, workspace, st, __FILE__, __LINE__);
        if (rc) return rc;
    }
    const int64_t np = mlp2_nparams(ns, h, na * n_atoms);
    C51GradArgs g;
    g.params = params, g.tparams = target_params;
    g.s = s, g.a = a, g.r = r, g.term = term, g.sn = s_next;
    g.n_used = n_used, g.isw = weights, g.ce_out = ce_out, g.proj_out = proj_out, g.sel_out = sel_out;
    g.batch = batch;
    g.ns = (int)ns, g.h = (int)h, g.na = (int)na, g.n_atoms = (int)n_atoms, g.np = (int)np;
    g.num_tiles = (int)((batch + DIST_GT - 1) / DIST_GT);
    g.double_dqn = double_dqn ? 1 : 0;
    g.gamma = gamma, g.v_min = v_min, g.v_max = v_max, g.delta = (v_max - v_min) / (float)(n_atoms - 1), g.fb = (float)batch;
    for (int n = 0; n < DIST_GPOW; ++n) g.gpow[n] = rlhip_gamma_pow(gamma, n);
    const int nb = (int)dist_num_blocks(np, batch, DIST_GT);
    g.partials = (float*)workspace;
    g.loss_partials = g.partials + (int64_t)nb * np;
    // the instantiation set: ACT in {0, 1}
    const int32_t rc = act == 0 ? c51_launch_grad<0>(g, nb, st) : c51_launch_grad<1>(g, nb, st);
    if (rc) return rc;
    RLHIP_LAUNCH_CHECK();
    return dist_reduce_launch(g.partials, g.loss_partials, nb, np, grad_out, loss_out, g.fb, st);
}

}  // extern "C"
