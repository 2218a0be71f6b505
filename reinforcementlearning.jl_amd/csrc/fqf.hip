// fqf.hip -- the fully parameterised quantile function (FQF) learner: forward / plan! as one launch, and the quantile-Huber loss /
// gradient of an ImplicitQuantileNet plus the fraction-proposal gradient on a MATERIALISED batch.  include/rlhip.h (the FQF section)
// is the specification (formulas, roundings, summation orders); tests/fqf_ref.py states the mathematics in Float64.
//
// The quantile network is iqn.hip's, evaluated at levels a second small network places: l = Wf psi(s) + bf, q = softmax(l), tau the
// cumulative sum of q, tau_hat the midpoints.  Staging, the cos block, the MFMA phi block, the head and the row walk are the stages of
// iqn_device.h; what this file adds:
//   fraction stage   Wf | bf staged in the phi block's LDS buffer (N (h + 1) <= 32 (h + 1) floats, idle until the first row block);
//                    one thread per (sample, i) runs the logit chain; ONE lane per sample then runs max / expf / sum / division and the
//                    cumulative sum sequentially (N <= 32 terms: that order is the specification) and leaves tau_hat in the level row
//                    the row walk reads, the interior tau in a second level row, q, log q and d = tau[i + 1] - tau[i] beside them
//   weighted Q       Q[o] = fmaf(d[i], th_i[o], .) over i ascending instead of IQN's mean
//   gradient rows    three kinds per sample.  The target rows (s' at tau_hat) and the N - 1 FORWARD-ONLY rows (s at the interior tau:
//                    only the taken action's head value is used) are two walks of iqn_rows_all; the N rows at tau_hat then run IQN's
//                    block loop (forward, pairwise term, backward, dWphi on the MFMA with the rows as k), so a forward-only row never
//                    enters a dWphi k-step
//   fraction grad    one lane per sample: gf, the descending suffix sum dq, the entropy term, the softmax pullback -> dl in LDS; then
//                    thread = element (i, j) of Wf | bf: one fmaf / add chain over the workgroup's samples in ascending order, carried
//                    from tile to tile through the workgroup's own partial row (as dist_backward carries the mlp2 learners' chains)
// The fraction gradient is part of the SAME launch: it adds no register that lives across the tile loop (profiles/fqf.md).  The partial
// row of a workgroup is [quantile net | fraction net]; fqf_reduce_kernel adds the rows in ascending order into the two outputs.  No
// float atomics: two calls give the same bytes.
#include "iqn_device.h"

namespace rlhip {

constexpr uint32_t TAG_FQF_INIT = 15;  // (0..8: the library's streams, 9..11: the IQN level draws, 12..14: NoisyDense)
constexpr int FQ_MAXN = 32;            // fractions per sample: N + (N - 1) online rows fit the 64 level slots of a sample
constexpr int FQ_DS = FQ_MAXN + 1;     // per-sample rows of l / q / d are 33 floats apart

__host__ __device__ __forceinline__ int64_t fqf_frac_nparams(int64_t h, int64_t N) { return N * h + N; }

// Wf | bf -> LDS (the phi block's buffer)
__device__ __forceinline__ void fqf_stage_frac(const float* __restrict__ F, int N, int h, float* l_wf) {
    for (int q = threadIdx.x; q < N * h + N; q += IQ_NT) l_wf[q] = F[q];
}

// l[i][k] = bf[k], then fmaf(Wf[k, j], psi[j], .) over j ascending: one thread per (sample slot i, logit k)
__device__ __forceinline__ void fqf_logits(const float* l_wf, const float* l_psi, int N, int h, float* l_lg) {
    static_assert(IQ_T * FQ_MAXN <= IQ_NT, "one thread per (sample, logit)");
    const int q = threadIdx.x;
    if (q < IQ_T * N) {
        const int i = q / N, k = q - i * N;
        const float* ps = l_psi + i;
        const float* w = l_wf + k;
        float acc = l_wf[N * h + k];
        for (int j0 = 0; j0 < h; j0 += 8) {  // (h is a multiple of 32) eight operand pairs in flight; the chain stays j ascending
            float wv[8], pv[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) wv[u] = w[N * (j0 + u)], pv[u] = ps[(j0 + u) * IQ_T];
#pragma unroll
            for (int u = 0; u < 8; ++u) acc = fmaf(wv[u], pv[u], acc);
        }
        l_lg[i * FQ_DS + k] = acc;
    }
}

// where the fractions of a launch are stored (every pointer nullable): tau ((N + 1) x n SoA), tau_hat (N x n), the entropy (n)
struct FqfFracOut {
    float *tau, *that, *ent;
    int64_t n;
};

// one lane = one sample: logits lg[0 .. N - 1] -> q, log q (over lg), tau_hat -> that, d, the interior tau[1 .. N - 1] -> taui
// (nullable); stores column `col` of the outputs where `valid`.  Sequential on purpose: this order is the specification
__device__ __forceinline__ void fqf_fractions(int N, float* lg, float* q, float* d, float* that, float* taui, const FqfFracOut& o, int64_t col,
                                              bool valid) {
    float mx = lg[0];
    for (int k = 1; k < N; ++k) mx = lg[k] > mx ? lg[k] : mx;
    float S = 0.f;
    for (int k = 0; k < N; ++k) {
        const float z = lg[k] - mx;
        const float e = expf(z);
        lg[k] = z, q[k] = e;
        S += e;
    }
    const float lS = logf(S);
    float tau = 0.f, H = 0.f;
    for (int k = 0; k < N; ++k) {
        const float qk = q[k] / S, lq = lg[k] - lS;
        q[k] = qk, lg[k] = lq;
        H = fmaf(-qk, lq, H);
        const float nxt = k == N - 1 ? 1.0f : tau + qk;
        const float th = 0.5f * (tau + nxt);
        that[k] = th, d[k] = nxt - tau;
        if (taui && k > 0) taui[k - 1] = tau;
        if (valid && o.tau) o.tau[(int64_t)k * o.n + col] = tau;
        if (valid && o.that) o.that[(int64_t)k * o.n + col] = th;
        tau = nxt;
    }
    if (valid && o.tau) o.tau[(int64_t)N * o.n + col] = 1.0f;
    if (valid && o.ent) o.ent[col] = H;
}

// Q of one action: 0, then fmaf(d[i], th[i], .) over i ascending
__device__ __forceinline__ float fqf_wsum(const float* d, const float* th, int N) {
    float q = 0.f;
    for (int k = 0; k < N; ++k) q = fmaf(d[k], th[k], q);
    return q;
}

struct FqfPlanArgs {
    const float* params;
    const float* fparams;
    const float* obs;
    float* q_out;          // nullable
    float* quantiles_out;  // nullable
    int32_t* actions;      // nullable: forward
    FqfFracOut frac;
    int64_t n;
    int ns, h, na, nc, N;
    double eps;
    uint64_t seed;
    uint32_t env_id_base, step;
};

template <int ACT>
__global__ __launch_bounds__(IQ_NT) void fqf_plan_kernel(FqfPlanArgs g) {
    constexpr int T = IQ_T;
    extern __shared__ __attribute__((aligned(16))) float iq_dyn[];
    __shared__ float l_x[16 * T];
    __shared__ float l_c[IQ_RB * IQ_CS];
    __shared__ float l_that[T * IQ_AS];
    __shared__ float l_th[T * IQ_LS];
    __shared__ float l_lg[T * FQ_DS], l_fq[T * FQ_DS], l_d[T * FQ_DS];
    __shared__ float l_q[MAXO * T];
    const int tid = threadIdx.x;
    const int ns = g.ns, h = g.h, na = g.na, nc = g.nc, N = g.N;
    const IqnLds L = iqn_lds(iq_dyn, h, nc);
    const int64_t e0 = (int64_t)blockIdx.x * T;
    const int nv = (int)(g.n - e0 < T ? g.n - e0 : T);
    dist_load_obs<T>(g.obs, g.n, e0, nv, ns, l_x);
    iqn_stage(g.params, ns, h, na, nc, L);
    fqf_stage_frac(g.fparams, N, h, L.phi);
    __syncthreads();
    dist_layer1<ACT, T, IQ_NT>(g.params, ns, h, l_x, L.psi);
    __syncthreads();
    fqf_logits(L.phi, L.psi, N, h, l_lg);
    __syncthreads();
    if (tid < T)
        fqf_fractions(N, l_lg + tid * FQ_DS, l_fq + tid * FQ_DS, l_d + tid * FQ_DS, l_that + tid * IQ_AS, nullptr, g.frac, e0 + tid, tid < nv);
    __syncthreads();  // (the row walk rewrites the phi buffer: the logits are done with Wf)
    iqn_rows_all(L, l_that, N, nv * N, h, na, nc, l_c, l_th);
    if (g.quantiles_out) {
        for (int q = tid; q < na * N * T; q += IQ_NT) {
            const int i = q % T, m = q / T;
            if (i < nv) g.quantiles_out[(int64_t)m * g.n + e0 + i] = l_th[i * IQ_LS + m];
        }
    }
    if (tid < na * T) {
        const int i = tid % T, o = tid / T;
        l_q[o * T + i] = i < nv ? fqf_wsum(l_d + i * FQ_DS, l_th + i * IQ_LS + o * N, N) : 0.f;
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

struct FqfGradArgs {
    const float* params;
    const float* tparams;
    const float* fparams;
    const float* s;
    const int32_t* a;
    const float* r;
    const uint8_t* term;
    const float* sn;
    const int32_t* n_used;  // nullable
    const float* isw;       // nullable
    float* partials;        // rows of np + nf floats
    float* loss_partials;
    float* ql_out;          // nullable, as are the ones below
    float* target_out;
    int32_t* sel_out;
    FqfFracOut frac;
    int64_t batch;
    int ns, h, na, nc, N, np, nf, num_tiles, double_dqn;
    float gamma, kappa, ent_coef, fN, fNB, fB;  // fNB = (float)N * (float)batch, one Float32 product
    float gpow[DIST_GPOW];
};

// dWphi of the block: D[j][e] += dphi[row][j] * c[row][e] over the block's rows ascending (A[m = j][k = row], B[k = row][n = e])
#define FQ_DWPHI(ACC, JB, EB)                                                                                             \
    if ((JB) * 32 < h && (EB) * 32 < nc) {                                                                                \
        _Pragma("unroll") for (int st = 0; st < IQ_RB / 2; ++st) {                                                      \
            const int row = 2 * st + kb;                                                                                  \
            ACC = __builtin_amdgcn_mfma_f32_32x32x2f32(L.phi[row * (h + 1) + (JB) * 32 + c], l_c[row * IQ_CS + (EB) * 32 + c], \
                                                       ACC, 0, 0, 0);                                                     \
        }                                                                                                                 \
    }
#define FQ_DWPHI_STORE(ACC, JB, EB)                                                                                       \
    if ((JB) * 32 < h && (EB) * 32 + c < nc) {                                                                            \
        _Pragma("unroll") for (int q = 0; q < 16; ++q)                                                                    \
            row_out[off_wp + (JB) * 32 + (q & 3) + 8 * (q >> 2) + 4 * kb + h * ((EB) * 32 + c)] = ACC[q];                 \
    }

template <int ACT>
__global__ __launch_bounds__(IQ_NT) void fqf_grad_kernel(FqfGradArgs g) {
    constexpr int T = IQ_T, NT = IQ_NT, AS = IQ_AS, LS = IQ_LS, DS = FQ_DS;
    static_assert(16 * T <= NT && 2 * MAXO * T <= NT && IQ_RB * MAXO <= NT, "thread maps of the tile");
    extern __shared__ __attribute__((aligned(16))) float iq_dyn[];
    __shared__ float l_x[16 * T], l_xn[16 * T];        // [16][T]
    __shared__ float l_c[IQ_RB * IQ_CS];               // cosine features of the block
    __shared__ float l_that[T * AS], l_taui[T * AS];   // tau_hat[0 .. N - 1], the interior tau[1 .. N - 1]
    __shared__ float l_tht[T * LS], l_tho[T * LS];     // target quantiles of s'; online ones of s' (Double DQN), then of s at the interior tau
    __shared__ float l_T[T * AS], l_rho[T * AS], l_tha[T * AS];  // T_j, rho_n, th(s, tau_hat_n)[a]
    __shared__ float l_lg[T * DS], l_fq[T * DS], l_d[T * DS];    // logits -> log q -> dl;  q;  d -> dq
    __shared__ float l_grow[IQ_RB];                    // g of the block's rows
    __shared__ float l_qt[MAXO * T], l_qo[MAXO * T];
    __shared__ float l_r[T], l_cc[T], l_w[T], l_loss[T], l_gp[DIST_GPOW];
    __shared__ int l_ai[T], l_as[T];
    const int ns = g.ns, h = g.h, na = g.na, nc = g.nc, N = g.N;
    const IqnLds L = iqn_lds(iq_dyn, h, nc);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, c = lane & 31, kb = lane >> 5;
    const float kappa = g.kappa;
    const int ne1 = h * ns + h;
    float* row_out = g.partials + (int64_t)blockIdx.x * (g.np + g.nf);
    float* frow = row_out + g.np;
    // the workgroup's chains of the quantile network, in registers for the whole launch
    iq_f32x16 aw00, aw01, aw10, aw11;  // dWphi: unit blocks wave, wave + 4 x feature blocks 0, 1
#pragma unroll
    for (int q = 0; q < 16; ++q) aw00[q] = 0.f, aw01[q] = 0.f, aw10[q] = 0.f, aw11[q] = 0.f;
    float a_w1[IQ_W1U], a_w2[MAXO] = {0.f, 0.f, 0.f, 0.f}, a_b2 = 0.f, a_bphi = 0.f, s_loss = 0.f;
#pragma unroll
    for (int u = 0; u < IQ_W1U; ++u) a_w1[u] = 0.f;
    dist_load_gpow<FqfGradArgs>(l_gp);

    for (int tile = blockIdx.x; tile < g.num_tiles; tile += gridDim.x) {
        const int64_t b0 = (int64_t)tile * T;
        const int nv = (int)(g.batch - b0 < T ? g.batch - b0 : T);
        dist_load_states<T>(g.s, g.sn, g.batch, b0, nv, ns, l_x, l_xn);
        for (int q = tid; q < T * (h + 1); q += NT) L.dpsi[q] = 0.f;
        fqf_stage_frac(g.fparams, N, h, L.phi);
        __syncthreads();  // (also: l_gp is written)
        dist_tile_scalars<T>(g, b0, nv, l_gp, l_r, l_cc, l_w, l_ai);
        // ---- the levels: the online fraction net on psi(s)
        dist_layer1<ACT, T, NT>(g.params, ns, h, l_x, L.psi);
        __syncthreads();
        fqf_logits(L.phi, L.psi, N, h, l_lg);
        __syncthreads();
        if (tid < T)
            fqf_fractions(N, l_lg + tid * DS, l_fq + tid * DS, l_d + tid * DS, l_that + tid * AS, l_taui + tid * AS, g.frac, b0 + tid,
                          tid < nv);
        // ---- target net on s' at tau_hat [, online net on s' at the same levels]
        iqn_stage(g.tparams, ns, h, na, nc, L);
        dist_layer1<ACT, T, NT>(g.tparams, ns, h, l_xn, L.psi);
        __syncthreads();  // tau_hat is written; the row walk rewrites the phi buffer
        iqn_rows_all(L, l_that, N, nv * N, h, na, nc, l_c, l_tht);
        if (g.double_dqn) {  // (uniform)
            iqn_stage(g.params, ns, h, na, nc, L);
            dist_layer1<ACT, T, NT>(g.params, ns, h, l_xn, L.psi);
            iqn_rows_all(L, l_that, N, nv * N, h, na, nc, l_c, l_tho);
        }
        if (tid < na * T) {
            const int i = tid % T, o = tid / T;
            l_qt[o * T + i] = i < nv ? fqf_wsum(l_d + i * DS, l_tht + i * LS + o * N, N) : 0.f;
        } else if (g.double_dqn && tid >= MAXO * T && tid < MAXO * T + na * T) {
            const int i = tid % T, o = (tid - MAXO * T) / T;
            l_qo[o * T + i] = i < nv ? fqf_wsum(l_d + i * DS, l_tho + i * LS + o * N, N) : 0.f;
        }
        __syncthreads();
        dist_select_action<T>(g.double_dqn ? l_qo : l_qt, na, l_as, g.sel_out, b0, nv);
        __syncthreads();
        for (int q = tid; q < N * T; q += NT) {  // T_j = fmaf(c, th_t(s', tau_hat_j)[a*], r)
            const int i = q % T, j = q / T;
            float t = 0.f;
            if (i < nv) {
                t = fmaf(l_cc[i], l_tht[i * LS + l_as[i] * N + j], l_r[i]);
                if (g.target_out) g.target_out[(int64_t)j * g.batch + b0 + i] = t;
            }
            l_T[i * AS + j] = t;
        }
        // ---- online net on s: the forward-only rows at the interior tau first, every head row -> l_tho[i][k + (N - 1) o]
        if (!g.double_dqn) iqn_stage(g.params, ns, h, na, nc, L);
        dist_layer1<ACT, T, NT>(g.params, ns, h, l_x, L.psi);
        iqn_rows_all(L, l_taui, N - 1, nv * (N - 1), h, na, nc, l_c, l_tho);
        // ---- then the rows at tau_hat, block by block: forward, pairwise term, backward
        const int nrows = nv * N;
        for (int row0 = 0; row0 < nrows; row0 += IQ_RB) {
            iqn_cos_block(l_that, N, row0, nrows, nc, l_c);
            __syncthreads();
            iqn_phi_block(L, l_c, h, nc);
            __syncthreads();
            if (tid < IQ_RB) {  // thread = row: theta_n of the action's head row, then rho_n and d_n over j ascending
                const int row = row0 + tid;
                float gk = 0.f;
                if (row < nrows) {
                    const int i = row / N, n = row - i * N;
                    const int a = l_ai[i];
                    const float thn = iqn_head(L, h, tid, i, a < 0 ? 0 : a);
                    const float tau = l_that[i * AS + n];
                    const float* tj = l_T + i * AS;
                    float rho = 0.f, d = 0.f;
                    for (int j = 0; j < N; ++j) {
                        const float u = tj[j] - thn;
                        const float au = fabsf(u);
                        const float hub = (au <= kappa ? 0.5f * u * u : kappa * (au - 0.5f * kappa)) / kappa;
                        const float dhub = fminf(fmaxf(u, -kappa), kappa) / kappa;
                        const float w = u < 0.f ? 1.0f - tau : tau;
                        rho = fmaf(w, hub, rho);
                        d = fmaf(w, dhub, d);
                    }
                    gk = -d / g.fNB;
                    if (g.isw) gk *= l_w[i];
                    l_rho[i * AS + n] = a < 0 ? 0.f : rho;
                    l_tha[i * AS + n] = thn;
                    gk = a < 0 ? 0.f : gk;
                }
                l_grow[tid] = gk;
            }
            __syncthreads();
            if (tid < h) {  // thread = unit j: the block's rows in ascending order
                const int j = tid;
                int i = row0 / N, n = row0 - i * N, ci = i;
                float dps = L.dpsi[ci * (h + 1) + j];
                for (int r = 0; r < IQ_RB; ++r) {
                    const int ic = i < T ? i : T - 1;  // (rows beyond nrows carry g = 0)
                    const float gk = l_grow[r];
                    const int a = l_ai[ic];
                    const float ph = L.phi[r * (h + 1) + j], ps = L.psi[j * T + ic];
                    const float m = ps * ph;
#pragma unroll
                    for (int o = 0; o < MAXO; ++o) a_w2[o] = (a == o) ? fmaf(gk, m, a_w2[o]) : a_w2[o];
                    a_b2 = (a == j) ? a_b2 + gk : a_b2;  // (threads 0 .. na - 1: db2[j])
                    const float dm = gk * L.w2[(a < 0 ? 0 : a) * h + j];
                    if (ic != ci) {
                        L.dpsi[ci * (h + 1) + j] = dps;
                        ci = ic;
                        dps = L.dpsi[ci * (h + 1) + j];
                    }
                    dps = fmaf(dm, ph, dps);
                    const float dph = ph > 0.f ? dm * ps : 0.f;
                    a_bphi += dph;
                    L.phi[r * (h + 1) + j] = dph;
                    if (++n == N) n = 0, ++i;
                }
                L.dpsi[ci * (h + 1) + j] = dps;
            }
            __syncthreads();
            FQ_DWPHI(aw00, wave, 0)
            FQ_DWPHI(aw01, wave, 1)
            FQ_DWPHI(aw10, wave + 4, 0)
            FQ_DWPHI(aw11, wave + 4, 1)
            __syncthreads();  // the next block rewrites c and phi
        }
        if (tid < T) {  // sample `tid`: L_i, then the pullback of the fraction loss -> dl (over log q)
            const int a = l_ai[tid];
            float Li = 0.f;
            if (a >= 0) {
                float sr = 0.f;
                for (int n = 0; n < N; ++n) sr += l_rho[tid * AS + n];
                Li = sr / g.fN;
                if (g.ql_out) g.ql_out[b0 + tid] = Li;
                if (g.isw) Li *= l_w[tid];
            } else if (tid < nv && g.ql_out) {
                g.ql_out[b0 + tid] = 0.f;
            }
            l_loss[tid] = Li;
            const float* ti = l_tho + tid * LS + (a < 0 ? 0 : a) * (N - 1);  // th(s, tau[k + 1])[a]
            const float* ta = l_tha + tid * AS;
            const float* fq = l_fq + tid * DS;
            float* lq = l_lg + tid * DS;
            float* dq = l_d + tid * DS;
            float sfx = 0.f;
            dq[N - 1] = 0.f;
            for (int k = N - 2; k >= 0; --k) {  // dq[k] = sum of gf[k + 1 .. N - 1], added from the top down
                sfx += (2.0f * ti[k] - ta[k + 1]) - ta[k];
                dq[k] = sfx;
            }
            float m = 0.f;
            for (int k = 0; k < N; ++k) {  // minus ent_coef times dH/dq = -(log q + 1)
                const float v = fmaf(g.ent_coef, lq[k] + 1.0f, dq[k]);
                dq[k] = v;
                m = fmaf(fq[k], v, m);
            }
            const float sc = (g.isw ? l_w[tid] : 1.0f) / g.fB;
            for (int k = 0; k < N; ++k) lq[k] = a >= 0 ? (fq[k] * (dq[k] - m)) * sc : 0.f;
        }
        for (int q = tid; q < h * T; q += NT) {  // dz = dpsi * act', in place
            const int i = q % T, j = q / T;
            const float hv = L.psi[q];
            L.dpsi[i * (h + 1) + j] *= (ACT == 0 ? (hv > 0.0f ? 1.0f : 0.0f) : (1.0f - hv * hv));
        }
        __syncthreads();
        if (tid == 0)
            for (int i = 0; i < nv; ++i) s_loss += l_loss[i];
        // ---- dW1 and db1: one chain per element over the tile's samples
#pragma unroll
        for (int u = 0; u < IQ_W1U; ++u) {
            const int e = tid + u * NT;
            if (e < ne1) {
                const bool bias = e >= h * ns;
                const int j = bias ? e - h * ns : e % h, k = bias ? 0 : e / h;
                float acc = a_w1[u];
                for (int i = 0; i < nv; ++i) {
                    const float dz = L.dpsi[i * (h + 1) + j];
                    acc = bias ? acc + dz : fmaf(dz, l_x[k * T + i], acc);
                }
                a_w1[u] = acc;
            }
        }
        // ---- dWf and dbf: thread = element, its chain carried through the workgroup's own partial row
        for (int e = tid; e < g.nf; e += NT) {
            const bool bias = e >= N * h;
            const int k = bias ? e - N * h : e % N, j = bias ? 0 : e / N;
            float acc = tile == (int)blockIdx.x ? 0.f : frow[e];
            for (int i = 0; i < nv; ++i) {
                const float dl = l_lg[i * DS + k];
                acc = bias ? acc + dl : fmaf(dl, L.psi[j * T + i], acc);
            }
            frow[e] = acc;
        }
        __syncthreads();  // the next tile rewrites every buffer
    }
    // ---- the workgroup's partial row: every element is written
    const int off_wp = ne1, off_bp = off_wp + h * nc, off_w2 = off_bp + h, off_b2 = off_w2 + na * h;
#pragma unroll
    for (int u = 0; u < IQ_W1U; ++u)
        if (tid + u * NT < ne1) row_out[tid + u * NT] = a_w1[u];
    FQ_DWPHI_STORE(aw00, wave, 0)
    FQ_DWPHI_STORE(aw01, wave, 1)
    FQ_DWPHI_STORE(aw10, wave + 4, 0)
    FQ_DWPHI_STORE(aw11, wave + 4, 1)
    if (tid < h) {
        row_out[off_bp + tid] = a_bphi;
#pragma unroll
        for (int o = 0; o < MAXO; ++o)
            if (o < na) row_out[off_w2 + o + na * tid] = a_w2[o];
        if (tid < na) row_out[off_b2 + tid] = a_b2;
    }
    if (tid == 0) g.loss_partials[blockIdx.x] = s_loss;
}

// element p of [quantile net | fraction net] and the loss: the partial rows / losses of workgroups 0, 1, .. in ascending order, from +0
__global__ __launch_bounds__(256) void fqf_reduce_kernel(const float* __restrict__ partials, const float* __restrict__ loss_partials, int nb,
                                                         int np, int nf, float* __restrict__ grad, float* __restrict__ fgrad,
                                                         float* __restrict__ loss, float fb) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p < np + nf) {
        float acc = 0.f;
#pragma unroll 8
        for (int b = 0; b < nb; ++b) acc += partials[(int64_t)b * (np + nf) + p];
        if (p < np) grad[p] = acc;
        else fgrad[p - np] = acc;
    }
    if (p == 0) {
        float a = 0.f;
        for (int b = 0; b < nb; ++b) a += loss_partials[b];
        loss[0] = a / fb;
    }
}

// Wf = 0.01 x Glorot-uniform for Dense(h, N), bf = 0
__global__ __launch_bounds__(256) void fqf_frac_init_kernel(float* __restrict__ p, int h, int N, uint64_t seed, uint32_t net_id) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= N * h + N) return;
    float val = 0.0f;
    if (q < N * h) {
        const u32x4 w = philox4x32_10(seed, (uint32_t)q, 0, net_id, TAG_FQF_INIT);
        val = ((2.0f * u01_f32(w.x) - 1.0f) * sqrtf(6.0f / (float)(h + N))) * 0.01f;
    }
    p[q] = val;
}

static bool fqf_fractions_ok(int64_t n) { return n >= 2 && n <= FQ_MAXN; }

template <int ACT>
static int32_t fqf_launch_plan(const FqfPlanArgs& g, hipStream_t s) {
    static unsigned long long done = 0;  // the opt-in is for the largest net of the envelope
    const int32_t rc = allow_big_lds(fqf_plan_kernel<ACT>, iqn_lds_bytes(IQ_HMAX, IQ_MAXC, false), &done);
    if (rc) return rc;
    hipLaunchKernelGGL((fqf_plan_kernel<ACT>), dim3((unsigned)((g.n + IQ_T - 1) / IQ_T)), dim3(IQ_NT), iqn_lds_bytes(g.h, g.nc, false), s, g);
    return RLHIP_OK;
}

template <int ACT>
static int32_t fqf_launch_grad(const FqfGradArgs& g, int nb, hipStream_t s) {
    static unsigned long long done = 0;
    const int32_t rc = allow_big_lds(fqf_grad_kernel<ACT>, iqn_lds_bytes(IQ_HMAX, IQ_MAXC, true), &done);
    if (rc) return rc;
    hipLaunchKernelGGL((fqf_grad_kernel<ACT>), dim3(nb), dim3(IQ_NT), iqn_lds_bytes(g.h, g.nc, true), s, g);
    return RLHIP_OK;
}

}  // namespace rlhip

using namespace rlhip;

#define FQ_REQUIRE_NET() \
    IQ_REQUIRE_NET();    \
    RLHIP_REQUIRE(fqf_fractions_ok(n_fractions), "the number of fractions must be 2..32")

static int32_t fqf_plan_launch(const float* params, const float* frac_params, int64_t ns, int64_t h, int64_t na, int64_t n_cos, int64_t N,
                               int32_t act, const float* obs, int64_t n, double eps, uint64_t seed, uint32_t env_id_base, uint32_t step,
                               int32_t* actions, float* q_out, float* quantiles_out, float* tau_out, float* tau_hat_out,
                               rlhip_stream_t stream) {
    FqfPlanArgs g;
    g.params = params, g.fparams = frac_params, g.obs = obs, g.q_out = q_out, g.quantiles_out = quantiles_out, g.actions = actions;
    g.frac.tau = tau_out, g.frac.that = tau_hat_out, g.frac.ent = nullptr, g.frac.n = n;
    g.n = n, g.ns = (int)ns, g.h = (int)h, g.na = (int)na, g.nc = (int)n_cos, g.N = (int)N;
    g.eps = eps, g.seed = seed, g.env_id_base = env_id_base, g.step = step;
    // the instantiation set: ACT in {0, 1}
    const int32_t rc = act == 0 ? fqf_launch_plan<0>(g, as_stream(stream)) : fqf_launch_plan<1>(g, as_stream(stream));
    if (rc) return rc;
    RLHIP_LAUNCH_CHECK();
    return RLHIP_OK;
}

extern "C" {

int64_t rlhip_fqf_frac_nparams(int64_t h, int64_t n_fractions) {
    if (h < 1 || n_fractions < 1) return -1;
    return fqf_frac_nparams(h, n_fractions);
}

int32_t rlhip_fqf_frac_init_f32(float* frac_params, int64_t h, int64_t n_fractions, uint64_t seed, uint32_t net_id, rlhip_stream_t stream) {
    RLHIP_REQUIRE(frac_params != nullptr && h >= 1 && n_fractions >= 1, "bad arguments");
    const int64_t nf = fqf_frac_nparams(h, n_fractions);
    RLHIP_REQUIRE(nf <= 0x7fffffffLL, "the network is too large");
    hipLaunchKernelGGL(fqf_frac_init_kernel, dim3((int)((nf + 255) / 256)), dim3(256), 0, as_stream(stream), frac_params, (int)h,
                       (int)n_fractions, seed, net_id);
    RLHIP_LAUNCH_CHECK();
    return RLHIP_OK;
}

int32_t rlhip_fqf_forward_f32(const float* params, const float* frac_params, int64_t ns, int64_t h, int64_t na, int64_t n_cos,
                              int64_t n_fractions, int32_t act, const float* obs, int64_t n, float* q_out, float* quantiles_out,
                              float* tau_out, float* tau_hat_out, rlhip_stream_t stream) {
    FQ_REQUIRE_NET();
    RLHIP_REQUIRE(n >= 0 && n <= 0x7fffffffLL, "env count must be 0 .. 2^31 - 1");
    RLHIP_REQUIRE(params && frac_params && obs && q_out, "NULL argument");
    if (n == 0) return RLHIP_OK;
    return fqf_plan_launch(params, frac_params, ns, h, na, n_cos, n_fractions, act, obs, n, 0.0, 0, 0, 0, nullptr, q_out, quantiles_out, tau_out,
                           tau_hat_out, stream);
}

int32_t rlhip_fqf_plan_f32(const float* params, const float* frac_params, int64_t ns, int64_t h, int64_t na, int64_t n_cos,
                           int64_t n_fractions, int32_t act, const float* obs, int64_t n, double eps, uint64_t seed, uint32_t env_id_base,
                           uint32_t step, int32_t* actions, float* q_out, rlhip_stream_t stream) {
    FQ_REQUIRE_NET();
    RLHIP_REQUIRE(n >= 0 && n <= 0x7fffffffLL, "env count must be 0 .. 2^31 - 1");
    RLHIP_REQUIRE(params && frac_params && obs && actions, "NULL argument");
    if (n == 0) return RLHIP_OK;
    return fqf_plan_launch(params, frac_params, ns, h, na, n_cos, n_fractions, act, obs, n, eps, seed, env_id_base, step, actions, q_out, nullptr,
                           nullptr, nullptr, stream);
}

int64_t rlhip_fqf_workspace_bytes(int64_t ns, int64_t h, int64_t na, int64_t n_cos, int64_t n_fractions, int64_t batch) {
    if (!iqn_net_ok(ns, h, na, n_cos) || !fqf_fractions_ok(n_fractions) || batch < 1) return -1;
    const int64_t nrow = iqn_nparams(ns, h, na, n_cos) + fqf_frac_nparams(h, n_fractions);
    return dist_num_blocks(nrow, batch, IQ_T) * (nrow + 1) * (int64_t)sizeof(float);  // partial rows | partial losses
}

int32_t rlhip_fqf_grad_batch_f32(int64_t ns, int64_t h, int64_t na, int64_t n_cos, int64_t n_fractions, int32_t act, float kappa,
                                 float ent_coef, const float* params, const float* target_params, const float* frac_params, const float* s,
                                 const int32_t* a, const float* r, const uint8_t* term, const float* s_next, int64_t batch, float gamma,
                                 const int32_t* n_used, const float* weights, int32_t double_dqn, void* workspace, float* grad_out,
                                 float* frac_grad_out, float* loss_out, float* ql_out, float* target_out, int32_t* sel_out, float* tau_out,
                                 float* tau_hat_out, float* ent_out, rlhip_stream_t stream) {
    FQ_REQUIRE_NET();
    RLHIP_REQUIRE(std::isfinite(kappa) && kappa > 0.f, "kappa must be finite and > 0");
    RLHIP_REQUIRE(std::isfinite(ent_coef) && ent_coef >= 0.f, "ent_coef must be finite and >= 0");
    RLHIP_REQUIRE(batch >= 1 && batch <= 0x7fffffffLL, "batch must be 1 .. 2^31 - 1");
    RLHIP_REQUIRE(params && target_params && frac_params && s && a && r && term && s_next && workspace && grad_out && frac_grad_out && loss_out,
                  "NULL argument");
    hipStream_t st = as_stream(stream);
    const int64_t np = iqn_nparams(ns, h, na, n_cos), nf = fqf_frac_nparams(h, n_fractions);
    FqfGradArgs g;
    g.params = params, g.tparams = target_params, g.fparams = frac_params;
    g.s = s, g.a = a, g.r = r, g.term = term, g.sn = s_next;
    g.n_used = n_used, g.isw = weights, g.ql_out = ql_out, g.target_out = target_out, g.sel_out = sel_out;
    g.frac.tau = tau_out, g.frac.that = tau_hat_out, g.frac.ent = ent_out, g.frac.n = batch;
    g.batch = batch;
    g.ns = (int)ns, g.h = (int)h, g.na = (int)na, g.nc = (int)n_cos, g.N = (int)n_fractions, g.np = (int)np, g.nf = (int)nf;
    g.num_tiles = (int)((batch + IQ_T - 1) / IQ_T);
    g.double_dqn = double_dqn ? 1 : 0;
    g.gamma = gamma, g.kappa = kappa, g.ent_coef = ent_coef;
    g.fN = (float)n_fractions, g.fB = (float)batch, g.fNB = g.fN * g.fB;
    for (int n = 0; n < DIST_GPOW; ++n) g.gpow[n] = rlhip_gamma_pow(gamma, n);
    const int nb = (int)dist_num_blocks(np + nf, batch, IQ_T);
    g.partials = (float*)workspace;
    g.loss_partials = g.partials + (int64_t)nb * (np + nf);
    // the instantiation set: ACT in {0, 1}
    const int32_t rc = act == 0 ? fqf_launch_grad<0>(g, nb, st) : fqf_launch_grad<1>(g, nb, st);
    if (rc) return rc;
    RLHIP_LAUNCH_CHECK();
    hipLaunchKernelGGL(fqf_reduce_kernel, dim3((int)((np + nf + 255) / 256)), dim3(256), 0, st, g.partials, g.loss_partials, nb, (int)np, (int)nf,
                       grad_out, frac_grad_out, loss_out, g.fB);
    RLHIP_LAUNCH_CHECK();
    return RLHIP_OK;
}

}  // extern "C"
