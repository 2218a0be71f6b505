// iqn.hip -- the implicit-quantile (IQN) distributional DQN learner: forward / plan! as one launch, and the quantile-Huber loss /
// gradient of an ImplicitQuantileNet(psi = Dense(ns, h, act), phi = Dense(n_cos, h, relu), header = Dense(h, na)) on a MATERIALISED
// batch (the SoA arrays rlhip_qrdqn_grad_batch_f32 takes).  include/rlhip.h is the specification (formulas, roundings, summation
// orders); tests/iqn_ref.py states the mathematics in Float64.
//
// Every sample is evaluated at N drawn levels, so the rows of the work are (sample, level) pairs and the bulk of it is the
// (rows x n_cos) x (n_cos x h) product in front of the head.  A workgroup of 256 threads walks the rows of a tile of 8 samples in
// blocks of 32:
//   staging      Wphi | bphi (a straight copy: column-major h x n_cos is the B-operand image) and W2 | b2 of the net in LDS, once per
//                net and tile; psi of the tile's samples once per sample (dist_layer1), not once per level
//   cos block    c[row][e] = cospif((e + 1) tau_row) for the block's 32 rows -> LDS, rows 65 floats apart (the A-operand image)
//   phi block    v_mfma_f32_32x32x2_f32: 32 rows x 32 hidden units per instruction, n_cos / 2 k-steps, bphi as the accumulator's
//                initial value, so that the chain is the header's ascending-e fmaf chain bit for bit (tools/micro/mfma_f32_l1.hip,
//                form 0: lane = unit, registers = rows).  Wave w owns the unit blocks w, w + 4.  relu on the accumulator registers
//   head         one thread per (row, head row): b2, then fmaf(W2[o, j], psi[j] * phi[j], .) over j ascending, operands from LDS
//   backward     thread = hidden unit j walks the block's rows in ascending order: dW2 / db2 / dbphi / dpsi chains in registers,
//                dphi written over phi; then dWphi[j, e] += dphi[row][j] c[row][e] on the same MFMA with the ROWS as the k dimension
//                (ascending), accumulators living in registers for the whole launch
//   pairwise     one thread per (sample, n): theta_n of the action's head row, then the two chains over the targets T_j in LDS
// Every gradient element is ONE chain from +0 over the workgroup's rows, kept in registers and stored once into the workgroup's
// partial row; dist_reduce_kernel (dist.hip) adds the rows in ascending order.  No float atomics: two calls give the same bytes.
// The tile loads, the gamma table, the per-tile scalars, psi's chain and a* are the stages of dist_device.h, shared with c51.hip and
// qrdqn.hip; staging, the cos / phi blocks and the head are the stages of iqn_device.h, shared with fqf.hip; the level draws and the
// register chains above are this file's own.
#include "iqn_device.h"

namespace rlhip {

constexpr uint32_t TAG_IQN_PLAN = 9, TAG_IQN_ONLINE = 10, TAG_IQN_TARGET = 11;  // Philox tags of the level draws (include/rlhip.h)

// tau = (float)(w >> 15) * 2^-17, w = word n % 4 of philox4x32_10(seed, idx, n / 4, t, tag)
__device__ __forceinline__ float iqn_tau(uint64_t seed, uint32_t idx, int n, uint32_t t, uint32_t tag) {
    const u32x4 w = philox4x32_10(seed, idx, (uint32_t)(n >> 2), t, tag);
    const int k = n & 3;
    const uint32_t x = k == 0 ? w.x : (k == 1 ? w.y : (k == 2 ? w.z : w.w));
    return (float)(x >> 15) * 0x1p-17f;
}

// Q of one action: (sum of th over the levels, ascending, from +0) / (float)(number of levels)
__device__ __forceinline__ float iqn_mean(const float* th, int NL) {
    float q = 0.f;
    for (int k = 0; k < NL; ++k) q += th[k];
    return q / (float)NL;
}

struct IqnPlanArgs {
    const float* params;
    const float* obs;
    float* q_out;          // nullable
    float* quantiles_out;  // nullable
    float* tau_out;        // nullable
    int32_t* actions;      // nullable: forward
    int64_t n;
    int ns, h, na, nc, K;
    double eps;
    uint64_t seed;
    uint32_t env_id_base, step;
};

template <int ACT>
__global__ __launch_bounds__(IQ_NT) void iqn_plan_kernel(IqnPlanArgs g) {
    constexpr int T = IQ_T;
    extern __shared__ __attribute__((aligned(16))) float iq_dyn[];
    __shared__ float l_x[16 * T];
    __shared__ float l_c[IQ_RB * IQ_CS];
    __shared__ float l_tau[T * IQ_AS];
    __shared__ float l_th[T * IQ_LS];
    __shared__ float l_q[MAXO * T];
    const int tid = threadIdx.x;
    const int ns = g.ns, h = g.h, na = g.na, nc = g.nc, K = g.K;
    const IqnLds L = iqn_lds(iq_dyn, h, nc);
    const int64_t e0 = (int64_t)blockIdx.x * T;
    const int nv = (int)(g.n - e0 < T ? g.n - e0 : T);
    dist_load_obs<T>(g.obs, g.n, e0, nv, ns, l_x);
    for (int q = tid; q < T * K; q += IQ_NT) {
        const int i = q / K, n = q - i * K;
        float tau = 0.f;
        if (i < nv) {
            tau = iqn_tau(g.seed, g.env_id_base + (uint32_t)(e0 + i), n, g.step, TAG_IQN_PLAN);
            if (g.tau_out) g.tau_out[(int64_t)n * g.n + e0 + i] = tau;
        }
        l_tau[i * IQ_AS + n] = tau;
    }
    iqn_stage(g.params, ns, h, na, nc, L);
    __syncthreads();
    dist_layer1<ACT, T, IQ_NT>(g.params, ns, h, l_x, L.psi);
    iqn_rows_all(L, l_tau, K, nv * K, h, na, nc, l_c, l_th);
    if (g.quantiles_out) {
        for (int q = tid; q < na * K * T; q += IQ_NT) {
            const int i = q % T, m = q / T;
            if (i < nv) g.quantiles_out[(int64_t)m * g.n + e0 + i] = l_th[i * IQ_LS + m];
        }
    }
    if (tid < na * T) {
        const int i = tid % T, o = tid / T;
        l_q[o * T + i] = i < nv ? iqn_mean(l_th + i * IQ_LS + o * K, K) : 0.f;
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

struct IqnGradArgs {
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
    float* ql_out;          // nullable, as are the five below
    float* target_out;
    int32_t* sel_out;
    float* tau_out;
    float* tau_target_out;
    int64_t batch;
    int ns, h, na, nc, N, Np, np, num_tiles, double_dqn;
    uint64_t seed;
    uint32_t draw_ctr;
    float gamma, kappa, fNp, fNB;  // fNB = (float)N' * (float)batch, one Float32 product
    float gpow[DIST_GPOW];
};

// dWphi of the block: D[j][e] += dphi[row][j] * c[row][e] over the block's rows ascending (A[m = j][k = row], B[k = row][n = e])
#define IQ_DWPHI(ACC, JB, EB)                                                                                             \
    if ((JB) * 32 < h && (EB) * 32 < nc) {                                                                                \
        _Pragma("unroll") for (int st = 0; st < IQ_RB / 2; ++st) {                                                      \
            const int row = 2 * st + kb;                                                                                  \
            ACC = __builtin_amdgcn_mfma_f32_32x32x2f32(L.phi[row * (h + 1) + (JB) * 32 + c], l_c[row * IQ_CS + (EB) * 32 + c], \
                                                       ACC, 0, 0, 0);                                                     \
        }                                                                                                                 \
    }
#define IQ_DWPHI_STORE(ACC, JB, EB)                                                                                       \
    if ((JB) * 32 < h && (EB) * 32 + c < nc) {                                                                            \
        _Pragma("unroll") for (int q = 0; q < 16; ++q)                                                                    \
            row_out[off_wp + (JB) * 32 + (q & 3) + 8 * (q >> 2) + 4 * kb + h * ((EB) * 32 + c)] = ACC[q];                 \
    }

template <int ACT>
__global__ __launch_bounds__(IQ_NT) void iqn_grad_kernel(IqnGradArgs g) {
    constexpr int T = IQ_T, NT = IQ_NT, AS = IQ_AS, LS = IQ_LS;
    static_assert(16 * T <= NT && 2 * MAXO * T <= NT && IQ_RB * MAXO <= NT, "thread maps of the tile");
    extern __shared__ __attribute__((aligned(16))) float iq_dyn[];
    __shared__ float l_x[16 * T], l_xn[16 * T];        // [16][T]
    __shared__ float l_c[IQ_RB * IQ_CS];               // cosine features of the block
    __shared__ float l_tau[T * AS], l_taup[T * AS];    // tau, tau'
    __shared__ float l_tht[T * LS], l_tho[T * LS];     // target / online quantiles of s' at tau'
    __shared__ float l_T[T * AS], l_rho[T * AS];       // T_j, rho_n
    __shared__ float l_grow[IQ_RB];                    // g of the block's rows
    __shared__ float l_qt[MAXO * T], l_qo[MAXO * T];
    __shared__ float l_r[T], l_cc[T], l_w[T], l_loss[T], l_gp[DIST_GPOW];
    __shared__ int l_ai[T], l_as[T];
    const int ns = g.ns, h = g.h, na = g.na, nc = g.nc, N = g.N, Np = g.Np;
    const IqnLds L = iqn_lds(iq_dyn, h, nc);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, c = lane & 31, kb = lane >> 5;
    const float kappa = g.kappa;
    const int ne1 = h * ns + h;
    // the workgroup's chains, in registers for the whole launch
    iq_f32x16 aw00, aw01, aw10, aw11;  // dWphi: unit blocks wave, wave + 4 x feature blocks 0, 1
#pragma unroll
    for (int q = 0; q < 16; ++q) aw00[q] = 0.f, aw01[q] = 0.f, aw10[q] = 0.f, aw11[q] = 0.f;
    float a_w1[IQ_W1U], a_w2[MAXO] = {0.f, 0.f, 0.f, 0.f}, a_b2 = 0.f, a_bphi = 0.f, s_loss = 0.f;
#pragma unroll
    for (int u = 0; u < IQ_W1U; ++u) a_w1[u] = 0.f;
    dist_load_gpow<IqnGradArgs>(l_gp);

    for (int tile = blockIdx.x; tile < g.num_tiles; tile += gridDim.x) {
        const int64_t b0 = (int64_t)tile * T;
        const int nv = (int)(g.batch - b0 < T ? g.batch - b0 : T);
        dist_load_states<T>(g.s, g.sn, g.batch, b0, nv, ns, l_x, l_xn);
        for (int q = tid; q < T * N; q += NT) {  // tau: (batch position, draw_ctr), the online tag
            const int i = q / N, n = q - i * N;
            float tau = 0.f;
            if (i < nv) {
                tau = iqn_tau(g.seed, (uint32_t)(b0 + i), n, g.draw_ctr, TAG_IQN_ONLINE);
                if (g.tau_out) g.tau_out[(int64_t)n * g.batch + b0 + i] = tau;
            }
            l_tau[i * AS + n] = tau;
        }
        for (int q = tid; q < T * Np; q += NT) {  // tau': the target tag
            const int i = q / Np, n = q - i * Np;
            float tau = 0.f;
            if (i < nv) {
                tau = iqn_tau(g.seed, (uint32_t)(b0 + i), n, g.draw_ctr, TAG_IQN_TARGET);
                if (g.tau_target_out) g.tau_target_out[(int64_t)n * g.batch + b0 + i] = tau;
            }
            l_taup[i * AS + n] = tau;
        }
        for (int q = tid; q < T * (h + 1); q += NT) L.dpsi[q] = 0.f;
        __syncthreads();  // (also: l_gp is written)
        dist_tile_scalars<T>(g, b0, nv, l_gp, l_r, l_cc, l_w, l_ai);
        // ---- target net on s' at tau' [, online net on s' at the same tau']
        iqn_stage(g.tparams, ns, h, na, nc, L);
        dist_layer1<ACT, T, NT>(g.tparams, ns, h, l_xn, L.psi);
        iqn_rows_all(L, l_taup, Np, nv * Np, h, na, nc, l_c, l_tht);
        if (g.double_dqn) {  // (uniform)
            iqn_stage(g.params, ns, h, na, nc, L);
            dist_layer1<ACT, T, NT>(g.params, ns, h, l_xn, L.psi);
            iqn_rows_all(L, l_taup, Np, nv * Np, h, na, nc, l_c, l_tho);
        }
        if (tid < na * T) {
            const int i = tid % T, o = tid / T;
            l_qt[o * T + i] = i < nv ? iqn_mean(l_tht + i * LS + o * Np, Np) : 0.f;
        } else if (g.double_dqn && tid >= MAXO * T && tid < MAXO * T + na * T) {
            const int i = tid % T, o = (tid - MAXO * T) / T;
            l_qo[o * T + i] = i < nv ? iqn_mean(l_tho + i * LS + o * Np, Np) : 0.f;
        }
        __syncthreads();
        dist_select_action<T>(g.double_dqn ? l_qo : l_qt, na, l_as, g.sel_out, b0, nv);
        __syncthreads();
        for (int q = tid; q < Np * T; q += NT) {  // T_j = fmaf(c, th_t(s', tau'_j)[a*], r)
            const int i = q % T, j = q / T;
            float t = 0.f;
            if (i < nv) {
                t = fmaf(l_cc[i], l_tht[i * LS + l_as[i] * Np + j], l_r[i]);
                if (g.target_out) g.target_out[(int64_t)j * g.batch + b0 + i] = t;
            }
            l_T[i * AS + j] = t;
        }
        // ---- online net on s at tau, block by block: forward, pairwise term, backward
        if (!g.double_dqn) iqn_stage(g.params, ns, h, na, nc, L);
        dist_layer1<ACT, T, NT>(g.params, ns, h, l_x, L.psi);
        const int nrows = nv * N;
        for (int row0 = 0; row0 < nrows; row0 += IQ_RB) {
            iqn_cos_block(l_tau, N, row0, nrows, nc, l_c);
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
                    const float tau = l_tau[i * AS + n];
                    const float* tj = l_T + i * AS;
                    float rho = 0.f, d = 0.f;
                    for (int j = 0; j < Np; ++j) {
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
            IQ_DWPHI(aw00, wave, 0)
            IQ_DWPHI(aw01, wave, 1)
            IQ_DWPHI(aw10, wave + 4, 0)
            IQ_DWPHI(aw11, wave + 4, 1)
            __syncthreads();  // the next block rewrites c and phi
        }
        if (tid < T) {  // L_i of sample `tid`
            float Li = 0.f;
            if (l_ai[tid] >= 0) {
                float sr = 0.f;
                for (int n = 0; n < N; ++n) sr += l_rho[tid * AS + n];
                Li = sr / g.fNp;
                if (g.ql_out) g.ql_out[b0 + tid] = Li;
                if (g.isw) Li *= l_w[tid];
            } else if (tid < nv && g.ql_out) {
                g.ql_out[b0 + tid] = 0.f;
            }
            l_loss[tid] = Li;
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
        __syncthreads();  // the next tile rewrites every buffer
    }
    // ---- the workgroup's partial row: every element is written
    float* row_out = g.partials + (int64_t)blockIdx.x * g.np;
    const int off_wp = ne1, off_bp = off_wp + h * nc, off_w2 = off_bp + h, off_b2 = off_w2 + na * h;
#pragma unroll
    for (int u = 0; u < IQ_W1U; ++u)
        if (tid + u * NT < ne1) row_out[tid + u * NT] = a_w1[u];
    IQ_DWPHI_STORE(aw00, wave, 0)
    IQ_DWPHI_STORE(aw01, wave, 1)
    IQ_DWPHI_STORE(aw10, wave + 4, 0)
    IQ_DWPHI_STORE(aw11, wave + 4, 1)
    if (tid < h) {
        row_out[off_bp + tid] = a_bphi;
#pragma unroll
        for (int o = 0; o < MAXO; ++o)
            if (o < na) row_out[off_w2 + o + na * tid] = a_w2[o];
        if (tid < na) row_out[off_b2 + tid] = a_b2;
    }
    if (tid == 0) g.loss_partials[blockIdx.x] = s_loss;
}

// Glorot-uniform per Dense layer, zero biases, by the rule of mlp2_init_kernel: tensor ids net_id * 4 + {0: W1, 1: Wphi, 2: W2}
__global__ __launch_bounds__(256) void iqn_init_kernel(float* __restrict__ p, int ns, int h, int na, int nc, uint64_t seed, uint32_t net_id) {
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t o1 = (int64_t)h * ns, o2 = o1 + h, o3 = o2 + (int64_t)h * nc, o4 = o3 + h, o5 = o4 + (int64_t)na * h;
    if (q >= o5 + na) return;
    float val = 0.0f;  // Flux Dense bias default: zeros
    int64_t off = -1;
    uint32_t tensor = 0;
    float fan = 1.0f;
    if (q < o1) off = q, tensor = 0, fan = (float)(ns + h);
    else if (q >= o2 && q < o3) off = q - o2, tensor = 1, fan = (float)(nc + h);
    else if (q >= o4 && q < o5) off = q - o4, tensor = 2, fan = (float)(h + na);
    if (off >= 0) {
        const u32x4 w = philox4x32_10(seed, (uint32_t)off, 0, net_id * 4u + tensor, TAG_INIT);
        val = (2.0f * u01_f32(w.x) - 1.0f) * sqrtf(6.0f / fan);
    }
    p[q] = val;
}

static bool iqn_levels_ok(int64_t n) { return n >= 1 && n <= IQ_MAXL; }

template <class K>
static int32_t iqn_allow_lds(K kernel, size_t bytes, unsigned long long* done) {
    return allow_big_lds(kernel, bytes, done);
}

}  // namespace rlhip

using namespace rlhip;

static int32_t iqn_plan_launch(const float* params, int64_t ns, int64_t h, int64_t na, int64_t n_cos, int64_t K, int32_t act, const float* obs,
                               int64_t n, double eps, uint64_t seed, uint32_t env_id_base, uint32_t step, int32_t* actions, float* q_out,
                               float* quantiles_out, float* tau_out, rlhip_stream_t stream) {
    IqnPlanArgs g;
    g.params = params, g.obs = obs, g.q_out = q_out, g.quantiles_out = quantiles_out, g.tau_out = tau_out, g.actions = actions;
    g.n = n, g.ns = (int)ns, g.h = (int)h, g.na = (int)na, g.nc = (int)n_cos, g.K = (int)K;
    g.eps = eps, g.seed = seed, g.env_id_base = env_id_base, g.step = step;
    const dim3 grid((unsigned)((n + IQ_T - 1) / IQ_T));
    const size_t lds = iqn_lds_bytes(h, n_cos, false);
    static unsigned long long done0 = 0, done1 = 0;  // the opt-in is for the largest net of the envelope
    const size_t lds_max = iqn_lds_bytes(IQ_HMAX, IQ_MAXC, false);
    // the instantiation set: ACT in {0, 1}
    if (act == 0) {
        const int32_t rc = iqn_allow_lds(iqn_plan_kernel<0>, lds_max, &done0);
        if (rc) return rc;
        hipLaunchKernelGGL((iqn_plan_kernel<0>), grid, dim3(IQ_NT), lds, as_stream(stream), g);
    } else {
        const int32_t rc = iqn_allow_lds(iqn_plan_kernel<1>, lds_max, &done1);
        if (rc) return rc;
        hipLaunchKernelGGL((iqn_plan_kernel<1>), grid, dim3(IQ_NT), lds, as_stream(stream), g);
    }
    RLHIP_LAUNCH_CHECK();
    return RLHIP_OK;
}

template <int ACT>
static int32_t iqn_launch_grad(const IqnGradArgs& g, int nb, hipStream_t s) {
    static unsigned long long done = 0;
    const int32_t rc = iqn_allow_lds(iqn_grad_kernel<ACT>, iqn_lds_bytes(IQ_HMAX, IQ_MAXC, true), &done);
    if (rc) return rc;
    hipLaunchKernelGGL((iqn_grad_kernel<ACT>), dim3(nb), dim3(IQ_NT), iqn_lds_bytes(g.h, g.nc, true), s, g);
    return RLHIP_OK;
}

extern "C" {

int64_t rlhip_iqn_nparams(int64_t ns, int64_t h, int64_t na, int64_t n_cos) {
    if (ns < 1 || h < 1 || na < 1 || n_cos < 1) return -1;
    return iqn_nparams(ns, h, na, n_cos);
}

int32_t rlhip_iqn_init_f32(float* params, int64_t ns, int64_t h, int64_t na, int64_t n_cos, uint64_t seed, uint32_t net_id,
                           rlhip_stream_t stream) {
    RLHIP_REQUIRE(params != nullptr && ns >= 1 && h >= 1 && na >= 1 && n_cos >= 1, "bad arguments");
    const int64_t np = iqn_nparams(ns, h, na, n_cos);
    RLHIP_REQUIRE(np <= 0x7fffffffLL, "the network is too large");
    hipLaunchKernelGGL(iqn_init_kernel, dim3((int)((np + 255) / 256)), dim3(256), 0, as_stream(stream), params, (int)ns, (int)h, (int)na,
                       (int)n_cos, seed, net_id);
    RLHIP_LAUNCH_CHECK();
    return RLHIP_OK;
}

int32_t rlhip_iqn_forward_f32(const float* params, int64_t ns, int64_t h, int64_t na, int64_t n_cos, int64_t n_levels, int32_t act,
                              const float* obs, int64_t n, uint64_t seed, uint32_t env_id_base, uint32_t step, float* q_out,
                              float* quantiles_out, float* tau_out, rlhip_stream_t stream) {
    IQ_REQUIRE_NET();
    RLHIP_REQUIRE(iqn_levels_ok(n_levels), "the number of levels must be 1..64");
    RLHIP_REQUIRE(n >= 0 && n <= 0x7fffffffLL, "env count must be 0 .. 2^31 - 1");
    RLHIP_REQUIRE(params && obs && q_out, "NULL argument");
    if (n == 0) return RLHIP_OK;
    return iqn_plan_launch(params, ns, h, na, n_cos, n_levels, act, obs, n, 0.0, seed, env_id_base, step, nullptr, q_out, quantiles_out, tau_out,
                           stream);
}

int32_t rlhip_iqn_plan_f32(const float* params, int64_t ns, int64_t h, int64_t na, int64_t n_cos, int64_t n_levels, int32_t act,
                           const float* obs, int64_t n, double eps, uint64_t seed, uint32_t env_id_base, uint32_t step, int32_t* actions,
                           float* q_out, float* tau_out, rlhip_stream_t stream) {
    IQ_REQUIRE_NET();
    RLHIP_REQUIRE(iqn_levels_ok(n_levels), "the number of levels must be 1..64");
    RLHIP_REQUIRE(n >= 0 && n <= 0x7fffffffLL, "env count must be 0 .. 2^31 - 1");
    RLHIP_REQUIRE(params && obs && actions, "NULL argument");
    if (n == 0) return RLHIP_OK;
    return iqn_plan_launch(params, ns, h, na, n_cos, n_levels, act, obs, n, eps, seed, env_id_base, step, actions, q_out, nullptr, tau_out,
                           stream);
}

int64_t rlhip_iqn_workspace_bytes(int64_t ns, int64_t h, int64_t na, int64_t n_cos, int64_t n_levels, int64_t n_target_levels,
                                  int64_t batch) {
    if (!iqn_net_ok(ns, h, na, n_cos) || !iqn_levels_ok(n_levels) || !iqn_levels_ok(n_target_levels) || batch < 1) return -1;
    const int64_t np = iqn_nparams(ns, h, na, n_cos);
    return dist_num_blocks(np, batch, IQ_T) * (np + 1) * (int64_t)sizeof(float);  // partial rows | partial losses
}

int32_t rlhip_iqn_grad_batch_f32(int64_t ns, int64_t h, int64_t na, int64_t n_cos, int64_t n_levels, int64_t n_target_levels, int32_t act,
                                 float kappa, const float* params, const float* target_params, const float* s, const int32_t* a,
                                 const float* r, const uint8_t* term, const float* s_next, int64_t batch, float gamma, const int32_t* n_used,
                                 const float* weights, int32_t double_dqn, uint64_t seed, uint32_t draw_ctr, void* workspace,
                                 float* grad_out, float* loss_out, float* ql_out, float* target_out, int32_t* sel_out, float* tau_out,
                                 float* tau_target_out, rlhip_stream_t stream) {
    IQ_REQUIRE_NET();
    RLHIP_REQUIRE(iqn_levels_ok(n_levels) && iqn_levels_ok(n_target_levels), "the number of levels must be 1..64");
    RLHIP_REQUIRE(std::isfinite(kappa) && kappa > 0.f, "kappa must be finite and > 0");
    RLHIP_REQUIRE(batch >= 1 && batch <= 0x7fffffffLL, "batch must be 1 .. 2^31 - 1");
    RLHIP_REQUIRE(params && target_params && s && a && r && term && s_next && workspace && grad_out && loss_out, "NULL argument");
    hipStream_t st = as_stream(stream);
    const int64_t np = iqn_nparams(ns, h, na, n_cos);
    IqnGradArgs g;
    g.params = params, g.tparams = target_params;
    g.s = s, g.a = a, g.r = r, g.term = term, g.sn = s_next;
    g.n_used = n_used, g.isw = weights, g.ql_out = ql_out, g.target_out = target_out, g.sel_out = sel_out;
    g.tau_out = tau_out, g.tau_target_out = tau_target_out;
    g.batch = batch;
    g.ns = (int)ns, g.h = (int)h, g.na = (int)na, g.nc = (int)n_cos, g.N = (int)n_levels, g.Np = (int)n_target_levels, g.np = (int)np;
    g.num_tiles = (int)((batch + IQ_T - 1) / IQ_T);
    g.double_dqn = double_dqn ? 1 : 0;
    g.seed = seed, g.draw_ctr = draw_ctr;
    g.gamma = gamma, g.kappa = kappa, g.fNp = (float)n_target_levels, g.fNB = g.fNp * (float)batch;
    for (int n = 0; n < DIST_GPOW; ++n) g.gpow[n] = rlhip_gamma_pow(gamma, n);
    const int nb = (int)dist_num_blocks(np, batch, IQ_T);
    g.partials = (float*)workspace;
    g.loss_partials = g.partials + (int64_t)nb * np;
    // the instantiation set: ACT in {0, 1}
    const int32_t rc = act == 0 ? iqn_launch_grad<0>(g, nb, st) : iqn_launch_grad<1>(g, nb, st);
    if (rc) return rc;
    RLHIP_LAUNCH_CHECK();
    return dist_reduce_launch(g.partials, g.loss_partials, nb, np, grad_out, loss_out, (float)batch, st);
}

}  // extern "C"
