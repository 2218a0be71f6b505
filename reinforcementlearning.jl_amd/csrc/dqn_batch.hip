// dqn_batch.hip -- DQN on observations of 5..16 Float32 components (AcrobotRK4Env has six): plan! as one launch, and the loss /
// gradient of a two-layer Q-network on a MATERIALISED batch (the SoA arrays rlhip_ring_gather / rlhip_ring_gather_nstep /
// rlhip_ring_sample_gather_nstep_prioritized write from a frame-layout ring).  dqn.hip keeps the record-ring learners (obs_dim 2..4,
// the draw and the gather inside the gradient launch); nothing of it moved here.
//
// K = ns <= 16 and N = na <= 4 are far below an MFMA tile: VALU work, as the note at the top of mlp_device.h argues.
//
//   dqn_plan_obsn_kernel<ACT, STAGED>  one lane per env, the weights wave-uniform (broadcast reads of the net staged in LDS; scalar
//                                    loads from global memory for nets too large to stage): the order of mlp2_forward_kernel
//                                    (ppo.hip) and of the oracle -- z = b1[j], fmaf over k ascending; q = b2, fmaf over j ascending --
//                                    then eps_greedy_select1 (select_device.h) in the same lane: byte for byte
//                                    rlhip_mlp2_forward_f32 -> rlhip_eps_greedy_select_f32
//   dqn_grad_batch_kernel<NSV, ACT>  the two-phase structure of dqn_grad_kernel on tiles of 64 samples, NSV = ceil(ns / 4) input
//                                    quads (LDS rows and registers are padded to 4 NSV inputs with zeros: a padded term is
//                                    fmaf(0, 0, z) behind the real chain)
//       phase 0   both nets -> LDS (one row per hidden unit), the tile's s / s' -> LDS, coalesced from the SoA batch
//       phase 1   row of 16 lanes = sample, lane c walks hidden units c, c + 16, ..: Q(s), Qt(s') [, Q(s') for Double DQN], the
//                 TD line in the same lanes; h(s) of every (sample, unit) is left in LDS
//       phase 2   thread = (hidden unit j, input quad): ONE fmaf chain per gradient element over the samples of the tile in
//                 ascending order, carried in registers over the workgroup's tiles -- no cross-lane sum.  The ReLU mask is read off
//                 the stored h (h > 0 <=> z > 0), so both phases see one z
//   dqn_batch_reduce_kernel          the partial rows, one per workgroup, in a fixed order (include/rlhip.h states it)
// No float atomics anywhere: two calls on the same inputs give the same bytes.
#include "mlp_device.h"
#include "select_device.h"

namespace rlhip {

constexpr int BTILE = 64;
constexpr int BTHREADS = 1024, BWAVES = BTHREADS / 64;
constexpr int BMAX_BLOCKS = 256;  // partial rows: a larger batch gives its workgroups further tiles
constexpr int BHMAX = 256;
constexpr int BHPAD = 16;         // h(s) rows of phase 1 are h + 16 floats apart: the four samples of a wave land in four bank groups
constexpr int BGPOW = 33;         // gamma^n for n = 0..32

struct DqnBatchArgs {
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
    float* td_out;  // nullable
    int64_t batch;
    int ns, h, na, np, num_tiles, double_dqn;
    float gamma, delta, fb;
    float gpow[BGPOW];
};

__host__ __device__ __forceinline__ int batch_lds_floats(int h, int nsv) {
    // nets | s tile | s' tile | h(s) | dL/dq | db2 + loss slots | gamma powers (padded)
    return 2 * h * (4 * nsv + 8) + 2 * BTILE * 4 * nsv + BTILE * (h + BHPAD) + BTILE * 4 + (MAXO + 1) * BTILE + 36;
}

template <int NSV, int ACT>
__global__ __launch_bounds__(BTHREADS) void dqn_grad_batch_kernel(DqnBatchArgs g) {
    constexpr int NSP = 4 * NSV;  // padded inputs
    constexpr int RV = NSV + 2;   // float4 per unit: W1[j, 0 .. NSP - 1] | {b1[j], W2[0..2, j]} | {W2[3, j], 0, 0, 0}
    static_assert(MAXO == 4 && BWAVES * 4 == BTILE, "one row of 16 lanes per sample");
    extern __shared__ float4 l_dyn[];
    const int h = g.h, na = g.na, ns = g.ns;
    const int HS = h + BHPAD;
    float4* l_rec = l_dyn;                                  // [2][h][RV]
    float4* l_x = l_rec + 2 * h * RV;                       // [BTILE][NSV]
    float4* l_xn = l_x + BTILE * NSV;                       // [BTILE][NSV]
    float4* l_dL = l_xn + BTILE * NSV;                      // [BTILE]
    float* l_hv = reinterpret_cast<float*>(l_dL + BTILE);   // [BTILE][HS]
    float* l_fin = l_hv + BTILE * HS;                       // [MAXO + 1][BTILE]
    float* l_gp = l_fin + (MAXO + 1) * BTILE;               // [BGPOW]

    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int row = lane >> 4, c = lane & 15;
    const int smp = 4 * w + row;  // phase 1: this row's sample of the tile
    const float* b2 = g.params + h * ns + h + na * h;
    const float* tb2 = g.tparams + h * ns + h + na * h;

    // phase 2: this thread's (unit, input quad)
    const bool p2 = tid < h * NSV;
    const int pj = p2 ? tid % h : 0, pch = p2 ? tid / h : 0;
    float gw1[4] = {0.f, 0.f, 0.f, 0.f}, gw2[MAXO] = {0.f, 0.f, 0.f, 0.f}, gb1 = 0.f;
    float gb2[MAXO] = {0.f, 0.f, 0.f, 0.f};  // (every lane of a row carries its sample slot's sums; lane c == 0 hands them over)
    float s_loss = 0.f;

    // ---- once per workgroup: both networks and the discount table -> LDS
    for (int q = tid; q < 2 * h; q += BTHREADS) {
        const int net = q >= h ? 1 : 0, u = q - net * h;
        const float* P = net ? g.tparams : g.params;
        float4* rec = l_rec + (net * h + u) * RV;
#pragma unroll
        for (int v = 0; v < NSV; ++v) {
            float w1[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) w1[k] = (4 * v + k < ns) ? P[u + h * (4 * v + k)] : 0.f;
            rec[v] = make_float4(w1[0], w1[1], w1[2], w1[3]);
        }
        float w2[MAXO];
#pragma unroll
        for (int o = 0; o < MAXO; ++o) w2[o] = (o < na) ? P[h * ns + h + o + na * u] : 0.f;
        rec[NSV] = make_float4(P[h * ns + u], w2[0], w2[1], w2[2]);
        rec[NSV + 1] = make_float4(w2[3], 0.f, 0.f, 0.f);
    }
    if (tid == 0) {
#pragma unroll
        for (int n = 0; n < BGPOW; ++n) l_gp[n] = g.gpow[n];
    }

    for (int tile = blockIdx.x; tile < g.num_tiles; tile += gridDim.x) {
        const int64_t b0 = (int64_t)tile * BTILE;
        // ---- phase 0: the tile's states, coalesced along the batch, one input component per wave and round
        for (int k = w; k < NSP; k += BWAVES) {
            const int64_t b = b0 + lane;
            float vs = 0.f, vn = 0.f;
            if (k < ns && b < g.batch) {
                vs = g.s[(int64_t)k * g.batch + b];
                vn = g.sn[(int64_t)k * g.batch + b];
            }
            reinterpret_cast<float*>(l_x)[lane * NSP + k] = vs;
            reinterpret_cast<float*>(l_xn)[lane * NSP + k] = vn;
        }
        // this row's sample: its scalars are requested before the barrier and arrive under the forward passes
        const int64_t b = b0 + smp;
        const bool valid = b < g.batch;
        const int64_t bl = valid ? b : 0;
        const float sr = g.r[bl];
        const int a = g.a[bl];
        const float cont = g.term[bl] ? 0.f : 1.f;
        int nu = g.n_used ? g.n_used[bl] : 0;
        const float wis = g.isw ? g.isw[bl] : 1.0f;
        float bq[MAXO], btq[MAXO];
#pragma unroll
        for (int o = 0; o < MAXO; ++o) {
            bq[o] = (o < na) ? b2[o] : 0.f;
            btq[o] = (o < na) ? tb2[o] : 0.f;
        }
        __syncthreads();
        // ---- phase 1: Q(s), Qt(s') [, Q(s')] of sample `smp`, then its TD line
        {
            float acc[MAXO] = {0.f, 0.f, 0.f, 0.f}, act_[MAXO] = {0.f, 0.f, 0.f, 0.f}, aco[MAXO] = {0.f, 0.f, 0.f, 0.f};
            {  // pass A: the online net on s; h(s) stays in LDS for phase 2
                float x[NSP];
#pragma unroll
                for (int v = 0; v < NSV; ++v) {
                    const float4 t = l_x[smp * NSV + v];
                    x[4 * v] = t.x, x[4 * v + 1] = t.y, x[4 * v + 2] = t.z, x[4 * v + 3] = t.w;
                }
#pragma unroll 1
                for (int jj = c; jj < h; jj += 16) {
                    const float4* ro = l_rec + jj * RV;
                    const float4 o1 = ro[NSV], o2 = ro[NSV + 1];
                    float z = o1.x;
#pragma unroll
                    for (int v = 0; v < NSV; ++v) {
                        const float4 wo = ro[v];
                        const float wa[4] = {wo.x, wo.y, wo.z, wo.w};
#pragma unroll
                        for (int k = 0; k < 4; ++k) z = fmaf(wa[k], x[4 * v + k], z);
                    }
                    const float hv = act_fwd_t<ACT>(z);
                    l_hv[smp * HS + jj] = hv;
                    const float w2o[MAXO] = {o1.y, o1.z, o1.w, o2.x};
#pragma unroll
                    for (int o = 0; o < MAXO; ++o) acc[o] = fmaf(w2o[o], hv, acc[o]);  // (rows o >= na are staged as zeros)
                }
            }
            {  // pass B: the target net on s' -- and, for Double DQN, the online net on s'
                float xn[NSP];
#pragma unroll
                for (int v = 0; v < NSV; ++v) {
                    const float4 u = l_xn[smp * NSV + v];
                    xn[4 * v] = u.x, xn[4 * v + 1] = u.y, xn[4 * v + 2] = u.z, xn[4 * v + 3] = u.w;
                }
#pragma unroll 1
                for (int jj = c; jj < h; jj += 16) {
                    const float4* rt = l_rec + (h + jj) * RV;
                    const float4 t1 = rt[NSV], t2 = rt[NSV + 1];
                    float zt = t1.x;
#pragma unroll
                    for (int v = 0; v < NSV; ++v) {
                        const float4 wt = rt[v];
                        const float wc[4] = {wt.x, wt.y, wt.z, wt.w};
#pragma unroll
                        for (int k = 0; k < 4; ++k) zt = fmaf(wc[k], xn[4 * v + k], zt);
                    }
                    const float ht = act_fwd_t<ACT>(zt);
                    const float w2t[MAXO] = {t1.y, t1.z, t1.w, t2.x};
#pragma unroll
                    for (int o = 0; o < MAXO; ++o) act_[o] = fmaf(w2t[o], ht, act_[o]);
                    if (g.double_dqn) {  // (uniform)
                        const float4* ro = l_rec + jj * RV;
                        const float4 o1 = ro[NSV], o2 = ro[NSV + 1];
                        float zo = o1.x;
#pragma unroll
                        for (int v = 0; v < NSV; ++v) {
                            const float4 wo = ro[v];
                            const float wa[4] = {wo.x, wo.y, wo.z, wo.w};
#pragma unroll
                            for (int k = 0; k < 4; ++k) zo = fmaf(wa[k], xn[4 * v + k], zo);
                        }
                        const float ho = act_fwd_t<ACT>(zo);
                        const float w2o[MAXO] = {o1.y, o1.z, o1.w, o2.x};
#pragma unroll
                        for (int o = 0; o < MAXO; ++o) aco[o] = fmaf(w2o[o], ho, aco[o]);
                    }
                }
            }
            float q[MAXO], qt[MAXO], qo[MAXO];
#pragma unroll
            for (int o = 0; o < MAXO; ++o) {
                q[o] = 0.f, qt[o] = 0.f, qo[o] = 0.f;
                if (o < na) {  // (uniform)
                    q[o] = group_sum_dpp<16>(acc[o]) + bq[o];
                    qt[o] = group_sum_dpp<16>(act_[o]) + btq[o];
                    if (g.double_dqn) qo[o] = group_sum_dpp<16>(aco[o]) + bq[o];
                }
            }
            float sel = qt[0];
            if (g.double_dqn) {  // Qt(s')[findmax(Q(s'))]: the first maximum wins (strict >)
                float m = qo[0];
#pragma unroll
                for (int o = 1; o < MAXO; ++o)
                    if (o < na && qo[o] > m) m = qo[o], sel = qt[o];
            } else {
#pragma unroll
                for (int o = 1; o < MAXO; ++o)
                    if (o < na && qt[o] > sel) sel = qt[o];
            }
            float disc = g.gamma;
            if (g.n_used) {
                nu = nu < 0 ? 0 : (nu > BGPOW - 1 ? BGPOW - 1 : nu);
                disc = l_gp[nu];
            }
            const float G = sr + (disc * cont) * sel;
            float qa = 0.f;
            bool known = false;  // the action is only ever COMPARED: an action outside 0 .. na - 1 selects nothing
#pragma unroll
            for (int o = 0; o < MAXO; ++o)
                if (o < na && o == a) qa = q[o], known = true;
            const float d = qa - G;
            const float e = fabsf(d);
            float l = (e < g.delta) ? (e * e) * 0.5f : g.delta * (e - 0.5f * g.delta);
            float gi = (e < g.delta) ? d : (d > 0.f ? g.delta : (d < 0.f ? -g.delta : 0.f));
            gi = gi / g.fb;
            if (g.isw) {  // loss = mean(w .* huber(td))
                gi *= wis;
                l *= wis;
            }
            float td = e;
            if (!valid || !known) gi = 0.f, l = 0.f, td = 0.f;
            if (valid && g.td_out && c == 0) g.td_out[b] = td;
            s_loss += l;
            float dl[MAXO];
#pragma unroll
            for (int o = 0; o < MAXO; ++o) {
                dl[o] = (o == a) ? gi : 0.f;
                gb2[o] += dl[o];
            }
            if (c == 0) {
                l_dL[smp] = make_float4(dl[0], dl[1], dl[2], dl[3]);
#pragma unroll
                for (int o = 0; o < MAXO; ++o) l_fin[o * BTILE + smp] = gb2[o];  // running sums over this workgroup's tiles: complete
                l_fin[MAXO * BTILE + smp] = s_loss;                              // after the last one, read by wave 0 behind the loop
            }
        }
        __syncthreads();
        // ---- phase 2: unit pj, inputs 4 pch .. 4 pch + 3, over the samples of the tile in ascending order
        if (p2) {
            const float4 r1 = l_rec[pj * RV + NSV], r2 = l_rec[pj * RV + NSV + 1];
            const float rw2[MAXO] = {r1.y, r1.z, r1.w, r2.x};
#pragma unroll 4
            for (int i = 0; i < BTILE; ++i) {
                const float hv = l_hv[i * HS + pj];
                const float4 d4 = l_dL[i], x4 = l_x[i * NSV + pch];
                const float dd[MAXO] = {d4.x, d4.y, d4.z, d4.w}, xv[4] = {x4.x, x4.y, x4.z, x4.w};
                float dh = 0.f;
#pragma unroll
                for (int o = 0; o < MAXO; ++o) {
                    gw2[o] = fmaf(dd[o], hv, gw2[o]);
                    dh = fmaf(dd[o], rw2[o], dh);
                }
                const float dz = dh * (ACT == 0 ? (hv > 0.0f ? 1.0f : 0.0f) : (1.0f - hv * hv));
                gb1 += dz;
#pragma unroll
                for (int k = 0; k < 4; ++k) gw1[k] = fmaf(dz, xv[k], gw1[k]);
            }
        }
        __syncthreads();  // the next tile rewrites l_x / l_hv / l_dL
    }
    float* out = g.partials + (int64_t)blockIdx.x * g.np;
    if (p2) {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (4 * pch + k < ns) out[pj + h * (4 * pch + k)] = gw1[k];
        if (pch == 0) {
            out[h * ns + pj] = gb1;
#pragma unroll
            for (int o = 0; o < MAXO; ++o)
                if (o < na) out[h * ns + h + o + na * pj] = gw2[o];
        }
    }
    // db2 and the loss: one slot per sample of the tile -> wave 0 (fixed tree)
    if (tid < BTILE) {
        float f[MAXO + 1];
#pragma unroll
        for (int o = 0; o <= MAXO; ++o) f[o] = wave_sum_f32(l_fin[o * BTILE + tid]);
        if (tid == 0) {
            for (int o = 0; o < na; ++o) out[h * ns + h + na * h + o] = f[o];
            g.loss_partials[blockIdx.x] = f[MAXO];
        }
    }
}

// gradient element p = four groups of partial rows, ascending inside a group, then ((g0 + g1) + g2) + g3; the loss = the partial
// losses lane-strided, a shuffle tree, divided by the batch
__global__ __launch_bounds__(256) void dqn_batch_reduce_kernel(const float* __restrict__ partials, const float* __restrict__ loss_partials,
                                                               int nb, int np, float* __restrict__ grad, float* __restrict__ loss, float fb) {
    __shared__ float l_g[4][64];
    const int lane = threadIdx.x & 63, grp = threadIdx.x >> 6;
    const int p = blockIdx.x * 64 + lane;
    const int per = (nb + 3) / 4;
    const int r0 = grp * per, r1 = min(nb, r0 + per);
    float acc = 0.f;
    if (p < np) {
#pragma unroll 8
        for (int b = r0; b < r1; ++b) acc += partials[(int64_t)b * np + p];
    }
    l_g[grp][lane] = acc;
    __syncthreads();
    if (grp == 0 && p < np) grad[p] = ((l_g[0][lane] + l_g[1][lane]) + l_g[2][lane]) + l_g[3][lane];
    if (blockIdx.x == 0 && loss != nullptr && grp == 1) {
        float a = 0.f;
        for (int b = lane; b < nb; b += 64) a += loss_partials[b];
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) a += __shfl_down(a, off, 64);
        if (lane == 0) loss[0] = a / fb;
    }
}

#ifdef RLHIP_BOUNDS_CHECK
__global__ __launch_bounds__(256) void dqn_batch_count_bad_actions_kernel(const int32_t* __restrict__ a, int64_t batch, int na, int* __restrict__ n_bad) {
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b < batch && (a[b] < 0 || a[b] >= na)) atomicAdd(n_bad, 1);
}
#endif

struct RegQn {
    const float* q;
    __device__ __forceinline__ float operator()(int k) const { return q[k]; }
};

// One lane per env.  STAGED: the whole network (np floats of dynamic LDS, nets of up to PLAN_LDS_MAX_PARAMS parameters) is copied into
// LDS first, one wave per workgroup: every lane then reads the same word of a unit's weights (a broadcast), and the reads of the next
// units do not depend on the running sums -- where wave-uniform loads from global memory (the other form, for larger nets) put a
// scalar-cache round trip per hidden unit on the dependent chain (n = 4096, 6 -> 128 -> 3: profiles/dqn_obsn.md).  The arithmetic and
// its order are the same in both forms.
constexpr int PLAN_LDS_MAX_PARAMS = 12288;  // 48 KB

template <int ACT, bool STAGED>
__global__ __launch_bounds__(STAGED ? 64 : 256) void dqn_plan_obsn_kernel(const float* __restrict__ params, int ns, int h, int na, int np,
                                                                          const float* __restrict__ obs, int64_t n, double eps,
                                                                          uint64_t seed, uint32_t env_id_base, uint32_t step,
                                                                          int32_t* __restrict__ actions, float* __restrict__ q_out) {
    extern __shared__ float l_params[];
    if constexpr (STAGED) {
        for (int q = threadIdx.x; q < np; q += 64) l_params[q] = params[q];
        __syncthreads();
    }
    const int64_t env = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (env >= n) return;
    float x[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) x[k] = (k < ns) ? obs[(int64_t)k * n + env] : 0.f;
    float q[MAXO];
    const int ob1 = h * ns, ow2 = ob1 + h, ob2 = ow2 + na * h;
    auto P = [&](int i) -> float {
        if constexpr (STAGED) return l_params[i];
        else return params[i];
    };
#pragma unroll
    for (int o = 0; o < MAXO; ++o) q[o] = (o < na) ? P(ob2 + o) : 0.f;
    // Branch-free: a weight beyond ns / na is read from a clamped index and its fmaf is dropped by a select, so that all loads of a
    // unit (and of the next ones) are issued together instead of one per basic block with a wait each -- the arithmetic that IS kept is
    // the chain b1[j], fmaf over k ascending; b2, fmaf over j ascending, bit for bit.
#pragma unroll 2
    for (int j = 0; j < h; ++j) {
        float w1[16], w2[MAXO];
#pragma unroll
        for (int k = 0; k < 16; ++k) w1[k] = P(j + h * (k < ns ? k : 0));
#pragma unroll
        for (int o = 0; o < MAXO; ++o) w2[o] = P(ow2 + (o < na ? o : 0) + na * j);
        float z = P(ob1 + j);
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const float t = fmaf(w1[k], x[k], z);
            z = (k < ns) ? t : z;
        }
        const float hv = act_fwd_t<ACT>(z);
#pragma unroll
        for (int o = 0; o < MAXO; ++o) {
            const float t = fmaf(w2[o], hv, q[o]);
            q[o] = (o < na) ? t : q[o];
        }
    }
    actions[env] = eps_greedy_select1(RegQn{q}, NoMask{}, na, eps, false, seed, env_id_base + (uint32_t)env, step);
    if (q_out) {
#pragma unroll
        for (int o = 0; o < MAXO; ++o)
            if (o < na) q_out[(int64_t)o * n + env] = q[o];
    }
}

template <int NSV, int ACT>
static int32_t launch_grad_batch(const DqnBatchArgs& g, int nb, hipStream_t s) {
    static unsigned long long big_lds_done = 0;
    const size_t lds = sizeof(float) * (size_t)batch_lds_floats(g.h, NSV);
    if (lds > 64 * 1024) {
        const int32_t rc = allow_big_lds(dqn_grad_batch_kernel<NSV, ACT>, lds, &big_lds_done);
        if (rc) return rc;
    }
    hipLaunchKernelGGL((dqn_grad_batch_kernel<NSV, ACT>), dim3(nb), dim3(BTHREADS), lds, s, g);
    return RLHIP_OK;
}

}  // namespace rlhip

using namespace rlhip;

extern "C" {

int64_t rlhip_dqn_batch_workspace_bytes(int64_t ns, int64_t h, int64_t na, int64_t batch) {
    if (ns < 5 || ns > 16 || h < 4 || h > BHMAX || h % 4 != 0 || na < 1 || na > MAXO || batch < 1) return -1;
    const int64_t tiles = (batch + BTILE - 1) / BTILE;
    const int64_t nb = tiles < BMAX_BLOCKS ? tiles : BMAX_BLOCKS;
    return nb * (mlp2_nparams(ns, h, na) + 1) * (int64_t)sizeof(float);  // partial rows | partial losses
}

int32_t rlhip_dqn_grad_batch_f32(int64_t ns, int64_t h, int64_t na, int32_t act, const float* params, const float* target_params,
                                 const float* s, const int32_t* a, const float* r, const uint8_t* term, const float* s_next,
                                 int64_t batch, float gamma, const int32_t* n_used, const float* weights, int32_t double_dqn,
                                 float huber_delta, void* workspace, float* grad_out, float* loss_out, float* td_out,
                                 rlhip_stream_t stream) {
    RLHIP_REQUIRE(ns >= 5 && ns <= 16, "obs dim must be 5..16 (record rings of 2..4 components: rlhip_dqn_grad_idx_f32)");
    RLHIP_REQUIRE(h >= 4 && h <= BHMAX && h % 4 == 0, "hidden must be a multiple of 4, <= 256");
    RLHIP_REQUIRE(na >= 1 && na <= MAXO, "na must be 1..4");
    RLHIP_REQUIRE(act == 0 || act == 1, "act must be 0 (relu) or 1 (tanh)");
    RLHIP_REQUIRE(batch >= 1, "empty batch");
    RLHIP_REQUIRE(params && target_params && s && a && r && term && s_next && workspace && grad_out && loss_out, "NULL argument");
    hipStream_t st = as_stream(stream);
#ifdef RLHIP_BOUNDS_CHECK
    {  // the debug build: an action outside 0 .. na - 1 is an error instead of a sample without a gradient
        int* cnt = (int*)workspace;
        int n_bad = 0;
        RLHIP_CHECK_HIP(hipMemsetAsync(cnt, 0, sizeof(int), st));
        hipLaunchKernelGGL(dqn_batch_count_bad_actions_kernel, dim3((int)((batch + 255) / 256)), dim3(256), 0, st, a, batch, (int)na, cnt);
        RLHIP_LAUNCH_CHECK();
        RLHIP_CHECK_HIP(hipMemcpyAsync(&n_bad, cnt, sizeof(int), hipMemcpyDeviceToHost, st));
        RLHIP_CHECK_HIP(hipStreamSynchronize(st));
        if (n_bad) {
            ::rlhip::set_error("%s:%d: %d of %lld actions are outside 0 .. %lld", __FILE__, __LINE__, n_bad, (long long)batch, (long long)na - 1);
            return RLHIP_EINVAL;
        }
    }
#endif
    const int64_t np = mlp2_nparams(ns, h, na);
    DqnBatchArgs g;
    g.params = params, g.tparams = target_params;
    g.s = s, g.a = a, g.r = r, g.term = term, g.sn = s_next;
    g.n_used = n_used, g.isw = weights, g.td_out = td_out;
    g.batch = batch;
    g.ns = (int)ns, g.h = (int)h, g.na = (int)na, g.np = (int)np;
    g.num_tiles = (int)((batch + BTILE - 1) / BTILE);
    g.double_dqn = double_dqn ? 1 : 0;
    g.gamma = gamma, g.delta = huber_delta, g.fb = (float)batch;
    for (int n = 0; n < BGPOW; ++n) g.gpow[n] = rlhip_gamma_pow(gamma, n);
    const int nb = g.num_tiles < BMAX_BLOCKS ? g.num_tiles : BMAX_BLOCKS;
    g.partials = (float*)workspace;
    g.loss_partials = g.partials + (int64_t)nb * np;
    const int nsv = (int)(ns + 3) / 4;
    int32_t rc;
    // the instantiation set: NSV in {2, 3, 4} x ACT in {0, 1}
    if (nsv == 2) rc = act == 0 ? launch_grad_batch<2, 0>(g, nb, st) : launch_grad_batch<2, 1>(g, nb, st);
    else if (nsv == 3) rc = act == 0 ? launch_grad_batch<3, 0>(g, nb, st) : launch_grad_batch<3, 1>(g, nb, st);
    else rc = act == 0 ? launch_grad_batch<4, 0>(g, nb, st) : launch_grad_batch<4, 1>(g, nb, st);
    if (rc) return rc;
    RLHIP_LAUNCH_CHECK();
    hipLaunchKernelGGL(dqn_batch_reduce_kernel, dim3((int)((np + 63) / 64)), dim3(256), 0, st, g.partials, g.loss_partials, nb, (int)np,
                       grad_out, loss_out, g.fb);
    RLHIP_LAUNCH_CHECK();
    return RLHIP_OK;
}

int32_t rlhip_dqn_plan_obsn_f32(const float* params, int64_t ns, int64_t h, int64_t na, int32_t act, const float* obs, int64_t n,
                                double eps, uint64_t seed, uint32_t env_id_base, uint32_t step, int32_t* actions, float* q_out,
                                rlhip_stream_t stream) {
    RLHIP_REQUIRE(ns >= 5 && ns <= 16, "obs dim must be 5..16 (2..4 components: rlhip_dqn_plan_f32)");
    RLHIP_REQUIRE(na >= 1 && na <= MAXO, "na must be 1..4");
    RLHIP_REQUIRE(h >= 1, "bad hidden size");
    RLHIP_REQUIRE(act == 0 || act == 1, "act must be 0 (relu) or 1 (tanh)");
    RLHIP_REQUIRE(n >= 0, "negative env count");
    RLHIP_REQUIRE(params && obs && actions, "NULL argument");
    if (n == 0) return RLHIP_OK;
    hipStream_t st = as_stream(stream);
    const int np = (int)mlp2_nparams(ns, h, na);
    // the instantiation set: ACT in {0, 1} x {staged in LDS, wave-uniform global loads}
#define LAUNCH_PLAN(ACT_, STAGED_, THREADS_, LDS_)                                                                                     \
    hipLaunchKernelGGL((dqn_plan_obsn_kernel<ACT_, STAGED_>), dim3((int)((n + THREADS_ - 1) / THREADS_)), dim3(THREADS_), LDS_, st, params, \
                       (int)ns, (int)h, (int)na, np, obs, n, eps, seed, env_id_base, step, actions, q_out)
    if (mlp2_nparams(ns, h, na) <= PLAN_LDS_MAX_PARAMS) {
        if (act == 0) LAUNCH_PLAN(0, true, 64, sizeof(float) * (size_t)np);
        else LAUNCH_PLAN(1, true, 64, sizeof(float) * (size_t)np);
    } else {
        if (act == 0) LAUNCH_PLAN(0, false, 256, 0);
        else LAUNCH_PLAN(1, false, 256, 0);
    }
#undef LAUNCH_PLAN
    RLHIP_LAUNCH_CHECK();
    return RLHIP_OK;
}

}  // extern "C"
