// noisy.hip -- NoisyDense networks (Fortunato et al. 2018, factorised Gaussian noise) for the categorical learner: the sixth Rainbow
// ingredient.  include/rlhip.h (the NoisyDense section) is the specification; tests/noisy_ref.py states it in Float64.
//
// A noisy layer is y = (Wmu + Wsg .* f(e_out) f(e_in)') x + bmu + bsg .* f(e_out), f(e) = sign(e) sqrt|e|.  The noisy vector is
// [ mu | sigma ], each half in the mlp2(ns, h, M) layout.  Two uses, two kernels:
//
//   noisy_c51_plan_kernel<ACT, T>   ACTING, fresh noise per ENV (4096 envs behind one plan! must not explore in one direction).  A
//       weight matrix per env cannot be folded, but the factorised form can be evaluated as two chains per output: with the factor
//       vectors a (ns), b (h), c (h), d (M) of an env,  z = zmu + b[j] zsg  where zsg runs over the pre-scaled input a .* x, and
//       l = lmu + d[m] lsg  where lsg runs over the pre-scaled hidden vector c .* hid.  ns + 2h + M normals per env instead of
//       ns h + h M.  Tile of T envs per workgroup of 256 threads:
//         phase A   the workgroup draws a (-> LDS) and d (-> the logit slots of LDS, which thread m later overwrites with its own
//                   logits) cooperatively, one Philox block + one Float64 Box-Muller per PAIR of neighbouring factors
//         phase B   layer 1, thread = (env, PAIR of hidden units): its 64 weights are requested first, then the thread draws the b
//                   pair and the c pair of exactly its two units in registers -- the Float64 log / sqrt / sincos run under the weight
//                   loads, and b and c never touch LDS or a barrier -- then the two chains; hid and v = c .* hid go to two LDS arrays
//         logits    thread = output row m: the W2mu row and the W2sg row stream from L2 once per tile, two accumulators per env, the
//                   hidden values read as float4 LDS broadcasts.  With M <= 128 rows the two halves of the workgroup take half of the
//                   tile's envs each (otherwise waves 2 and 3 would idle through the longest chain of the kernel)
//         then dist_plan_tail (dist_device.h), as c51_plan_kernel: c51_probs_q per (env, action), eps_greedy_select1 per env
//   noisy_fold_kernel / noisy_unfold_kernel   LEARNING, one sample per update and net (NoisyNet-DQN): eff = fmaf(sigma, xi, mu) is a
//       plain mlp2 vector that rlhip_c51_grad_batch_f32 takes unchanged; the gradient maps back as dmu = g, dsigma = g xi, the draws
//       REGENERATED from the key.  Every workgroup stages the ns + 2h + M factors in LDS once, then streams its elements; blockIdx.y
//       selects the net (online / target: two Philox tags) as in the dueling fold.
//   noisy_c51_plan_kernel<ACT, T, DUEL = true>   a noisy DUELING head (include/rlhip.h, the dueling distributional section): the same
//       phases on M' = (1 + na) K rows -- na K advantage rows, then K value rows -- and, before dist_plan_tail, the combine in the LDS
//       logit tile, thread = (env, atom): l[k, o] = (v[k] + a[k, o]) - mean_o' a[k, o'] (the output domain, the reference's own form)
//   noisy_dueling_fold_kernel / noisy_dueling_unfold_kernel   the update path of a noisy dueling net, one launch each: byte for byte
//       noisy_fold_kernel on M' rows followed by the dueling fold of dist_dueling.hip (the unfold: the reverse), without the M'-row
//       vector in between.  Workgroups [0, l1_blocks) own W1 | b1 and stage only the a and b factors; the others own the head, stage
//       only c and d, and give one thread one (k, j): it forms the 1 + na noisy weights fmaf(sigma, xi, mu) of its atom in registers and
//       combines them (the unfold: dmu and dsigma = g xi of the 1 + na rows from the same registers).
// No float atomics, no cross-lane sums: two calls on the same inputs give the same bytes.
#include "dist_host.h"    // dist_device.h; the lists of bounds
#include "head_device.h"  // normal_draw_pair
#include "dist_dueling_device.h"  // the dueling combine (the DUEL axis of the plan kernel, the fused noisy dueling folds)

namespace rlhip {

constexpr uint32_t TAG_NOISY_ACT = 12, TAG_NOISY_ONLINE = 13, TAG_NOISY_TARGET = 14;  // (9..11 are the IQN level draws)
// factor q of a net: the index does not depend on the shape, and every region starts on an even index (a Philox block serves q, q + 1)
constexpr int NZ_QA = 0, NZ_QB = 16, NZ_QC = 16 + 256, NZ_QD = 16 + 2 * 256, NZ_QN = 16 + 3 * 256;
constexpr int NZ_THREADS = 256;
#ifndef RLHIP_NOISY_TILE
#define RLHIP_NOISY_TILE 8  // envs per workgroup of the plan kernel (profiles/noisy.md has the A/B against 16)
#endif
constexpr int NZ_PT = RLHIP_NOISY_TILE;
constexpr int NZ_FOLD_MAX_BLOCKS = 64;

__device__ __forceinline__ float noisy_f(float e) { return copysignf(sqrtf(fabsf(e)), e); }

// f of factors q and q + 1 (q even) of (seed, id, step) under `tag`
__device__ __forceinline__ void noisy_factor_pair(uint64_t seed, uint32_t id, uint32_t step, int q, uint32_t tag, float& f0, float& f1) {
    float e0, e1;
    normal_draw_pair(seed, id, step, q, e0, e1, tag);
    f0 = noisy_f(e0), f1 = noisy_f(e1);
}

struct NoisyPlanArgs {
    const float* noisy;
    const float* obs;
    DistPlanOut out;  // rows_raw: logits, rows_out: probabilities
    int ns, h, na, n_atoms;
    float v_min, delta;
};

// rows m of SPT envs starting at i0: lmu = b2mu[m], fmaf(W2mu[m, j], hid[j], .);  lsg = b2sg[m], fmaf(W2sg[m, j], v[j], .), both over j
// ascending;  l = fmaf(d[m], lsg, lmu), where d[m] of env i waits in l_l[i][m] and is replaced by l
template <int T, int SPT, int WCH>
__device__ __forceinline__ void noisy_logits(const float* __restrict__ Pm, const float* __restrict__ Ps, int ns, int h, int M, int m, int i0,
                                             const float* l_h, const float* l_v, float* l_l, int ls) {
    static_assert(SPT % 4 == 0 && WCH % 4 == 0, "the hidden values of a thread's envs are read as float4; h is a multiple of 4");
    const float* Wm = Pm + h * ns + h;
    const float* Ws = Ps + h * ns + h;
    float am[SPT], as[SPT];
    const float bm = Wm[M * h + m], bs = Ws[M * h + m];
#pragma unroll
    for (int s = 0; s < SPT; ++s) am[s] = bm, as[s] = bs;
    // both rows come from L2 in chunks of WCH weights, the next chunk requested before the current one is used (dist_rows' scheme);
    // weights beyond h are read from a clamped index and never used
    float cm[WCH], cs[WCH], nm[WCH], nsg[WCH];
#pragma unroll
    for (int u = 0; u < WCH; ++u) {
        const int o = m + M * (u < h ? u : h - 1);
        cm[u] = Wm[o], cs[u] = Ws[o];
    }
    for (int j0 = 0; j0 < h; j0 += WCH) {
#pragma unroll
        for (int u = 0; u < WCH; ++u) {
            const int jn = j0 + WCH + u;
            const int o = m + M * (jn < h ? jn : h - 1);
            nm[u] = Wm[o], nsg[u] = Ws[o];
        }
#pragma unroll
        for (int u = 0; u < WCH; ++u) {
            if (j0 + (u & ~3) < h) {  // (uniform; h is a multiple of 4)
                const float wm = cm[u], ws = cs[u];
                const float4* hv = reinterpret_cast<const float4*>(l_h + (j0 + u) * T + i0);
                const float4* vv = reinterpret_cast<const float4*>(l_v + (j0 + u) * T + i0);
#pragma unroll
                for (int v = 0; v < SPT / 4; ++v) {
                    const float4 t = hv[v], r = vv[v];
                    am[4 * v] = fmaf(wm, t.x, am[4 * v]);
                    am[4 * v + 1] = fmaf(wm, t.y, am[4 * v + 1]);
                    am[4 * v + 2] = fmaf(wm, t.z, am[4 * v + 2]);
                    am[4 * v + 3] = fmaf(wm, t.w, am[4 * v + 3]);
                    as[4 * v] = fmaf(ws, r.x, as[4 * v]);
                    as[4 * v + 1] = fmaf(ws, r.y, as[4 * v + 1]);
                    as[4 * v + 2] = fmaf(ws, r.z, as[4 * v + 2]);
                    as[4 * v + 3] = fmaf(ws, r.w, as[4 * v + 3]);
                }
            }
        }
#pragma unroll
        for (int u = 0; u < WCH; ++u) cm[u] = nm[u], cs[u] = nsg[u];
    }
#pragma unroll
    for (int s = 0; s < SPT; ++s) {
        float* l = l_l + (i0 + s) * ls + m;
        *l = fmaf(*l, as[s], am[s]);
    }
}

template <int ACT, int T, bool DUEL = false>
__global__ __launch_bounds__(NZ_THREADS) void noisy_c51_plan_kernel(NoisyPlanArgs g) {
    constexpr int NT = NZ_THREADS, LS = DIST_MAXM + 1;
    static_assert(16 * T <= NT && MAXO * T <= NT && T % 8 == 0, "thread maps of the tile; half a tile is a multiple of 4 envs");
    // LDS: static, sized for h = 256 and 256 rows (26 KB at T = 8, 51 KB at T = 16), so that every address is an immediate
    __shared__ float l_x[16 * T], l_a[16 * T];                                     // [k][T]: the observation, f of the input factors
    __shared__ __attribute__((aligned(16))) float l_h[DIST_HMAX * T];               // [j][T]: hid
    __shared__ __attribute__((aligned(16))) float l_v[DIST_HMAX * T];               // [j][T]: c .* hid
    __shared__ float l_l[T * LS];                                                  // [i][m]: d, then logits, then probabilities
    __shared__ float l_q[MAXO * T];
    const int tid = threadIdx.x;
    // M: the rows the network computes -- with DUEL the na K advantage rows and the K value rows (<= 256: they fit the logit tile)
    const int ns = g.ns, h = g.h, na = g.na, n_atoms = g.n_atoms, M = (DUEL ? na + 1 : na) * n_atoms;
    const int64_t e0 = (int64_t)blockIdx.x * T;
    const int nv = (int)(g.out.n - e0 < T ? g.out.n - e0 : T);
    const uint32_t id0 = g.out.env_id_base + (uint32_t)e0;  // (wraps: the env id is a 32-bit counter word)
    const float* Pm = g.noisy;
    const float* Ps = g.noisy + mlp2_nparams(ns, h, M);
    dist_load_obs<T>(g.obs, g.out.n, e0, nv, ns, l_x);
    // ---- phase A: a -> l_a, d -> the logit slots (a slot of an env beyond nv is drawn too: it is never stored)
    {
        const int npa = (ns + 1) >> 1, npd = (M + 1) >> 1;
        for (int q = tid; q < (npa + npd) * T; q += NT) {
            const int i = q % T, p = q / T;
            const int m0 = 2 * (p - npa);
            float f0, f1;  // (one draw call for both regions: a wave that holds both kinds does not run it twice)
            noisy_factor_pair(g.out.seed, id0 + (uint32_t)i, g.out.step, p < npa ? NZ_QA + 2 * p : NZ_QD + m0, TAG_NOISY_ACT, f0, f1);
            if (p < npa) {
                l_a[(2 * p) * T + i] = f0, l_a[(2 * p + 1) * T + i] = f1;  // (2 p + 1 <= 15)
            } else {
                l_l[i * LS + m0] = f0;
                if (m0 + 1 < M) l_l[i * LS + m0 + 1] = f1;
            }
        }
    }
    __syncthreads();
    // ---- phase B: layer 1, thread = (env i, hidden units j0, j0 + 1)
    for (int q = tid; q < (h >> 1) * T; q += NT) {
        const int i = q % T, j0 = 2 * (q / T);
        // branch-free as in dist_layer1: a weight beyond ns is read from a clamped index and its fmaf dropped by a select
        float wm0[16], wm1[16], ws0[16], ws1[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const int o = j0 + h * (k < ns ? k : 0);
            wm0[k] = Pm[o], wm1[k] = Pm[o + 1], ws0[k] = Ps[o], ws1[k] = Ps[o + 1];
        }
        float zm0 = Pm[h * ns + j0], zm1 = Pm[h * ns + j0 + 1], zs0 = Ps[h * ns + j0], zs1 = Ps[h * ns + j0 + 1];
        // the output factors of layer 1 and the input factors of layer 2 of these two units: in registers, under the loads above
        float b0, b1, c0, c1;
        noisy_factor_pair(g.out.seed, id0 + (uint32_t)i, g.out.step, NZ_QB + j0, TAG_NOISY_ACT, b0, b1);
        noisy_factor_pair(g.out.seed, id0 + (uint32_t)i, g.out.step, NZ_QC + j0, TAG_NOISY_ACT, c0, c1);
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const float x = l_x[k * T + i];
            const float u = l_a[k * T + i] * x;
            const float tm0 = fmaf(wm0[k], x, zm0), tm1 = fmaf(wm1[k], x, zm1);
            const float ts0 = fmaf(ws0[k], u, zs0), ts1 = fmaf(ws1[k], u, zs1);
            zm0 = (k < ns) ? tm0 : zm0, zm1 = (k < ns) ? tm1 : zm1;
            zs0 = (k < ns) ? ts0 : zs0, zs1 = (k < ns) ? ts1 : zs1;
        }
        const float h0 = act_fwd_t<ACT>(fmaf(b0, zs0, zm0)), h1 = act_fwd_t<ACT>(fmaf(b1, zs1, zm1));
        l_h[j0 * T + i] = h0, l_h[(j0 + 1) * T + i] = h1;
        l_v[j0 * T + i] = c0 * h0, l_v[(j0 + 1) * T + i] = c1 * h1;
    }
    __syncthreads();
    // ---- logits, thread = row m
    if (M <= NT / 2) {  // (uniform) two halves of the workgroup, half of the tile's envs each
        const int m = tid & (NT / 2 - 1);
        if (m < M) noisy_logits<T, T / 2, 8>(Pm, Ps, ns, h, M, m, (tid / (NT / 2)) * (T / 2), l_h, l_v, l_l, LS);
    } else if (tid < M) {
        noisy_logits<T, T, 4>(Pm, Ps, ns, h, M, tid, 0, l_h, l_v, l_l, LS);
    }
    __syncthreads();
    if constexpr (DUEL) {  // the combine in the logit tile, thread = (env i, atom k): the value row na K + k joins the na rows k + K o
        for (int q = tid; q < n_atoms * T; q += NT) {
            const int i = q % T, k = q / T;
            float* l = l_l + i * LS + k;
            float x[MAXO] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int o = 0; o < MAXO; ++o)
                if (o < na) x[o] = l[n_atoms * o];
            dist_duel_combine(l[n_atoms * na], x, na);
#pragma unroll
            for (int o = 0; o < MAXO; ++o)
                if (o < na) l[n_atoms * o] = x[o];
        }
        __syncthreads();
    }
    dist_plan_tail<T, NT, LS, true>(g.out, e0, nv, na, n_atoms, l_l, l_q, [&](float* l) { return c51_probs_q<1>(l, n_atoms, g.v_min, g.delta); });
}

// ------------------------------------------------------------------------------------------------------------- fold / unfold / init
struct NoisyFoldArgs {
    const float* src[2];  // fold: the noisy vectors [mu | sigma];  unfold: the gradient of the effective vector
    float* dst[2];        // fold: the effective vectors;            unfold: the gradient of the noisy vector [dmu | dsigma]
    uint32_t tag[2];
    int vec[2][3];        // 16-byte aligned: {src, src + np, dst} (fold), {src, dst, dst + np} (unfold)
    int64_t np;
    int ns, h, M;
    uint64_t seed;
    uint32_t counter;
};

// f of every factor of (seed, id = 0, step = counter) under `tag` -> l_f[q], by the whole workgroup (the caller's barrier publishes them)
// `layers`: bit 0 the factors of layer 1 (a, b), bit 1 those of layer 2 (c, d)
__device__ __forceinline__ void noisy_stage_factors(float* l_f, int ns, int h, int M, uint64_t seed, uint32_t counter, uint32_t tag,
                                                    int layers = 3) {
    for (int p = threadIdx.x; p < NZ_QN / 2; p += NZ_THREADS) {
        const int q = 2 * p;
        const bool used = ((layers & 1) && (q < ns || (q >= NZ_QB && q < NZ_QB + h))) ||
                          ((layers & 2) && ((q >= NZ_QC && q < NZ_QC + h) || (q >= NZ_QD && q < NZ_QD + M)));
        if (used) noisy_factor_pair(seed, 0u, counter, q, tag, l_f[q], l_f[q + 1]);
    }
}

// xi of element p of the mlp2 layout: f_out[o] * f_in[i] (ONE product) for a weight, f_out[o] for a bias
__device__ __forceinline__ float noisy_xi(const float* l_f, int64_t p64, int ns, int h, int M) {
    int p = (int)p64;
    if (p < h * ns) return l_f[NZ_QB + p % h] * l_f[NZ_QA + p / h];
    p -= h * ns;
    if (p < h) return l_f[NZ_QB + p];
    p -= h;
    if (p < M * h) return l_f[NZ_QD + p % M] * l_f[NZ_QC + p / M];
    return l_f[NZ_QD + p - M * h];
}

// n <= 4 floats at p: one 16-byte access where the pointer allows it and the quad is whole
__device__ __forceinline__ void nz_load4(const float* __restrict__ p, int n, int vec, float v[4]) {
    if (vec && n == 4) {
        const float4 t = *reinterpret_cast<const float4*>(p);
        v[0] = t.x, v[1] = t.y, v[2] = t.z, v[3] = t.w;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = k < n ? p[k] : 0.f;
    }
}
__device__ __forceinline__ void nz_store4(float* __restrict__ p, int n, int vec, const float v[4]) {
    if (vec && n == 4) {
        *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (k < n) p[k] = v[k];
    }
}

// noisy = [mu | sigma] -> eff = fmaf(sigma, xi, mu)
__global__ __launch_bounds__(NZ_THREADS) void noisy_fold_kernel(NoisyFoldArgs g) {
    __shared__ float l_f[NZ_QN];
    const int net = blockIdx.y;
    const float* __restrict__ mu = g.src[net];
    const float* __restrict__ sg = mu + g.np;
    float* __restrict__ eff = g.dst[net];
    noisy_stage_factors(l_f, g.ns, g.h, g.M, g.seed, g.counter, g.tag[net]);
    __syncthreads();
    for (int64_t i = 4 * ((int64_t)blockIdx.x * NZ_THREADS + threadIdx.x); i < g.np; i += 4 * (int64_t)gridDim.x * NZ_THREADS) {
        const int n = (int)(g.np - i < 4 ? g.np - i : 4);
        float m[4], s[4], e[4];
        nz_load4(mu + i, n, g.vec[net][0], m);
        nz_load4(sg + i, n, g.vec[net][1], s);
#pragma unroll
        for (int k = 0; k < 4; ++k) e[k] = k < n ? fmaf(s[k], noisy_xi(l_f, i + k, g.ns, g.h, g.M), m[k]) : 0.f;
        nz_store4(eff + i, n, g.vec[net][2], e);
    }
}

// g = the gradient of eff -> [dmu = g | dsigma = g * xi], the online draws regenerated
__global__ __launch_bounds__(NZ_THREADS) void noisy_unfold_kernel(NoisyFoldArgs g) {
    __shared__ float l_f[NZ_QN];
    const float* __restrict__ ge = g.src[0];
    float* __restrict__ dmu = g.dst[0];
    float* __restrict__ dsg = dmu + g.np;
    noisy_stage_factors(l_f, g.ns, g.h, g.M, g.seed, g.counter, g.tag[0]);
    __syncthreads();
    for (int64_t i = 4 * ((int64_t)blockIdx.x * NZ_THREADS + threadIdx.x); i < g.np; i += 4 * (int64_t)gridDim.x * NZ_THREADS) {
        const int n = (int)(g.np - i < 4 ? g.np - i : 4);
        float v[4], d[4];
        nz_load4(ge + i, n, g.vec[0][0], v);
#pragma unroll
        for (int k = 0; k < 4; ++k) d[k] = k < n ? v[k] * noisy_xi(l_f, i + k, g.ns, g.h, g.M) : 0.f;
        nz_store4(dmu + i, n, g.vec[0][1], v);
        nz_store4(dsg + i, n, g.vec[0][2], d);
    }
}

// ------------------------------------------------------------------------------------------- the fused noisy dueling fold / unfold
struct NoisyDuelArgs {
    const float* src[2];  // fold: the noisy dueling vectors [mu | sigma], M' rows;  unfold: the gradient of the effective vector, M rows
    float* dst[2];        // fold: the effective vectors, M rows;                    unfold: the gradient [dmu | dsigma], M' rows
    uint32_t tag[2];
    int vec[2][3];        // 16-byte aligned: {src, src + np', dst} (fold), {src, dst, dst + np'} (unfold)
    int npd;              // np' = mlp2_nparams(ns, h, M'): the length of one half of the noisy vector
    int nbase;            // h ns + h: W1 | b1, at the same offset in every layout
    int l1_blocks;        // workgroups [0, l1_blocks) own W1 | b1, the rest the head
    int ns, h, na, K;
    uint64_t seed;
    uint32_t counter;
};

// the (k, j) items of the head, (h + 1) K of them (j = h: the bias column), strided over the head's workgroups
#define NOISY_DUEL_HEAD_LOOP(g, k, j)                                                                                    \
    for (int t_ = ((int)blockIdx.x - (g).l1_blocks) * NZ_THREADS + (int)threadIdx.x, j = t_ / (g).K, k = t_ - j * (g).K; \
         t_ < ((g).h + 1) * (g).K; t_ += ((int)gridDim.x - (g).l1_blocks) * NZ_THREADS, j = t_ / (g).K, k = t_ - j * (g).K)

// xi of row m of column j of a head: d[m] c[j] (ONE product, noisy_xi's), d[m] in the bias column
__device__ __forceinline__ float noisy_head_xi(const float* l_f, int m, int j, int h) {
    const float d = l_f[NZ_QD + m];
    return j < h ? d * l_f[NZ_QC + j] : d;
}

// noisy = [mu | sigma] on M' = (1 + na) K rows -> eff on M = na K rows: fmaf(sigma, xi, mu) per element, then the dueling combine
__global__ __launch_bounds__(NZ_THREADS) void noisy_dueling_fold_kernel(NoisyDuelArgs g) {
    __shared__ float l_f[NZ_QN];
    const int net = blockIdx.y;
    const float* __restrict__ mu = g.src[net];
    const float* __restrict__ sg = mu + g.npd;
    float* __restrict__ eff = g.dst[net];
    const int na = g.na, K = g.K, M = na * K, Mp = M + K;
    const bool head = (int)blockIdx.x >= g.l1_blocks;
    noisy_stage_factors(l_f, g.ns, g.h, Mp, g.seed, g.counter, g.tag[net], head ? 2 : 1);
    __syncthreads();
    if (!head) {  // W1 | b1: noisy_fold_kernel's lines on the first nbase elements
        for (int i = 4 * ((int)blockIdx.x * NZ_THREADS + (int)threadIdx.x); i < g.nbase; i += 4 * g.l1_blocks * NZ_THREADS) {
            const int n = g.nbase - i < 4 ? g.nbase - i : 4;
            float m[4], s[4], e[4];
            nz_load4(mu + i, n, g.vec[net][0], m);
            nz_load4(sg + i, n, g.vec[net][1], s);
#pragma unroll
            for (int u = 0; u < 4; ++u) e[u] = u < n ? fmaf(s[u], noisy_xi(l_f, i + u, g.ns, g.h, Mp), m[u]) : 0.f;
            nz_store4(eff + i, n, g.vec[net][2], e);
        }
        return;
    }
    NOISY_DUEL_HEAD_LOOP(g, k, j) {
        const int in = g.nbase + j * Mp + k;  // row k of column j; the rows of atom k are K apart, its value row is the last
        float w[MAXO] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int o = 0; o < MAXO; ++o)
            if (o < na) w[o] = fmaf(sg[in + K * o], noisy_head_xi(l_f, k + K * o, j, g.h), mu[in + K * o]);
        dist_duel_combine(fmaf(sg[in + M], noisy_head_xi(l_f, M + k, j, g.h), mu[in + M]), w, na);
        float* out = eff + g.nbase + j * M + k;
#pragma unroll
        for (int o = 0; o < MAXO; ++o)
            if (o < na) out[K * o] = w[o];
    }
}

// g = the gradient of eff (M rows) -> [dmu | dsigma = dmu * xi] on M' rows, the online draws regenerated
__global__ __launch_bounds__(NZ_THREADS) void noisy_dueling_unfold_kernel(NoisyDuelArgs g) {
    __shared__ float l_f[NZ_QN];
    const float* __restrict__ ge = g.src[0];
    float* __restrict__ dmu = g.dst[0];
    float* __restrict__ dsg = dmu + g.npd;
    const int na = g.na, K = g.K, M = na * K, Mp = M + K;
    const bool head = (int)blockIdx.x >= g.l1_blocks;
    noisy_stage_factors(l_f, g.ns, g.h, Mp, g.seed, g.counter, g.tag[0], head ? 2 : 1);
    __syncthreads();
    if (!head) {  // gW1 | gb1: noisy_unfold_kernel's lines on the first nbase elements
        for (int i = 4 * ((int)blockIdx.x * NZ_THREADS + (int)threadIdx.x); i < g.nbase; i += 4 * g.l1_blocks * NZ_THREADS) {
            const int n = g.nbase - i < 4 ? g.nbase - i : 4;
            float v[4], d[4];
            nz_load4(ge + i, n, g.vec[0][0], v);
#pragma unroll
            for (int u = 0; u < 4; ++u) d[u] = u < n ? v[u] * noisy_xi(l_f, i + u, g.ns, g.h, Mp) : 0.f;
            nz_store4(dmu + i, n, g.vec[0][1], v);
            nz_store4(dsg + i, n, g.vec[0][2], d);
        }
        return;
    }
    NOISY_DUEL_HEAD_LOOP(g, k, j) {
        const float* in = ge + g.nbase + j * M + k;
        float x[MAXO] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int o = 0; o < MAXO; ++o)
            if (o < na) x[o] = in[K * o];
        const float s = dist_duel_uncombine(x, na);
        const int out = g.nbase + j * Mp + k;
#pragma unroll
        for (int o = 0; o < MAXO; ++o)
            if (o < na) dmu[out + K * o] = x[o], dsg[out + K * o] = x[o] * noisy_head_xi(l_f, k + K * o, j, g.h);
        dmu[out + M] = s, dsg[out + M] = s * noisy_head_xi(l_f, M + k, j, g.h);
    }
}

// mu = (2 u - 1) / sqrt(fan_in), sigma = sigma0 / sqrt(fan_in); u by the rule of mlp2_init_kernel, tensor ids 0: W1, 1: b1, 2: W2, 3: b2
__global__ __launch_bounds__(256) void noisy_init_kernel(float* __restrict__ p, int ns, int h, int M, uint64_t seed, uint32_t net_id,
                                                         float sigma0) {
    const int64_t np = mlp2_nparams(ns, h, M);
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= np) return;
    const int64_t o1 = (int64_t)h * ns, o2 = o1 + h, o3 = o2 + (int64_t)M * h;
    const uint32_t tensor = q < o1 ? 0u : (q < o2 ? 1u : (q < o3 ? 2u : 3u));
    const int64_t off = q < o1 ? q : (q < o2 ? q - o1 : (q < o3 ? q - o2 : q - o3));
    const float rt = sqrtf((float)(q < o2 ? ns : h));
    const u32x4 w = philox4x32_10(seed, (uint32_t)off, 0, net_id * 4u + tensor, TAG_INIT);
    p[q] = (2.0f * u01_f32(w.x) - 1.0f) / rt;
    p[np + q] = sigma0 / rt;
}

// the bounds of a noisy net of M output rows, stated once (dist_host.h: a list of bounds hands each one to B)
#define NOISY_NET_BOUNDS(B, M)                                                           \
    B(ns >= 2 && ns <= 16, "obs dim must be 2..16");                                     \
    B(h >= 4 && h <= DIST_HMAX && h % 4 == 0, "hidden must be a multiple of 4, <= 256"); \
    B((M) >= 2 && (M) <= DIST_MAXM, "the network has 2..256 output rows")

static bool noisy_net_ok(int64_t ns, int64_t h, int64_t n_out) {
    NOISY_NET_BOUNDS(DIST_BOUND_HOLDS, n_out);
    return true;
}

static inline int nz_aligned16(const void* p) { return (((uintptr_t)p) & 15) == 0; }
static inline bool nz_overlap(const float* a, int64_t na, const float* b, int64_t nb) {
    return (uintptr_t)a < (uintptr_t)(b + nb) && (uintptr_t)b < (uintptr_t)(a + na);
}
static inline int nz_fold_blocks(int64_t np) {
    const int64_t b = (np + 4 * NZ_THREADS - 1) / (4 * NZ_THREADS);
    return (int)(b < NZ_FOLD_MAX_BLOCKS ? b : NZ_FOLD_MAX_BLOCKS);
}

}  // namespace rlhip

using namespace rlhip;

#define NOISY_REQUIRE_NET(M) NOISY_NET_BOUNDS(RLHIP_REQUIRE, M)

#define NOISY_REQUIRE_SHAPE()                                                                       \
    NOISY_REQUIRE_NET(na * n_atoms);                                                                \
    RLHIP_REQUIRE(na >= 1 && na <= MAXO, "na must be 1..4");                                        \
    RLHIP_REQUIRE(n_atoms >= 2 && n_atoms <= DIST_MAXK, "n_atoms must be 2..64");                    \
    RLHIP_REQUIRE(act == 0 || act == 1, "act must be 0 (relu) or 1 (tanh)");                        \
    RLHIP_REQUIRE(std::isfinite(v_min) && std::isfinite(v_max) && v_min < v_max, "the support needs finite v_min < v_max")

// a noisy dueling C51 net: K = n_atoms in 2..64, (1 + na) K <= 256 rows
#define NOISY_REQUIRE_DUEL_SHAPE()                                                                  \
    DIST_DUEL_BOUNDS(RLHIP_REQUIRE, 2);                                                             \
    RLHIP_REQUIRE(act == 0 || act == 1, "act must be 0 (relu) or 1 (tanh)");                        \
    RLHIP_REQUIRE(std::isfinite(v_min) && std::isfinite(v_max) && v_min < v_max, "the support needs finite v_min < v_max")

// the arguments of a fused noisy dueling launch and its grid: l1_blocks workgroups for W1 | b1, then the head's
static int noisy_duel_args(NoisyDuelArgs& g, int64_t ns, int64_t h, int64_t na, int64_t K, uint64_t seed, uint32_t counter) {
    g.npd = (int)mlp2_nparams(ns, h, (1 + na) * K), g.nbase = (int)(h * ns + h);
    g.ns = (int)ns, g.h = (int)h, g.na = (int)na, g.K = (int)K, g.seed = seed, g.counter = counter;
    g.l1_blocks = nz_fold_blocks(g.nbase);
    return g.l1_blocks + nz_fold_blocks(4 * (h + 1) * K);  // (a head thread owns one (k, j), not a quad)
}

static int32_t noisy_plan_launch(const float* noisy, int64_t ns, int64_t h, int64_t na, int64_t n_atoms, int32_t act, float v_min,
                                 float v_max, const float* obs, int64_t n, double eps, uint64_t seed, uint32_t env_id_base, uint32_t step,
                                 int32_t* actions, float* q_out, float* probs_out, float* logits_out, rlhip_stream_t stream,
                                 bool duel = false) {
    NoisyPlanArgs g;
    g.noisy = noisy, g.obs = obs, g.out = DistPlanOut{q_out, logits_out, probs_out, actions, n, eps, seed, env_id_base, step};
    g.ns = (int)ns, g.h = (int)h, g.na = (int)na, g.n_atoms = (int)n_atoms;
    g.v_min = v_min, g.delta = (v_max - v_min) / (float)(n_atoms - 1);
    const dim3 grid((unsigned)((n + NZ_PT - 1) / NZ_PT));
    // the instantiation set: ACT in {0, 1} x DUEL in {false, true}
    if (duel) {
        if (act == 0) hipLaunchKernelGGL((noisy_c51_plan_kernel<0, NZ_PT, true>), grid, dim3(NZ_THREADS), 0, as_stream(stream), g);
        else hipLaunchKernelGGL((noisy_c51_plan_kernel<1, NZ_PT, true>), grid, dim3(NZ_THREADS), 0, as_stream(stream), g);
    } else if (act == 0) hipLaunchKernelGGL((noisy_c51_plan_kernel<0, NZ_PT>), grid, dim3(NZ_THREADS), 0, as_stream(stream), g);
    else hipLaunchKernelGGL((noisy_c51_plan_kernel<1, NZ_PT>), grid, dim3(NZ_THREADS), 0, as_stream(stream), g);
    RLHIP_LAUNCH_CHECK();
    return RLHIP_OK;
}

extern "C" {

int64_t rlhip_noisy_nparams(int64_t ns, int64_t h, int64_t n_out) {
    return noisy_net_ok(ns, h, n_out) ? 2 * mlp2_nparams(ns, h, n_out) : -1;
}

int64_t rlhip_noisy_plan_tile(void) { return NZ_PT; }

int32_t rlhip_noisy_init_f32(float* params, int64_t ns, int64_t h, int64_t n_out, uint64_t seed, uint32_t net_id, float sigma0,
                             rlhip_stream_t stream) {
    NOISY_REQUIRE_NET(n_out);
    RLHIP_REQUIRE(params != nullptr, "NULL argument");
    RLHIP_REQUIRE(std::isfinite(sigma0) && sigma0 >= 0.f, "sigma0 must be finite and >= 0");
    const int64_t np = mlp2_nparams(ns, h, n_out);
    hipLaunchKernelGGL(noisy_init_kernel, dim3((unsigned)((np + 255) / 256)), dim3(256), 0, as_stream(stream), params, (int)ns, (int)h,
                       (int)n_out, seed, net_id, sigma0);
    RLHIP_LAUNCH_CHECK();
    return RLHIP_OK;
}

int32_t rlhip_noisy_c51_forward_f32(const float* noisy, int64_t ns, int64_t h, int64_t na, int64_t n_atoms, int32_t act, float v_min,
                                    float v_max, const float* obs, int64_t n, uint64_t seed, uint32_t env_id_base, uint32_t step,
                                    float* q_out, float* probs_out, float* logits_out, rlhip_stream_t stream) {
    NOISY_REQUIRE_SHAPE();
    RLHIP_REQUIRE(n >= 0 && n <= 0x7fffffffLL, "env count must be 0 .. 2^31 - 1");
    RLHIP_REQUIRE(noisy && obs && q_out, "NULL argument");
    if (n == 0) return RLHIP_OK;
    return noisy_plan_launch(noisy, ns, h, na, n_atoms, act, v_min, v_max, obs, n, 0.0, seed, env_id_base, step, nullptr, q_out, probs_out,
                             logits_out, stream);
}

int32_t rlhip_noisy_c51_plan_f32(const float* noisy, int64_t ns, int64_t h, int64_t na, int64_t n_atoms, int32_t act, float v_min,
                                 float v_max, const float* obs, int64_t n, double eps, uint64_t seed, uint32_t env_id_base, uint32_t step,
                                 int32_t* actions, float* q_out, rlhip_stream_t stream) {
    NOISY_REQUIRE_SHAPE();
    RLHIP_REQUIRE(n >= 0 && n <= 0x7fffffffLL, "env count must be 0 .. 2^31 - 1");
    RLHIP_REQUIRE(noisy && obs && actions, "NULL argument");
    if (n == 0) return RLHIP_OK;
    return noisy_plan_launch(noisy, ns, h, na, n_atoms, act, v_min, v_max, obs, n, eps, seed, env_id_base, step, actions, q_out, nullptr,
                             nullptr, stream);
}

int32_t rlhip_noisy_fold_f32(const float* noisy, float* eff, const float* noisy2, float* eff2, int64_t ns, int64_t h, int64_t n_out,
                             uint64_t seed, uint32_t counter, rlhip_stream_t stream) {
    NOISY_REQUIRE_NET(n_out);
    RLHIP_REQUIRE(noisy && eff, "NULL argument");
    RLHIP_REQUIRE((noisy2 == nullptr) == (eff2 == nullptr), "the second net is a pair: both noisy2 and eff2, or neither");
    const int64_t np = mlp2_nparams(ns, h, n_out);
    RLHIP_REQUIRE(!nz_overlap(eff, np, noisy, 2 * np), "eff must not overlap the noisy vector");
    RLHIP_REQUIRE(!noisy2 || (!nz_overlap(eff2, np, noisy2, 2 * np) && !nz_overlap(eff2, np, eff, np) && !nz_overlap(eff2, np, noisy, 2 * np) &&
                              !nz_overlap(eff, np, noisy2, 2 * np)),
                  "the second pair must not overlap the first pair's output or its own input");
    NoisyFoldArgs g;
    g.np = np, g.ns = (int)ns, g.h = (int)h, g.M = (int)n_out, g.seed = seed, g.counter = counter;
    g.src[0] = noisy, g.dst[0] = eff, g.tag[0] = TAG_NOISY_ONLINE;
    g.src[1] = noisy2, g.dst[1] = eff2, g.tag[1] = TAG_NOISY_TARGET;
    for (int k = 0; k < 2; ++k) {
        g.vec[k][0] = g.src[k] ? nz_aligned16(g.src[k]) : 0;
        g.vec[k][1] = g.src[k] ? nz_aligned16(g.src[k] + np) : 0;
        g.vec[k][2] = g.dst[k] ? nz_aligned16(g.dst[k]) : 0;
    }
    hipLaunchKernelGGL(noisy_fold_kernel, dim3(nz_fold_blocks(np), noisy2 ? 2 : 1), dim3(NZ_THREADS), 0, as_stream(stream), g);
    RLHIP_LAUNCH_CHECK();
    return RLHIP_OK;
}

int32_t rlhip_noisy_unfold_grad_f32(const float* grad_eff, float* grad_noisy, int64_t ns, int64_t h, int64_t n_out, uint64_t seed,
                                    uint32_t counter, rlhip_stream_t stream) {
    NOISY_REQUIRE_NET(n_out);
    RLHIP_REQUIRE(grad_eff && grad_noisy, "NULL argument");
    const int64_t np = mlp2_nparams(ns, h, n_out);
    RLHIP_REQUIRE(!nz_overlap(grad_noisy, 2 * np, grad_eff, np), "grad_noisy must not overlap grad_eff");
    NoisyFoldArgs g;
    g.np = np, g.ns = (int)ns, g.h = (int)h, g.M = (int)n_out, g.seed = seed, g.counter = counter;
    g.src[0] = grad_eff, g.dst[0] = grad_noisy, g.tag[0] = TAG_NOISY_ONLINE;
    g.src[1] = nullptr, g.dst[1] = nullptr, g.tag[1] = 0;
    g.vec[0][0] = nz_aligned16(grad_eff), g.vec[0][1] = nz_aligned16(grad_noisy), g.vec[0][2] = nz_aligned16(grad_noisy + np);
    g.vec[1][0] = g.vec[1][1] = g.vec[1][2] = 0;
    hipLaunchKernelGGL(noisy_unfold_kernel, dim3(nz_fold_blocks(np)), dim3(NZ_THREADS), 0, as_stream(stream), g);
    RLHIP_LAUNCH_CHECK();
    return RLHIP_OK;
}

// ---- noisy dueling heads (include/rlhip.h, the dueling distributional section)
int32_t rlhip_noisy_c51_dueling_forward_f32(const float* noisy, int64_t ns, int64_t h, int64_t na, int64_t n_atoms, int32_t act,
                                            float v_min, float v_max, const float* obs, int64_t n, uint64_t seed, uint32_t env_id_base,
                                            uint32_t step, float* q_out, float* probs_out, float* logits_out, rlhip_stream_t stream) {
    const int64_t K = n_atoms;
    NOISY_REQUIRE_DUEL_SHAPE();
    RLHIP_REQUIRE(n >= 0 && n <= 0x7fffffffLL, "env count must be 0 .. 2^31 - 1");
    RLHIP_REQUIRE(noisy && obs && q_out, "NULL argument");
    if (n == 0) return RLHIP_OK;
    return noisy_plan_launch(noisy, ns, h, na, n_atoms, act, v_min, v_max, obs, n, 0.0, seed, env_id_base, step, nullptr, q_out, probs_out,
                             logits_out, stream, true);
}

int32_t rlhip_noisy_c51_dueling_plan_f32(const float* noisy, int64_t ns, int64_t h, int64_t na, int64_t n_atoms, int32_t act, float v_min,
                                         float v_max, const float* obs, int64_t n, double eps, uint64_t seed, uint32_t env_id_base,
                                         uint32_t step, int32_t* actions, float* q_out, rlhip_stream_t stream) {
    const int64_t K = n_atoms;
    NOISY_REQUIRE_DUEL_SHAPE();
    RLHIP_REQUIRE(n >= 0 && n <= 0x7fffffffLL, "env count must be 0 .. 2^31 - 1");
    RLHIP_REQUIRE(noisy && obs && actions, "NULL argument");
    if (n == 0) return RLHIP_OK;
    return noisy_plan_launch(noisy, ns, h, na, n_atoms, act, v_min, v_max, obs, n, eps, seed, env_id_base, step, actions, q_out, nullptr,
                             nullptr, stream, true);
}

int32_t rlhip_noisy_dueling_fold_f32(const float* noisy, float* eff, const float* noisy2, float* eff2, int64_t ns, int64_t h, int64_t na,
                                     int64_t K, uint64_t seed, uint32_t counter, rlhip_stream_t stream) {
    DIST_DUEL_BOUNDS(RLHIP_REQUIRE, 2);
    RLHIP_REQUIRE(noisy && eff, "NULL argument");
    RLHIP_REQUIRE((noisy2 == nullptr) == (eff2 == nullptr), "the second net is a pair: both noisy2 and eff2, or neither");
    NoisyDuelArgs g;
    const int blocks = noisy_duel_args(g, ns, h, na, K, seed, counter);
    const int64_t npd = g.npd, ne = mlp2_nparams(ns, h, na * K);
    RLHIP_REQUIRE(!nz_overlap(eff, ne, noisy, 2 * npd), "eff must not overlap the noisy vector");
    RLHIP_REQUIRE(!noisy2 || (!nz_overlap(eff2, ne, noisy2, 2 * npd) && !nz_overlap(eff2, ne, eff, ne) &&
                              !nz_overlap(eff2, ne, noisy, 2 * npd) && !nz_overlap(eff, ne, noisy2, 2 * npd)),
                  "the second pair must not overlap the first pair's output or its own input");
    g.src[0] = noisy, g.dst[0] = eff, g.tag[0] = TAG_NOISY_ONLINE;
    g.src[1] = noisy2, g.dst[1] = eff2, g.tag[1] = TAG_NOISY_TARGET;
    for (int k = 0; k < 2; ++k) {
        g.vec[k][0] = g.src[k] ? nz_aligned16(g.src[k]) : 0;
        g.vec[k][1] = g.src[k] ? nz_aligned16(g.src[k] + npd) : 0;
        g.vec[k][2] = g.dst[k] ? nz_aligned16(g.dst[k]) : 0;
    }
    hipLaunchKernelGGL(noisy_dueling_fold_kernel, dim3(blocks, noisy2 ? 2 : 1), dim3(NZ_THREADS), 0, as_stream(stream), g);
    RLHIP_LAUNCH_CHECK();
    return RLHIP_OK;
}

int32_t rlhip_noisy_dueling_unfold_grad_f32(const float* grad_eff, float* grad_noisy, int64_t ns, int64_t h, int64_t na, int64_t K,
                                            uint64_t seed, uint32_t counter, rlhip_stream_t stream) {
    DIST_DUEL_BOUNDS(RLHIP_REQUIRE, 2);
    RLHIP_REQUIRE(grad_eff && grad_noisy, "NULL argument");
    NoisyDuelArgs g;
    const int blocks = noisy_duel_args(g, ns, h, na, K, seed, counter);
    const int64_t npd = g.npd;
    RLHIP_REQUIRE(!nz_overlap(grad_noisy, 2 * npd, grad_eff, mlp2_nparams(ns, h, na * K)), "grad_noisy must not overlap grad_eff");
    g.src[0] = grad_eff, g.dst[0] = grad_noisy, g.tag[0] = TAG_NOISY_ONLINE;
    g.src[1] = nullptr, g.dst[1] = nullptr, g.tag[1] = 0;
    g.vec[0][0] = nz_aligned16(grad_eff), g.vec[0][1] = nz_aligned16(grad_noisy), g.vec[0][2] = nz_aligned16(grad_noisy + npd);
    g.vec[1][0] = g.vec[1][1] = g.vec[1][2] = 0;
    hipLaunchKernelGGL(noisy_dueling_unfold_kernel, dim3(blocks), dim3(NZ_THREADS), 0, as_stream(stream), g);
    RLHIP_LAUNCH_CHECK();
    return RLHIP_OK;
}

}  // extern "C"
