// cov_heads.hip -- the full-covariance Gaussian head and the rest of the reference's distribution functions on the device.
//
// Reference: RLCore/src/utils/networks.jl -- CovGaussianNetwork (:221-381: one sample :247-272, K samples per state :300-312,
// (state, action) evaluation :327-343, vec_to_tril / cholesky_columns / softplusbeta / cholesky_matrix_to_vector_index :359-381)
// and RLCore/src/utils/distributions.jl -- mvnormlogpdf (:46-66), logdetLorU (:75-77, the device method), mvnormkldivergence
// (:88-109), diagnormkldivergence (:117-129), normkldivergence (:137-139).
//
// Layouts (Float32, column-major in the reference's sense): mu (da x n), chol_vec (nv x n) with nv = da (da + 1) / 2, L (da x da x n),
// actions (da x K x n), log-probabilities (K x n).  `randn(rng, Float32, da, K, n)` is the shared Philox NORMAL stream exactly as
// heads.hip uses it: element (k, j) of state i is draw k + da * j of (seed, env_id_base + i, step).
//
// ORDER OF OPERATIONS (all Float32, -ffp-contract=off; tests/mvnorm_ref.py replays it):
//   softplusbeta(x) = logf(expf(x / 10.0f) + 1.0f) * 10.0f                 (:360, the naive form)
//   L[i,i] = softplusbeta(v) + 1.0e-5f;  L[i,j] = v for i > j;  0 above the diagonal;  1-based vector index of (i, j):
//       ((2 da - j)(j - 1)) / 2 + i                                          (:359)
//   sample   acc = L[i,1] eps[1];  acc = acc + L[i,j] eps[j], j = 2 ... i;  z[i] = mu[i] + acc
//   solve    dx[i] = x[i] - mu[i];  t = dx[i];  t = t - L[i,j] y[j], j = 1 ... i - 1 ascending;  y[i] = t / L[i,i]
//   logpdf   ld = 0 + logf(L[1,1]) + ... ascending;  logdet = 2 ld;  ss = 0 + y[1] y[1] + ... ascending;
//            out = -(((float)da * log2pi + logdet) + ss) / 2
//   mvn KL   logdet = 2 ld(L2) - 2 ld(L1);  trace = 0 + sum_c sum_{i >= c} w[i,c]^2 with w[:,c] = L2 \ L1[:,c] (columns ascending, rows
//            ascending inside a column; the solve of column c starts at row c: the rows above hold exact zeros);
//            sq = sum_i (L2 \ (mu2 - mu1))[i]^2;  out = (((logdet - (float)da) + trace) + sq) / 2
//   diag KL  v = s s;  logdet = sum logf(v2) - sum logf(v1);  trace = sum v1 / v2;  sq = sum ((mu2 - mu1)(mu2 - mu1)) / v2  (sums from 0,
//            ascending);  out = (((logdet - (float)d) + trace) + sq) / 2
//   1-D KL   ((logf(s2) - logf(s1)) + (s1 s1 + (mu1 - mu2)(mu1 - mu2)) / (2 (s2 s2))) - 0.5f
// Both loops over the columns of L visit a row's terms in ascending j, so the column-wise form below IS the row-wise order above.
//
// Shape of the kernels: one lane per (sample j, state i), da a template argument (1 ... 16) so that L (packed lower triangle), eps
// and y are registers with compile-time indices -- nothing lands in scratch (tests/test_cov_head_kernel_resources.py).  The head
// kernels evaluate softplusbeta once per (state, diagonal) of the block, into LDS, before the lanes of the K samples read it.
// Two layouts of the head exist: every lane walking its own Cholesky vector (cov_head_kernel), and the block's vectors staged through
// LDS with coalesced loads (cov_head_staged_kernel); which one a launch takes was decided by measurement (cov_logp_staged below).
#include "cov_device.h"

namespace rlhip {

// vec_to_tril (:378-381): one lane per element of L, coalesced stores
__global__ __launch_bounds__(256) void vec_to_tril_kernel(const float* __restrict__ chol_vec, int da, int64_t total,
                                                          float* __restrict__ L) {
    const int dd = da * da, nv = (da * (da + 1)) / 2;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int64_t i = e / dd;
        const int rem = (int)(e - i * dd), c = rem / da, r = rem - c * da;
        float o = 0.0f;
        if (r >= c) {
            const float x = chol_vec[i * nv + tril_index(r, c, da)];
            o = r == c ? chol_diag(x) : x;
        }
        L[e] = o;
    }
}

// draws q0 ... q0 + DA - 1 of (seed, id, step): the values of normal_draw, with the Philox block, the log and the square root of a
// pair (2 p, 2 p + 1) evaluated once.  q0 is odd only for odd DA; the parity is resolved by selects, not by indexing.
template <int DA>
__device__ __forceinline__ void normal_draws(uint64_t seed, uint32_t id, uint32_t step, int q0, float (&eps)[DA]) {
    constexpr int M = (DA + 1) / 2;
    const int par = (DA & 1) ? (q0 & 1) : 0;
    float cs[M + 1], sn[M + 1];
#pragma unroll
    for (int m = 0; m < M; ++m) {
        const u32x4 w = philox4x32_10(seed, id, (uint32_t)((q0 >> 1) + m), step, TAG_NORMAL);
        const double u1 = (double)((w.x >> 8) + 1u) * 0x1p-24;
        const double u2 = (double)(w.y >> 8) * 0x1p-24;
        const double r = ::sqrt(-2.0 * ::log(u1));
        const double a = 6.283185307179586 * u2;
        cs[m] = (float)(r * ::cos(a));
        sn[m] = (float)(r * ::sin(a));
    }
    cs[M] = 0.0f;
    sn[M] = 0.0f;
#pragma unroll
    for (int k = 0; k < DA; ++k) {
        const float even = (k & 1) ? sn[k / 2] : cs[k / 2];            // q0 even: draw q0 + k is half (k & 1) of pair k / 2
        const float odd = (k & 1) ? cs[(k + 1) / 2] : sn[k / 2];      // q0 odd: draw q0 + k is half (~k & 1) of pair (k + 1) / 2
        eps[k] = par ? odd : even;
    }
}

// column c of the lower triangle `A` solved against `B`, rows c ... DA - 1: trace += sum of squares (mvnormkldivergence)
template <int DA, int C>
__device__ __forceinline__ float kl_trace_column(const Cov<DA>& L1, const Cov<DA>& L2, float trace) {
    float t[DA];
#pragma unroll
    for (int r = 0; r < DA; ++r) t[r] = r >= C ? L1.T[tril_index(r >= C ? r : C, C, DA)] : 0.0f;
    trace = L2.template solve_sq<C>(t, trace);
    if constexpr (C + 1 < DA) trace = kl_trace_column<DA, C + 1>(L1, L2, trace);
    return trace;
}

template <int DA>
__global__ __launch_bounds__(256) void mvnormlogpdf_kernel(const float* __restrict__ mu, const float* __restrict__ L,
                                                           const float* __restrict__ x, int64_t n, int K,
                                                           float* __restrict__ out) {
    const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (gid >= n * K) return;
    const int64_t i = gid / K;
    Cov<DA> cov;
    cov.from_dense(L + i * (DA * DA));
    float m[DA], xs[DA];
#pragma unroll
    for (int k = 0; k < DA; ++k) {
        m[k] = mu[i * DA + k];
        xs[k] = x[gid * DA + k];
    }
    out[gid] = cov.logpdf(m, xs);
}

// The head: vec_to_tril, then the draw and the product (EVAL = 0) or the given action (EVAL = 1), then the solve and the log-density.
// A block covers 256 consecutive (sample, state) pairs = at most 256 states.
template <int DA, int EVAL>
__global__ __launch_bounds__(256) void cov_head_kernel(const float* __restrict__ mu, const float* __restrict__ chol_vec,
                                                       const float* __restrict__ action_in, int64_t n, int K, uint64_t seed,
                                                       uint32_t env_id_base, uint32_t step, float* __restrict__ action_out,
                                                       float* __restrict__ logp_out, float* __restrict__ L_out) {
    constexpr int NV = Cov<DA>::NV;
    __shared__ float s_diag[DA * 256];  // [diagonal k][state of the block]
    const int64_t total = n * K, g0 = (int64_t)blockIdx.x * 256;
    const int64_t glast = g0 + 255 < total ? g0 + 255 : total - 1;
    const int64_t i0 = g0 / K;
    const int nsl = (int)(glast / K - i0) + 1;
    for (int w = threadIdx.x; w < nsl * DA; w += 256) {
        const int k = w / nsl, s = w - k * nsl;
        s_diag[k * 256 + s] = chol_diag(chol_vec[(i0 + s) * NV + tril_index(k, k, DA)]);
    }
    __syncthreads();
    const int64_t gid = g0 + threadIdx.x;
    if (gid >= total) return;
    const int64_t i = gid / K;
    const int j = (int)(gid - i * K);
    Cov<DA> cov;
    cov.from_vec(chol_vec + i * NV, s_diag + (int)(i - i0), 256);
    if (L_out && j == 0) cov.to_dense(L_out + i * (DA * DA));
    float m[DA], z[DA];
#pragma unroll
    for (int k = 0; k < DA; ++k) m[k] = mu[i * DA + k];
    if (EVAL) {
#pragma unroll
        for (int k = 0; k < DA; ++k) z[k] = action_in[gid * DA + k];
    } else {
        float eps[DA];
        normal_draws<DA>(seed, env_id_base + (uint32_t)i, step, DA * j, eps);
        cov.sample(m, eps, z);
#pragma unroll
        for (int k = 0; k < DA; ++k) action_out[gid * DA + k] = z[k];
    }
    if (logp_out) logp_out[gid] = cov.logpdf(m, z);
}

// The same head with the block's Cholesky vectors staged through LDS: the block's states hold ONE contiguous run of nsl * NV floats,
// read with consecutive lanes on consecutive words, instead of every lane walking its own NV-float vector at a lane stride of NV
// floats.  Rows of the LDS image are padded to an odd stride (no bank conflicts at a lane stride of one row); the workgroup shrinks
// until the image fits 64 KB.  Both forms were built and measured; the library instantiates EVAL = 1 at da = 6 ... 12 only.
template <int DA>
struct CovStage {
    static constexpr int NV = Cov<DA>::NV, NVP = NV | 1;
    static constexpr int BLOCK = NVP * 4 * 256 <= 65536 ? 256 : (NVP * 4 * 128 <= 65536 ? 128 : 64);
};

template <int DA, int EVAL>
__global__ __launch_bounds__(CovStage<DA>::BLOCK) void cov_head_staged_kernel(
    const float* __restrict__ mu, const float* __restrict__ chol_vec, const float* __restrict__ action_in, int64_t n, int K,
    uint64_t seed, uint32_t env_id_base, uint32_t step, float* __restrict__ action_out, float* __restrict__ logp_out,
    float* __restrict__ L_out) {
    constexpr int NV = CovStage<DA>::NV, NVP = CovStage<DA>::NVP, B = CovStage<DA>::BLOCK;
    __shared__ float s_vec[B * NVP];
    const int64_t total = n * K, g0 = (int64_t)blockIdx.x * B;
    const int64_t glast = g0 + (B - 1) < total ? g0 + (B - 1) : total - 1;
    const int64_t i0 = g0 / K;
    const int nsl = (int)(glast / K - i0) + 1;  // <= B states
    const float* __restrict__ src = chol_vec + i0 * NV;
    for (int w = threadIdx.x; w < nsl * NV; w += B) {
        const int s = w / NV, e = w - s * NV;
        s_vec[s * NVP + e] = src[w];
    }
    __syncthreads();
    for (int w = threadIdx.x; w < nsl * DA; w += B) {
        const int k = w / nsl, s = w - k * nsl;
        float* p = &s_vec[s * NVP + tril_index(k, k, DA)];
        *p = chol_diag(*p);
    }
    __syncthreads();
    const int64_t gid = g0 + threadIdx.x;
    if (gid >= total) return;
    const int64_t i = gid / K;
    const int j = (int)(gid - i * K);
    Cov<DA> cov;
    {
        const float* row = s_vec + (int)(i - i0) * NVP;
#pragma unroll
        for (int e = 0; e < NV; ++e) cov.T[e] = row[e];
    }
    if (L_out && j == 0) cov.to_dense(L_out + i * (DA * DA));
    float m[DA], z[DA];
#pragma unroll
    for (int k = 0; k < DA; ++k) m[k] = mu[i * DA + k];
    if (EVAL) {
#pragma unroll
        for (int k = 0; k < DA; ++k) z[k] = action_in[gid * DA + k];
    } else {
        float eps[DA];
        normal_draws<DA>(seed, env_id_base + (uint32_t)i, step, DA * j, eps);
        cov.sample(m, eps, z);
#pragma unroll
        for (int k = 0; k < DA; ++k) action_out[gid * DA + k] = z[k];
    }
    if (logp_out) logp_out[gid] = cov.logpdf(m, z);
}

template <int DA>
__global__ __launch_bounds__(256) void mvnormkl_kernel(const float* __restrict__ mu1, const float* __restrict__ L1,
                                                       const float* __restrict__ mu2, const float* __restrict__ L2, int64_t n,
                                                       float* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    Cov<DA> c1, c2;
    c1.from_dense(L1 + i * (DA * DA));
    c2.from_dense(L2 + i * (DA * DA));
    const float logdet = 2.0f * c2.sum_log_diag() - 2.0f * c1.sum_log_diag();  // :94
    const float trace = kl_trace_column<DA, 0>(c1, c2, 0.0f);                   // :95-100, tr(inv(S2) S1) = |L2 \ L1|_F^2
    float t[DA];
#pragma unroll
    for (int k = 0; k < DA; ++k) t[k] = mu2[i * DA + k] - mu1[i * DA + k];
    const float sq = c2.template solve_sq<0>(t, 0.0f);  // :101
    out[i] = (((logdet - (float)DA) + trace) + sq) / 2.0f;
}

// diagnormkldivergence :117-124, one lane per column
__global__ __launch_bounds__(256) void diagnormkl_kernel(const float* __restrict__ mu1, const float* __restrict__ s1,
                                                         const float* __restrict__ mu2, const float* __restrict__ s2, int d,
                                                         int64_t n, float* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float l1 = 0.0f, l2 = 0.0f, trace = 0.0f, sq = 0.0f;
    for (int k = 0; k < d; ++k) {
        const float a = s1[i * d + k], b = s2[i * d + k], dm = mu2[i * d + k] - mu1[i * d + k];
        const float v1 = a * a, v2 = b * b;
        l2 = l2 + logf(v2);
        l1 = l1 + logf(v1);
        trace = trace + v1 / v2;
        sq = sq + (dm * dm) / v2;
    }
    out[i] = ((((l2 - l1) - (float)d) + trace) + sq) / 2.0f;
}

// normkldivergence :137-139, elementwise
__global__ __launch_bounds__(256) void normkl_kernel(const float* __restrict__ mu1, const float* __restrict__ s1,
                                                     const float* __restrict__ mu2, const float* __restrict__ s2, int64_t n,
                                                     float* __restrict__ out) {
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (int64_t)gridDim.x * 256) {
        const float a = s1[e], b = s2[e], dm = mu1[e] - mu2[e];
        out[e] = ((logf(b) - logf(a)) + (a * a + dm * dm) / (2.0f * (b * b))) - 0.5f;
    }
}

}  // namespace rlhip

using namespace rlhip;

// which layout serves the (state, action) launch: the LDS-staged kernel where it measured faster (K = 1, da = 6 ... 12: 27.6 / 39.6 /
// 80.4 / 114 us against 31.7 / 77.4 / 121 / 150 us at da = 6 / 8 / 10 / 12 and 2^20 states), the per-lane walk everywhere else (da <= 4:
// up to 15 % faster; da = 16, where the staged image forces 64-thread workgroups: 22 % faster; K = 16: 3 - 30 % faster).  The
// sampling launch keeps the per-lane walk at every da: up to da = 12 the two layouts are within 6 % of each other there, with no
// consistent sign, and at da = 16 the staged one loses 15 % (profiles/cov_heads.md).  Both layouts give the same bits.
constexpr int COV_STAGED_DA_LO = 6, COV_STAGED_DA_HI = 12;
static inline bool cov_logp_staged(int64_t da, int64_t K) { return K == 1 && da >= COV_STAGED_DA_LO && da <= COV_STAGED_DA_HI; }
#define RLHIP_COV_STAGED_DISPATCH(da, LAUNCH)                                                                       \
    switch (da) {                                                                                                   \
        case 6: LAUNCH(6); break;                                                                                   \
        case 7: LAUNCH(7); break;                                                                                   \
        case 8: LAUNCH(8); break;                                                                                   \
        case 9: LAUNCH(9); break;                                                                                   \
        case 10: LAUNCH(10); break;                                                                                 \
        case 11: LAUNCH(11); break;                                                                                 \
        default: LAUNCH(12); break;                                                                                 \
    }

extern "C" {

int32_t rlhip_vec_to_tril_f32(const float* chol_vec, int64_t da, int64_t n, float* L_out, rlhip_stream_t stream) {
    RLHIP_REQUIRE(chol_vec && L_out, "NULL argument");
    RLHIP_COV_SHAPE(da, n, 1);
    if (n == 0) return RLHIP_OK;
    const int64_t total = n * da * da;
    hipLaunchKernelGGL(vec_to_tril_kernel, dim3(grid_for(total, 256)), dim3(256), 0, as_stream(stream), chol_vec, (int)da, total,
                       L_out);
    RLHIP_LAUNCH_CHECK();
    return RLHIP_OK;
}

int32_t rlhip_mvnormlogpdf_f32(const float* mu, const float* L, const float* x, int64_t da, int64_t K, int64_t n, float* out,
                               rlhip_stream_t stream) {
    RLHIP_REQUIRE(mu && L && x && out, "NULL argument");
    RLHIP_COV_SHAPE(da, n, K);
    if (n == 0) return RLHIP_OK;
    const dim3 grid((unsigned)((n * K + 255) / 256)), block(256);
#define LAUNCH(D) hipLaunchKernelGGL(mvnormlogpdf_kernel<D>, grid, block, 0, as_stream(stream), mu, L, x, n, (int)K, out)
    RLHIP_COV_DISPATCH(da, LAUNCH)
#undef LAUNCH
    RLHIP_LAUNCH_CHECK();
    return RLHIP_OK;
}

int32_t rlhip_cov_gaussian_head_sample_f32(const float* mu, const float* chol_vec, int64_t da, int64_t n, int64_t K,
                                           uint64_t seed, uint32_t env_id_base, uint32_t step, float* action_out,
                                           float* logp_out, float* L_out, rlhip_stream_t stream) {
    RLHIP_REQUIRE(mu && chol_vec && action_out, "NULL argument");
    RLHIP_COV_SHAPE(da, n, K);
    if (n == 0) return RLHIP_OK;
    const dim3 grid((unsigned)((n * K + 255) / 256)), block(256);
#define LAUNCH(D)                                                                                                        \
    hipLaunchKernelGGL((cov_head_kernel<D, 0>), grid, block, 0, as_stream(stream), mu, chol_vec, nullptr, n, (int)K, seed, \
                       env_id_base, step, action_out, logp_out, L_out)
    RLHIP_COV_DISPATCH(da, LAUNCH)
#undef LAUNCH
    RLHIP_LAUNCH_CHECK();
    return RLHIP_OK;
}

int32_t rlhip_cov_gaussian_head_logp_f32(const float* mu, const float* chol_vec, const float* action, int64_t da, int64_t n,
                                         int64_t K, float* logp_out, float* L_out, rlhip_stream_t stream) {
    RLHIP_REQUIRE(mu && chol_vec && action && logp_out, "NULL argument");
    RLHIP_COV_SHAPE(da, n, K);
    if (n == 0) return RLHIP_OK;
    const dim3 grid((unsigned)((n * K + 255) / 256)), block(256);
    if (cov_logp_staged(da, K)) {
#define LAUNCH(D)                                                                                                              \
    hipLaunchKernelGGL((cov_head_staged_kernel<D, 1>), dim3((unsigned)((n * K + CovStage<D>::BLOCK - 1) / CovStage<D>::BLOCK)), \
                       dim3(CovStage<D>::BLOCK), 0, as_stream(stream), mu, chol_vec, action, n, (int)K, 0ull, 0u, 0u, nullptr,  \
                       logp_out, L_out)
        RLHIP_COV_STAGED_DISPATCH(da, LAUNCH)
#undef LAUNCH
    } else {
#define LAUNCH(D)                                                                                                          \
    hipLaunchKernelGGL((cov_head_kernel<D, 1>), grid, block, 0, as_stream(stream), mu, chol_vec, action, n, (int)K, 0ull, 0u, \
                       0u, nullptr, logp_out, L_out)
        RLHIP_COV_DISPATCH(da, LAUNCH)
#undef LAUNCH
    }
    RLHIP_LAUNCH_CHECK();
    return RLHIP_OK;
}

int32_t rlhip_normkldivergence_f32(const float* mu1, const float* s1, const float* mu2, const float* s2, int64_t n, float* out,
                                   rlhip_stream_t stream) {
    RLHIP_REQUIRE(mu1 && s1 && mu2 && s2 && out, "NULL argument");
    RLHIP_REQUIRE(n >= 0, "bad shape");
    if (n == 0) return RLHIP_OK;
    hipLaunchKernelGGL(normkl_kernel, dim3(grid_for(n, 256)), dim3(256), 0, as_stream(stream), mu1, s1, mu2, s2, n, out);
    RLHIP_LAUNCH_CHECK();
    return RLHIP_OK;
}

int32_t rlhip_diagnormkldivergence_f32(const float* mu1, const float* s1, const float* mu2, const float* s2, int64_t d,
                                       int64_t n, float* out, rlhip_stream_t stream) {
    RLHIP_REQUIRE(mu1 && s1 && mu2 && s2 && out, "NULL argument");
    RLHIP_REQUIRE(d >= 1 && d <= 0x7FFFFFFFll && n >= 0 && n <= 0x7FFFFFFFll * 256, "bad shape");
    if (n == 0) return RLHIP_OK;
    hipLaunchKernelGGL(diagnormkl_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, as_stream(stream), mu1, s1, mu2, s2,
                       (int)d, n, out);
    RLHIP_LAUNCH_CHECK();
    return RLHIP_OK;
}

int32_t rlhip_mvnormkldivergence_f32(const float* mu1, const float* L1, const float* mu2, const float* L2, int64_t da, int64_t n,
                                     float* out, rlhip_stream_t stream) {
    RLHIP_REQUIRE(mu1 && L1 && mu2 && L2 && out, "NULL argument");
    RLHIP_COV_SHAPE(da, n, 1);
    if (n == 0) return RLHIP_OK;
    const dim3 grid((unsigned)((n + 255) / 256)), block(256);
#define LAUNCH(D) hipLaunchKernelGGL(mvnormkl_kernel<D>, grid, block, 0, as_stream(stream), mu1, L1, mu2, L2, n, out)
    RLHIP_COV_DISPATCH(da, LAUNCH)
#undef LAUNCH
    RLHIP_LAUNCH_CHECK();
    return RLHIP_OK;
}

}  // extern "C"
