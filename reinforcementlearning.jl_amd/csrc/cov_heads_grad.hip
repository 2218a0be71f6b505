// cov_heads_grad.hip -- the pullbacks of csrc/cov_heads.hip: mvnormlogpdf, vec_to_tril, (model::CovGaussianNetwork)(state, action) and
// the three Gaussian KL divergences.
//
// Reference: RLCore/src/utils/distributions.jl introduces mvnormlogpdf (:46-66), mvnormkldivergence (:88-109), diagnormkldivergence
// (:117-129) and normkldivergence (:137-139) as "GPU automatic differentiable" versions and RLCore/src/utils/networks.jl writes vec_to_tril
// (:359-381) so that Zygote can pull back through it; these kernels are those pullbacks in closed form.  Layouts as in cov_heads.hip; a
// cotangent has the shape of the forward output, a gradient the shape of the forward input; dL is dense (da x da x n) with +0 above the
// diagonal.  Every output pointer is nullable and its work is skipped.
//
// ORDER OF OPERATIONS (all Float32, -ffp-contract=off; tests/mvnorm_grad_ref.py replays it bit for bit; the one libm call is the expf
// of the sigmoid).  g is the upstream cotangent.
//   mvnormlogpdf(mu, L, x), per state i, the samples k = 1 ... K visited in ascending order by ONE lane (sequential sums: the result
//   cannot depend on the launch geometry, there are no atomics):
//       y = L \ (x_k - mu)            the forward solve of cov_heads.hip (row i: t = t - L[i,j] y[j], j ascending; y[i] = t / L[i,i])
//       u = L^T \ y                   columns c = da ... 1: u[c] = t[c] / L[c,c]; then t[r] = t[r] - L[c,r] u[c] for r < c
//       gu[r] = g_k u[r];  dx_k[r] = -gu[r]
//       dmu[r] = 0 + sum_k gu_k[r];  S[r,c] = 0 + sum_k gu_k[r] y_k[c] (r >= c);  gs = 0 + sum_k g_k
//       dL[r,c] = S[r,c] (r > c);  dL[c,c] = S[c,c] - gs / L[c,c];  +0 above the diagonal
//   vec_to_tril:  dvec = dL[r,c] below the diagonal;  dvec = dL[c,c] * (1.0f / (1.0f + expf(-(v / 10.0f)))) on it
//   (model)(state, action): vec_to_tril, the mvnormlogpdf pullback and the vec_to_tril pullback in one launch, the same operations
//   mvnormkldivergence(mu1, L1, mu2, L2), per state:
//       m = L2 \ (mu2 - mu1);  q = L2^T \ m;  dmu2[r] = g q[r];  dmu1[r] = -(g q[r]);  W[r,j] = q[r] m[j] (r >= j)
//       for c = 1 ... da:  a = L2 \ L1[:,c] from row c (the rows above are +0);  p = L2^T \ a (all rows);
//           dL1[r,c] = g p[r] (r > c);  dL1[c,c] = g (p[c] - 1.0f / L1[c,c]);
//           W[r,j] = W[r,j] + p[r] a[j] for c <= j <= r
//       dL2[r,j] = g (-W[r,j]) (r > j);  dL2[j,j] = g (1.0f / L2[j,j] - W[j,j])
//   diagnormkldivergence, per component (a = s1, b = s2, dm = mu2 - mu1, v1 = a a, v2 = b b, g of the column):
//       w = dm / v2;  dmu2 = g w;  dmu1 = -(g w);  ds1 = g (a / v2 - 1.0f / a);  ds2 = g (1.0f / b - (v1 + dm dm) / (v2 b))
//   normkldivergence, elementwise (dm = mu1 - mu2, v2 = b b):
//       w = dm / v2;  dmu1 = g w;  dmu2 = -(g w);  ds1 = g (a / v2 - 1.0f / a);  ds2 = g (1.0f / b - (a a + dm dm) / (v2 b))
//
// Shape of the kernels: one lane per state, da a template argument (1 ... 16): L, the accumulators S / W and the solved vectors are
// registers with compile-time indices, nothing lands in scratch (tests/test_cov_head_grad_kernel_resources.py).  The K samples of a state
// are a loop of its lane, which is what keeps the sums sequential; the nv + da outputs of a state need no parallelism over K to fill the
// machine at the batch sizes a learner runs.
#include "cov_device.h"

namespace rlhip {

// d softplusbeta(v) / dv in the form that stays finite where expf(v / 10) overflows
__device__ __forceinline__ float softplusbeta_grad(float v) { return 1.0f / (1.0f + expf(-(v / 10.0f))); }

// FUSED = 0: `Lsrc` is a dense L, `dL_out` a dense dL.  FUSED = 1: `Lsrc` is the Cholesky vector, `dL_out` its gradient dvec.
template <int DA, int FUSED>
__global__ __launch_bounds__(256) void mvnormlogpdf_bwd_kernel(const float* __restrict__ mu, const float* __restrict__ Lsrc,
                                                               const float* __restrict__ x, const float* __restrict__ g,
                                                               int64_t n, int K, float* __restrict__ dmu_out,
                                                               float* __restrict__ dL_out, float* __restrict__ dx_out) {
    constexpr int NV = Cov<DA>::NV;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    Cov<DA> cov;
    float vd[DA];  // the diagonal's inputs (FUSED)
    if (FUSED) {
        const float* __restrict__ v = Lsrc + i * NV;
        float dg[DA];
#pragma unroll
        for (int c = 0; c < DA; ++c) {
            vd[c] = v[tril_index(c, c, DA)];
            dg[c] = chol_diag(vd[c]);
        }
        cov.from_vec(v, dg, 1);
    } else {
        cov.from_dense(Lsrc + i * (DA * DA));
    }
    float m[DA], dm[DA], S[NV];
#pragma unroll
    for (int r = 0; r < DA; ++r) {
        m[r] = mu[i * DA + r];
        dm[r] = 0.0f;
    }
#pragma unroll
    for (int e = 0; e < NV; ++e) S[e] = 0.0f;
    float gs = 0.0f;
    for (int k = 0; k < K; ++k) {
        const int64_t gid = i * K + k;
        const float gk = g[gid];
        float y[DA], u[DA];
#pragma unroll
        for (int r = 0; r < DA; ++r) y[r] = x[gid * DA + r] - m[r];
        cov.template solve<0>(y);
#pragma unroll
        for (int r = 0; r < DA; ++r) u[r] = y[r];
        cov.solve_transposed(u);
#pragma unroll
        for (int r = 0; r < DA; ++r) u[r] = gk * u[r];
        if (dx_out) {
#pragma unroll
            for (int r = 0; r < DA; ++r) dx_out[gid * DA + r] = -u[r];
        }
        if (dmu_out) {
#pragma unroll
            for (int r = 0; r < DA; ++r) dm[r] = dm[r] + u[r];
        }
        if (dL_out) {
#pragma unroll
            for (int c = 0; c < DA; ++c)
#pragma unroll
                for (int r = c; r < DA; ++r) S[tril_index(r, c, DA)] = S[tril_index(r, c, DA)] + u[r] * y[c];
            gs = gs + gk;
        }
    }
    if (dmu_out) {
#pragma unroll
        for (int r = 0; r < DA; ++r) dmu_out[i * DA + r] = dm[r];
    }
    if (!dL_out) return;
#pragma unroll
    for (int c = 0; c < DA; ++c) S[tril_index(c, c, DA)] = S[tril_index(c, c, DA)] - gs / cov.T[tril_index(c, c, DA)];
    if (FUSED) {
        float* __restrict__ dv = dL_out + i * NV;
#pragma unroll
        for (int c = 0; c < DA; ++c)
#pragma unroll
            for (int r = c; r < DA; ++r)
                dv[tril_index(r, c, DA)] = r == c ? S[tril_index(c, c, DA)] * softplusbeta_grad(vd[c]) : S[tril_index(r, c, DA)];
    } else {
        float* __restrict__ dL = dL_out + i * (DA * DA);
#pragma unroll
        for (int c = 0; c < DA; ++c)
#pragma unroll
            for (int r = 0; r < DA; ++r) dL[c * DA + r] = r >= c ? S[tril_index(r >= c ? r : c, c, DA)] : 0.0f;
    }
}

// the vec_to_tril pullback: one lane per element of the dense dL, the elements above the diagonal are not read
__global__ __launch_bounds__(256) void vec_to_tril_bwd_kernel(const float* __restrict__ chol_vec, const float* __restrict__ dL, int da,
                                                              int64_t total, float* __restrict__ dvec) {
    const int dd = da * da, nv = (da * (da + 1)) / 2;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int64_t i = e / dd;
        const int rem = (int)(e - i * dd), c = rem / da, r = rem - c * da;
        if (r < c) continue;
        const int64_t at = i * nv + tril_index(r, c, da);
        const float d = dL[e];
        dvec[at] = r == c ? d * softplusbeta_grad(chol_vec[at]) : d;
    }
}

// column C of the mvnormkldivergence pullback, then the columns after it
template <int DA, int C>
__device__ __forceinline__ void kl_bwd_column(const Cov<DA>& L2, const float* __restrict__ L1, float g, float (&W)[Cov<DA>::NV],
                                              float* __restrict__ dL1, bool want_W) {
    float a[DA], p[DA];
#pragma unroll
    for (int r = 0; r < DA; ++r) a[r] = r >= C ? L1[C * DA + r] : 0.0f;
    const float l1cc = a[C];
    L2.template solve<C>(a);
#pragma unroll
    for (int r = 0; r < DA; ++r) p[r] = a[r];
    L2.solve_transposed(p);
    if (dL1) {
#pragma unroll
        for (int r = 0; r < DA; ++r) dL1[C * DA + r] = r > C ? g * p[r] : (r == C ? g * (p[C] - 1.0f / l1cc) : 0.0f);
    }
    if (want_W) {
#pragma unroll
        for (int j = C; j < DA; ++j)
#pragma unroll
            for (int r = j; r < DA; ++r) W[tril_index(r, j, DA)] = W[tril_index(r, j, DA)] + p[r] * a[j];
    }
    if constexpr (C + 1 < DA) kl_bwd_column<DA, C + 1>(L2, L1, g, W, dL1, want_W);
}

template <int DA>
__global__ __launch_bounds__(256) void mvnormkl_bwd_kernel(const float* __restrict__ mu1, const float* __restrict__ L1,
                                                           const float* __restrict__ mu2, const float* __restrict__ L2,
                                                           const float* __restrict__ gout, int64_t n, float* __restrict__ dmu1,
                                                           float* __restrict__ dL1, float* __restrict__ dmu2,
                                                           float* __restrict__ dL2) {
    constexpr int NV = Cov<DA>::NV;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float g = gout[i];
    Cov<DA> c2;
    c2.from_dense(L2 + i * (DA * DA));
    float m[DA], q[DA];
#pragma unroll
    for (int r = 0; r < DA; ++r) m[r] = mu2[i * DA + r] - mu1[i * DA + r];
    c2.template solve<0>(m);
#pragma unroll
    for (int r = 0; r < DA; ++r) q[r] = m[r];
    c2.solve_transposed(q);
    if (dmu2) {
#pragma unroll
        for (int r = 0; r < DA; ++r) dmu2[i * DA + r] = g * q[r];
    }
    if (dmu1) {
#pragma unroll
        for (int r = 0; r < DA; ++r) dmu1[i * DA + r] = -(g * q[r]);
    }
    if (!dL1 && !dL2) return;
    float W[NV];
#pragma unroll
    for (int j = 0; j < DA; ++j)
#pragma unroll
        for (int r = j; r < DA; ++r) W[tril_index(r, j, DA)] = q[r] * m[j];
    kl_bwd_column<DA, 0>(c2, L1 + i * (DA * DA), g, W, dL1 ? dL1 + i * (DA * DA) : nullptr, dL2 != nullptr);
    if (!dL2) return;
    float* __restrict__ o = dL2 + i * (DA * DA);
#pragma unroll
    for (int j = 0; j < DA; ++j)
#pragma unroll
        for (int r = 0; r < DA; ++r) {
            const float w = W[tril_index(r >= j ? r : j, j, DA)];
            o[j * DA + r] = r > j ? g * (-w) : (r == j ? g * (1.0f / c2.T[tril_index(j, j, DA)] - w) : 0.0f);
        }
}

// the diagnormkldivergence pullback, one lane per element of the (d x n) arrays; g is per column
__global__ __launch_bounds__(256) void diagnormkl_bwd_kernel(const float* __restrict__ mu1, const float* __restrict__ s1,
                                                             const float* __restrict__ mu2, const float* __restrict__ s2,
                                                             const float* __restrict__ gout, int64_t d, int64_t total,
                                                             float* __restrict__ dmu1, float* __restrict__ ds1,
                                                             float* __restrict__ dmu2, float* __restrict__ ds2) {
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const float g = gout[e / d], a = s1[e], b = s2[e], dm = mu2[e] - mu1[e];
        const float v1 = a * a, v2 = b * b, w = dm / v2;
        if (dmu2) dmu2[e] = g * w;
        if (dmu1) dmu1[e] = -(g * w);
        if (ds1) ds1[e] = g * (a / v2 - 1.0f / a);
        if (ds2) ds2[e] = g * (1.0f / b - (v1 + dm * dm) / (v2 * b));
    }
}

// the normkldivergence pullback, elementwise
__global__ __launch_bounds__(256) void normkl_bwd_kernel(const float* __restrict__ mu1, const float* __restrict__ s1,
                                                         const float* __restrict__ mu2, const float* __restrict__ s2,
                                                         const float* __restrict__ gout, int64_t n, float* __restrict__ dmu1,
                                                         float* __restrict__ ds1, float* __restrict__ dmu2, float* __restrict__ ds2) {
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (int64_t)gridDim.x * 256) {
        const float g = gout[e], a = s1[e], b = s2[e], dm = mu1[e] - mu2[e];
        const float v2 = b * b, w = dm / v2;
        if (dmu1) dmu1[e] = g * w;
        if (dmu2) dmu2[e] = -(g * w);
        if (ds1) ds1[e] = g * (a / v2 - 1.0f / a);
        if (ds2) ds2[e] = g * (1.0f / b - (a * a + dm * dm) / (v2 * b));
    }
}

}  // namespace rlhip

using namespace rlhip;

extern "C" {

int32_t rlhip_mvnormlogpdf_bwd_f32(const float* mu, const float* L, const float* x, const float* dlogp, int64_t da, int64_t K,
                                   int64_t n, float* dmu_out, float* dL_out, float* dx_out, rlhip_stream_t stream) {
    RLHIP_REQUIRE(mu && L && x && dlogp, "NULL argument");
    RLHIP_COV_SHAPE(da, n, K);
    if (n == 0 || !(dmu_out || dL_out || dx_out)) return RLHIP_OK;
    const dim3 grid((unsigned)((n + 255) / 256)), block(256);
#define LAUNCH(D)                                                                                                            \
    hipLaunchKernelGGL((mvnormlogpdf_bwd_kernel<D, 0>), grid, block, 0, as_stream(stream), mu, L, x, dlogp, n, (int)K, dmu_out, \
                       dL_out, dx_out)
    RLHIP_COV_DISPATCH(da, LAUNCH)
#undef LAUNCH
    RLHIP_LAUNCH_CHECK();
    return RLHIP_OK;
}

int32_t rlhip_vec_to_tril_bwd_f32(const float* chol_vec, const float* dL, int64_t da, int64_t n, float* dvec_out,
                                  rlhip_stream_t stream) {
    RLHIP_REQUIRE(chol_vec && dL && dvec_out, "NULL argument");
    RLHIP_COV_SHAPE(da, n, 1);
    if (n == 0) return RLHIP_OK;
    const int64_t total = n * da * da;
    hipLaunchKernelGGL(vec_to_tril_bwd_kernel, dim3(grid_for(total, 256)), dim3(256), 0, as_stream(stream), chol_vec, dL, (int)da,
                       total, dvec_out);
    RLHIP_LAUNCH_CHECK();
    return RLHIP_OK;
}

int32_t rlhip_cov_gaussian_head_logp_bwd_f32(const float* mu, const float* chol_vec, const float* action, const float* dlogp,
                                             int64_t da, int64_t n, int64_t K, float* dmu_out, float* dvec_out,
                                             rlhip_stream_t stream) {
    RLHIP_REQUIRE(mu && chol_vec && action && dlogp, "NULL argument");
    RLHIP_COV_SHAPE(da, n, K);
    if (n == 0 || !(dmu_out || dvec_out)) return RLHIP_OK;
    const dim3 grid((unsigned)((n + 255) / 256)), block(256);
#define LAUNCH(D)                                                                                                             \
    hipLaunchKernelGGL((mvnormlogpdf_bwd_kernel<D, 1>), grid, block, 0, as_stream(stream), mu, chol_vec, action, dlogp, n, (int)K, \
                       dmu_out, dvec_out, nullptr)
    RLHIP_COV_DISPATCH(da, LAUNCH)
#undef LAUNCH
    RLHIP_LAUNCH_CHECK();
    return RLHIP_OK;
}

int32_t rlhip_mvnormkldivergence_bwd_f32(const float* mu1, const float* L1, const float* mu2, const float* L2, const float* dout,
                                         int64_t da, int64_t n, float* dmu1_out, float* dL1_out, float* dmu2_out, float* dL2_out,
                                         rlhip_stream_t stream) {
    RLHIP_REQUIRE(mu1 && L1 && mu2 && L2 && dout, "NULL argument");
    RLHIP_COV_SHAPE(da, n, 1);
    if (n == 0 || !(dmu1_out || dL1_out || dmu2_out || dL2_out)) return RLHIP_OK;
    const dim3 grid((unsigned)((n + 255) / 256)), block(256);
#define LAUNCH(D)                                                                                                        \
    hipLaunchKernelGGL(mvnormkl_bwd_kernel<D>, grid, block, 0, as_stream(stream), mu1, L1, mu2, L2, dout, n, dmu1_out, dL1_out, \
                       dmu2_out, dL2_out)
    RLHIP_COV_DISPATCH(da, LAUNCH)
#undef LAUNCH
    RLHIP_LAUNCH_CHECK();
    return RLHIP_OK;
}

int32_t rlhip_diagnormkldivergence_bwd_f32(const float* mu1, const float* s1, const float* mu2, const float* s2, const float* dout,
                                           int64_t d, int64_t n, float* dmu1_out, float* ds1_out, float* dmu2_out, float* ds2_out,
                                           rlhip_stream_t stream) {
    RLHIP_REQUIRE(mu1 && s1 && mu2 && s2 && dout, "NULL argument");
    RLHIP_REQUIRE(d >= 1 && d <= 0x7FFFFFFFll && n >= 0 && n <= 0x7FFFFFFFll * 256, "bad shape");
    RLHIP_REQUIRE(n <= INT64_MAX / d, "bad shape");
    if (n == 0 || !(dmu1_out || ds1_out || dmu2_out || ds2_out)) return RLHIP_OK;
    hipLaunchKernelGGL(diagnormkl_bwd_kernel, dim3(grid_for(n * d, 256)), dim3(256), 0, as_stream(stream), mu1, s1, mu2, s2, dout, d,
                       n * d, dmu1_out, ds1_out, dmu2_out, ds2_out);
    RLHIP_LAUNCH_CHECK();
    return RLHIP_OK;
}

int32_t rlhip_normkldivergence_bwd_f32(const float* mu1, const float* s1, const float* mu2, const float* s2, const float* dout,
                                       int64_t n, float* dmu1_out, float* ds1_out, float* dmu2_out, float* ds2_out,
                                       rlhip_stream_t stream) {
    RLHIP_REQUIRE(mu1 && s1 && mu2 && s2 && dout, "NULL argument");
    RLHIP_REQUIRE(n >= 0, "bad shape");
    if (n == 0 || !(dmu1_out || ds1_out || dmu2_out || ds2_out)) return RLHIP_OK;
    hipLaunchKernelGGL(normkl_bwd_kernel, dim3(grid_for(n, 256)), dim3(256), 0, as_stream(stream), mu1, s1, mu2, s2, dout, n,
                       dmu1_out, ds1_out, dmu2_out, ds2_out);
    RLHIP_LAUNCH_CHECK();
    return RLHIP_OK;
}

}  // extern "C"
