// cov_device.h -- what the forward kernels (cov_heads.hip) and the pullbacks (cov_heads_grad.hip) of the full-covariance Gaussian
// head share: the map between the Cholesky vector and the lower triangle, softplusbeta, and Cov<DA>, the packed lower triangle of one
// state's L in registers with its solves.  The order of operations is stated in cov_heads.hip / cov_heads_grad.hip and include/rlhip.h.
#pragma once
#include "ppo_sample_device.h"

namespace rlhip {

constexpr int COV_MAX_DA = 16;

__device__ __forceinline__ float softplusbeta(float x) { return logf(expf(x / 10.0f) + 1.0f) * 10.0f; }  // :360
__device__ __forceinline__ float chol_diag(float x) { return softplusbeta(x) + 1.0e-5f; }                 // :364
// 0-based position of L[r,c] (r >= c) in the Cholesky vector: cholesky_matrix_to_vector_index(r + 1, c + 1, da) - 1  (:359)
__host__ __device__ constexpr int tril_index(int r, int c, int da) { return ((2 * da - c - 1) * c) / 2 + r; }

template <int DA>
struct Cov {
    static constexpr int NV = (DA * (DA + 1)) / 2;
    float T[NV];  // the lower triangle in the order of the Cholesky vector

    // vec_to_tril with the diagonal already evaluated (diag[k * stride])
    __device__ __forceinline__ void from_vec(const float* __restrict__ v, const float* diag, int stride) {
#pragma unroll
        for (int c = 0; c < DA; ++c)
#pragma unroll
            for (int r = c; r < DA; ++r) T[tril_index(r, c, DA)] = r == c ? diag[c * stride] : v[tril_index(r, c, DA)];
    }
    // the lower triangle of a dense (DA x DA) column-major L
    __device__ __forceinline__ void from_dense(const float* __restrict__ L) {
#pragma unroll
        for (int c = 0; c < DA; ++c)
#pragma unroll
            for (int r = c; r < DA; ++r) T[tril_index(r, c, DA)] = L[c * DA + r];
    }
    __device__ __forceinline__ void to_dense(float* __restrict__ L) const {
#pragma unroll
        for (int c = 0; c < DA; ++c)
#pragma unroll
            for (int r = 0; r < DA; ++r) L[c * DA + r] = r >= c ? T[tril_index(r, c, DA)] : 0.0f;
    }
    // z = mu + L eps  (:259, :308)
    __device__ __forceinline__ void sample(const float (&mu)[DA], const float (&eps)[DA], float (&z)[DA]) const {
        float acc[DA];
#pragma unroll
        for (int c = 0; c < DA; ++c)
#pragma unroll
            for (int r = c; r < DA; ++r) {
                const float p = T[tril_index(r, c, DA)] * eps[c];
                acc[r] = c == 0 ? p : acc[r] + p;
            }
#pragma unroll
        for (int r = 0; r < DA; ++r) z[r] = mu[r] + acc[r];
    }
    // t := L \ t from row `from` on (the rows above are not touched); returns 0 + sum of the squares of the solved rows, ascending
    template <int FROM>
    __device__ __forceinline__ float solve_sq(float (&t)[DA], float ss) const {
#pragma unroll
        for (int c = FROM; c < DA; ++c) {
            const float y = t[c] / T[tril_index(c, c, DA)];
            ss = ss + y * y;
#pragma unroll
            for (int r = c + 1; r < DA; ++r) t[r] = t[r] - T[tril_index(r, c, DA)] * y;
        }
        return ss;
    }
    __device__ __forceinline__ float sum_log_diag() const {  // the ld of logdetLorU :76
        float ld = 0.0f;
#pragma unroll
        for (int c = 0; c < DA; ++c) ld = ld + logf(T[tril_index(c, c, DA)]);
        return ld;
    }
    // mvnormlogpdf :46-50 of one sample
    __device__ __forceinline__ float logpdf(const float (&mu)[DA], const float (&x)[DA]) const {
        float t[DA];
#pragma unroll
        for (int r = 0; r < DA; ++r) t[r] = x[r] - mu[r];
        const float ss = solve_sq<0>(t, 0.0f);
        const float logdet = 2.0f * sum_log_diag();
        return -(((float)DA * LOG2PI_F + logdet) + ss) / 2.0f;
    }
    // t := L \ t from row `from` on, in the order of solve_sq, keeping the solved rows
    template <int FROM>
    __device__ __forceinline__ void solve(float (&t)[DA]) const {
#pragma unroll
        for (int c = FROM; c < DA; ++c) {
            const float y = t[c] / T[tril_index(c, c, DA)];
            t[c] = y;
#pragma unroll
            for (int r = c + 1; r < DA; ++r) t[r] = t[r] - T[tril_index(r, c, DA)] * y;
        }
    }
    // t := L^T \ t, back substitution over the columns c = DA ... 1: u[c] = t[c] / L[c,c], then t[r] = t[r] - L[c,r] u[c] for r < c (a
    // row's terms are visited with j descending)
    __device__ __forceinline__ void solve_transposed(float (&t)[DA]) const {
#pragma unroll
        for (int c = DA - 1; c >= 0; --c) {
            const float u = t[c] / T[tril_index(c, c, DA)];
            t[c] = u;
#pragma unroll
            for (int r = 0; r < c; ++r) t[r] = t[r] - T[tril_index(c, r, DA)] * u;
        }
    }
};

}  // namespace rlhip

// one case per supported da: a dropped one is a missing instantiation (tests/test_cov_head_kernel_resources.py counts them)
#define RLHIP_COV_DISPATCH(da, LAUNCH)                                                                              \
    switch (da) {                                                                                                   \
        case 1: LAUNCH(1); break;                                                                                   \
        case 2: LAUNCH(2); break;                                                                                   \
        case 3: LAUNCH(3); break;                                                                                   \
        case 4: LAUNCH(4); break;                                                                                   \
        case 5: LAUNCH(5); break;                                                                                   \
        case 6: LAUNCH(6); break;                                                                                   \
        case 7: LAUNCH(7); break;                                                                                   \
        case 8: LAUNCH(8); break;                                                                                   \
        case 9: LAUNCH(9); break;                                                                                   \
        case 10: LAUNCH(10); break;                                                                                 \
        case 11: LAUNCH(11); break;                                                                                 \
        case 12: LAUNCH(12); break;                                                                                 \
        case 13: LAUNCH(13); break;                                                                                 \
        case 14: LAUNCH(14); break;                                                                                 \
        case 15: LAUNCH(15); break;                                                                                 \
        default: LAUNCH(16); break;                                                                                 \
    }

#define RLHIP_COV_SHAPE(da, n, K)                                                                                   \
    RLHIP_REQUIRE(da >= 1 && da <= COV_MAX_DA, "da must be in 1 ... 16");                                           \
    RLHIP_REQUIRE(n >= 0 && K >= 1 && K <= 0x7FFFFFFFll / COV_MAX_DA && n <= 0x7FFFFFFFll * 256 / K, "bad shape")
