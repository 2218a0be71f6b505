// heads_grad.hip -- the pullbacks of the diagonal Gaussian heads (csrc/heads.hip) and of normlogpdf / diagnormlogpdf (csrc/optim.hip).
//
// Reference: RLCore/src/utils/distributions.jl introduces normlogpdf (:14-21) and diagnormlogpdf (:26-34) as "GPU automatic
// differentiable"; RLCore/src/utils/networks.jl differentiates GaussianNetwork through its log-probabilities (the draw is under
// ignore_derivatives :69, :94) and SoftGaussianNetwork through its actions AND its log-probabilities (z = mu .+ sigma .* noise is the
// reparameterisation trick :153-185).  These kernels are those pullbacks in closed form, onto the outputs of the mu / sigma
// sub-networks.  Layouts as in heads.hip: mu, raw_sigma (d x n) column-major, actions (d x K x n), dlogp (K x n).  Every gradient output is
// nullable.
//
// ORDER OF OPERATIONS (all Float32, -ffp-contract=off; tests/heads_grad_ref.py replays it; g is the upstream cotangent):
//   sg = clampj(raw, lo, hi);  pass = !(raw > hi) && !(raw < lo)  (inclusive bounds, a NaN passes: the reference's clamp rule);
//   s = sg + 1.0e-8f;  draw_sigma = pass ? dsg : +0.0f  -- a select, never a product: a non-finite dsg at a clamped component gives 0
//   normlogpdf(mu, sigma, x), elementwise (s = sigma + 1.0e-8f):
//       z = (x - mu) / s;  w = z / s;  dmu = g w;  dx = -(g w);  dsigma = g ((z z - 1.0f) / s)
//   diagnormlogpdf(mu, sigma, x), per component, g of the column:
//       v = s s;  e = x - mu;  w = e / v;  dmu = g w;  dx = -(g w);  dsigma = g (((e e) / v - 1.0f) / s)
//       (d log(prod v) / ds in its closed form 2 / s: finite where prod(v) over- or underflows and the forward value is already +-Inf)
//   (model)(state, action):  z = (soft || squash) ? atanhf(a) : a  -- the actions are data: no gradient, the tanh correction is constant
//       soft = 0:  e = z - mu;  v = s s;  dmu[k] = 0 + sum_j g_j (e / v);  dsg[k] = 0 + sum_j g_j (((e e) / v - 1.0f) / s)
//       soft = 1:  zz = (z - mu) / s;  w = zz / s;  dmu[k] = 0 + sum_j g_j w;  dsg[k] = 0 + sum_j g_j ((zz zz - 1.0f) / s)
//   the sampling calls: eps = normal_draw(seed, env_id_base + i, step, k + d j) and z = mu + sg eps are REGENERATED, bit for bit the
//   forward's, so nothing of size (d x K x n) has to be kept between forward and backward (and for a tanh head the saved action could not
//   stand in for z: tanhf saturates to +-1 at |z| of about 9 and atanhf of that is +-Inf)
//       soft = 0:  z is a constant; the soft = 0 sums above at the regenerated z
//       soft = 1:  t = tanhf(z);  zz = (z - mu) / s;  w = zz / s;
//                  dz = 0;  if dlogp: dz = g (2.0f t - w);  if dact: dz = dz + da (1.0f - t t)
//                  dmu[k] = 0 + sum_j ((dlogp ? g w : 0) + dz);  dsg[k] = 0 + sum_j ((dlogp ? g ((zz zz - 1.0f) / s) : 0) + dz eps)
//                  (2 t is the exact derivative of the reference's correction -2 (log 2 - z - softplus(-2 z)))
//   every sum over the K samples of a state runs in ascending j, sequentially, in ONE lane: no atomics, no dependence on the launch
//   geometry.
//
// Shape of the kernels: one lane per (state, component), looping over the K samples of the state.  Loads of mu / raw_sigma and the
// stores of both gradients are contiguous over the lanes; the diagonal forms need no reduction across components.  The sampling
// pullback with an even d takes one lane per PAIR of neighbouring components instead, which share a Philox block and its Box-Muller
// transform: the same bits, 1.5 - 1.6 times faster on the MI355X (profiles/heads_grad.md).
#include "head_device.h"

namespace rlhip {

// one component of one state: its clamped sigma and the two running sums over the K samples
template <int SOFT, int SAMPLE>
struct HeadGrad {
    float m, sg, s, am = 0.0f, as = 0.0f;
    bool pass;
    __device__ __forceinline__ HeadGrad(float mu, float raw, float lo, float hi)
        : m(mu), sg(clampj(raw, lo, hi)), s(sg + 1.0e-8f), pass(!(raw > hi) && !(raw < lo)) {}
    // sample j: z the pre-squash value, eps its draw (SAMPLE), g = dlogp[j] (has_g), da = dact[k, j] (has_da)
    __device__ __forceinline__ void add(float z, float eps, float g, bool has_g, float da, bool has_da) {
        if (SOFT) {
            const float zz = (z - m) / s, w = zz / s;
            if (SAMPLE) {
                const float t = tanhf(z);
                float dz = 0.0f;
                if (has_g) dz = g * (2.0f * t - w);
                if (has_da) dz = dz + da * (1.0f - t * t);
                am = am + ((has_g ? g * w : 0.0f) + dz);
                as = as + ((has_g ? g * ((zz * zz - 1.0f) / s) : 0.0f) + dz * eps);
            } else {
                am = am + g * w;
                as = as + g * ((zz * zz - 1.0f) / s);
            }
        } else {
            const float dx = z - m, v = s * s;
            am = am + g * (dx / v);
            as = as + g * (((dx * dx) / v - 1.0f) / s);
        }
    }
    __device__ __forceinline__ float draw_sigma() const { return pass ? as : 0.0f; }
};

template <int SOFT, int SAMPLE>
__global__ __launch_bounds__(256) void gaussian_head_bwd_kernel(const float* __restrict__ mu, const float* __restrict__ raw_sigma,
                                                                const float* __restrict__ action, const float* __restrict__ dact,
                                                                const float* __restrict__ dlogp, int d, int64_t total, int K,
                                                                float min_sigma, float max_sigma, int squash, uint64_t seed,
                                                                uint32_t env_id_base, uint32_t step, float* __restrict__ dmu_out,
                                                                float* __restrict__ draw_sigma_out) {
    const bool sq = SOFT || squash;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int64_t i = e / d;
        const int k = (int)(e - i * d);
        HeadGrad<SOFT, SAMPLE> c(mu[e], raw_sigma[e], min_sigma, max_sigma);
        for (int j = 0; j < K; ++j) {
            const int64_t gid = i * K + j;
            const float g = dlogp ? dlogp[gid] : 0.0f;
            float z, eps = 0.0f;
            if (SAMPLE) {
                eps = normal_draw(seed, env_id_base + (uint32_t)i, step, k + d * j);
                z = c.m + c.sg * eps;
            } else {
                const float a = action[gid * d + k];
                z = sq ? atanhf(a) : a;
            }
            c.add(z, eps, g, dlogp != nullptr, dact ? dact[gid * d + k] : 0.0f, dact != nullptr);
        }
        if (dmu_out) dmu_out[e] = c.am;
        if (draw_sigma_out) draw_sigma_out[e] = c.draw_sigma();
    }
}

// The sampling pullback for even d: one lane per PAIR of neighbouring components (k even, k + 1).  Their draws k + d j and k + 1 + d j are
// the cosine and the sine half of ONE Philox block / Box-Muller transform (normal_draw_pair), so the lane evaluates the block, the
// Float64 log and sqrt once for both -- half of what gaussian_head_bwd_kernel<SOFT, 1> spends on them per value.  With odd d a block
// straddles two samples of one component pair and that kernel is used.
template <int SOFT>
__global__ __launch_bounds__(256) void gaussian_head_sample_bwd_pair_kernel(const float* __restrict__ mu, const float* __restrict__ raw_sigma,
                                                                            const float* __restrict__ dact, const float* __restrict__ dlogp,
                                                                            int d, int64_t pairs, int K, float min_sigma, float max_sigma,
                                                                            uint64_t seed, uint32_t env_id_base, uint32_t step,
                                                                            float* __restrict__ dmu_out, float* __restrict__ draw_sigma_out) {
    for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < pairs; p += (int64_t)gridDim.x * 256) {
        const int64_t e = 2 * p, i = e / d;
        const int k = (int)(e - i * d);  // even, k + 1 < d
        HeadGrad<SOFT, 1> c0(mu[e], raw_sigma[e], min_sigma, max_sigma), c1(mu[e + 1], raw_sigma[e + 1], min_sigma, max_sigma);
        for (int j = 0; j < K; ++j) {
            const int64_t gid = i * K + j;
            const float g = dlogp ? dlogp[gid] : 0.0f;
            float eps0, eps1;
            normal_draw_pair(seed, env_id_base + (uint32_t)i, step, k + d * j, eps0, eps1);
            c0.add(c0.m + c0.sg * eps0, eps0, g, dlogp != nullptr, dact ? dact[gid * d + k] : 0.0f, dact != nullptr);
            c1.add(c1.m + c1.sg * eps1, eps1, g, dlogp != nullptr, dact ? dact[gid * d + k + 1] : 0.0f, dact != nullptr);
        }
        if (dmu_out) {
            dmu_out[e] = c0.am;
            dmu_out[e + 1] = c1.am;
        }
        if (draw_sigma_out) {
            draw_sigma_out[e] = c0.draw_sigma();
            draw_sigma_out[e + 1] = c1.draw_sigma();
        }
    }
}

__global__ __launch_bounds__(256) void normlogpdf_bwd_kernel(const float* __restrict__ mu, const float* __restrict__ sigma,
                                                             const float* __restrict__ x, const float* __restrict__ dout, int64_t n,
                                                             float* __restrict__ dmu, float* __restrict__ dsigma,
                                                             float* __restrict__ dx) {
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (int64_t)gridDim.x * 256) {
        const float g = dout[e], s = sigma[e] + 1.0e-8f;
        const float z = (x[e] - mu[e]) / s, w = z / s;
        if (dmu) dmu[e] = g * w;
        if (dx) dx[e] = -(g * w);
        if (dsigma) dsigma[e] = g * ((z * z - 1.0f) / s);
    }
}

// one lane per element of the (d x n) arrays; g is per column
__global__ __launch_bounds__(256) void diagnormlogpdf_bwd_kernel(const float* __restrict__ mu, const float* __restrict__ sigma,
                                                                 const float* __restrict__ x, const float* __restrict__ dout, int64_t d,
                                                                 int64_t total, float* __restrict__ dmu, float* __restrict__ dsigma,
                                                                 float* __restrict__ dx) {
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const float g = dout[e / d], s = sigma[e] + 1.0e-8f;
        const float v = s * s, df = x[e] - mu[e], w = df / v;
        if (dmu) dmu[e] = g * w;
        if (dx) dx[e] = -(g * w);
        if (dsigma) dsigma[e] = g * (((df * df) / v - 1.0f) / s);
    }
}

}  // namespace rlhip

using namespace rlhip;

#define RLHIP_HEAD_SHAPE(d, n, K)                                                                                                 \
    RLHIP_REQUIRE((d) >= 1 && (d) <= HEAD_MAX_D, "d must be in 1 ... 64");                                                        \
    RLHIP_REQUIRE((n) >= 0 && (K) >= 1 && (K) <= 0x7FFFFFFFll / HEAD_MAX_D && (n) <= (0x7FFFFFFFll * 256) / (K), "bad shape")

extern "C" {

int32_t rlhip_normlogpdf_bwd_f32(const float* mu, const float* sigma, const float* x, const float* dout, int64_t n, float* dmu_out,
                                 float* dsigma_out, float* dx_out, rlhip_stream_t stream) {
    RLHIP_REQUIRE(mu && sigma && x && dout, "NULL argument");
    RLHIP_REQUIRE(n >= 0, "bad shape");
    if (n == 0 || !(dmu_out || dsigma_out || dx_out)) return RLHIP_OK;
    hipLaunchKernelGGL(normlogpdf_bwd_kernel, dim3(grid_for(n, 256)), dim3(256), 0, as_stream(stream), mu, sigma, x, dout, n, dmu_out,
                       dsigma_out, dx_out);
    RLHIP_LAUNCH_CHECK();
    return RLHIP_OK;
}

int32_t rlhip_diagnormlogpdf_bwd_f32(const float* mu, const float* sigma, const float* x, const float* dout, int64_t d, int64_t n,
                                     float* dmu_out, float* dsigma_out, float* dx_out, rlhip_stream_t stream) {
    RLHIP_REQUIRE(mu && sigma && x && dout, "NULL argument");
    RLHIP_REQUIRE(d >= 1 && d <= HEAD_MAX_D, "d must be in 1 ... 64");
    RLHIP_REQUIRE(n >= 0 && n <= 0x7FFFFFFFll * 256, "bad shape");
    if (n == 0 || !(dmu_out || dsigma_out || dx_out)) return RLHIP_OK;
    hipLaunchKernelGGL(diagnormlogpdf_bwd_kernel, dim3(grid_for(n * d, 256)), dim3(256), 0, as_stream(stream), mu, sigma, x, dout, d,
                       n * d, dmu_out, dsigma_out, dx_out);
    RLHIP_LAUNCH_CHECK();
    return RLHIP_OK;
}

int32_t rlhip_gaussian_head_logp_bwd_f32(const float* mu, const float* raw_sigma, const float* action, const float* dlogp, int64_t d,
                                         int64_t n, int64_t K, float min_sigma, float max_sigma, int32_t squash, int32_t soft,
                                         float* dmu_out, float* draw_sigma_out, rlhip_stream_t stream) {
    RLHIP_REQUIRE(mu && raw_sigma && action && dlogp, "NULL argument");
    RLHIP_HEAD_SHAPE(d, n, K);
    RLHIP_REQUIRE((squash == 0 || squash == 1) && (soft == 0 || soft == 1), "squash / soft must be 0 or 1");
    if (n == 0 || !(dmu_out || draw_sigma_out)) return RLHIP_OK;
    const dim3 grid(grid_for(n * d, 256)), block(256);
    if (soft)
        hipLaunchKernelGGL((gaussian_head_bwd_kernel<1, 0>), grid, block, 0, as_stream(stream), mu, raw_sigma, action, nullptr, dlogp,
                           (int)d, n * d, (int)K, min_sigma, max_sigma, 1, 0ull, 0u, 0u, dmu_out, draw_sigma_out);
    else
        hipLaunchKernelGGL((gaussian_head_bwd_kernel<0, 0>), grid, block, 0, as_stream(stream), mu, raw_sigma, action, nullptr, dlogp,
                           (int)d, n * d, (int)K, min_sigma, max_sigma, squash, 0ull, 0u, 0u, dmu_out, draw_sigma_out);
    RLHIP_LAUNCH_CHECK();
    return RLHIP_OK;
}

int32_t rlhip_gaussian_head_sample_bwd_f32(const float* mu, const float* raw_sigma, int64_t d, int64_t n, int64_t K, float min_sigma,
                                           float max_sigma, int32_t squash, int32_t soft, uint64_t seed, uint32_t env_id_base,
                                           uint32_t step, const float* dact, const float* dlogp, float* dmu_out,
                                           float* draw_sigma_out, rlhip_stream_t stream) {
    RLHIP_REQUIRE(mu && raw_sigma, "NULL argument");
    RLHIP_HEAD_SHAPE(d, n, K);
    RLHIP_REQUIRE((squash == 0 || squash == 1) && (soft == 0 || soft == 1), "squash / soft must be 0 or 1");
    if (soft) {
        RLHIP_REQUIRE(dact || dlogp, "NULL argument: a SoftGaussianNetwork pullback needs dact or dlogp");
    } else {
        RLHIP_REQUIRE(!dact, "dact must be NULL for soft = 0: the actions of a GaussianNetwork carry no gradient");
        RLHIP_REQUIRE(dlogp, "NULL argument");
    }
    if (n == 0 || !(dmu_out || draw_sigma_out)) return RLHIP_OK;
    const dim3 block(256);
    const char* pair_env = getenv("RLHIP_HEAD_GRAD_PAIR");  // A/B hook of tools/heads_grad_time.py: "0" = one lane per component for every d
    if (d % 2 == 0 && !(pair_env && pair_env[0] == '0')) {
        const dim3 grid(grid_for(n * d / 2, 256));
        if (soft)
            hipLaunchKernelGGL(gaussian_head_sample_bwd_pair_kernel<1>, grid, block, 0, as_stream(stream), mu, raw_sigma, dact, dlogp, (int)d,
                               n * d / 2, (int)K, min_sigma, max_sigma, seed, env_id_base, step, dmu_out, draw_sigma_out);
        else
            hipLaunchKernelGGL(gaussian_head_sample_bwd_pair_kernel<0>, grid, block, 0, as_stream(stream), mu, raw_sigma, nullptr, dlogp,
                               (int)d, n * d / 2, (int)K, min_sigma, max_sigma, seed, env_id_base, step, dmu_out, draw_sigma_out);
        RLHIP_LAUNCH_CHECK();
        return RLHIP_OK;
    }
    const dim3 grid(grid_for(n * d, 256));
    if (soft)
        hipLaunchKernelGGL((gaussian_head_bwd_kernel<1, 1>), grid, block, 0, as_stream(stream), mu, raw_sigma, nullptr, dact, dlogp,
                           (int)d, n * d, (int)K, min_sigma, max_sigma, 1, seed, env_id_base, step, dmu_out, draw_sigma_out);
    else
        hipLaunchKernelGGL((gaussian_head_bwd_kernel<0, 1>), grid, block, 0, as_stream(stream), mu, raw_sigma, nullptr, nullptr, dlogp,
                           (int)d, n * d, (int)K, min_sigma, max_sigma, squash, seed, env_id_base, step, dmu_out, draw_sigma_out);
    RLHIP_LAUNCH_CHECK();
    return RLHIP_OK;
}

}  // extern "C"
