// dist.hip -- the launches the distributional learners share (csrc/c51.hip, csrc/qrdqn.hip, csrc/iqn.hip): the reduction of the
// workgroups' partial rows, and the debug build's check of the batch's actions (also rlhip_dqn_grad_batch_f32's, csrc/dqn_batch.hip).
// The check is compiled in by RLHIP_BOUNDS_CHECK, and that macro is named HERE, not in a header: the `bounds` variant of build.py
// recompiles the sources whose own text names it.
#include "dist_host.h"

namespace rlhip {

// gradient element p and the loss: the partial rows / losses of workgroups 0, 1, .. in ascending order, from +0
__global__ __launch_bounds__(256) void dist_reduce_kernel(const float* __restrict__ partials, const float* __restrict__ loss_partials, int nb,
                                                          int np, float* __restrict__ grad, float* __restrict__ loss, float fb) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p < np) {
        float acc = 0.f;
#pragma unroll 8
        for (int b = 0; b < nb; ++b) acc += partials[(int64_t)b * np + p];
        grad[p] = acc;
    }
    if (p == 0) {
        float a = 0.f;
        for (int b = 0; b < nb; ++b) a += loss_partials[b];
        loss[0] = a / fb;
    }
}

int32_t dist_reduce_launch(const float* partials, const float* loss_partials, int64_t nb, int64_t np, float* grad, float* loss, float fb,
                           hipStream_t st) {
    hipLaunchKernelGGL(dist_reduce_kernel, dim3((int)((np + 255) / 256)), dim3(256), 0, st, partials, loss_partials, (int)nb, (int)np, grad,
                       loss, fb);
    RLHIP_LAUNCH_CHECK();
    return RLHIP_OK;
}

#ifdef RLHIP_BOUNDS_CHECK
__global__ __launch_bounds__(256) void dist_count_bad_actions_kernel(const int32_t* __restrict__ a, int64_t batch, int na, int* __restrict__ n_bad) {
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b < batch && (a[b] < 0 || a[b] >= na)) atomicAdd(n_bad, 1);
}
#endif

int32_t dist_check_actions(const int32_t* a, int64_t batch, int64_t na, void* workspace, hipStream_t st, const char* file, int line) {
#ifdef RLHIP_BOUNDS_CHECK
    int* cnt = (int*)workspace;
    int n_bad = 0;
    RLHIP_CHECK_HIP(hipMemsetAsync(cnt, 0, sizeof(int), st));
    hipLaunchKernelGGL(dist_count_bad_actions_kernel, dim3((int)((batch + 255) / 256)), dim3(256), 0, st, a, batch, (int)na, cnt);
    RLHIP_LAUNCH_CHECK();
    RLHIP_CHECK_HIP(hipMemcpyAsync(&n_bad, cnt, sizeof(int), hipMemcpyDeviceToHost, st));
    RLHIP_CHECK_HIP(hipStreamSynchronize(st));
    if (n_bad) {
        ::rlhip::set_error("%s:%d: %d of %lld actions are outside 0 .. %lld", file, line, n_bad, (long long)batch, (long long)na - 1);
        return RLHIP_EINVAL;
    }
#endif
    return RLHIP_OK;
}

}  // namespace rlhip
