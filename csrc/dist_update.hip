// Fused update kernels for the C++ dist server (csrc/server_dist.cpp): one
// HIP launch on the server's stream instead of the aten add_ chain (1-3
// dispatcher launches per update on the default stream, ROADMAP §1). The
// arithmetic is the local engines' own — the REG=false steps of
// update_step.h, which this separately built extension includes too.

#include <hip/hip_runtime.h>
#include "dist_launchers.h"  // checks the two definitions below
#include "update_step.h"

namespace {

__global__ void dist_sgd_update_kernel(float* __restrict__ w,
                                       const float* __restrict__ g,
                                       float gamma_k, float inv_batch,
                                       int d) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < d) asgd_step<false>(w[i], g[i], gamma_k * inv_batch);
}

__global__ void dist_saga_update_kernel(float* __restrict__ w,
                                        const float* __restrict__ g,
                                        float* __restrict__ alpha_bar,
                                        float gamma, float inv_batch,
                                        float inv_N, int d) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < d)
    saga_step<false>(w[i], alpha_bar[i], g[i], gamma, inv_batch, inv_N);
}

}  // namespace

extern "C" {

void launch_dist_sgd_update(float* w, const float* g, float gamma_k,
                            float inv_batch, int d, hipStream_t stream) {
  const int grid = (d + 255) / 256;
  hipLaunchKernelGGL(dist_sgd_update_kernel, dim3(grid), dim3(256), 0,
                     stream, w, g, gamma_k, inv_batch, d);
}

void launch_dist_saga_update(float* w, const float* g, float* alpha_bar,
                             float gamma, float inv_batch, float inv_N,
                             int d, hipStream_t stream) {
  const int grid = (d + 255) / 256;
  hipLaunchKernelGGL(dist_saga_update_kernel, dim3(grid), dim3(256), 0,
                     stream, w, g, alpha_bar, gamma, inv_batch, inv_N, d);
}

}  // extern "C"
