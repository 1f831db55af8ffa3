// The one declaration of the two _dist_core launchers: csrc/dist_update.hip
// defines them, csrc/server_dist.cpp calls them (inside its
// __HIP_PLATFORM_AMD__ guard only — this header names a HIP type).
#pragma once
#include <hip/hip_runtime_api.h>

extern "C" {

void launch_dist_sgd_update(float* w, const float* g, float gamma_k,
                            float inv_batch, int d, hipStream_t stream);

void launch_dist_saga_update(float* w, const float* g, float* alpha_bar,
                             float gamma, float inv_batch, float inv_N,
                             int d, hipStream_t stream);

}  // extern "C"
