// The link function: a row's scalar gradient coefficient e from its score
// z = x.w and label y, for every gradient kernel (csrc/kernels.hip and the
// resident engine). The objective code travels as an int from Python
// (ops._OBJ_CODE, engine/native.py::_OBJ):
//   0 lsq      e = z - y
//   1 logistic e = sigmoid(z) - y
//   2 hinge    e = -s when 1 > s*z, else 0, with s = 2y - 1 for labels in
//              {0,1} (MLlib HingeGradient; the inequality is strict, so a
//              row exactly on the margin contributes nothing)
// e is one scalar per row for all three, which is all the SAGA history
// (alpha, the staged scalars, alpha_bar) ever stores.
//
// HINGE is a template argument of the gradient kernels, chosen by their
// launchers from the objective code: the lsq / logistic instantiations are
// then the very code they were before hinge existed. A third runtime case
// inside the one body moved the register allocation of the pipelined
// kernels (a few shapes crossed a waves-per-SIMD step: 128 -> 130 VGPRs),
// although the link itself needs two registers at most.
#pragma once

#include <hip/hip_runtime.h>

template <bool HINGE>
__device__ __forceinline__ float link_residual(float z, float yv, int obj) {
  if constexpr (HINGE) {
    // never taken (the launchers pick HINGE from obj == 2), but it keeps
    // the shape the other instantiations have — a uniform branch around the
    // link — and with it their register allocation: without it the hinge
    // forms of the pipelined kernels took up to 22 more VGPRs than their
    // twins and two of them spilled
    if (obj != 2) return z - yv;
    const float s = 2.0f * yv - 1.0f;
    return 1.0f > s * z ? -s : 0.0f;
  } else {
    if (obj == 1) return 1.0f / (1.0f + __expf(-z)) - yv;  // logistic
    return z - yv;                                         // lsq
  }
}

// the objective code as a runtime value (resident engine)
__device__ __forceinline__ float link_residual_rt(float z, float yv,
                                                  int obj) {
  return obj == 2 ? link_residual<true>(z, yv, obj)
                  : link_residual<false>(z, yv, obj);
}
