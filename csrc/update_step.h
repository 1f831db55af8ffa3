// The weight-update step, once: every update kernel (csrc/kernels.hip and
// the dist server's csrc/dist_update.hip) applies one of the two scalar
// steps below to the value it already holds in a register.
//
// REG=true is the elastic-net form, which minimises
//   F(w) = (1/N) sum_i f_i(w) + (l2/2)|w|^2 + l1*|w|_1
// with one step per applied update:
//   v = w - eta*(ghat + l2*w)                  L2: exact gradient step
//   w = v > t ? v - t : (v < -t ? v + t : +0)  L1: prox, t = eta*l1
// written as v = fma(-step, g, dec*w) with dec = fma(-eta, l2, 1) — for
// l1 = 0 literally MLlib's SquaredL2Updater w*(1 - eta*l2) - eta*ghat, for
// l2 = 0 its L1Updater. Every product and sum of the REG=true bodies is an
// explicit single-rounding intrinsic, so the rounding count the tests assume
// does not depend on the contraction mode. The REG=false bodies are the
// plain expressions the unregularised kernels have always compiled (their
// bits DO follow the contraction mode, so the expressions must not change).
#pragma once

#include <hip/hip_runtime.h>

__device__ __forceinline__ float reg_dec(float eta, float l2) {
  return fmaf(-eta, l2, 1.f);
}
__device__ __forceinline__ float reg_thr(float eta, float l1) {
  return __fmul_rn(eta, l1);
}
// |v| - t is computed unconditionally and its sign decides (v - t for
// v > t and v + t for v < -t are +-(|v| - t) with the same single rounding;
// anything else, a NaN included, is +0): two selects, no divergent branch —
// the nested-ternary form compiled to an exec-mask branch per element.
__device__ __forceinline__ float reg_prox(float v, float t) {
  const float a = __fsub_rn(fabsf(v), t);
  return a > 0.f ? copysignf(a, v) : 0.f;
}
// v for a step whose data term is step*g
__device__ __forceinline__ float reg_step(float w, float g, float step,
                                          float dec, float t) {
  return reg_prox(fmaf(-step, g, __fmul_rn(dec, w)), t);
}

// ASGD: w -= scale*g. REG: dec = reg_dec(eta, l2), t = reg_thr(eta, l1) for
// the step's bare eta (scale may carry further divisors).
template <bool REG>
__device__ __forceinline__ void asgd_step(float& w, float g, float scale,
                                          float dec = 1.f, float t = 0.f) {
  if constexpr (REG) w = reg_step(w, g, scale, dec, t);
  else w -= scale * g;
}

// SAGA: w -= gamma*(inv_batch*g + alpha_bar_old); alpha_bar += inv_N*g —
// w reads the OLD alpha_bar (reference SparkASAGASync.scala:300-304 /
// SparkASAGAThread.scala:217-220). REG is prox-SAGA: ghat = inv_batch*g +
// alpha_bar_old, eta = gamma; the penalty stays out of alpha_bar (and out of
// the history table).
template <bool REG>
__device__ __forceinline__ void saga_step(float& w, float& ab, float g,
                                          float gamma, float inv_batch,
                                          float inv_N, float dec = 1.f,
                                          float t = 0.f) {
  if constexpr (REG) {
    w = reg_step(w, fmaf(inv_batch, g, ab), gamma, dec, t);
    ab = fmaf(inv_N, g, ab);
  } else {
    w -= gamma * (inv_batch * g + ab);
    ab += inv_N * g;
  }
}

// f(v0, v1, ...) once per float component of the operands, which are all
// float or all float4: the vectorised kernels spell a scalar step once.
template <int C, typename V>
__device__ __forceinline__ auto& lane_of(V& v) {
  if constexpr (sizeof(V) == sizeof(float)) return v;
  else if constexpr (C == 0) return v.x;
  else if constexpr (C == 1) return v.y;
  else if constexpr (C == 2) return v.z;
  else return v.w;
}
template <typename F, typename... V>
__device__ __forceinline__ void for_lanes(F&& f, V&... v) {
  f(lane_of<0>(v)...);
  if constexpr (((sizeof(V) == sizeof(float4)) && ...)) {
    f(lane_of<1>(v)...);
    f(lane_of<2>(v)...);
    f(lane_of<3>(v)...);
  }
}
