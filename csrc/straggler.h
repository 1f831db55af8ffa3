// The reference's straggler model (SparkASGDThread.scala:124-141 selection,
// :287-312 injection, :177-186,:247-252 calibration) as pure host+device
// functions: the ONE copy the native engine (async and sync), the dist
// server and the resident engine's server block all run. HIP-free, like
// philox_core.h. engine/delay.py is the Python counterpart; the two differ
// only where Python's half-to-even round() and C's half-away round() differ
// (docs/TESTING.md).
#pragma once
#include <cmath>
#include <cstdint>

#include "philox_core.h"

namespace straggler {

// 0 none, 1 normal (1.5-2.5x), 2 long-tail (2.5-10x). 25% of the P workers
// straggle: length = round(0.25 P) of them at wid = c*4, the first
// length - round(0.8 length) long-tail, the rest normal.
ASYNCAMD_HD inline int kind(long long P, long long wid) {
  const int length = (int)std::lround(0.25 * (double)P);
  const int length_normal = (int)std::lround(0.8 * length);
  const int length_longtail = length - length_normal;
  if (wid < 0 || wid >= P || wid % 4 != 0) return 0;
  const long long c = wid / 4;
  if (c >= length) return 0;
  return (c < length_longtail) ? 2 : 1;
}

// Injected delay in ms for worker ``wid`` at round ``round_k``. ``active``
// is the calibration's delay_flag. coeff: 0 off, -1 the cloud long-tail
// model, > 0 slows worker 0 alone by coeff * avg.
ASYNCAMD_HD inline double delay_ms(long long P, double coeff, uint64_t seed,
                                   double avg_delay_ms, bool active,
                                   long long wid, long long round_k) {
  if (!active || coeff == 0.0) return 0.0;
  if (coeff != -1.0) {
    if (wid == 0 && coeff > 0) return std::round(coeff * avg_delay_ms);
    return 0.0;
  }
  const int kd = kind(P, wid);
  if (kd == 2) {
    const double u = philox_uniform01(seed, (uint32_t)round_k, (uint32_t)wid);
    return std::round((u * 7.5 + 2.5) * avg_delay_ms);
  }
  if (kd == 1) {
    const double u = philox_uniform01(seed, (uint32_t)round_k, (uint32_t)wid);
    return std::round((u + 1.5) * avg_delay_ms);
  }
  return 0.0;
}

// Calibration of avg_delay_ms from task times. The caller decides which
// tasks are samples (its window test); the first activation check with
// k > window fixes the average and raises the flag for good.
struct Calibration {
  double cul_time_ms = 0;
  long long cul_count = 0;
  double avg_delay_ms = 0;
  bool delay_flag = false;

  ASYNCAMD_HD void record(double ms, long long n) {
    cul_time_ms += ms;
    cul_count += n;
  }

  ASYNCAMD_HD void maybe_activate(long long k, long long window) {
    if (delay_flag || k <= window) return;
    if (cul_count > 0) avg_delay_ms = cul_time_ms / (double)cul_count;
    delay_flag = true;
  }
};

}  // namespace straggler
