// Philox4x32-10, written once for host and device. Plain C++17 with no HIP
// include, so the host-only dist server (csrc/server_dist.cpp) and the HIP
// translation units share the same rounds. MUST stay bit-identical to the
// numpy reference in asyncframework_amd/utils/philox.py.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define ASYNCAMD_HD __host__ __device__
#else
#define ASYNCAMD_HD
#endif

// The ten rounds, in place on the four counter words; key = (seed_lo,
// seed_hi).
ASYNCAMD_HD inline __attribute__((always_inline)) void philox4x32_10(
    uint64_t seed, uint32_t& c0, uint32_t& c1, uint32_t& c2, uint32_t& c3) {
  uint32_t k0 = (uint32_t)(seed & 0xFFFFFFFFull);
  uint32_t k1 = (uint32_t)(seed >> 32);
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int r = 0; r < 10; ++r) {
    uint64_t p0 = 0xD2511F53ull * (uint64_t)c0;
    uint64_t p1 = 0xCD9E8D57ull * (uint64_t)c2;
    uint32_t hi0 = (uint32_t)(p0 >> 32), lo0 = (uint32_t)p0;
    uint32_t hi1 = (uint32_t)(p1 >> 32), lo1 = (uint32_t)p1;
    uint32_t n0 = hi1 ^ c1 ^ k0;
    uint32_t n1 = lo1;
    uint32_t n2 = hi0 ^ c3 ^ k1;
    uint32_t n3 = lo0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
}

// One uniform in [0, 1) from counters (0, 0, round, stream): the straggler
// draw (utils/philox.py uniform01 with n = 1). A 32-bit integer over 2^32,
// so exact in fp64.
ASYNCAMD_HD inline double philox_uniform01(uint64_t seed, uint32_t round_k,
                                           uint32_t stream) {
  uint32_t c0 = 0u, c1 = 0u, c2 = round_k, c3 = stream;
  philox4x32_10(seed, c0, c1, c2, c3);
  return c0 / 4294967296.0;
}
