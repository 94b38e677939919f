// Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11; the Random123 constants and round
// function) in plain integer C++, the same function on the host (tacex_philox4x32) and in the kernels that draw random numbers
// (fem_marker_flow_library_kernel).  Counter-based: the output depends on (counter, key) alone, so a draw is addressed, not consumed.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define TACEX_HD __host__ __device__
#else
#define TACEX_HD
#endif

namespace tacex {

TACEX_HD inline void philox4x32_10(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4]) {
  const uint32_t kM0 = 0xD2511F53u, kM1 = 0xCD9E8D57u;  // multipliers
  const uint32_t kW0 = 0x9E3779B9u, kW1 = 0xBB67AE85u;  // Weyl increments of the key (golden ratio, sqrt(3) - 1)
  uint32_t c0 = ctr[0], c1 = ctr[1], c2 = ctr[2], c3 = ctr[3], k0 = key[0], k1 = key[1];
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)kM0 * c0, p1 = (uint64_t)kM1 * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    k0 += kW0; k1 += kW1;  // (the bump after the last round is unused)
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// uniform in (0, 1) from one 32-bit word: (w + 0.5) * 2^-32, exact in float64 - never 0, never 1
TACEX_HD inline double philox_uniform(uint32_t w) { return ((double)w + 0.5) * (1.0 / 4294967296.0); }

}  // namespace tacex
