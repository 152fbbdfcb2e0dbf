// Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC 2011), the counter-based
// generator of the samplers (ck_sample.hip).  Host and device: tests/sampling_restatement.py restates it in numpy.
//
// Contract of the samplers:
//   key     = (seed_lo, seed_hi)              the two 32-bit halves of the 64-bit seed
//   counter = (n, node, j, 0)                 n: the sample (row of the output); node: the GLOBAL fold id of the node that
//                                             draws (the fold's index in the concatenation of every layer's folds, in plan
//                                             order); j: the draw of that node (0: every node draws once per sample)
//   uniform u = (x0 >> 8) * 2^-24             in [0, 1): the categorical draw of a node takes output word x0
//   normal  z = sqrt(-2 ln u1) cos(2 pi u2)   Box-Muller on ONE call: u1 = ((x0 >> 8) + 1) * 2^-24 in (0, 1],
//                                             u2 = (x1 >> 8) * 2^-24
// A sample's draws therefore depend on (seed, n, node) only: not on the launch shape, the tile a sample falls in, or the
// order in which the nodes are visited.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define CK_PHILOX_FN __host__ __device__ __forceinline__
#else
#define CK_PHILOX_FN inline
#endif

namespace ck {

struct Philox4 {
  uint32_t x[4];
};

CK_PHILOX_FN Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
  constexpr uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u;  // round multipliers
  constexpr uint32_t W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;  // Weyl key increments
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = static_cast<uint64_t>(M0) * c0;
    const uint64_t p1 = static_cast<uint64_t>(M1) * c2;
    const uint32_t hi0 = static_cast<uint32_t>(p0 >> 32), lo0 = static_cast<uint32_t>(p0);
    const uint32_t hi1 = static_cast<uint32_t>(p1 >> 32), lo1 = static_cast<uint32_t>(p1);
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
    k0 += W0;
    k1 += W1;
  }
  return Philox4{{c0, c1, c2, c3}};
}

// u in [0, 1) with 24 random bits (exact in fp32)
CK_PHILOX_FN float philox_uniform(uint32_t x) { return static_cast<float>(x >> 8) * 5.9604644775390625e-8f; }

}  // namespace ck
