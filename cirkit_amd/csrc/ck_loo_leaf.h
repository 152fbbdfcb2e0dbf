// What the leaves of the derivative pass share ("Leave-one-out conditionals" and "Autoregressive
// conditionals and coding"): ck_loo.hip answers Q query variables per row, ck_ar.hip one query variable per row, from the
// same leaf-entry table and the same derivative arena.
#pragma once

#include <math.h>

#include "ck_down.h"

namespace ck {

__device__ __forceinline__ bool finite_d(float d) { return d > -INFINITY && d < INFINITY; }
// exp(D - m), 0 for a unit without a derivative (m is finite whenever some D is)
__device__ __forceinline__ float shifted_exp(float d, float m) { return finite_d(d) ? expf(d - m) : 0.f; }

// Per variable the entries start[q] .. start[q + 1] - 1, one per input fold over it, five int64 each: (global fold, units K,
// states C of the fold's table, element offset of its (K, C) block in `ntab` -- or of its K means / standard deviations --,
// element offset of its K log normalisers log Z_k in `lz`).
struct LooEntry {
  int64_t g, K, C, off, zoff;
};

// max_k D_k over the finite D_k of the entries s0 .. s1 - 1 at row n, strided over the lanes of a wave (not yet reduced)
__device__ __forceinline__ float entries_max(const LooEntry* __restrict__ ent, int s0, int s1, const float* __restrict__ der,
                                             const int64_t* __restrict__ val_off, int64_t n, int first, int step) {
  float mx = -INFINITY;
  for (int s = s0; s < s1; ++s) {
    const LooEntry e = ent[s];
    const float* dr = der + val_off[e.g] + n * e.K;
    for (int k = first; k < e.K; k += step)
      if (finite_d(dr[k])) mx = fmaxf(mx, dr[k]);
  }
  return mx;
}

}  // namespace ck
