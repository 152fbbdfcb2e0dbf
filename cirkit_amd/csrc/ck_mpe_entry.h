// The value of one entry of a max-product unit ("Most probable explanation"), shared by the upward
// pass and the argmax walk of ck_mpe.hip: the walk recomputes the entries of a unit with the same instructions on the same
// operands, so the maximum it finds is bit for bit the unit value the upward pass stored, and the argmax is exact.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/cirkit_hip.h"

namespace ck {

// One v_add_f32 / v_max3_f32 each.  A plain -O3 build may SLP-pack neighbouring f32 adds into v_pk_add_f32 (register
// pairs, extra moves) and put canonicalising v_max_f32 around fmaxf; the max-plus loop is exactly these two instructions.
__device__ __forceinline__ float mpe_add(float a, float b) {
  float r;
  asm("v_add_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}
__device__ __forceinline__ float mpe_max3(float a, float b, float c) {
  float r;
  asm("v_max3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
  return r;
}

// Child value of entry i of a sum-type unit at chunk row nl.  ch: the fold's (H) global child fold ids; val_off[g] + nl Ki
// is the start of child fold g's Ki values at that row.  Sum / mixing: unit i % Ki of input i / Ki; CP-T: unit i of every
// input, added in input order; Tucker (arity 2): v0[i / Ki] + v1[i % Ki].
__device__ __forceinline__ float mpe_entry(int type, const int32_t* __restrict__ ch, int H, int Ki,
                                           const float* __restrict__ vals, const int64_t* __restrict__ val_off, int64_t nl,
                                           int i) {
  const int64_t r = nl * Ki;
  if (type == CK_SAMPLE_SUM) return vals[val_off[ch[i / Ki]] + r + i % Ki];
  if (type == CK_SAMPLE_CPT) {
    float v = vals[val_off[ch[0]] + r + i];
    for (int h = 1; h < H; ++h) v = mpe_add(v, vals[val_off[ch[h]] + r + i]);
    return v;
  }
  return mpe_add(vals[val_off[ch[0]] + r + i / Ki], vals[val_off[ch[1]] + r + i % Ki]);  // CK_SAMPLE_TUCKER
}

// Value of the entry under its log weight: log w + entry (log w = -inf for w <= 0).
__device__ __forceinline__ float mpe_term(float lw, float e) { return mpe_add(lw, e); }

// log N(x; mu, sd) (+ log_partition), as the Gaussian forward computes it; at x = mu it is the unit's maximum.
__device__ __forceinline__ float mpe_gauss(float x, float mu, float sd, const float* lz, int64_t o) {
  const float inv_two_var = 1.f / (2.f * (sd * sd));
  const float d = x - mu;
  float lp = -(d * d) * inv_two_var - __logf(sd) - 0.91893853320467274178f;
  if (lz != nullptr) lp += lz[o];
  return lp;
}

}  // namespace ck
