// The categorical draw of the samplers (ck_sample.hip, ck_sample_cond.hip) from a CDF row of unnormalised masses.
#pragma once

#include <hip/hip_runtime.h>

namespace ck {

// smallest i with t < cdf[i]: an entry whose own mass is positive (t < T is guaranteed by the caller)
__device__ __forceinline__ int cdf_search(const float* __restrict__ row, int M, float t) {
  int lo = 0, hi = M - 1;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (t < row[mid]) hi = mid;
    else lo = mid + 1;
  }
  return lo;
}

__device__ __forceinline__ int cdf_draw(const float* __restrict__ row, int M, float u) {
  const float T = row[M - 1];
  if (!(T > 0.f)) return 0;  // (a row with no mass is never reached from a root of positive mass)
  float t = u * T;
  if (t >= T) t = __int_as_float(__float_as_int(T) - 1);  // the float below T (T > 0)
  return cdf_search(row, M, t);
}

}  // namespace ck
