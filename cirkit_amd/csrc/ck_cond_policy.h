// The walk policy of conditional sampling (ck_sample_cond.hip), shared with the soft-evidence decoding walks
// (ck_soft_decode.hip), DESIGN.md section 11: as MpeArgmax is in ck_mpe_policy.h.
#pragma once

#include <math.h>

#include "ck_walk.h"

namespace ck {

// The walk policy of conditional sampling (ck::evidence_walk_kernel): a row whose evidence has no finite mass draws nothing;
// a sum-type unit draws entry i in proportion to w_i exp(v_i), from its (F, Ko, M) linear weights; an unobserved input
// draws from its unconditional CDF row or Gaussian.  Random numbers as the unconditional walk's.
struct CondDraw {
  uint32_t key0, key1;

  __device__ bool root(int64_t, float r) const { return isfinite(r); }

  __device__ int choose(const ck_sample_layer& L, const float* __restrict__ wr, const int32_t* __restrict__ ch,
                        const float* __restrict__ vals, const int64_t* __restrict__ val_off, int64_t nl, int64_t n, int g,
                        int lane) const {
    // log mass of entry i minus log w_i: -inf for a weight <= 0 (its child value is not read) or a NaN value
    auto logv = [&](int i, float& wi) -> float {
      wi = wr[i];
      if (!(wi > 0.f)) return -INFINITY;
      const float v = ck::entry_value(L.type, ch, L.H, L.Ki, vals, val_off, nl, i);
      return isnan(v) ? -INFINITY : v;
    };
    float w0 = 0.f;  // the first 64 entries stay in registers (one memory pass when M <= 64)
    const float l0 = lane < L.M ? logv(lane, w0) : -INFINITY;
    float vmax = l0;
    for (int m0 = ck::kWave; m0 < L.M; m0 += ck::kWave) {
      float wi;
      if (m0 + lane < L.M) vmax = fmaxf(vmax, logv(m0 + lane, wi));
    }
    vmax = ck::wave_max(vmax);
    if (!isfinite(vmax)) return -1;
    // inclusive scan of c_i = w_i exp(v_i - vmax) over the 64 entries from m0; the same arithmetic in both passes,
    // so the total T of the first pass is bit for bit the last CDF value of the second
    auto scan = [&](int m0) -> float {
      float c = 0.f, wi = w0;
      if (m0 + lane < L.M) {
        const float l = m0 == 0 ? l0 : logv(m0 + lane, wi);
        if (l != -INFINITY) c = wi * expf(l - vmax);
      }
#pragma unroll
      for (int d = 1; d < ck::kWave; d <<= 1) {
        const float o = __shfl_up(c, d);
        if (lane >= d) c += o;
      }
      return c;
    };
    const float c0 = scan(0);
    float T = __shfl(c0, ck::kWave - 1);
    for (int m0 = ck::kWave; m0 < L.M; m0 += ck::kWave) T += __shfl(scan(m0), ck::kWave - 1);
    float t = ck::philox_uniform(ck::walk_philox(n, g, key0, key1).x[0]) * T;
    if (t >= T) t = __int_as_float(__float_as_int(T) - 1);  // the float below T (T >= the largest w_i > 0)
    float carry = 0.f;
    int last = -1;  // the last entry that raised the CDF so far
    for (int m0 = 0; m0 < L.M; m0 += ck::kWave) {
      const float c = m0 == 0 ? c0 : scan(m0);
      const uint64_t hit = __ballot(m0 + lane < L.M && t < carry + c);
      if (hit != 0) return m0 + __ffsll(static_cast<unsigned long long>(hit)) - 1;
      const float prev = __shfl_up(c, 1);
      const uint64_t up = __ballot(m0 + lane < L.M && c > (lane == 0 ? 0.f : prev));
      if (up != 0) last = m0 + 63 - __clzll(static_cast<long long>(up));
      carry += __shfl(c, ck::kWave - 1);
    }
    // (T and the last CDF value come from the same arithmetic, so t < T always hits; should a compiler ever contract
    // the two scans differently, t within rounding of T takes the last entry with mass instead of drawing nothing)
    return last;
  }

  __device__ void fill(const ck_sample_layer& L, int, int f, int k, int64_t n, int g, void* __restrict__ x, int x_float,
                       int64_t o) const {
    ck::draw_input(L, f, k, ck::walk_philox(n, g, key0, key1), x, x_float, o);
  }
};

}  // namespace ck
