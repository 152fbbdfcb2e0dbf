// What the MPE kernels (ck_mpe.hip) share with marginal MAP (ck_mmap.hip), DESIGN.md section 11: the tile shape of the upward
// contraction and the argmax walk policy.  Marginal MAP's max folds run MPE's arithmetic, and its walk policy wraps MpeArgmax.
#pragma once

#include <math.h>

#include "ck_walk.h"

namespace ck {

constexpr int kUpThreads = 256;
constexpr int kRM = 4;   // rows of a thread's register micro-tile
constexpr int kKM = 4;   // units of a thread's register micro-tile
constexpr int kMC = 16;  // entries staged in LDS per step

// ---- argmax walk ---------------------------------------------------------------------------------------------------
// The walk policy of MPE (ck::evidence_walk_kernel): rows without finite mass, and rows with bad evidence, stay empty, and
// logv[n] gets the root value (NaN where bad[n]); a sum-type unit on a tree is one wave: 64 entries at a time through the
// shared entry helper, a wave max, and the first lane of the ballot of the entries equal to it; an unobserved input takes
// its unit's argmax category or the Gaussian mean.
struct MpeArgmax {
  const int32_t* const* amax;
  const int32_t* bad;
  float* logv;

  __device__ bool root(int64_t n, float r) const {
    const bool b = bad[n] != 0;
    logv[n] = b ? NAN : r;
    return !b && isfinite(r);
  }

  __device__ int choose(const ck_sample_layer& L, const float* __restrict__ wr, const int32_t* __restrict__ ch,
                        const float* __restrict__ vals, const int64_t* __restrict__ val_off, int64_t nl, int64_t, int,
                        int lane) const {
    int choice = -1;
    float best = -INFINITY;
    for (int m0 = 0; m0 < L.M; m0 += ck::kWave) {
      const int i = m0 + lane;
      float v = -INFINITY;
      if (i < L.M) {
        const float lwi = wr[i];
        if (lwi != -INFINITY) v = ck::mpe_term(lwi, ck::entry_value(L.type, ch, L.H, L.Ki, vals, val_off, nl, i));
        if (isnan(v)) v = -INFINITY;
      }
      const float cm = ck::wave_max(v);
      if (cm > best) {  // strict: an earlier block keeps a tie
        best = cm;
        choice = m0 + __ffsll(static_cast<unsigned long long>(__ballot(v == cm))) - 1;
      }
    }
    return choice;
  }

  __device__ void fill(const ck_sample_layer& L, int li, int f, int k, int64_t, int, void* __restrict__ x, int x_float,
                       int64_t o) const {
    const int64_t u = static_cast<int64_t>(f) * L.Ko + k;
    if (L.type == CK_SAMPLE_GAUSSIAN) ck::store_value(x, x_float, o, L.mean[u]);
    else ck::store_category(x, x_float, o, amax[li][u]);
  }
};

inline int64_t blocks_of(int64_t items, int threads) { return (items + threads - 1) / threads; }

}  // namespace ck
