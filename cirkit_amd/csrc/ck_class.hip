// The class head of a class-conditional circuit ("Classification"): from the (B, C) class
// log-likelihoods of the root fold to the loss statistics, the posterior, the prediction and the gradient seed, in one launch
// plus a fixed-order finisher for the statistics.
//
//   j_bc = l_bc + pi_c,  m_b = max_c j_bc (lowest c on ties),  e_b = m_b + log1p(sum_{c != argmax} exp(j_bc - m_b)),
//   q_bc = (j_bc - m_b) - (e_b - m_b)
//
// One row per group of G lanes, G the next power of two >= C capped at 64 (a wave holds 64 / G rows; classes beyond 64 are
// walked in chunks of 64 and re-read from the cache).  The sum l + pi and the row maximum are formed in double, so the one
// rounding of the exponent's argument is that of the DIFFERENCE j - m (exact whenever the two share a binade), not that of
// two values of magnitude |j|; everything behind it is fp32.  Reductions inside a group are xor shuffles below G; no LDS
// besides the block's partial statistics.
#include <algorithm>
#include <cmath>

#include "ck_internal.h"

namespace {

constexpr int kThreads = 256;
constexpr int kStats = CK_CLASS_NUM_STATS;

template <int G, class T>
__device__ __forceinline__ T group_sum(T v) {
#pragma unroll
  for (int o = 1; o < G; o <<= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// per-block partial statistics: [sum gen, sum disc, live, labelled live, correct, dead] (fp64; the counts are exact)
template <int G>
__global__ void __launch_bounds__(kThreads)
    class_head_kernel(const float* __restrict__ x, int B, int C, int stride, const int64_t* __restrict__ labels,
                      const float* __restrict__ log_prior, float uniform_lp, float w_gen, float w_disc, float inv_gb,
                      float* __restrict__ seed, float* __restrict__ log_post, float* __restrict__ log_evid,
                      int64_t* __restrict__ pred, double* __restrict__ partials, int32_t* __restrict__ bad_flag) {
  __shared__ double part[kThreads / 64][kStats];
  constexpr int kGroups = kThreads / G;
  const int lane = threadIdx.x & (G - 1), group = threadIdx.x / G;
  double acc[kStats] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};  // (meaningful on lane 0 of a group; zero elsewhere)

  // every lane of the block takes every trip (the shuffles below want whole waves); `valid` masks the ragged end
  for (int64_t row0 = static_cast<int64_t>(blockIdx.x) * kGroups; row0 < B; row0 += static_cast<int64_t>(gridDim.x) * kGroups) {
    const int64_t row = row0 + group;
    const bool valid = row < B;
    const float* xr = x + (valid ? row : 0) * stride;
    const int64_t y = (labels != nullptr && valid) ? labels[row] : -1;
    auto prior = [&](int c) { return static_cast<double>(log_prior != nullptr ? log_prior[c] : uniform_lp); };
    auto joint = [&](int c) { return static_cast<double>(xr[c]) + prior(c); };

    // pass 1: the row maximum with its lowest index, NaN anywhere in the row
    double m = -INFINITY, j0 = -INFINITY;
    int mi = 0x7fffffff, nan = 0;
    for (int c = lane; c < C; c += G) {
      const double j = joint(c);
      if (c == lane) j0 = j;
      nan |= (j != j);
      if (j > m || (j == m && c < mi)) m = j, mi = c;
    }
#pragma unroll
    for (int o = 1; o < G; o <<= 1) {
      const double om = __shfl_xor(m, o, 64);
      const int oi = __shfl_xor(mi, o, 64);
      nan |= __shfl_xor(nan, o, 64);
      if (om > m || (om == m && oi < mi)) m = om, mi = oi;
    }
    auto shifted = [&](int c) { return static_cast<float>((c == lane ? j0 : joint(c)) - m); };  // j - m, rounded once

    // pass 2: e - m = log1p(sum over the classes other than the argmax)
    float s = 0.f;
    for (int c = lane; c < C; c += G)
      if (c != mi) s += expf(shifted(c));
    s = group_sum<G>(s);
    const float logs = log1pf(s);
    const bool finite_e = !nan && m > -INFINITY && m < INFINITY;

    const bool bad = labels != nullptr && valid && (y < -1 || y >= C);
    const bool labelled = y >= 0 && y < C;
    const double jy = labelled ? joint(static_cast<int>(y)) : 0.0;
    const bool dead = !finite_e || bad || (labelled && !(jy > -INFINITY));

    // pass 3: posterior and seed
    const float nan_f = __builtin_nanf("");
    for (int c = lane; c < C && valid; c += G) {
      const float d = shifted(c);
      const float q = d - logs;
      if (log_post != nullptr) log_post[row * C + c] = finite_e ? q : nan_f;
      if (seed != nullptr) {
        float v = 0.f;
        if (!dead && d > -INFINITY) {
          const float p = expf(q);
          const float delta = (labelled && c == y) ? 1.f : 0.f;
          v = labelled ? -inv_gb * (w_gen * delta + w_disc * (delta - p)) : -inv_gb * (w_gen * p);
        }
        seed[row * stride + c] = v;
      }
    }
    if (seed != nullptr && valid)
      for (int c = C + lane; c < stride; c += G) seed[row * stride + c] = 0.f;  // padded units take no gradient

    if (lane == 0 && valid) {
      if (pred != nullptr) pred[row] = finite_e ? mi : -1;
      if (log_evid != nullptr)  // (an impossible row has log p(x) = -inf; only a NaN or +inf in the row gives NaN)
        log_evid[row] = finite_e ? static_cast<float>(m + static_cast<double>(logs)) : ((!nan && m < INFINITY) ? -INFINITY : nan_f);
      if (bad && bad_flag != nullptr) *bad_flag = 1;
      if (dead) {
        acc[5] += 1.0;
      } else {
        acc[2] += 1.0;
        if (labelled) {
          const float qy = static_cast<float>(jy - m) - logs;
          acc[0] += jy;
          acc[1] += static_cast<double>(qy);
          acc[3] += 1.0;
          acc[4] += (mi == y) ? 1.0 : 0.0;
        } else {
          acc[0] += m + static_cast<double>(logs);
        }
      }
    }
  }

  if (partials == nullptr) return;
  // groups of a wave, then the waves of the block, then (finisher) the blocks: always in the same order
#pragma unroll
  for (int k = 0; k < kStats; ++k) {
    double v = acc[k];
#pragma unroll
    for (int o = G; o < 64; o <<= 1) v += __shfl_xor(v, o, 64);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6][k] = v;
  }
  __syncthreads();
  if (threadIdx.x < kStats) {
    double t = 0.0;
    for (int w = 0; w < kThreads / 64; ++w) t += part[w][threadIdx.x];
    partials[static_cast<int64_t>(blockIdx.x) * kStats + threadIdx.x] = t;
  }
}

__global__ void __launch_bounds__(64) class_stats_kernel(const double* __restrict__ partials, int n_blocks, double* __restrict__ stats) {
  if (threadIdx.x < kStats) {
    double t = 0.0;
    for (int b = 0; b < n_blocks; ++b) t += partials[static_cast<int64_t>(b) * kStats + threadIdx.x];
    stats[threadIdx.x] = t;
  }
}

template <int G>
int launch_head(int n_blocks, void* stream, const float* x, int B, int C, int stride, const int64_t* labels, const float* log_prior,
                float uniform_lp, float w_gen, float w_disc, float inv_gb, float* seed, float* log_post, float* log_evid,
                int64_t* pred, double* partials, int32_t* bad_flag) {
  return ck::launch(class_head_kernel<G>, dim3(n_blocks), dim3(kThreads), 0, stream, x, B, C, stride, labels, log_prior, uniform_lp,
                    w_gen, w_disc, inv_gb, seed, log_post, log_evid, pred, partials, bad_flag);
}

}  // namespace

extern "C" {

int ck_class_head(const float* x, int B, int C, int stride, const int64_t* labels, const float* log_prior, float w_gen, float w_disc,
                  float inv_gb, float* seed, float* log_post, float* log_evid, int64_t* pred, double* stats, double* partials,
                  int32_t* bad_flag, void* stream) {
  CK_REQUIRE(x != nullptr, "ck_class_head: null input block");
  CK_REQUIRE(B > 0 && C > 0 && stride >= C, "ck_class_head: B %d, C %d, stride %d", B, C, stride);
  CK_REQUIRE((stats == nullptr) == (partials == nullptr), "ck_class_head: stats and partials come together");
  CK_REQUIRE(std::isfinite(w_gen) && std::isfinite(w_disc) && std::isfinite(inv_gb), "ck_class_head: non-finite weight");
  int G = 1;
  while (G < C && G < 64) G <<= 1;
  const int rows_per_block = kThreads / G;
  // the cap bounds the `partials` scratch the caller lends (and the finisher's loop); the grid-stride loop covers the rest
  const int n_blocks = static_cast<int>(std::min<int64_t>((static_cast<int64_t>(B) + rows_per_block - 1) / rows_per_block,
                                                           CK_CLASS_MAX_BLOCKS));
  const float uniform_lp = static_cast<float>(-std::log(static_cast<double>(C)));
  int st;
#define CK_HEAD(g)                                                                                                              \
  case g:                                                                                                                       \
    st = launch_head<g>(n_blocks, stream, x, B, C, stride, labels, log_prior, uniform_lp, w_gen, w_disc, inv_gb, seed, log_post, \
                        log_evid, pred, partials, bad_flag);                                                                    \
    break;
  switch (G) {
    CK_HEAD(1)
    CK_HEAD(2)
    CK_HEAD(4)
    CK_HEAD(8)
    CK_HEAD(16)
    CK_HEAD(32)
    default:
      st = launch_head<64>(n_blocks, stream, x, B, C, stride, labels, log_prior, uniform_lp, w_gen, w_disc, inv_gb, seed, log_post,
                           log_evid, pred, partials, bad_flag);
  }
#undef CK_HEAD
  if (st != 0 || stats == nullptr) return st;
  return ck::launch(class_stats_kernel, dim3(1), dim3(64), 0, stream, partials, n_blocks, stats);
}

}  // extern "C"
