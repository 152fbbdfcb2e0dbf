// Exact ancestral sampling of a smooth, decomposable, monotonic circuit: the prepare launch turns
// weights and child partition functions into conditional CDF rows, the walk launch draws samples top down.
#include <math.h>

#include "ck_internal.h"
#include "ck_walk.h"

namespace {

constexpr int kWalkThreads = 256;
constexpr int kCdfRowsPerBlock = 4;  // one wave per row

// CDF row r = (f, k) of length M:  c_i = w[f, k, i] * exp(lz[f, i] - max), CDF_i = c_0 + ... + c_i.  Entries with w = 0
// contribute exactly 0 whatever their lz is (padded units).  flag |= 1: a negative weight; |= 2: a NaN weight, or a
// NaN / +inf log-weight or child log Z under a positive weight.
__global__ void __launch_bounds__(kCdfRowsPerBlock * ck::kWave)
    sample_cdf_kernel(const float* __restrict__ w, int64_t w_sf, int64_t w_sk, int64_t w_sm, int w_log,
                      const float* __restrict__ lz, int R, int M, int64_t rows, float* __restrict__ cdf, int32_t* flag) {
  const int lane = threadIdx.x & (ck::kWave - 1);
  const int64_t row = static_cast<int64_t>(blockIdx.x) * kCdfRowsPerBlock + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int64_t f = row / R, k = row % R;
  const float* wr = w + f * w_sf + k * w_sk;
  const float* lr = lz == nullptr ? nullptr : lz + f * M;
  float* out = cdf + row * M;
  int bad = 0;
  auto logw = [&](int m) -> float {  // log of the entry's weight times its child's Z, -inf for a zero weight
    const float v = wr[m * w_sm];
    float lw;
    if (w_log) {
      if (isnan(v) || v == INFINITY) bad |= 2;
      lw = v;
    } else {
      if (v < 0.f) bad |= 1;
      if (isnan(v)) bad |= 2;
      lw = v > 0.f ? logf(v) : -INFINITY;
    }
    if (lw == -INFINITY || isnan(lw)) return -INFINITY;
    if (lr != nullptr) {
      const float z = lr[m];
      if (isnan(z) || z == INFINITY) bad |= 2;
      lw = isnan(z) ? -INFINITY : lw + z;
    }
    return lw;
  };
  float mx = -INFINITY;
  for (int m0 = 0; m0 < M; m0 += ck::kWave) {
    const int m = m0 + lane;
    if (m < M) mx = fmaxf(mx, logw(m));
  }
  mx = ck::wave_reduce<true>(mx);
  float carry = 0.f;
  for (int m0 = 0; m0 < M; m0 += ck::kWave) {
    const int m = m0 + lane;
    float v = 0.f;
    if (m < M && mx != -INFINITY) {
      const float l = logw(m);
      v = l == -INFINITY ? 0.f : expf(l - mx);
    }
#pragma unroll
    for (int d = 1; d < ck::kWave; d <<= 1) {  // inclusive scan across the wave
      const float o = __shfl_up(v, d);
      if (lane >= d) v += o;
    }
    if (m < M) out[m] = carry + v;
    carry += __shfl(v, ck::kWave - 1);
  }
  if (bad) atomicOr(flag, bad);
}

// One workgroup owns `S` consecutive samples (the sel table and layer order of ck_walk.h); every item is one thread, a draw
// from a CDF row prepared once per parameter state.
__global__ void __launch_bounds__(kWalkThreads)
    sample_walk_kernel(const ck_sample_layer* __restrict__ layers, int n_layers, int root_fold, int root_unit, int total_folds,
                       int S, int64_t N, int D, uint32_t key0, uint32_t key1, void* __restrict__ x, int x_float) {
  extern __shared__ int16_t sel[];
  const int64_t n0 = static_cast<int64_t>(blockIdx.x) * S;
  const int ns = static_cast<int>(N - n0 < S ? N - n0 : S);
  ck::walk_init(sel, total_folds, S, layers, n_layers, root_fold);
  __syncthreads();
  for (int s = threadIdx.x; s < ns; s += blockDim.x) sel[root_fold * S + s] = static_cast<int16_t>(root_unit);
  __syncthreads();
  for (int li = n_layers - 1; li >= 0; --li) {
    const ck_sample_layer L = layers[li];
    ck::walk_items(L, sel, S, ns, [&](int f, int s, int g, int k) {
      const int64_t n = n0 + s;
      if (k < 0) {
        ck::walk_record(L, f, N, n, -1);
        return;
      }
      const ck::Philox4 p = ck::walk_philox(n, g, key0, key1);
      if (ck::is_input(L.type)) {
        ck::draw_input(L, f, k, p, x, x_float, n * D + L.scope[f]);
        return;
      }
      const int i = ck::cdf_draw(L.cdf + (static_cast<int64_t>(f) * L.Ko + k) * L.M, L.M, ck::philox_uniform(p.x[0]));
      ck::walk_record(L, f, N, n, i);
      ck::walk_child(L, L.child + static_cast<int64_t>(f) * L.H, sel, S, s, i);
    });
    __syncthreads();
  }
}

}  // namespace

int ck_sample_cdf(const float* w, int64_t w_sf, int64_t w_sk, int64_t w_sm, int w_log, const float* lz, int64_t F, int R,
                  int M, float* cdf, int32_t* flag, void* stream) {
  CK_REQUIRE(w != nullptr && cdf != nullptr && flag != nullptr, "ck_sample_cdf: null pointer");
  CK_REQUIRE(F > 0 && R > 0 && M > 0, "ck_sample_cdf: non-positive size");
  const int64_t rows = F * R;
  const int64_t blocks = (rows + kCdfRowsPerBlock - 1) / kCdfRowsPerBlock;
  CK_REQUIRE(blocks <= 0x7fffffff, "ck_sample_cdf: too many rows");
  return ck::launch(sample_cdf_kernel, dim3(static_cast<unsigned>(blocks)), dim3(kCdfRowsPerBlock * ck::kWave), 0, stream, w,
                    w_sf, w_sk, w_sm, w_log, lz, R, M, rows, cdf, flag);
}

int ck_sample_walk(const ck_sample_layer* layers, int n_layers, int root_fold, int root_unit, int total_folds, int S,
                   int64_t N, int D, uint64_t seed, void* x, int x_float, void* stream) {
  CK_REQUIRE(layers != nullptr && x != nullptr, "ck_sample_walk: null pointer");
  size_t lds;
  unsigned blocks;
  if (int st = ck::walk_grid("ck_sample_walk", n_layers, root_fold, root_unit, total_folds, S, N, D, lds, blocks)) return st;
  const uint32_t k0 = static_cast<uint32_t>(seed), k1 = static_cast<uint32_t>(seed >> 32);
  return ck::launch(sample_walk_kernel, dim3(blocks), dim3(kWalkThreads), lds, stream, layers, n_layers, root_fold, root_unit,
                    total_folds, S, N, D, k0, k1, x, x_float);
}
