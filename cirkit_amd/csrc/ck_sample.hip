// Exact ancestral sampling of a smooth, decomposable, monotonic circuit: the prepare launch turns
// weights and child partition functions into conditional CDF rows, the walk launch draws samples top down.
#include <math.h>

#include "ck_internal.h"
#include "ck_philox.h"
#include "ck_sample_draw.h"

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

// One workgroup owns `S` consecutive samples; sel[g * S + s] = the unit of global fold g on sample s's induced tree, -1 if g
// is not on it.  Layers are walked from the last to the first; a fold writes the units of its children, which belong to
// earlier layers, so one barrier per layer orders the walk.
__global__ void __launch_bounds__(kWalkThreads)
    sample_walk_kernel(const ck_sample_layer* __restrict__ layers, int n_layers, int root_fold, int root_unit, int total_folds,
                       int S, int64_t N, int D, uint32_t key0, uint32_t key1, void* __restrict__ x, int x_float) {
  extern __shared__ int16_t sel[];
  const int64_t n0 = static_cast<int64_t>(blockIdx.x) * S;
  const int ns = static_cast<int>(N - n0 < S ? N - n0 : S);
  for (int i = threadIdx.x; i < total_folds * S; i += blockDim.x) sel[i] = -1;
  __syncthreads();
  for (int s = threadIdx.x; s < ns; s += blockDim.x) sel[root_fold * S + s] = static_cast<int16_t>(root_unit);
  __syncthreads();
  for (int li = n_layers - 1; li >= 0; --li) {
    const ck_sample_layer L = layers[li];
    const int items = L.F * ns;
    const bool input = L.type == CK_SAMPLE_CATEGORICAL || L.type == CK_SAMPLE_GAUSSIAN;
    for (int it = threadIdx.x; it < items; it += blockDim.x) {
      // inner layers: consecutive threads = consecutive samples of one fold (one CDF row region, coalesced `choices`);
      // input layers: consecutive threads = consecutive folds of one sample (neighbouring variables of one output row)
      const int f = input ? it % L.F : it / ns;
      const int s = input ? it / L.F : it % ns;
      const int64_t n = n0 + s;
      const int g = L.fold_off + f;
      const int k = sel[g * S + s];
      const bool on = k >= 0 && k < L.Ko;
      if (!on) {
        if (L.choices != nullptr) L.choices[static_cast<int64_t>(f) * N + n] = -1;
        continue;
      }
      const int32_t* ch = L.child + static_cast<int64_t>(f) * L.H;
      if (L.type == CK_SAMPLE_HADAMARD) {
        for (int h = 0; h < L.H; ++h) sel[ch[h] * S + s] = static_cast<int16_t>(k);
        continue;
      }
      if (L.type == CK_SAMPLE_KRONECKER) {  // unit k = (u_0, ..., u_{H-1}) in base Ki, input 0 most significant
        int r = k;
        for (int h = L.H - 1; h >= 0; --h) {
          sel[ch[h] * S + s] = static_cast<int16_t>(r % L.Ki);
          r /= L.Ki;
        }
        continue;
      }
      const ck::Philox4 p = ck::philox4x32_10(static_cast<uint32_t>(n), static_cast<uint32_t>(g), 0u, 0u, key0, key1);
      if (L.type == CK_SAMPLE_GAUSSIAN) {
        const float u1 = static_cast<float>((p.x[0] >> 8) + 1u) * 5.9604644775390625e-8f;
        const float u2 = ck::philox_uniform(p.x[1]);
        const float z = sqrtf(-2.f * logf(u1)) * cospif(2.f * u2);
        const int64_t o = n * D + L.scope[f];
        const float v = L.mean[static_cast<int64_t>(f) * L.Ko + k] + L.stddev[static_cast<int64_t>(f) * L.Ko + k] * z;
        if (x_float) static_cast<float*>(x)[o] = v;
        continue;  // (a Gaussian layer makes the output fp32: DESIGN.md section 11)
      }
      const int i = ck::cdf_draw(L.cdf + (static_cast<int64_t>(f) * L.Ko + k) * L.M, L.M, ck::philox_uniform(p.x[0]));
      if (L.type == CK_SAMPLE_CATEGORICAL) {
        const int64_t o = n * D + L.scope[f];
        if (x_float) static_cast<float*>(x)[o] = static_cast<float>(i);
        else static_cast<int64_t*>(x)[o] = i;
        continue;
      }
      if (L.choices != nullptr) L.choices[static_cast<int64_t>(f) * N + n] = L.cmap != nullptr ? L.cmap[i] : i;
      if (L.type == CK_SAMPLE_SUM) {
        sel[ch[i / L.Ki] * S + s] = static_cast<int16_t>(i % L.Ki);
      } else if (L.type == CK_SAMPLE_CPT) {
        for (int h = 0; h < L.H; ++h) sel[ch[h] * S + s] = static_cast<int16_t>(i);
      } else {  // CK_SAMPLE_TUCKER, arity 2
        sel[ch[0] * S + s] = static_cast<int16_t>(i / L.Ki);
        sel[ch[1] * S + s] = static_cast<int16_t>(i % L.Ki);
      }
    }
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
  return ck::dispatch(
      [=](hipStream_t s) {
        hipLaunchKernelGGL(sample_cdf_kernel, dim3(static_cast<unsigned>(blocks)), dim3(kCdfRowsPerBlock * ck::kWave), 0, s,
                           w, w_sf, w_sk, w_sm, w_log, lz, R, M, rows, cdf, flag);
        return hipGetLastError();
      },
      stream);
}

int ck_sample_walk(const ck_sample_layer* layers, int n_layers, int root_fold, int root_unit, int total_folds, int S,
                   int64_t N, int D, uint64_t seed, void* x, int x_float, void* stream) {
  CK_REQUIRE(layers != nullptr && x != nullptr, "ck_sample_walk: null pointer");
  CK_REQUIRE(n_layers > 0 && total_folds > 0 && N > 0 && D > 0 && S > 0, "ck_sample_walk: non-positive size");
  CK_REQUIRE(root_fold >= 0 && root_fold < total_folds && root_unit >= 0 && root_unit < 32768,
             "ck_sample_walk: root out of range");
  const int64_t lds = static_cast<int64_t>(total_folds) * S * 2;
  CK_REQUIRE(lds <= CK_SAMPLE_MAX_LDS, "ck_sample_walk: %d folds x %d samples exceed the LDS budget", total_folds, S);
  const int64_t blocks = (N + S - 1) / S;
  CK_REQUIRE(blocks <= 0x7fffffff, "ck_sample_walk: too many samples");
  const uint32_t k0 = static_cast<uint32_t>(seed), k1 = static_cast<uint32_t>(seed >> 32);
  return ck::dispatch(
      [=](hipStream_t s) {
        hipLaunchKernelGGL(sample_walk_kernel, dim3(static_cast<unsigned>(blocks)), dim3(kWalkThreads),
                           static_cast<size_t>(lds), s, layers, n_layers, root_fold, root_unit, total_folds, S, N, D, k0, k1,
                           x, x_float);
        return hipGetLastError();
      },
      stream);
}
