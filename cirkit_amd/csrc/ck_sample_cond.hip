// Conditional sampling given evidence ("Conditional sampling"): each row n draws its unobserved
// variables from p(x_S | x_O) = c(x_O, x_S) / c(x_O).  The per-row log value of every unit under the row's evidence comes
// from the layer-wise marginal forward (one arena, (F, B, Ko) per layer); the walk weights each draw by those values, so the
// CDF rows depend on the sample and are built on the device, one wave per (fold, sample).
#include <math.h>

#include "ck_internal.h"
#include "ck_philox.h"
#include "ck_sample_draw.h"

namespace {

constexpr int kCondThreads = 1024;  // 16 waves: the walk is latency-bound, a workgroup's LDS table limits residency
constexpr int kCondWaves = kCondThreads / ck::kWave;

// log value of entry i of a sum-type row at chunk row nl: the child value the entry's weight multiplies.  ch: the fold's
// (H) global child fold ids; the Ki values of one child at one row are contiguous.
__device__ __forceinline__ float entry_value(int type, const int32_t* __restrict__ ch, int H, int Ki,
                                             const float* __restrict__ vals, const int64_t* __restrict__ val_off, int64_t nl,
                                             int i) {
  const int64_t r = nl * Ki;
  if (type == CK_SAMPLE_SUM) return vals[val_off[ch[i / Ki]] + r + i % Ki];
  if (type == CK_SAMPLE_CPT) {
    float v = 0.f;
    for (int h = 0; h < H; ++h) v += vals[val_off[ch[h]] + r + i];
    return v;
  }
  return vals[val_off[ch[0]] + r + i / Ki] + vals[val_off[ch[1]] + r + i % Ki];  // CK_SAMPLE_TUCKER, arity 2
}

// One workgroup owns `S` consecutive rows of the chunk; sel[g * S + s] as in sample_walk_kernel (ck_sample.hip).  Sum-type
// layers draw with one wave per (fold, sample); Hadamard, Kronecker and input layers with one thread per item.
__global__ void __launch_bounds__(kCondThreads)
    sample_cond_walk_kernel(const ck_sample_layer* __restrict__ layers, const float* const* __restrict__ weights, int n_layers,
                            int root_fold, int root_unit, int total_folds, int S, const float* __restrict__ vals,
                            const int64_t* __restrict__ val_off, int64_t row0, int64_t B, int64_t N, int D, uint32_t key0,
                            uint32_t key1, const void* __restrict__ ev, void* __restrict__ x, int x_float) {
  extern __shared__ int16_t sel[];
  const int64_t b0 = static_cast<int64_t>(blockIdx.x) * S;  // chunk row of the workgroup's sample 0
  const int ns = static_cast<int>(B - b0 < S ? B - b0 : S);
  const int lane = threadIdx.x & (ck::kWave - 1);
  const int wave = threadIdx.x / ck::kWave;
  for (int i = threadIdx.x; i < total_folds * S; i += blockDim.x) sel[i] = -1;
  int root_ko = 0;
  for (int j = 0; j < n_layers; ++j) {
    if (root_fold >= layers[j].fold_off && root_fold < layers[j].fold_off + layers[j].F) root_ko = layers[j].Ko;
  }
  __syncthreads();
  for (int s = threadIdx.x; s < ns; s += blockDim.x) {  // a row whose evidence has no finite mass draws nothing
    const float r = vals[val_off[root_fold] + (b0 + s) * root_ko + root_unit];
    if (isfinite(r)) sel[root_fold * S + s] = static_cast<int16_t>(root_unit);
  }
  __syncthreads();
  for (int li = n_layers - 1; li >= 0; --li) {
    const ck_sample_layer& L = layers[li];
    if (L.type == CK_SAMPLE_SUM || L.type == CK_SAMPLE_CPT || L.type == CK_SAMPLE_TUCKER) {
      const float* __restrict__ W = weights[li];
      for (int it = wave; it < L.F * ns; it += kCondWaves) {  // (wave-uniform: every lane of a wave has the same item)
        const int f = it / ns, s = it % ns;
        const int64_t nl = b0 + s, n = row0 + nl;
        const int g = L.fold_off + f;
        const int k = sel[g * S + s];
        const int32_t* ch = L.child + static_cast<int64_t>(f) * L.H;
        int choice = -1;
        if (k >= 0 && k < L.Ko) {
          const float* wr = W + (static_cast<int64_t>(f) * L.Ko + k) * L.M;
          // log mass of entry i minus log w_i: -inf for a weight <= 0 (its child value is not read) or a NaN value
          auto logv = [&](int i, float& wi) -> float {
            wi = wr[i];
            if (!(wi > 0.f)) return -INFINITY;
            const float v = entry_value(L.type, ch, L.H, L.Ki, vals, val_off, nl, i);
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
          if (isfinite(vmax)) {
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
            const ck::Philox4 p = ck::philox4x32_10(static_cast<uint32_t>(n), static_cast<uint32_t>(g), 0u, 0u, key0, key1);
            float t = ck::philox_uniform(p.x[0]) * T;
            if (t >= T) t = __int_as_float(__float_as_int(T) - 1);  // the float below T (T >= the largest w_i > 0)
            float carry = 0.f;
            int last = -1;  // the last entry that raised the CDF so far
            for (int m0 = 0; m0 < L.M; m0 += ck::kWave) {
              const float c = m0 == 0 ? c0 : scan(m0);
              const uint64_t hit = __ballot(m0 + lane < L.M && t < carry + c);
              if (hit != 0) {
                choice = m0 + __ffsll(static_cast<unsigned long long>(hit)) - 1;
                break;
              }
              const float prev = __shfl_up(c, 1);
              const uint64_t up = __ballot(m0 + lane < L.M && c > (lane == 0 ? 0.f : prev));
              if (up != 0) last = m0 + 63 - __clzll(static_cast<long long>(up));
              carry += __shfl(c, ck::kWave - 1);
            }
            // (T and the last CDF value come from the same arithmetic, so t < T always hits; should a compiler ever contract
            // the two scans differently, t within rounding of T takes the last entry with mass instead of drawing nothing)
            if (choice < 0) choice = last;
          }
        }
        if (lane == 0) {
          if (choice >= 0) {
            if (L.type == CK_SAMPLE_SUM) {
              sel[ch[choice / L.Ki] * S + s] = static_cast<int16_t>(choice % L.Ki);
            } else if (L.type == CK_SAMPLE_CPT) {
              for (int h = 0; h < L.H; ++h) sel[ch[h] * S + s] = static_cast<int16_t>(choice);
            } else {
              sel[ch[0] * S + s] = static_cast<int16_t>(choice / L.Ki);
              sel[ch[1] * S + s] = static_cast<int16_t>(choice % L.Ki);
            }
          }
          if (L.choices != nullptr)
            L.choices[static_cast<int64_t>(f) * N + n] = choice < 0 ? -1 : (L.cmap != nullptr ? L.cmap[choice] : choice);
        }
      }
      __syncthreads();
      continue;
    }
    const int items = L.F * ns;
    const bool input = L.type == CK_SAMPLE_CATEGORICAL || L.type == CK_SAMPLE_GAUSSIAN;
    for (int it = threadIdx.x; it < items; it += blockDim.x) {
      const int f = input ? it % L.F : it / ns;
      const int s = input ? it / L.F : it % ns;
      const int64_t nl = b0 + s, n = row0 + nl;
      const int g = L.fold_off + f;
      const int k = sel[g * S + s];
      if (k < 0 || k >= L.Ko) continue;
      const int32_t* ch = L.child + static_cast<int64_t>(f) * L.H;
      if (L.type == CK_SAMPLE_HADAMARD) {
        for (int h = 0; h < L.H; ++h) sel[ch[h] * S + s] = static_cast<int16_t>(k);
        continue;
      }
      if (L.type == CK_SAMPLE_KRONECKER) {
        int r = k;
        for (int h = L.H - 1; h >= 0; --h) {
          sel[ch[h] * S + s] = static_cast<int16_t>(r % L.Ki);
          r /= L.Ki;
        }
        continue;
      }
      // input layers: an observed variable keeps its value (the output starts as a copy of the evidence).  Sentinels: NaN
      // for a continuous layer, a negative category for a discrete one (a float batch is truncated: > -1 is observed)
      const int64_t o = nl * D + L.scope[f];
      if (x_float) {
        const float e = static_cast<const float*>(ev)[o];
        if (L.type == CK_SAMPLE_GAUSSIAN ? !isnan(e) : e > -1.f) continue;
      } else if (static_cast<const int64_t*>(ev)[o] >= 0) {
        continue;
      }
      const ck::Philox4 p = ck::philox4x32_10(static_cast<uint32_t>(n), static_cast<uint32_t>(g), 0u, 0u, key0, key1);
      if (L.type == CK_SAMPLE_GAUSSIAN) {
        const float u1 = static_cast<float>((p.x[0] >> 8) + 1u) * 5.9604644775390625e-8f;
        const float u2 = ck::philox_uniform(p.x[1]);
        const float z = sqrtf(-2.f * logf(u1)) * cospif(2.f * u2);
        const float v = L.mean[static_cast<int64_t>(f) * L.Ko + k] + L.stddev[static_cast<int64_t>(f) * L.Ko + k] * z;
        if (x_float) static_cast<float*>(x)[o] = v;
        continue;
      }
      const int i = ck::cdf_draw(L.cdf + (static_cast<int64_t>(f) * L.Ko + k) * L.M, L.M, ck::philox_uniform(p.x[0]));
      if (x_float) static_cast<float*>(x)[o] = static_cast<float>(i);
      else static_cast<int64_t*>(x)[o] = i;
    }
    __syncthreads();
  }
}

}  // namespace

int ck_sample_cond_walk(const ck_sample_layer* layers, const float* const* weights, int n_layers, int root_fold, int root_unit,
                        int total_folds, int S, const float* vals, const int64_t* val_off, int64_t row0, int64_t B, int64_t N,
                        int D, uint64_t seed, const void* ev, void* x, int x_float, void* stream) {
  CK_REQUIRE(layers != nullptr && weights != nullptr && vals != nullptr && val_off != nullptr && ev != nullptr && x != nullptr,
             "ck_sample_cond_walk: null pointer");
  CK_REQUIRE(n_layers > 0 && total_folds > 0 && B > 0 && D > 0 && S > 0, "ck_sample_cond_walk: non-positive size");
  CK_REQUIRE(row0 >= 0 && row0 + B <= N, "ck_sample_cond_walk: rows %lld .. %lld outside the %lld rows of the choices",
             static_cast<long long>(row0), static_cast<long long>(row0 + B), static_cast<long long>(N));
  CK_REQUIRE(root_fold >= 0 && root_fold < total_folds && root_unit >= 0 && root_unit < 32768,
             "ck_sample_cond_walk: root out of range");
  const int64_t lds = static_cast<int64_t>(total_folds) * S * 2;
  CK_REQUIRE(lds <= CK_SAMPLE_MAX_LDS, "ck_sample_cond_walk: %d folds x %d samples exceed the LDS budget", total_folds, S);
  const int64_t blocks = (B + S - 1) / S;
  CK_REQUIRE(blocks <= 0x7fffffff, "ck_sample_cond_walk: too many rows");
  const uint32_t k0 = static_cast<uint32_t>(seed), k1 = static_cast<uint32_t>(seed >> 32);
  return ck::dispatch(
      [=](hipStream_t s) {
        hipLaunchKernelGGL(sample_cond_walk_kernel, dim3(static_cast<unsigned>(blocks)), dim3(kCondThreads),
                           static_cast<size_t>(lds), s, layers, weights, n_layers, root_fold, root_unit, total_folds, S, vals,
                           val_off, row0, B, N, D, k0, k1, ev, x, x_float);
        return hipGetLastError();
      },
      stream);
}
