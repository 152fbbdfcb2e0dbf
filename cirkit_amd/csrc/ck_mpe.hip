// Most probable explanation ("Most probable explanation"): the max-product ("Viterbi") upward pass of
// a masked batch, one launch per layer into an (F, B, Ko)-per-layer arena, then the argmax walk top down.  A sum-type unit's
// value is max_i (log w_i + v_i), a product unit's the sum of its children's values, an input unit's log p(x_v) where x_v
// is observed and max_c log p(c) where it is maximised.  The walk picks the smallest entry index among the maxima.
#include <math.h>

#include "ck_internal.h"
#include "ck_mpe_entry.h"

namespace {

constexpr int kUpThreads = 256;
constexpr int kRM = 4;   // rows of a thread's register micro-tile
constexpr int kKM = 4;   // units of a thread's register micro-tile
constexpr int kMC = 16;  // entries staged in LDS per step
constexpr int kWalkThreads = 1024;  // 16 waves, as the conditional walk
constexpr int kWalkWaves = kWalkThreads / ck::kWave;

// ---- per-parameter-state input tables ------------------------------------------------------------------------------
// Per (fold, unit): the largest log value over the categories and its smallest index (a Categorical / Binomial table read at
// tab + f sf + k sk + c sc, log-probabilities when t_log, probabilities otherwise), or the Gaussian's value at its mean.
__global__ void __launch_bounds__(256)
    mpe_input_max_kernel(int type, const float* __restrict__ tab, int64_t sf, int64_t sk, int64_t sc, int t_log, int C,
                         const float* __restrict__ mean, const float* __restrict__ stddev, const float* __restrict__ lz,
                         int64_t F, int K, float* __restrict__ vmax, int32_t* __restrict__ amax) {
  const int64_t o = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (o >= F * K) return;
  if (type == CK_SAMPLE_GAUSSIAN) {
    vmax[o] = ck::mpe_gauss(mean[o], mean[o], stddev[o], lz, o);
    amax[o] = 0;
    return;
  }
  const float* row = tab + (o / K) * sf + (o % K) * sk;
  float best = -INFINITY;
  int arg = 0;
  for (int c = 0; c < C; ++c) {
    const float p = row[c * sc];
    const float v = t_log ? p : logf(p);
    if (v > best) {  // strict: the smallest index among equal maxima
      best = v;
      arg = c;
    }
  }
  vmax[o] = best;
  amax[o] = arg;
}

// ---- upward pass ---------------------------------------------------------------------------------------------------
// Input layer: out[f, n, k] from the masked batch ev (B, D), int64 or fp32 (x_float).  Sentinels: a negative int64; NaN in
// fp32, or a value <= -1 for a discrete layer (a float batch is truncated, as the forward does).  An observed category
// outside 0 .. C - 1 sets *flag (when given) and bad[n], and the entry is NaN.
__global__ void __launch_bounds__(256)
    mpe_up_input_kernel(int type, const int64_t* __restrict__ scope, const float* __restrict__ tab, int64_t sf, int64_t sk,
                        int64_t sc, int t_log, int C, const float* __restrict__ mean, const float* __restrict__ stddev,
                        const float* __restrict__ lz, const float* __restrict__ vmax, int64_t F, int K,
                        const void* __restrict__ ev, int x_float, int64_t B, int D, float* __restrict__ vals,
                        const int64_t* __restrict__ val_off, int fold_off, int32_t* flag, int32_t* bad) {
  const int64_t idx = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (idx >= F * B * K) return;
  const int k = static_cast<int>(idx % K);
  const int64_t rest = idx / K;
  const int64_t n = rest % B, f = rest / B;
  const int64_t o = f * K + k;
  const int64_t e_at = n * D + scope[f];
  float v;
  if (type == CK_SAMPLE_GAUSSIAN) {
    const float x = static_cast<const float*>(ev)[e_at];
    v = isnan(x) ? vmax[o] : ck::mpe_gauss(x, mean[o], stddev[o], lz, o);
  } else {
    int64_t c;
    if (x_float) {
      const float x = static_cast<const float*>(ev)[e_at];
      c = !(x > -1.f) ? -1 : (x >= static_cast<float>(C) ? C : static_cast<int64_t>(x));
    } else {
      c = static_cast<const int64_t*>(ev)[e_at];
    }
    if (c < 0) {
      v = vmax[o];
    } else if (c >= C) {
      v = NAN;
      if (k == 0) {
        bad[n] = 1;
        if (flag != nullptr) atomicOr(flag, 1);
      }
    } else {
      const float p = tab[f * sf + k * sk + c * sc];
      v = t_log ? p : logf(p);
    }
  }
  vals[val_off[fold_off + f] + n * K + k] = v;
}

// Sum, mixing, CP-T and Tucker layers: a max-plus contraction per fold of the (rows x M) entry values with the (Ko x M) log
// weights.  A workgroup owns one fold, TR rows and TK units; each step stages kMC entries of its rows (through the shared
// entry helper) and of its units' log weights in LDS, and every thread keeps a kRM x kKM micro-tile of maxima in registers:
// two entries per v_max3_f32, each after its v_add_f32.
template <int TK>
__global__ void __launch_bounds__(kUpThreads)
    mpe_up_sum_kernel(int type, const int32_t* __restrict__ child, const float* __restrict__ lw, int64_t F, int H, int Ki,
                      int Ko, int M, float* __restrict__ vals, const int64_t* __restrict__ val_off, int fold_off, int64_t B,
                      int64_t row_tiles) {
  constexpr int TKT = TK / kKM;          // threads along the units
  constexpr int TRT = kUpThreads / TKT;  // threads along the rows
  constexpr int TR = TRT * kRM;          // rows of the tile
  constexpr int EP = TR + 4;             // (padded LDS row: the staging writes spread over the banks)
  __shared__ float4 sE[kMC * EP / 4];    // sE[m][r]: entry m0 + m of tile row r
  __shared__ float4 sW[kMC * TK / 4];    // sW[m][k]: log weight of unit k0 + k, entry m0 + m
  float* const sEf = reinterpret_cast<float*>(sE);
  float* const sWf = reinterpret_cast<float*>(sW);
  const int64_t f = blockIdx.x / row_tiles;
  const int64_t n0 = (blockIdx.x % row_tiles) * TR;
  const int k0 = blockIdx.y * TK;
  const int tk = threadIdx.x % TKT, tr = threadIdx.x / TKT;
  const int32_t* ch = child + f * H;
  const float* wf = lw + f * Ko * M;
  float acc[kRM][kKM];
#pragma unroll
  for (int i = 0; i < kRM; ++i)
#pragma unroll
    for (int j = 0; j < kKM; ++j) acc[i][j] = -INFINITY;
  for (int m0 = 0; m0 < M; m0 += kMC) {
    for (int t = threadIdx.x; t < TR * kMC; t += kUpThreads) {
      const int m = t % kMC, r = t / kMC;
      float e = 0.f;  // (padding entries: 0 under a log weight of -inf)
      if (m0 + m < M && n0 + r < B) e = ck::mpe_entry(type, ch, H, Ki, vals, val_off, n0 + r, m0 + m);
      sEf[m * EP + r] = e;
    }
    for (int t = threadIdx.x; t < TK * kMC; t += kUpThreads) {
      const int m = t % kMC, k = t / kMC;
      sWf[m * TK + k] = (m0 + m < M && k0 + k < Ko) ? wf[static_cast<int64_t>(k0 + k) * M + m0 + m] : -INFINITY;
    }
    __syncthreads();
#pragma unroll
    for (int m = 0; m < kMC; m += 2) {
      const float4 e0 = sE[(m * EP) / 4 + tr], e1 = sE[((m + 1) * EP) / 4 + tr];
      const float4 w0 = sW[(m * TK) / 4 + tk], w1 = sW[((m + 1) * TK) / 4 + tk];
      const float ea[kRM] = {e0.x, e0.y, e0.z, e0.w}, eb[kRM] = {e1.x, e1.y, e1.z, e1.w};
      const float wa[kKM] = {w0.x, w0.y, w0.z, w0.w}, wb[kKM] = {w1.x, w1.y, w1.z, w1.w};
#pragma unroll
      for (int i = 0; i < kRM; ++i)
#pragma unroll
        for (int j = 0; j < kKM; ++j)
          acc[i][j] = ck::mpe_max3(acc[i][j], ck::mpe_term(wa[j], ea[i]), ck::mpe_term(wb[j], eb[i]));
    }
    __syncthreads();
  }
  float* out = vals + val_off[fold_off + f];
#pragma unroll
  for (int i = 0; i < kRM; ++i) {
    const int64_t n = n0 + tr * kRM + i;
    if (n >= B) continue;
#pragma unroll
    for (int j = 0; j < kKM; ++j) {
      const int k = k0 + tk * kKM + j;
      if (k < Ko) out[n * Ko + k] = acc[i][j];
    }
  }
}

// Hadamard: unit k adds unit k of every input; Kronecker: unit k adds, input 0 most significant, the digits of k in base Ki.
__global__ void __launch_bounds__(256)
    mpe_up_product_kernel(int type, const int32_t* __restrict__ child, int64_t F, int H, int Ki, int Ko,
                          float* __restrict__ vals, const int64_t* __restrict__ val_off, int fold_off, int64_t B) {
  const int64_t idx = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (idx >= F * B * Ko) return;
  const int k = static_cast<int>(idx % Ko);
  const int64_t rest = idx / Ko;
  const int64_t n = rest % B, f = rest / B;
  const int32_t* ch = child + f * H;
  float v = 0.f;
  if (type == CK_SAMPLE_HADAMARD) {
    for (int h = 0; h < H; ++h) v += vals[val_off[ch[h]] + n * Ki + k];
  } else {
    int r = k;
    for (int h = H - 1; h >= 0; --h) {
      v += vals[val_off[ch[h]] + n * Ki + r % Ki];
      r /= Ki;
    }
  }
  vals[val_off[fold_off + f] + n * Ko + k] = v;
}

// ---- argmax walk ---------------------------------------------------------------------------------------------------
// One workgroup owns S consecutive rows of the chunk; sel[g * S + s] is the unit of global fold g on row s's tree (-1: off
// the tree), as in the conditional walk (ck_sample_cond.hip).  A sum-type unit on a tree is one wave: 64 entries at a time
// through the shared entry helper, a wave max, and the first lane of the ballot of the entries equal to it.
__global__ void __launch_bounds__(kWalkThreads)
    mpe_walk_kernel(const ck_sample_layer* __restrict__ layers, const float* const* __restrict__ logw,
                    const int32_t* const* __restrict__ amax, int n_layers, int root_fold, int root_unit, int total_folds, int S,
                    const float* __restrict__ vals, const int64_t* __restrict__ val_off, const int32_t* __restrict__ bad,
                    int64_t row0, int64_t B, int64_t N, int D, const void* __restrict__ ev, void* __restrict__ x, int x_float,
                    float* __restrict__ logv) {
  extern __shared__ int16_t sel[];
  const int64_t b0 = static_cast<int64_t>(blockIdx.x) * S;
  const int ns = static_cast<int>(B - b0 < S ? B - b0 : S);
  const int lane = threadIdx.x & (ck::kWave - 1);
  const int wave = threadIdx.x / ck::kWave;
  for (int i = threadIdx.x; i < total_folds * S; i += blockDim.x) sel[i] = -1;
  int root_ko = 0;
  for (int j = 0; j < n_layers; ++j) {
    if (root_fold >= layers[j].fold_off && root_fold < layers[j].fold_off + layers[j].F) root_ko = layers[j].Ko;
  }
  __syncthreads();
  for (int s = threadIdx.x; s < ns; s += blockDim.x) {  // rows without finite mass, and rows with bad evidence, stay empty
    const int64_t n = row0 + b0 + s;
    const float r = vals[val_off[root_fold] + (b0 + s) * root_ko + root_unit];
    const bool b = bad[n] != 0;
    logv[n] = b ? NAN : r;
    if (!b && isfinite(r)) sel[root_fold * S + s] = static_cast<int16_t>(root_unit);
  }
  __syncthreads();
  for (int li = n_layers - 1; li >= 0; --li) {
    const ck_sample_layer& L = layers[li];
    if (L.type == CK_SAMPLE_SUM || L.type == CK_SAMPLE_CPT || L.type == CK_SAMPLE_TUCKER) {
      const float* __restrict__ W = logw[li];
      for (int it = wave; it < L.F * ns; it += kWalkWaves) {  // (wave-uniform)
        const int f = it / ns, s = it % ns;
        const int64_t nl = b0 + s, n = row0 + nl;
        const int k = sel[(L.fold_off + f) * S + s];
        const int32_t* ch = L.child + static_cast<int64_t>(f) * L.H;
        int choice = -1;
        if (k >= 0 && k < L.Ko) {
          const float* wr = W + (static_cast<int64_t>(f) * L.Ko + k) * L.M;
          float best = -INFINITY;
          for (int m0 = 0; m0 < L.M; m0 += ck::kWave) {
            const int i = m0 + lane;
            float v = -INFINITY;
            if (i < L.M) {
              const float lwi = wr[i];
              if (lwi != -INFINITY) v = ck::mpe_term(lwi, ck::mpe_entry(L.type, ch, L.H, L.Ki, vals, val_off, nl, i));
              if (isnan(v)) v = -INFINITY;
            }
            const float cm = ck::wave_max(v);
            if (cm > best) {  // strict: an earlier block keeps a tie
              best = cm;
              choice = m0 + __ffsll(static_cast<unsigned long long>(__ballot(v == cm))) - 1;
            }
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
      const int64_t nl = b0 + s;
      const int k = sel[(L.fold_off + f) * S + s];
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
      // input layers write only maximised entries (the output starts as a copy of the masked evidence)
      const int64_t o = nl * D + L.scope[f];
      if (x_float) {
        const float e = static_cast<const float*>(ev)[o];
        if (L.type == CK_SAMPLE_GAUSSIAN ? !isnan(e) : e > -1.f) continue;
      } else if (static_cast<const int64_t*>(ev)[o] >= 0) {
        continue;
      }
      const int64_t u = static_cast<int64_t>(f) * L.Ko + k;
      if (L.type == CK_SAMPLE_GAUSSIAN) {
        if (x_float) static_cast<float*>(x)[o] = L.mean[u];
        continue;
      }
      const int c = amax[li][u];
      if (x_float) static_cast<float*>(x)[o] = static_cast<float>(c);
      else static_cast<int64_t*>(x)[o] = c;
    }
    __syncthreads();
  }
}

int64_t blocks_of(int64_t items, int threads) { return (items + threads - 1) / threads; }

}  // namespace

int ck_mpe_input_max(int type, const float* tab, int64_t sf, int64_t sk, int64_t sc, int t_log, int C, const float* mean,
                     const float* stddev, const float* log_partition, int64_t F, int K, float* vmax, int32_t* amax,
                     void* stream) {
  CK_REQUIRE(type == CK_SAMPLE_CATEGORICAL || type == CK_SAMPLE_GAUSSIAN, "ck_mpe_input_max: not an input layer type");
  CK_REQUIRE(vmax != nullptr && amax != nullptr, "ck_mpe_input_max: null pointer");
  CK_REQUIRE(type == CK_SAMPLE_GAUSSIAN ? (mean != nullptr && stddev != nullptr) : (tab != nullptr && C > 0),
             "ck_mpe_input_max: missing parameters");
  CK_REQUIRE(F > 0 && K > 0, "ck_mpe_input_max: non-positive size");
  const int64_t blocks = blocks_of(F * K, 256);
  CK_REQUIRE(blocks <= 0x7fffffff, "ck_mpe_input_max: too many units");
  return ck::dispatch(
      [=](hipStream_t s) {
        hipLaunchKernelGGL(mpe_input_max_kernel, dim3(static_cast<unsigned>(blocks)), dim3(256), 0, s, type, tab, sf, sk, sc,
                           t_log, C, mean, stddev, log_partition, F, K, vmax, amax);
        return hipGetLastError();
      },
      stream);
}

int ck_mpe_up_input(int type, const int64_t* scope, const float* tab, int64_t sf, int64_t sk, int64_t sc, int t_log, int C,
                    const float* mean, const float* stddev, const float* log_partition, const float* vmax, int64_t F, int K,
                    const void* ev, int x_float, int64_t B, int D, float* vals, const int64_t* val_off, int fold_off,
                    int32_t* flag, int32_t* bad, void* stream) {
  CK_REQUIRE(type == CK_SAMPLE_CATEGORICAL || type == CK_SAMPLE_GAUSSIAN, "ck_mpe_up_input: not an input layer type");
  CK_REQUIRE(scope != nullptr && vmax != nullptr && ev != nullptr && vals != nullptr && val_off != nullptr && bad != nullptr,
             "ck_mpe_up_input: null pointer");
  CK_REQUIRE(type == CK_SAMPLE_GAUSSIAN ? (mean != nullptr && stddev != nullptr && x_float) : (tab != nullptr && C > 0),
             "ck_mpe_up_input: missing parameters (a Gaussian layer reads an fp32 batch)");
  CK_REQUIRE(F > 0 && K > 0 && B > 0 && D > 0 && fold_off >= 0, "ck_mpe_up_input: non-positive size");
  const int64_t blocks = blocks_of(F * B * K, 256);
  CK_REQUIRE(blocks <= 0x7fffffff, "ck_mpe_up_input: too many entries");
  return ck::dispatch(
      [=](hipStream_t s) {
        hipLaunchKernelGGL(mpe_up_input_kernel, dim3(static_cast<unsigned>(blocks)), dim3(256), 0, s, type, scope, tab, sf, sk,
                           sc, t_log, C, mean, stddev, log_partition, vmax, F, K, ev, x_float, B, D, vals, val_off, fold_off,
                           flag, bad);
        return hipGetLastError();
      },
      stream);
}

int ck_mpe_up_sum(int type, const int32_t* child, const float* lw, int64_t F, int H, int Ki, int Ko, int M, float* vals,
                  const int64_t* val_off, int fold_off, int64_t B, void* stream) {
  CK_REQUIRE(type == CK_SAMPLE_SUM || type == CK_SAMPLE_CPT || type == CK_SAMPLE_TUCKER, "ck_mpe_up_sum: not a sum-type layer");
  CK_REQUIRE(child != nullptr && lw != nullptr && vals != nullptr && val_off != nullptr, "ck_mpe_up_sum: null pointer");
  CK_REQUIRE(F > 0 && H > 0 && Ki > 0 && Ko > 0 && M > 0 && B > 0 && fold_off >= 0, "ck_mpe_up_sum: non-positive size");
  CK_REQUIRE(M == (type == CK_SAMPLE_SUM ? H * Ki : type == CK_SAMPLE_CPT ? Ki : Ki * Ki) && (type != CK_SAMPLE_TUCKER || H == 2),
             "ck_mpe_up_sum: %d entries for type %d, arity %d, %d input units", M, type, H, Ki);
  const int tk = Ko <= 16 ? 16 : Ko <= 32 ? 32 : 64;
  const int tr = kUpThreads / (tk / kKM) * kRM;
  const int64_t row_tiles = (B + tr - 1) / tr, unit_tiles = (Ko + tk - 1) / tk;
  CK_REQUIRE(F * row_tiles <= 0x7fffffff && unit_tiles <= 65535, "ck_mpe_up_sum: grid too large");
  const dim3 grid(static_cast<unsigned>(F * row_tiles), static_cast<unsigned>(unit_tiles));
  return ck::dispatch(
      [=](hipStream_t s) {
        if (tk == 16)
          hipLaunchKernelGGL(mpe_up_sum_kernel<16>, grid, dim3(kUpThreads), 0, s, type, child, lw, F, H, Ki, Ko, M, vals, val_off,
                             fold_off, B, row_tiles);
        else if (tk == 32)
          hipLaunchKernelGGL(mpe_up_sum_kernel<32>, grid, dim3(kUpThreads), 0, s, type, child, lw, F, H, Ki, Ko, M, vals, val_off,
                             fold_off, B, row_tiles);
        else
          hipLaunchKernelGGL(mpe_up_sum_kernel<64>, grid, dim3(kUpThreads), 0, s, type, child, lw, F, H, Ki, Ko, M, vals, val_off,
                             fold_off, B, row_tiles);
        return hipGetLastError();
      },
      stream);
}

int ck_mpe_up_product(int type, const int32_t* child, int64_t F, int H, int Ki, int Ko, float* vals, const int64_t* val_off,
                      int fold_off, int64_t B, void* stream) {
  CK_REQUIRE(type == CK_SAMPLE_HADAMARD || type == CK_SAMPLE_KRONECKER, "ck_mpe_up_product: not a product layer");
  CK_REQUIRE(child != nullptr && vals != nullptr && val_off != nullptr, "ck_mpe_up_product: null pointer");
  CK_REQUIRE(F > 0 && H > 0 && Ki > 0 && Ko > 0 && B > 0 && fold_off >= 0, "ck_mpe_up_product: non-positive size");
  CK_REQUIRE(type == CK_SAMPLE_HADAMARD ? Ko == Ki : true, "ck_mpe_up_product: Hadamard with %d inputs, %d outputs", Ki, Ko);
  const int64_t blocks = blocks_of(F * B * Ko, 256);
  CK_REQUIRE(blocks <= 0x7fffffff, "ck_mpe_up_product: too many entries");
  return ck::dispatch(
      [=](hipStream_t s) {
        hipLaunchKernelGGL(mpe_up_product_kernel, dim3(static_cast<unsigned>(blocks)), dim3(256), 0, s, type, child, F, H, Ki,
                           Ko, vals, val_off, fold_off, B);
        return hipGetLastError();
      },
      stream);
}

int ck_mpe_walk(const ck_sample_layer* layers, const float* const* logw, const int32_t* const* amax, int n_layers,
                int root_fold, int root_unit, int total_folds, int S, const float* vals, const int64_t* val_off,
                const int32_t* bad, int64_t row0, int64_t B, int64_t N, int D, const void* ev, void* x, int x_float,
                float* logv, void* stream) {
  CK_REQUIRE(layers != nullptr && logw != nullptr && amax != nullptr && vals != nullptr && val_off != nullptr &&
                 bad != nullptr && ev != nullptr && x != nullptr && logv != nullptr,
             "ck_mpe_walk: null pointer");
  CK_REQUIRE(n_layers > 0 && total_folds > 0 && B > 0 && D > 0 && S > 0, "ck_mpe_walk: non-positive size");
  CK_REQUIRE(row0 >= 0 && row0 + B <= N, "ck_mpe_walk: rows %lld .. %lld outside the %lld rows of the batch",
             static_cast<long long>(row0), static_cast<long long>(row0 + B), static_cast<long long>(N));
  CK_REQUIRE(root_fold >= 0 && root_fold < total_folds && root_unit >= 0 && root_unit < 32768, "ck_mpe_walk: root out of range");
  const int64_t lds = static_cast<int64_t>(total_folds) * S * 2;
  CK_REQUIRE(lds <= CK_SAMPLE_MAX_LDS, "ck_mpe_walk: %d folds x %d rows exceed the LDS budget", total_folds, S);
  const int64_t blocks = (B + S - 1) / S;
  CK_REQUIRE(blocks <= 0x7fffffff, "ck_mpe_walk: too many rows");
  return ck::dispatch(
      [=](hipStream_t s) {
        hipLaunchKernelGGL(mpe_walk_kernel, dim3(static_cast<unsigned>(blocks)), dim3(kWalkThreads), static_cast<size_t>(lds),
                           s, layers, logw, amax, n_layers, root_fold, root_unit, total_folds, S, vals, val_off, bad, row0, B, N,
                           D, ev, x, x_float, logv);
        return hipGetLastError();
      },
      stream);
}
