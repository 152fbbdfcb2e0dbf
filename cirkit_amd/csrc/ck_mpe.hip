// Most probable explanation ("Most probable explanation"): the max-product ("Viterbi") upward pass of
// a masked batch, one launch per layer into an (F, B, Ko)-per-layer arena, then the argmax walk top down.  A sum-type unit's
// value is max_i (log w_i + v_i), a product unit's the sum of its children's values, an input unit's log p(x_v) where x_v
// is observed and max_c log p(c) where it is maximised.  The walk picks the smallest entry index among the maxima.
#include <math.h>

#include "ck_mpe_policy.h"

namespace {

// (the tile shape and the walk policy MpeArgmax: ck_mpe_policy.h, shared with ck_mmap.hip)
using ck::blocks_of;
using ck::kKM;
using ck::kMC;
using ck::kRM;
using ck::kUpThreads;
using ck::MpeArgmax;

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
  float v, x = 0.f;
  int64_t c = 0;
  if (!ck::observed(ev, e_at, x_float, type == CK_SAMPLE_GAUSSIAN, x, c)) {
    v = vmax[o];
  } else if (type == CK_SAMPLE_GAUSSIAN) {
    v = ck::mpe_gauss(x, mean[o], stddev[o], lz, o);
  } else {
    if (x_float) c = x >= static_cast<float>(C) ? C : static_cast<int64_t>(x);
    if (c >= C) {
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
      if (m0 + m < M && n0 + r < B) e = ck::entry_value(type, ch, H, Ki, vals, val_off, n0 + r, m0 + m);
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
  return ck::launch(mpe_input_max_kernel, dim3(static_cast<unsigned>(blocks)), dim3(256), 0, stream, type, tab, sf, sk, sc, t_log,
                    C, mean, stddev, log_partition, F, K, vmax, amax);
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
  return ck::launch(mpe_up_input_kernel, dim3(static_cast<unsigned>(blocks)), dim3(256), 0, stream, type, scope, tab, sf, sk, sc,
                    t_log, C, mean, stddev, log_partition, vmax, F, K, ev, x_float, B, D, vals, val_off, fold_off, flag, bad);
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
  decltype(&mpe_up_sum_kernel<16>) kern;
  if (tk == 16) kern = mpe_up_sum_kernel<16>;
  else if (tk == 32) kern = mpe_up_sum_kernel<32>;
  else kern = mpe_up_sum_kernel<64>;
  return ck::launch(kern, grid, dim3(kUpThreads), 0, stream, type, child, lw, F, H, Ki, Ko, M, vals, val_off, fold_off, B,
                    row_tiles);
}

int ck_mpe_up_product(int type, const int32_t* child, int64_t F, int H, int Ki, int Ko, float* vals, const int64_t* val_off,
                      int fold_off, int64_t B, void* stream) {
  CK_REQUIRE(type == CK_SAMPLE_HADAMARD || type == CK_SAMPLE_KRONECKER, "ck_mpe_up_product: not a product layer");
  CK_REQUIRE(child != nullptr && vals != nullptr && val_off != nullptr, "ck_mpe_up_product: null pointer");
  CK_REQUIRE(F > 0 && H > 0 && Ki > 0 && Ko > 0 && B > 0 && fold_off >= 0, "ck_mpe_up_product: non-positive size");
  CK_REQUIRE(type == CK_SAMPLE_HADAMARD ? Ko == Ki : true, "ck_mpe_up_product: Hadamard with %d inputs, %d outputs", Ki, Ko);
  const int64_t blocks = blocks_of(F * B * Ko, 256);
  CK_REQUIRE(blocks <= 0x7fffffff, "ck_mpe_up_product: too many entries");
  return ck::launch(mpe_up_product_kernel, dim3(static_cast<unsigned>(blocks)), dim3(256), 0, stream, type, child, F, H, Ki, Ko,
                    vals, val_off, fold_off, B);
}

int ck_mpe_walk(const ck_sample_layer* layers, const float* const* logw, const int32_t* const* amax, int n_layers,
                int root_fold, int root_unit, int total_folds, int S, const float* vals, const int64_t* val_off,
                const int32_t* bad, int64_t row0, int64_t B, int64_t N, int D, const void* ev, void* x, int x_float,
                float* logv, void* stream) {
  CK_REQUIRE(amax != nullptr && bad != nullptr && logv != nullptr, "ck_mpe_walk: null pointer");
  return ck::evidence_walk("ck_mpe_walk", layers, logw, n_layers, root_fold, root_unit, total_folds, S, vals, val_off, row0,
                           B, N, D, ev, x, x_float, MpeArgmax{amax, bad, logv}, stream);
}
