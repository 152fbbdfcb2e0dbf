// Marginal MAP ("Marginal MAP"): the mixed sum / max upward pass of a masked batch into MPE's
// (F, B, Ko)-per-layer arena, then the argmax walk that stops where the summing starts.  The query set Q is one per call:
// max_fold[g] says whether global fold g has a query variable in its scope.  A sum-type unit of a max fold is MPE's
// max_i (log w_i + v_i), of a sum fold log sum_i w_i exp(v_i), the value of the marginal forward; an input unit gives
// log p(x_v) where observed, vmax where its variable is in Q, and its log integral vsum where it is summed out.  Product
// layers run ck_mpe_up_product.
#include <math.h>

#include "ck_mpe_policy.h"

namespace {

using ck::blocks_of;
using ck::kKM;
using ck::kMC;
using ck::kRM;
using ck::kUpThreads;

// ---- per-parameter-state input table -------------------------------------------------------------------------------
// Per (fold, unit): the log integral of the unit, the number the marginal forward gives an integrated unit of the layer.  A
// Gaussian: log_partition or 0.  A table with an integral row (row_c: the Binomial log-pmf table's row C): that row.  A
// table of logits: their logsumexp, in the arithmetic of the forward's integral row (ck_param.hip).  Probabilities: 0.
__global__ void __launch_bounds__(256)
    mmap_input_sum_kernel(int type, const float* __restrict__ tab, int64_t sf, int64_t sk, int64_t sc, int t_log, int C,
                          int row_c, const float* __restrict__ lz, int64_t F, int K, float* __restrict__ vsum) {
  const int64_t o = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (o >= F * K) return;
  float v = 0.f;
  if (type == CK_SAMPLE_GAUSSIAN) {
    if (lz != nullptr) v = lz[o];
  } else {
    const float* row = tab + (o / K) * sf + (o % K) * sk;
    if (row_c) {
      v = row[C * sc];
    } else if (t_log) {
      float mx = -INFINITY;
      for (int c = 0; c < C; ++c) mx = fmaxf(mx, row[c * sc]);
      float sacc = 0.f;
      for (int c = 0; c < C; ++c) sacc += expf(row[c * sc] - mx);
      v = mx + logf(sacc);
    }
  }
  vsum[o] = v;
}

// ---- upward pass ---------------------------------------------------------------------------------------------------
// Input layer: mpe_up_input_kernel (ck_mpe.hip) with the role of an unobserved entry read from is_query: vmax for a query
// variable, vsum for any other.  The same sentinels, range check, bad and flag.
__global__ void __launch_bounds__(256)
    mmap_up_input_kernel(int type, const int64_t* __restrict__ scope, const float* __restrict__ tab, int64_t sf, int64_t sk,
                         int64_t sc, int t_log, int C, const float* __restrict__ mean, const float* __restrict__ stddev,
                         const float* __restrict__ lz, const float* __restrict__ vmax, const float* __restrict__ vsum,
                         const uint8_t* __restrict__ is_query, int64_t F, int K, const void* __restrict__ ev, int x_float,
                         int64_t B, int D, float* __restrict__ vals, const int64_t* __restrict__ val_off, int fold_off,
                         int32_t* flag, int32_t* bad) {
  const int64_t idx = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (idx >= F * B * K) return;
  const int k = static_cast<int>(idx % K);
  const int64_t rest = idx / K;
  const int64_t n = rest % B, f = rest / B;
  const int64_t o = f * K + k;
  const int64_t var = scope[f];
  const int64_t e_at = n * D + var;
  float v, x = 0.f;
  int64_t c = 0;
  if (!ck::observed(ev, e_at, x_float, type == CK_SAMPLE_GAUSSIAN, x, c)) {
    v = is_query[var] ? vmax[o] : vsum[o];
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

// Sum, mixing, CP-T and Tucker layers, mpe_up_sum_kernel's tiling (ck_mpe.hip): a workgroup owns one fold, TR rows and TK
// units, stages kMC entries per step in LDS, and every thread keeps a kRM x kKM micro-tile in registers.  The semiring is the
// fold's: max_fold[fold_off + f] is read once, so the branch is workgroup-uniform.
//   max fold: MPE's loop, the same helpers in the same order, so the values are MPE's bit for bit.
//   sum fold of a mixing layer (block-diagonal weights): elementwise, a maximum per unit.
//   any other sum fold: linear space.  A first sweep forms the row maximum m_r of the entry values (16 threads per row; Tucker:
//   max v0 + max v1, which is the maximum of its entries exactly, from 2 Ki reads instead of Ki^2); the staging step writes
//   exp(e - m_r) and the linear weight (0 for padding, e = -inf and w <= 0), the micro-tile accumulates acc += w p, one fma
//   per entry and no transcendental, and the store is m_r + log(acc): -inf, never NaN, for a row whose entries are all -inf.
template <int TK>
__global__ void __launch_bounds__(kUpThreads)
    mmap_up_sum_kernel(int type, const int32_t* __restrict__ child, const float* __restrict__ lw, const float* __restrict__ w,
                       const uint8_t* __restrict__ max_fold, int mixing, int64_t F, int H, int Ki, int Ko, int M,
                       float* __restrict__ vals, const int64_t* __restrict__ val_off, int fold_off, int64_t B,
                       int64_t row_tiles) {
  constexpr int TKT = TK / kKM;          // threads along the units
  constexpr int TRT = kUpThreads / TKT;  // threads along the rows
  constexpr int TR = TRT * kRM;          // rows of the tile
  constexpr int EP = TR + 4;             // (padded LDS row: the staging writes spread over the banks)
  static_assert((TR * kMC) % kUpThreads == 0, "the row sweep keeps every lane of a wave in its shuffles");
  __shared__ float4 sE[kMC * EP / 4];    // sE[m][r]: entry m0 + m of tile row r (sum fold: exp(entry - m_r))
  __shared__ float4 sW[kMC * TK / 4];    // sW[m][k]: log weight of unit k0 + k, entry m0 + m (sum fold: the weight)
  __shared__ float4 sM[TR / 4];          // sM[r]: m_r of a sum fold
  float* const sEf = reinterpret_cast<float*>(sE);
  float* const sWf = reinterpret_cast<float*>(sW);
  float* const sMf = reinterpret_cast<float*>(sM);
  const int64_t f = blockIdx.x / row_tiles;
  const int64_t n0 = (blockIdx.x % row_tiles) * TR;
  const int k0 = blockIdx.y * TK;
  const int tk = threadIdx.x % TKT, tr = threadIdx.x / TKT;
  const int32_t* ch = child + f * H;
  const bool maximise = max_fold[fold_off + f] != 0;
  float acc[kRM][kKM];
  if (maximise) {
    const float* wf = lw + f * Ko * M;
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
  } else if (mixing) {
    // a unit of a mixing fold reads one entry per input, unit k of input h: its own maximum over the inputs, as the
    // reference's mixing layer takes it (a row maximum over other units' entries could underflow every term of this one)
    const float* wf = w + f * Ko * M;
#pragma unroll
    for (int i = 0; i < kRM; ++i) {
      const int64_t n = n0 + tr * kRM + i;
#pragma unroll
      for (int j = 0; j < kKM; ++j) {
        const int k = k0 + tk * kKM + j;
        acc[i][j] = 0.f;
        if (n >= B || k >= Ko) continue;
        float mx = -INFINITY, sum = 0.f;
        for (int h = 0; h < H; ++h) mx = fmaxf(mx, vals[val_off[ch[h]] + n * Ki + k]);
        for (int h = 0; h < H; ++h) {
          const float e = vals[val_off[ch[h]] + n * Ki + k];
          const float wv = wf[static_cast<int64_t>(k) * M + h * Ki + k];
          if (wv > 0.f && e != -INFINITY) sum = fmaf(wv, __expf(e - mx), sum);
        }
        acc[i][j] = mx + __logf(sum);
      }
    }
  } else {
    const float* wf = w + f * Ko * M;
    for (int t = threadIdx.x; t < TR * kMC; t += kUpThreads) {  // the row maxima: 16 neighbouring lanes per row
      const int q = t % kMC, r = t / kMC;
      float mx = 0.f;
      if (n0 + r < B) {
        if (type == CK_SAMPLE_TUCKER) {
          const float* v0 = vals + val_off[ch[0]] + (n0 + r) * Ki;
          const float* v1 = vals + val_off[ch[1]] + (n0 + r) * Ki;
          float a = -INFINITY, b = -INFINITY;
          for (int j = q; j < Ki; j += kMC) {
            a = fmaxf(a, v0[j]);
            b = fmaxf(b, v1[j]);
          }
#pragma unroll
          for (int d = kMC / 2; d > 0; d >>= 1) {
            a = fmaxf(a, __shfl_xor(a, d, kMC));
            b = fmaxf(b, __shfl_xor(b, d, kMC));
          }
          mx = a + b;
        } else {
          mx = -INFINITY;
          for (int i = q; i < M; i += kMC) mx = fmaxf(mx, ck::entry_value(type, ch, H, Ki, vals, val_off, n0 + r, i));
#pragma unroll
          for (int d = kMC / 2; d > 0; d >>= 1) mx = fmaxf(mx, __shfl_xor(mx, d, kMC));
        }
      }
      if (q == 0) sMf[r] = mx;
    }
#pragma unroll
    for (int i = 0; i < kRM; ++i)
#pragma unroll
      for (int j = 0; j < kKM; ++j) acc[i][j] = 0.f;
    __syncthreads();
    for (int m0 = 0; m0 < M; m0 += kMC) {
      for (int t = threadIdx.x; t < TR * kMC; t += kUpThreads) {
        const int m = t % kMC, r = t / kMC;
        float p = 0.f;
        if (m0 + m < M && n0 + r < B) {
          const float e = ck::entry_value(type, ch, H, Ki, vals, val_off, n0 + r, m0 + m);
          if (e != -INFINITY) p = __expf(e - sMf[r]);
        }
        sEf[m * EP + r] = p;
      }
      for (int t = threadIdx.x; t < TK * kMC; t += kUpThreads) {
        const int m = t % kMC, k = t / kMC;
        float wv = 0.f;
        if (m0 + m < M && k0 + k < Ko) wv = wf[static_cast<int64_t>(k0 + k) * M + m0 + m];
        sWf[m * TK + k] = wv > 0.f ? wv : 0.f;
      }
      __syncthreads();
#pragma unroll
      for (int m = 0; m < kMC; ++m) {
        const float4 e0 = sE[(m * EP) / 4 + tr];
        const float4 w0 = sW[(m * TK) / 4 + tk];
        const float ea[kRM] = {e0.x, e0.y, e0.z, e0.w};
        const float wa[kKM] = {w0.x, w0.y, w0.z, w0.w};
#pragma unroll
        for (int i = 0; i < kRM; ++i)
#pragma unroll
          for (int j = 0; j < kKM; ++j) acc[i][j] = fmaf(wa[j], ea[i], acc[i][j]);
      }
      __syncthreads();
    }
    const float4 m4 = sM[tr];
    const float mr[kRM] = {m4.x, m4.y, m4.z, m4.w};
#pragma unroll
    for (int i = 0; i < kRM; ++i)
#pragma unroll
      for (int j = 0; j < kKM; ++j) acc[i][j] = mr[i] + __logf(acc[i][j]);
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

// ---- argmax walk ---------------------------------------------------------------------------------------------------
// MPE's policy with the two rules of marginal MAP: a sum fold on the tree takes no entry, so the walk ends there (nothing
// below it holds a query variable), and an input unit writes only a query variable (a summed-out entry keeps its sentinel).
struct MmapArgmax {
  ck::MpeArgmax mpe;
  const uint8_t* max_fold;
  const uint8_t* is_query;

  __device__ bool root(int64_t n, float r) const { return mpe.root(n, r); }

  __device__ int choose(const ck_sample_layer& L, const float* __restrict__ wr, const int32_t* __restrict__ ch,
                        const float* __restrict__ vals, const int64_t* __restrict__ val_off, int64_t nl, int64_t n, int g,
                        int lane) const {
    return max_fold[g] ? mpe.choose(L, wr, ch, vals, val_off, nl, n, g, lane) : -1;
  }

  __device__ void fill(const ck_sample_layer& L, int li, int f, int k, int64_t n, int g, void* __restrict__ x, int x_float,
                       int64_t o) const {
    if (is_query[L.scope[f]]) mpe.fill(L, li, f, k, n, g, x, x_float, o);
  }
};

}  // namespace

int ck_mmap_input_sum(int type, const float* tab, int64_t sf, int64_t sk, int64_t sc, int t_log, int C, int row_c,
                      const float* log_partition, int64_t F, int K, float* vsum, void* stream) {
  CK_REQUIRE(type == CK_SAMPLE_CATEGORICAL || type == CK_SAMPLE_GAUSSIAN, "ck_mmap_input_sum: not an input layer type");
  CK_REQUIRE(vsum != nullptr, "ck_mmap_input_sum: null pointer");
  CK_REQUIRE(type == CK_SAMPLE_GAUSSIAN || (tab != nullptr && C > 0), "ck_mmap_input_sum: missing parameters");
  CK_REQUIRE(F > 0 && K > 0, "ck_mmap_input_sum: non-positive size");
  const int64_t blocks = blocks_of(F * K, 256);
  CK_REQUIRE(blocks <= 0x7fffffff, "ck_mmap_input_sum: too many units");
  return ck::launch(mmap_input_sum_kernel, dim3(static_cast<unsigned>(blocks)), dim3(256), 0, stream, type, tab, sf, sk, sc,
                    t_log, C, row_c, log_partition, F, K, vsum);
}

int ck_mmap_up_input(int type, const int64_t* scope, const float* tab, int64_t sf, int64_t sk, int64_t sc, int t_log, int C,
                     const float* mean, const float* stddev, const float* log_partition, const float* vmax, const float* vsum,
                     const uint8_t* is_query, int64_t F, int K, const void* ev, int x_float, int64_t B, int D, float* vals,
                     const int64_t* val_off, int fold_off, int32_t* flag, int32_t* bad, void* stream) {
  CK_REQUIRE(type == CK_SAMPLE_CATEGORICAL || type == CK_SAMPLE_GAUSSIAN, "ck_mmap_up_input: not an input layer type");
  CK_REQUIRE(scope != nullptr && vmax != nullptr && vsum != nullptr && is_query != nullptr && ev != nullptr &&
                 vals != nullptr && val_off != nullptr && bad != nullptr,
             "ck_mmap_up_input: null pointer");
  CK_REQUIRE(type == CK_SAMPLE_GAUSSIAN ? (mean != nullptr && stddev != nullptr && x_float) : (tab != nullptr && C > 0),
             "ck_mmap_up_input: missing parameters (a Gaussian layer reads an fp32 batch)");
  CK_REQUIRE(F > 0 && K > 0 && B > 0 && D > 0 && fold_off >= 0, "ck_mmap_up_input: non-positive size");
  const int64_t blocks = blocks_of(F * B * K, 256);
  CK_REQUIRE(blocks <= 0x7fffffff, "ck_mmap_up_input: too many entries");
  return ck::launch(mmap_up_input_kernel, dim3(static_cast<unsigned>(blocks)), dim3(256), 0, stream, type, scope, tab, sf, sk,
                    sc, t_log, C, mean, stddev, log_partition, vmax, vsum, is_query, F, K, ev, x_float, B, D, vals, val_off,
                    fold_off, flag, bad);
}

int ck_mmap_up_sum(int type, const int32_t* child, const float* lw, const float* w, const uint8_t* max_fold, int mixing,
                   int64_t F, int H, int Ki, int Ko, int M, float* vals, const int64_t* val_off, int fold_off, int64_t B,
                   void* stream) {
  CK_REQUIRE(type == CK_SAMPLE_SUM || type == CK_SAMPLE_CPT || type == CK_SAMPLE_TUCKER, "ck_mmap_up_sum: not a sum-type layer");
  CK_REQUIRE(child != nullptr && lw != nullptr && w != nullptr && max_fold != nullptr && vals != nullptr && val_off != nullptr,
             "ck_mmap_up_sum: null pointer");
  CK_REQUIRE(F > 0 && H > 0 && Ki > 0 && Ko > 0 && M > 0 && B > 0 && fold_off >= 0, "ck_mmap_up_sum: non-positive size");
  CK_REQUIRE(M == (type == CK_SAMPLE_SUM ? H * Ki : type == CK_SAMPLE_CPT ? Ki : Ki * Ki) && (type != CK_SAMPLE_TUCKER || H == 2),
             "ck_mmap_up_sum: %d entries for type %d, arity %d, %d input units", M, type, H, Ki);
  CK_REQUIRE(!mixing || (type == CK_SAMPLE_SUM && Ko == Ki), "ck_mmap_up_sum: a mixing layer is a sum layer with Ko == Ki");
  const int tk = Ko <= 16 ? 16 : Ko <= 32 ? 32 : 64;
  const int tr = kUpThreads / (tk / kKM) * kRM;
  const int64_t row_tiles = (B + tr - 1) / tr, unit_tiles = (Ko + tk - 1) / tk;
  CK_REQUIRE(F * row_tiles <= 0x7fffffff && unit_tiles <= 65535, "ck_mmap_up_sum: grid too large");
  const dim3 grid(static_cast<unsigned>(F * row_tiles), static_cast<unsigned>(unit_tiles));
  decltype(&mmap_up_sum_kernel<16>) kern;
  if (tk == 16) kern = mmap_up_sum_kernel<16>;
  else if (tk == 32) kern = mmap_up_sum_kernel<32>;
  else kern = mmap_up_sum_kernel<64>;
  return ck::launch(kern, grid, dim3(kUpThreads), 0, stream, type, child, lw, w, max_fold, mixing, F, H, Ki, Ko, M, vals,
                    val_off, fold_off, B, row_tiles);
}

int ck_mmap_walk(const ck_sample_layer* layers, const float* const* logw, const int32_t* const* amax,
                 const uint8_t* max_fold, const uint8_t* is_query, int n_layers, int root_fold, int root_unit,
                 int total_folds, int S, const float* vals, const int64_t* val_off, const int32_t* bad, int64_t row0, int64_t B,
                 int64_t N, int D, const void* ev, void* x, int x_float, float* logv, void* stream) {
  CK_REQUIRE(amax != nullptr && bad != nullptr && logv != nullptr && max_fold != nullptr && is_query != nullptr,
             "ck_mmap_walk: null pointer");
  return ck::evidence_walk("ck_mmap_walk", layers, logw, n_layers, root_fold, root_unit, total_folds, S, vals, val_off, row0,
                           B, N, D, ev, x, x_float, MmapArgmax{ck::MpeArgmax{amax, bad, logv}, max_fold, is_query}, stream);
}
