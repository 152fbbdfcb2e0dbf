// The top-down message pass shared by the flow pass (ck_flow.hip: posterior marginals, expected statistics, EM) and the
// derivative pass (ck_loo.hip: leave-one-out conditionals), DESIGN.md section 11, "The top-down message pass".  Both carry
// one number per unit down an arena laid out as the value arena (global fold g's (B, Ko) block at val_off[g]).  A sum-type
// layer is sent down in two launches, neither with a float atomic: the contraction writes one (B, Ki) MESSAGE block per
// message slot into a scratch buffer, then every child fold combines the messages of its consumers in list order (CSR), so
// results are bit-identical from call to call and for any chunking of the rows.  The pass policy P, a stateless struct of
// static functions, supplies what the two passes do differently:
//   key(x, v)           the log-scale size of a unit of arena value x and log value v (-inf: the unit drops out); the row
//                       maximum m of the keys is the shift;
//   factor(x, v, m)     the unit's shifted linear factor a, the row of the contraction T_i = sum_k a_k w[k, i];
//   emit(tucker, ..., T, m, ..) stores the message(s) of entry i -- nothing for a Tucker layer (`tucker`: the matrix-core
//                       kernel never sees one and passes a constant) -- and returns the value staged for Tucker;
//   tucker(row, ...)    the message of unit u of Tucker input s from the row's staged (Ki, Ki) entry values;
//   identity(), combine(a, b)   the segment combine.
#pragma once

#include "ck_walk.h"

namespace ck {

typedef float f32x16 __attribute__((ext_vector_type(16)));
constexpr int kThreads = 256;
constexpr int kWaves = kThreads / kWave;
constexpr int kMaxLds = 48 * 1024;

inline int64_t blocks_of(int64_t items, int threads) { return (items + threads - 1) / threads; }

// x exp(a + b) to ~2e-7 relative, whatever the size of a and b: the sum is taken exactly as hi + lo (Knuth's two-sum), so
// that its rounding -- |a + b| 2^-24, 4e-5 where observed pixels put the values near -700 -- does not reach the exponential:
// x exp(hi) (1 + lo).  A plain fp32 sum of the log-space terms put ~3e-7 of relative error into every flow of every layer;
// fp64 exp / log, tried first, cost 5.9 ms of flow pass at config 2, 4096 rows.  The core is for
// callers that keep hi small themselves (ck_stats.hip: below its kSlowShift).
__device__ __forceinline__ float scaled_exp_core(float x, float a, float b) {
  const float hi = a + b;
  const float t = hi - a;
  const float lo = (a - (hi - t)) + (b - t);
  const float e = x * expf(hi);
  return fmaf(e, lo, e);
}
// The same for any a + b: where exp(hi) alone would overflow (the product is still <= 1: a unit or an entry with hardly any
// flow) the fp64 expression is used.
__device__ __forceinline__ float scaled_exp(float x, float a, float b) {
  if (__builtin_expect(!(a + b < 80.f), 0))
    return static_cast<float>(static_cast<double>(x) * exp(static_cast<double>(a) + static_cast<double>(b)));
  return scaled_exp_core(x, a, b);
}
// log f - v of a unit that carries flow; a unit with f = 0 (or NaN), or with v = -inf (or not finite), drops out.  Only the
// row maximum m is taken from it, and m is only a shift (the same fp32 value on both sides): the fast logarithm will do.
__device__ __forceinline__ float flow_lg(float f, float v) {
  return (f > 0.f && v > -INFINITY && v < INFINITY) ? __logf(f) - v : -INFINITY;
}
// f exp(-v - m), 0 for a dropped unit (m = -inf only when every unit dropped)
template <bool CHECKED = true>
__device__ __forceinline__ float flow_a(float f, float v, float m) {
  if (!(f > 0.f && v > -INFINITY && v < INFINITY)) return 0.f;
  return CHECKED ? scaled_exp(f, -v, -m) : scaled_exp_core(f, -v, -m);
}

// ---- the contraction, plain VALU path: any layer type, any unit counts ---------------------------------------------
// A workgroup owns one fold and TR rows.  LDS: sa[TR][Ko] = the factors, sm[TR] = m, and for Tucker sf[TR][M] what emit
// returned.
template <class P>
__global__ void __launch_bounds__(kThreads)
    down_sum_generic(int type, int diag, const int32_t* __restrict__ child, const float* __restrict__ w, int64_t F, int H, int Ki,
                     int Ko, int M, const float* __restrict__ vals, const float* __restrict__ arena,
                     const int64_t* __restrict__ val_off, int fold_off, int64_t B, int TR, int64_t row_tiles,
                     float* __restrict__ msg) {
  extern __shared__ float sh[];
  float* const sa = sh;
  float* const sm = sa + TR * Ko;
  float* const sf = sm + TR;
  const int64_t f = blockIdx.x / row_tiles;
  const int64_t n0 = (blockIdx.x % row_tiles) * TR;
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const int64_t blk = val_off[fold_off + f];
  for (int r = wave; r < TR; r += kWaves) {
    const int64_t n = n0 + r;
    float mx = -INFINITY;
    for (int k = lane; k < Ko; k += kWave)
      if (n < B) mx = fmaxf(mx, P::key(arena[blk + n * Ko + k], vals[blk + n * Ko + k]));
    const float m = wave_max(mx);
    for (int k = lane; k < Ko; k += kWave)
      sa[r * Ko + k] = n < B ? P::factor(arena[blk + n * Ko + k], vals[blk + n * Ko + k], m) : 0.f;
    if (lane == 0) sm[r] = m;
  }
  __syncthreads();
  const int32_t* ch = child + f * H;
  const float* wf = w + f * Ko * M;
  for (int it = threadIdx.x; it < TR * M; it += kThreads) {
    const int r = it / M, i = it % M;
    const int64_t n = n0 + r;
    float staged = P::identity();
    if (n < B) {
      float T = 0.f;
      if (diag) {  // mixing: the (K, H K) weight is block diagonal, entry i only meets unit i % Ki
        const int k = i % Ki;
        T = sa[r * Ko + k] * wf[static_cast<int64_t>(k) * M + i];
      } else {
        for (int k = 0; k < Ko; ++k) T = fmaf(sa[r * Ko + k], wf[static_cast<int64_t>(k) * M + i], T);
      }
      staged = P::emit(type == CK_SAMPLE_TUCKER, type, ch, f, H, Ki, B, n, i, T, sm[r], vals, val_off, msg);
    }
    if (type == CK_SAMPLE_TUCKER) sf[it] = staged;
  }
  if (type != CK_SAMPLE_TUCKER) return;
  __syncthreads();
  // Tucker: slot 2 f + s, input 0 unit a reduces over b, input 1 unit b over a
  for (int it = threadIdx.x; it < TR * 2 * Ki; it += kThreads) {
    const int u = it % Ki, s = (it / Ki) % 2, r = it / (2 * Ki);
    const int64_t n = n0 + r;
    if (n >= B) continue;
    msg[((f * 2 + s) * B + n) * Ki + u] = P::tucker(sf + r * M, Ki, s, u, ch, vals, val_off, n);
  }
}

// ---- the contraction on the fp32 matrix cores: sum and CP-T layers of KO = 32 / 64 units, M a multiple of 32 ---------
// One wave owns (fold, 32 rows) and walks the entry tiles: T (32 rows x 32 entries) = a (32 x KO) W (KO x 32) on
// v_mfma_f32_32x32x2_f32.  Lane (b = lane & 31, hi = lane >> 5) holds a[row b][hi KO/2 + kk], so step kk contracts units kk
// and KO/2 + kk: a fixed order, the same for every row wherever its tile starts.
template <class P, int KO>
__global__ void __launch_bounds__(kThreads)
    down_sum_mfma(int type, const int32_t* __restrict__ child, const float* __restrict__ w, int64_t F, int H, int Ki, int M,
                  const float* __restrict__ vals, const float* __restrict__ arena, const int64_t* __restrict__ val_off,
                  int fold_off, int64_t B, int64_t row_tiles, float* __restrict__ msg) {
  constexpr int KH = KO / 2;
  __shared__ float sm[kWaves][32];
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const int b = lane & 31, hi = lane >> 5;
  const int64_t tile = static_cast<int64_t>(blockIdx.x) * kWaves + wave;
  if (tile >= F * row_tiles) return;  // (no workgroup barrier below: the LDS row is the wave's own)
  const int64_t f = tile / row_tiles, n0 = (tile % row_tiles) * 32;
  const int64_t nb = n0 + b < B ? n0 + b : B - 1;
  const int64_t at = val_off[fold_off + f] + nb * KO + hi * KH;
  float a[KH], vk[KH];
  float mx = -INFINITY;
#pragma unroll
  for (int kk = 0; kk < KH; ++kk) {
    a[kk] = arena[at + kk];
    vk[kk] = vals[at + kk];
    mx = fmaxf(mx, P::key(a[kk], vk[kk]));
  }
  const float m = xhalf_max(mx);
#pragma unroll
  for (int kk = 0; kk < KH; ++kk) a[kk] = P::factor(a[kk], vk[kk], m);
  if (hi == 0) sm[wave][b] = m;
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  const int32_t* ch = child + f * H;
  const float* wf = w + f * KO * M + static_cast<int64_t>(hi) * KH * M + b;
  for (int i0 = 0; i0 < M; i0 += 32) {
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
    for (int kk = 0; kk < KH; ++kk)
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[kk], wf[static_cast<int64_t>(kk) * M + i0], acc, 0, 0, 0);
    const int i = i0 + b;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = 8 * (r >> 2) + 4 * hi + (r & 3);
      const int64_t n = n0 + row;
      if (n >= B) continue;
      P::emit(false, type, ch, f, H, Ki, B, n, i, acc[r], sm[wave][row], vals, val_off, msg);
    }
  }
}

// ---- accumulation: every child fold combines its consumers' blocks in list order -----------------------------------
// Child c of the launch (global fold cfold[c]) has the items cstart[c] .. cstart[c + 1] - 1.  An item is a message slot of
// `src` ((B, Ki) block at item B Ki), or with src_is_arena a global fold of the arena itself (the flow pass's Hadamard: unit k
// of every input receives f_k).  cfirst[c] != 0: no earlier launch of this pass wrote the child, the result is stored, not
// combined.
template <class P>
__global__ void __launch_bounds__(kThreads)
    segment_combine(const float* __restrict__ src, int src_is_arena, const int32_t* __restrict__ cstart,
                    const int32_t* __restrict__ cfold, const int32_t* __restrict__ cfirst, const int32_t* __restrict__ items,
                    float* arena, const int64_t* __restrict__ val_off, int64_t n_child, int Ki, int64_t B) {
  const int64_t idx = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  const int64_t per = B * Ki;
  if (idx >= n_child * per) return;
  const int64_t c = idx / per, rem = idx % per;
  float* dst = arena + val_off[cfold[c]] + rem;
  float acc = cfirst[c] ? P::identity() : *dst;
  for (int s = cstart[c]; s < cstart[c + 1]; ++s) {
    const int64_t base = src_is_arena ? val_off[items[s]] : static_cast<int64_t>(items[s]) * per;
    acc = P::combine(acc, src[base + rem]);
  }
  *dst = acc;
}

// ---- launches ------------------------------------------------------------------------------------------------------
template <class P>
int launch_down_sum(const char* fn, int type, int diag, const int32_t* child, const float* w, int64_t F, int H, int Ki, int Ko,
                    int M, const float* vals, const float* arena, const int64_t* val_off, int fold_off, int64_t B, float* msg,
                    void* stream) {
  CK_REQUIRE(type == CK_SAMPLE_SUM || type == CK_SAMPLE_CPT || type == CK_SAMPLE_TUCKER, "%s: not a sum-type layer", fn);
  CK_REQUIRE(child != nullptr && w != nullptr && vals != nullptr && arena != nullptr && val_off != nullptr && msg != nullptr,
             "%s: null pointer", fn);
  CK_REQUIRE(F > 0 && H > 0 && Ki > 0 && Ko > 0 && M > 0 && B > 0 && fold_off >= 0, "%s: non-positive size", fn);
  CK_REQUIRE(M == (type == CK_SAMPLE_SUM ? H * Ki : type == CK_SAMPLE_CPT ? Ki : Ki * Ki) && (type != CK_SAMPLE_TUCKER || H == 2),
             "%s: %d entries for type %d, arity %d, %d input units", fn, M, type, H, Ki);
  CK_REQUIRE(!diag || (type == CK_SAMPLE_SUM && Ko == Ki), "%s: a mixing layer is a sum layer with Ko = Ki", fn);
  if (!diag && type != CK_SAMPLE_TUCKER && (Ko == 32 || Ko == 64) && Ki % 32 == 0) {
    const int64_t row_tiles = (B + 31) / 32;
    const int64_t blocks = blocks_of(F * row_tiles, kWaves);
    CK_REQUIRE(blocks <= 0x7fffffff, "%s: grid too large", fn);
    auto kern = Ko == 32 ? down_sum_mfma<P, 32> : down_sum_mfma<P, 64>;
    return launch(kern, dim3(static_cast<unsigned>(blocks)), dim3(kThreads), 0, stream, type, child, w, F, H, Ki, M, vals, arena,
                  val_off, fold_off, B, row_tiles, msg);
  }
  const int64_t per_row = static_cast<int64_t>(Ko) + 1 + (type == CK_SAMPLE_TUCKER ? M : 0);
  int TR = 16;
  while (TR > 1 && TR * per_row * 4 > kMaxLds) TR /= 2;
  CK_REQUIRE(TR * per_row * 4 <= kMaxLds, "%s: %d units and %d entries exceed the LDS budget", fn, Ko, M);
  const int64_t row_tiles = (B + TR - 1) / TR;
  CK_REQUIRE(F * row_tiles <= 0x7fffffff, "%s: grid too large", fn);
  const size_t lds = static_cast<size_t>(TR * per_row * 4);
  return launch(down_sum_generic<P>, dim3(static_cast<unsigned>(F * row_tiles)), dim3(kThreads), lds, stream, type, diag, child,
                w, F, H, Ki, Ko, M, vals, arena, val_off, fold_off, B, TR, row_tiles, msg);
}

template <class P>
int launch_segment(const char* fn, const float* src, int src_is_arena, const int32_t* cstart, const int32_t* cfold,
                   const int32_t* cfirst, const int32_t* items, float* arena, const int64_t* val_off, int64_t n_child, int Ki,
                   int64_t B, void* stream) {
  CK_REQUIRE(src != nullptr && cstart != nullptr && cfold != nullptr && cfirst != nullptr && items != nullptr &&
                 arena != nullptr && val_off != nullptr,
             "%s: null pointer", fn);
  CK_REQUIRE(n_child > 0 && Ki > 0 && B > 0, "%s: non-positive size", fn);
  const int64_t blocks = blocks_of(n_child * B * Ki, kThreads);
  CK_REQUIRE(blocks <= 0x7fffffff, "%s: too many entries", fn);
  return launch(segment_combine<P>, dim3(static_cast<unsigned>(blocks)), dim3(kThreads), 0, stream, src, src_is_arena, cstart,
                cfold, cfirst, items, arena, val_off, n_child, Ki, B);
}

// The unit counts of a product layer: Hadamard Ko = Ki, Kronecker Ko = Ki^H.
inline int check_product_shape(const char* fn, int type, int H, int Ki, int Ko) {
  if (type == CK_SAMPLE_HADAMARD) {
    CK_REQUIRE(Ko == Ki, "%s: Hadamard with %d inputs, %d outputs", fn, Ki, Ko);
  } else {
    int64_t p = 1;
    for (int h = 0; h < H && p <= Ko; ++h) p *= Ki;
    CK_REQUIRE(p == Ko, "%s: Kronecker of %d inputs of %d units with %d outputs", fn, H, Ki, Ko);
  }
  return 0;
}

}  // namespace ck
