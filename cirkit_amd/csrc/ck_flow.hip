// Posterior marginals ("Posterior marginals"): the top-down FLOW pass behind
// `HipCircuit.posterior_marginals`.  With v the per-row log values of the layer-wise marginal forward of the evidence, the
// flow of a unit is f(u) = d log c(x_O) / d log u, in LINEAR space, f(root) = 1.  Flows live in an fp32 arena laid out as the
// value arena (global fold g's (B, Ko) block at val_off[g]).  A layer is sent down in two launches, neither with a float
// atomic: the contraction writes one (B, Ki) MESSAGE block per (fold, input slot) into a scratch buffer, then every child
// fold adds the messages of its consumers in list order (CSR), so results are bit-identical from call to call.
#include <math.h>

#include "ck_walk.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
constexpr int kThreads = 256;
constexpr int kWaves = kThreads / ck::kWave;
constexpr int kMaxLds = 48 * 1024;

// log f - v of a unit that carries flow; a unit with f = 0 (or NaN), or with v = -inf (or not finite), drops out.  Only the
// row maximum m is taken from it, and m is only a shift (the same fp32 value on both sides): the fast logarithm will do.
__device__ __forceinline__ float flow_lg(float f, float v) {
  return (f > 0.f && v > -INFINITY && v < INFINITY) ? __logf(f) - v : -INFINITY;
}
// x exp(a + b) to ~2e-7 relative, whatever the size of a and b: the sum is taken exactly as hi + lo (Knuth's two-sum), so
// that its rounding -- |a + b| 2^-24, 4e-5 where observed pixels put the values near -700 -- does not reach the exponential:
// x exp(hi) (1 + lo).  A plain fp32 sum of the log-space terms put ~3e-7 of relative error into every flow of every layer;
// fp64 exp / log, tried first, cost 5.9 ms of flow pass at config 2, 4096 rows.  Where exp(hi) alone
// would overflow (the product is still <= 1: a unit or an entry with hardly any flow) the fp64 expression is used.
__device__ __forceinline__ float scaled_exp(float x, float a, float b) {
  const float hi = a + b;
  const float t = hi - a;
  const float lo = (a - (hi - t)) + (b - t);
  if (__builtin_expect(!(hi < 80.f), 0))
    return static_cast<float>(static_cast<double>(x) * exp(static_cast<double>(a) + static_cast<double>(b)));
  const float e = x * expf(hi);
  return fmaf(e, lo, e);
}
// f exp(-v - m), 0 for a dropped unit (m = -inf only when every unit dropped)
__device__ __forceinline__ float flow_a(float f, float v, float m) {
  return (f > 0.f && v > -INFINITY && v < INFINITY) ? scaled_exp(f, -v, -m) : 0.f;
}
// T exp(m + e) with nothing exponentiated unshifted; T = 0 gives exactly 0, e = -inf gives 0.
__device__ __forceinline__ float flow_out(float T, float m, float e) {
  if (!(T > 0.f)) return 0.f;
  if (e == -INFINITY) return 0.f;
  return scaled_exp(T, m, e);
}

// Where the flow of entry i of fold f at row n goes: sum / mixing slot f H + i / Ki unit i % Ki; CP-T slot f unit i.
__device__ __forceinline__ int64_t msg_index(int type, int64_t f, int H, int Ki, int64_t B, int64_t n, int i) {
  const int64_t slot = type == CK_SAMPLE_SUM ? f * H + i / Ki : f;
  const int unit = type == CK_SAMPLE_SUM ? i % Ki : i;
  return (slot * B + n) * Ki + unit;
}

// ---- the contraction, plain VALU path: any layer type, any unit counts ---------------------------------------------
// A workgroup owns one fold and TR rows.  LDS: sa[TR][Ko] = exp(lg - m), sm[TR] = m, and for Tucker sf[TR][M] entry flows.
__global__ void __launch_bounds__(kThreads)
    flow_down_sum_generic(int type, int diag, const int32_t* __restrict__ child, const float* __restrict__ w, int64_t F, int H,
                          int Ki, int Ko, int M, const float* __restrict__ vals, const float* __restrict__ flow,
                          const int64_t* __restrict__ val_off, int fold_off, int64_t B, int TR, int64_t row_tiles,
                          float* __restrict__ msg) {
  extern __shared__ float sh[];
  float* const sa = sh;
  float* const sm = sa + TR * Ko;
  float* const sf = sm + TR;
  const int64_t f = blockIdx.x / row_tiles;
  const int64_t n0 = (blockIdx.x % row_tiles) * TR;
  const int lane = threadIdx.x & (ck::kWave - 1), wave = threadIdx.x / ck::kWave;
  const int64_t blk = val_off[fold_off + f];
  for (int r = wave; r < TR; r += kWaves) {
    const int64_t n = n0 + r;
    float mx = -INFINITY;
    for (int k = lane; k < Ko; k += ck::kWave)
      if (n < B) mx = fmaxf(mx, flow_lg(flow[blk + n * Ko + k], vals[blk + n * Ko + k]));
    const float m = ck::wave_max(mx);
    for (int k = lane; k < Ko; k += ck::kWave)
      sa[r * Ko + k] = n < B ? flow_a(flow[blk + n * Ko + k], vals[blk + n * Ko + k], m) : 0.f;
    if (lane == 0) sm[r] = m;
  }
  __syncthreads();
  const int32_t* ch = child + f * H;
  const float* wf = w + f * Ko * M;
  for (int it = threadIdx.x; it < TR * M; it += kThreads) {
    const int r = it / M, i = it % M;
    const int64_t n = n0 + r;
    float fl = 0.f;
    if (n < B) {
      float T = 0.f;
      if (diag) {  // mixing: the (K, H K) weight is block diagonal, entry i only meets unit i % Ki
        const int k = i % Ki;
        T = sa[r * Ko + k] * wf[static_cast<int64_t>(k) * M + i];
      } else {
        for (int k = 0; k < Ko; ++k) T = fmaf(sa[r * Ko + k], wf[static_cast<int64_t>(k) * M + i], T);
      }
      if (T > 0.f) fl = flow_out(T, sm[r], ck::entry_value(type, ch, H, Ki, vals, val_off, n, i));
      if (type != CK_SAMPLE_TUCKER) msg[msg_index(type, f, H, Ki, B, n, i)] = fl;
    }
    if (type == CK_SAMPLE_TUCKER) sf[it] = fl;
  }
  if (type != CK_SAMPLE_TUCKER) return;
  __syncthreads();
  // Tucker: input 0 unit a receives the sum over b, input 1 unit b the sum over a
  for (int it = threadIdx.x; it < TR * 2 * Ki; it += kThreads) {
    const int u = it % Ki, s = (it / Ki) % 2, r = it / (2 * Ki);
    const int64_t n = n0 + r;
    if (n >= B) continue;
    const float* row = sf + r * M;
    float acc = 0.f;
    if (s == 0) {
      for (int b = 0; b < Ki; ++b) acc += row[u * Ki + b];
    } else {
      for (int a = 0; a < Ki; ++a) acc += row[a * Ki + u];
    }
    msg[((f * 2 + s) * B + n) * Ki + u] = acc;
  }
}

// ---- the contraction on the fp32 matrix cores: sum and CP-T layers of KO = 32 / 64 units, M a multiple of 32 ---------
// One wave owns (fold, 32 rows) and walks the entry tiles: T (32 rows x 32 entries) = a (32 x KO) W (KO x 32) on
// v_mfma_f32_32x32x2_f32.  Lane (b = lane & 31, hi = lane >> 5) holds a[row b][hi KO/2 + kk], so step kk contracts units kk
// and KO/2 + kk: a fixed order, the same for every row wherever its tile starts.
template <int KO>
__global__ void __launch_bounds__(kThreads)
    flow_down_sum_mfma(int type, const int32_t* __restrict__ child, const float* __restrict__ w, int64_t F, int H, int Ki,
                       int M, const float* __restrict__ vals, const float* __restrict__ flow,
                       const int64_t* __restrict__ val_off, int fold_off, int64_t B, int64_t row_tiles,
                       float* __restrict__ msg) {
  constexpr int KH = KO / 2;
  __shared__ float sm[kWaves][32];
  const int lane = threadIdx.x & (ck::kWave - 1), wave = threadIdx.x / ck::kWave;
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
    a[kk] = flow[at + kk];
    vk[kk] = vals[at + kk];
    mx = fmaxf(mx, flow_lg(a[kk], vk[kk]));
  }
  const float m = ck::xhalf_max(mx);
#pragma unroll
  for (int kk = 0; kk < KH; ++kk) a[kk] = flow_a(a[kk], vk[kk], m);
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
      const float T = acc[r];
      float fl = 0.f;
      if (T > 0.f) fl = flow_out(T, sm[wave][row], ck::entry_value(type, ch, H, Ki, vals, val_off, n, i));
      msg[msg_index(type, f, H, Ki, B, n, i)] = fl;
    }
  }
}

// ---- accumulation: every child fold adds its consumers' blocks in list order ----------------------------------------
// Child c of the launch (global fold cfold[c]) has the items cstart[c] .. cstart[c + 1] - 1.  An item is a message slot of
// `src` ((B, Ki) block at item B Ki), or with src_is_flow a global fold of the flow arena itself (Hadamard: unit k of every
// input receives f_k).  cfirst[c] != 0: no earlier launch of this pass wrote the child, the sum is stored, not added.
__global__ void __launch_bounds__(kThreads)
    flow_add_rows_kernel(const float* __restrict__ src, int src_is_flow, const int32_t* __restrict__ cstart,
                         const int32_t* __restrict__ cfold, const int32_t* __restrict__ cfirst,
                         const int32_t* __restrict__ items, float* flow, const int64_t* __restrict__ val_off, int64_t n_child,
                         int Ki, int64_t B) {
  const int64_t idx = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  const int64_t per = B * Ki;
  if (idx >= n_child * per) return;
  const int64_t c = idx / per, rem = idx % per;
  float* dst = flow + val_off[cfold[c]] + rem;
  float acc = cfirst[c] ? 0.f : *dst;
  for (int s = cstart[c]; s < cstart[c + 1]; ++s) {
    const int64_t base = src_is_flow ? val_off[items[s]] : static_cast<int64_t>(items[s]) * per;
    acc += src[base + rem];
  }
  *dst = acc;
}

// Kronecker: item (parent global fold g, input position h); unit i of the child receives the sum of the parent's flow over
// the outputs whose digit h (base Ki, input 0 most significant) is i, in ascending output order.
__global__ void __launch_bounds__(kThreads)
    flow_kron_kernel(const int32_t* __restrict__ cstart, const int32_t* __restrict__ cfold, const int32_t* __restrict__ cfirst,
                     const int32_t* __restrict__ items, float* flow, const int64_t* __restrict__ val_off, int64_t n_child,
                     int H, int Ki, int Ko, int64_t B) {
  const int64_t idx = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  const int64_t per = B * Ki;
  if (idx >= n_child * per) return;
  const int64_t c = idx / per, rem = idx % per;
  const int64_t n = rem / Ki;
  const int i = static_cast<int>(rem % Ki);
  float* dst = flow + val_off[cfold[c]] + rem;
  float acc = cfirst[c] ? 0.f : *dst;
  for (int s = cstart[c]; s < cstart[c + 1]; ++s) {
    const float* p = flow + val_off[items[2 * s]] + n * Ko;
    int stride = 1;
    for (int h = H - 1; h > items[2 * s + 1]; --h) stride *= Ki;
    for (int top = 0; top < Ko / (stride * Ki); ++top)
      for (int lo = 0; lo < stride; ++lo) acc += p[(top * Ki + i) * stride + lo];
  }
  *dst = acc;
}

// ---- leaves --------------------------------------------------------------------------------------------------------
// Per query variable q the entries qstart[q] .. qstart[q + 1] - 1, one per input fold over that variable, four int64 each:
// (global fold, units K, states C of the fold's table, element offset of its (K, C) block in `ntab` -- or of its K means /
// standard deviations for the Gaussian kernel).
struct LeafEntry {
  int64_t g, K, C, off;
};

// A row has a posterior when its root value is finite and its evidence was in range (bad[n] == 0, ck_flow_check_evidence).
__device__ __forceinline__ bool row_ok(const float* __restrict__ vals, const int64_t* __restrict__ val_off, int root_fold,
                                       int root_ko, const int32_t* __restrict__ bad, int64_t n) {
  const float r = vals[val_off[root_fold] + n * root_ko];
  return r > -INFINITY && r < INFINITY && bad[n] == 0;
}

// logev[n]: the root value of the row, NaN where its evidence was out of range.
__global__ void __launch_bounds__(kThreads)
    flow_logev_kernel(const float* __restrict__ vals, const int64_t* __restrict__ val_off, int root_fold, int root_ko,
                      const int32_t* __restrict__ bad, int64_t B, float* __restrict__ logev) {
  const int64_t n = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (n < B) logev[n] = bad[n] ? NAN : vals[val_off[root_fold] + n * root_ko];
}

// The range check of a chunk of masked evidence ev (B, D), int64 or fp32 (x_float), against states[d], the number of states
// the discrete input layers index variable d with (0: none does).  clean gets the evidence with every out-of-range observed
// category replaced by 0, so that the evidence forward stays finite for the other rows; bad[n] = 1 and *flag |= 1 (flag may be
// NULL) for a row that held one.  Sentinels as the forward reads them: a negative int64; in fp32 NaN or a value <= -1 (a float
// batch is truncated).
__global__ void __launch_bounds__(kThreads)
    flow_check_evidence_kernel(const void* __restrict__ ev, int x_float, const int32_t* __restrict__ states, int64_t B, int D,
                               void* __restrict__ clean, int32_t* __restrict__ bad, int32_t* flag) {
  const int64_t o = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (o >= B * D) return;
  const int S = states[o % D];
  bool out_of_range = false;
  if (x_float) {
    const float e = static_cast<const float*>(ev)[o];
    out_of_range = S > 0 && e > -1.f && e >= static_cast<float>(S);
    static_cast<float*>(clean)[o] = out_of_range ? 0.f : e;
  } else {
    const int64_t c = static_cast<const int64_t*>(ev)[o];
    out_of_range = S > 0 && c >= S;
    static_cast<int64_t*>(clean)[o] = out_of_range ? 0 : c;
  }
  if (out_of_range) {
    bad[o / D] = 1;
    if (flag != nullptr) atomicOr(flag, 1);
  }
}

__global__ void __launch_bounds__(kThreads)
    flow_leaf_cat_generic(const LeafEntry* __restrict__ ent, const int32_t* __restrict__ qstart, int Q, int Cout,
                          const float* __restrict__ ntab, const float* __restrict__ flow, const float* __restrict__ vals,
                          const int64_t* __restrict__ val_off, int root_fold, int root_ko, const int32_t* __restrict__ bad, int64_t B,
                          float* __restrict__ out) {
  const int64_t idx = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (idx >= B * Q * Cout) return;
  const int c = static_cast<int>(idx % Cout);
  const int q = static_cast<int>((idx / Cout) % Q);
  const int64_t n = idx / (static_cast<int64_t>(Cout) * Q);
  float acc = 0.f;
  if (!row_ok(vals, val_off, root_fold, root_ko, bad, n)) {
    acc = NAN;
  } else {
    for (int s = qstart[q]; s < qstart[q + 1]; ++s) {
      const LeafEntry e = ent[s];
      if (c >= e.C) continue;
      const float* fr = flow + val_off[e.g] + n * e.K;
      const float* t = ntab + e.off + c;
      for (int k = 0; k < e.K; ++k) acc = fmaf(fr[k], t[k * e.C], acc);
    }
  }
  out[idx] = acc;
}

// The same on the fp32 matrix cores, every entry with K units: a workgroup owns (q, 32 rows), its waves the 32-state column
// tiles; (32 rows x K) flows x (K x 32) normalised table rows per entry, the unit order of flow_down_sum_mfma.  A wave
// stores, per accumulator register, two rows of 32 consecutive states: whole 128-byte lines.
template <int K>
__global__ void __launch_bounds__(kThreads)
    flow_leaf_cat_mfma(const LeafEntry* __restrict__ ent, const int32_t* __restrict__ qstart, int Q, int Cout,
                       const float* __restrict__ ntab, const float* __restrict__ flow, const float* __restrict__ vals,
                       const int64_t* __restrict__ val_off, int root_fold, int root_ko, const int32_t* __restrict__ bad, int64_t B,
                       int64_t row_tiles, float* __restrict__ out) {
  constexpr int KH = K / 2;
  __shared__ float sok[kWaves][32];
  const int lane = threadIdx.x & (ck::kWave - 1), wave = threadIdx.x / ck::kWave;
  const int b = lane & 31, hi = lane >> 5;
  const int q = static_cast<int>(blockIdx.x / row_tiles);
  const int64_t n0 = (blockIdx.x % row_tiles) * 32;
  const int64_t nb = n0 + b < B ? n0 + b : B - 1;
  if (hi == 0) sok[wave][b] = row_ok(vals, val_off, root_fold, root_ko, bad, nb) ? 0.f : NAN;
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  const int s0 = qstart[q], s1 = qstart[q + 1];
  for (int c0 = wave * 32; c0 < Cout; c0 += kWaves * 32) {
    const int c = c0 + b;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    for (int s = s0; s < s1; ++s) {
      const LeafEntry e = ent[s];
      const int C = static_cast<int>(e.C);
      const float* fr = flow + val_off[e.g] + nb * K + hi * KH;
      const float* t = ntab + e.off + static_cast<int64_t>(hi) * KH * C + (c < C ? c : C - 1);
      const float keep = c < C ? 1.f : 0.f;
#pragma unroll
      for (int kk = 0; kk < KH; ++kk)
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(fr[kk], keep * t[static_cast<int64_t>(kk) * C], acc, 0, 0, 0);
    }
    if (c >= Cout) continue;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = 8 * (r >> 2) + 4 * hi + (r & 3);
      const int64_t n = n0 + row;
      if (n < B) out[(n * Q + q) * Cout + c] = acc[r] + sok[wave][row];
    }
  }
}

// Gaussian query variables: out[n, q] = (S1, S2 - S1^2) with S1 = sum f_k mean_k and S2 = sum f_k (stddev_k^2 + mean_k^2)
// over the units of the variable's input folds: the mean and the variance of the mixture sum_k f_k N(mean_k, stddev_k^2).
__global__ void __launch_bounds__(kThreads)
    flow_leaf_gauss_kernel(const LeafEntry* __restrict__ ent, const int32_t* __restrict__ qstart, int Q,
                           const float* __restrict__ mean, const float* __restrict__ stddev, const float* __restrict__ flow,
                           const float* __restrict__ vals, const int64_t* __restrict__ val_off, int root_fold, int root_ko,
                           const int32_t* __restrict__ bad, int64_t B, float* __restrict__ out) {
  const int64_t idx = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (idx >= B * Q) return;
  const int q = static_cast<int>(idx % Q);
  const int64_t n = idx / Q;
  float s1 = 0.f, s2 = 0.f;
  if (!row_ok(vals, val_off, root_fold, root_ko, bad, n)) {
    s1 = s2 = NAN;
  } else {
    for (int s = qstart[q]; s < qstart[q + 1]; ++s) {
      const LeafEntry e = ent[s];
      const float* fr = flow + val_off[e.g] + n * e.K;
      for (int k = 0; k < e.K; ++k) {
        const float mu = mean[e.off + k], sd = stddev[e.off + k];
        s1 = fmaf(fr[k], mu, s1);
        s2 = fmaf(fr[k], fmaf(sd, sd, mu * mu), s2);
      }
    }
  }
  out[idx * 2] = s1;
  out[idx * 2 + 1] = s2 - s1 * s1;
}

int64_t blocks_of(int64_t items, int threads) { return (items + threads - 1) / threads; }

}  // namespace

int ck_flow_down_sum(int type, int diag, const int32_t* child, const float* w, int64_t F, int H, int Ki, int Ko, int M,
                     const float* vals, const float* flow, const int64_t* val_off, int fold_off, int64_t B, float* msg,
                     void* stream) {
  CK_REQUIRE(type == CK_SAMPLE_SUM || type == CK_SAMPLE_CPT || type == CK_SAMPLE_TUCKER, "ck_flow_down_sum: not a sum-type layer");
  CK_REQUIRE(child != nullptr && w != nullptr && vals != nullptr && flow != nullptr && val_off != nullptr && msg != nullptr,
             "ck_flow_down_sum: null pointer");
  CK_REQUIRE(F > 0 && H > 0 && Ki > 0 && Ko > 0 && M > 0 && B > 0 && fold_off >= 0, "ck_flow_down_sum: non-positive size");
  CK_REQUIRE(M == (type == CK_SAMPLE_SUM ? H * Ki : type == CK_SAMPLE_CPT ? Ki : Ki * Ki) && (type != CK_SAMPLE_TUCKER || H == 2),
             "ck_flow_down_sum: %d entries for type %d, arity %d, %d input units", M, type, H, Ki);
  CK_REQUIRE(!diag || (type == CK_SAMPLE_SUM && Ko == Ki), "ck_flow_down_sum: a mixing layer is a sum layer with Ko = Ki");
  if (!diag && type != CK_SAMPLE_TUCKER && (Ko == 32 || Ko == 64) && Ki % 32 == 0) {
    const int64_t row_tiles = (B + 31) / 32;
    const int64_t blocks = blocks_of(F * row_tiles, kWaves);
    CK_REQUIRE(blocks <= 0x7fffffff, "ck_flow_down_sum: grid too large");
    return ck::dispatch(
        [=](hipStream_t s) {
          if (Ko == 32)
            hipLaunchKernelGGL(flow_down_sum_mfma<32>, dim3(static_cast<unsigned>(blocks)), dim3(kThreads), 0, s, type, child, w,
                               F, H, Ki, M, vals, flow, val_off, fold_off, B, row_tiles, msg);
          else
            hipLaunchKernelGGL(flow_down_sum_mfma<64>, dim3(static_cast<unsigned>(blocks)), dim3(kThreads), 0, s, type, child, w,
                               F, H, Ki, M, vals, flow, val_off, fold_off, B, row_tiles, msg);
          return hipGetLastError();
        },
        stream);
  }
  const int64_t per_row = static_cast<int64_t>(Ko) + 1 + (type == CK_SAMPLE_TUCKER ? M : 0);
  int TR = 16;
  while (TR > 1 && TR * per_row * 4 > kMaxLds) TR /= 2;
  CK_REQUIRE(TR * per_row * 4 <= kMaxLds, "ck_flow_down_sum: %d units and %d entries exceed the LDS budget", Ko, M);
  const int64_t row_tiles = (B + TR - 1) / TR;
  CK_REQUIRE(F * row_tiles <= 0x7fffffff, "ck_flow_down_sum: grid too large");
  const size_t lds = static_cast<size_t>(TR * per_row * 4);
  return ck::dispatch(
      [=](hipStream_t s) {
        hipLaunchKernelGGL(flow_down_sum_generic, dim3(static_cast<unsigned>(F * row_tiles)), dim3(kThreads), lds, s, type, diag,
                           child, w, F, H, Ki, Ko, M, vals, flow, val_off, fold_off, B, TR, row_tiles, msg);
        return hipGetLastError();
      },
      stream);
}

int ck_flow_segment_add(const float* msg, const int32_t* cstart, const int32_t* cfold, const int32_t* cfirst,
                        const int32_t* items, float* flow, const int64_t* val_off, int64_t n_child, int Ki, int64_t B,
                        void* stream) {
  CK_REQUIRE(msg != nullptr && cstart != nullptr && cfold != nullptr && cfirst != nullptr && items != nullptr &&
                 flow != nullptr && val_off != nullptr,
             "ck_flow_segment_add: null pointer");
  CK_REQUIRE(n_child > 0 && Ki > 0 && B > 0, "ck_flow_segment_add: non-positive size");
  const int64_t blocks = blocks_of(n_child * B * Ki, kThreads);
  CK_REQUIRE(blocks <= 0x7fffffff, "ck_flow_segment_add: too many entries");
  return ck::dispatch(
      [=](hipStream_t s) {
        hipLaunchKernelGGL(flow_add_rows_kernel, dim3(static_cast<unsigned>(blocks)), dim3(kThreads), 0, s, msg, 0, cstart, cfold,
                           cfirst, items, flow, val_off, n_child, Ki, B);
        return hipGetLastError();
      },
      stream);
}

int ck_flow_down_product(int type, const int32_t* cstart, const int32_t* cfold, const int32_t* cfirst, const int32_t* items,
                         float* flow, const int64_t* val_off, int64_t n_child, int H, int Ki, int Ko, int64_t B,
                         void* stream) {
  CK_REQUIRE(type == CK_SAMPLE_HADAMARD || type == CK_SAMPLE_KRONECKER, "ck_flow_down_product: not a product layer");
  CK_REQUIRE(cstart != nullptr && cfold != nullptr && cfirst != nullptr && items != nullptr && flow != nullptr &&
                 val_off != nullptr,
             "ck_flow_down_product: null pointer");
  CK_REQUIRE(n_child > 0 && H > 0 && Ki > 0 && Ko > 0 && B > 0, "ck_flow_down_product: non-positive size");
  if (type == CK_SAMPLE_HADAMARD) {
    CK_REQUIRE(Ko == Ki, "ck_flow_down_product: Hadamard with %d inputs, %d outputs", Ki, Ko);
  } else {
    int64_t p = 1;
    for (int h = 0; h < H && p <= Ko; ++h) p *= Ki;
    CK_REQUIRE(p == Ko, "ck_flow_down_product: Kronecker of %d inputs of %d units with %d outputs", H, Ki, Ko);
  }
  const int64_t blocks = blocks_of(n_child * B * Ki, kThreads);
  CK_REQUIRE(blocks <= 0x7fffffff, "ck_flow_down_product: too many entries");
  return ck::dispatch(
      [=](hipStream_t s) {
        if (type == CK_SAMPLE_HADAMARD)
          hipLaunchKernelGGL(flow_add_rows_kernel, dim3(static_cast<unsigned>(blocks)), dim3(kThreads), 0, s, flow, 1, cstart,
                             cfold, cfirst, items, flow, val_off, n_child, Ki, B);
        else
          hipLaunchKernelGGL(flow_kron_kernel, dim3(static_cast<unsigned>(blocks)), dim3(kThreads), 0, s, cstart, cfold, cfirst,
                             items, flow, val_off, n_child, H, Ki, Ko, B);
        return hipGetLastError();
      },
      stream);
}

// The (B,) log evidence behind a leaf launch (logev may be NULL).
static int launch_logev(const float* vals, const int64_t* val_off, int root_fold, int root_ko, const int32_t* bad, int64_t B,
                        float* logev, void* stream) {
  if (logev == nullptr) return 0;
  const int64_t blocks = blocks_of(B, kThreads);
  return ck::dispatch(
      [=](hipStream_t s) {
        hipLaunchKernelGGL(flow_logev_kernel, dim3(static_cast<unsigned>(blocks)), dim3(kThreads), 0, s, vals, val_off, root_fold,
                           root_ko, bad, B, logev);
        return hipGetLastError();
      },
      stream);
}

int ck_flow_check_evidence(const void* ev, int x_float, const int32_t* states, int64_t B, int D, void* clean, int32_t* bad,
                           int32_t* flag, void* stream) {
  CK_REQUIRE(ev != nullptr && states != nullptr && clean != nullptr && bad != nullptr, "ck_flow_check_evidence: null pointer");
  CK_REQUIRE(B > 0 && D > 0, "ck_flow_check_evidence: non-positive size");
  const int64_t blocks = blocks_of(B * D, kThreads);
  CK_REQUIRE(blocks <= 0x7fffffff, "ck_flow_check_evidence: too many entries");
  return ck::dispatch(
      [=](hipStream_t s) {
        hipLaunchKernelGGL(flow_check_evidence_kernel, dim3(static_cast<unsigned>(blocks)), dim3(kThreads), 0, s, ev, x_float,
                           states, B, D, clean, bad, flag);
        return hipGetLastError();
      },
      stream);
}

int ck_flow_leaf_categorical(const int64_t* entries, const int32_t* qstart, int Q, int Cout, int K_uniform, const float* ntab,
                             const float* flow, const float* vals, const int64_t* val_off, int root_fold, int root_ko,
                             const int32_t* bad, int64_t B, float* out, float* logev, void* stream) {
  CK_REQUIRE(entries != nullptr && qstart != nullptr && ntab != nullptr && flow != nullptr && vals != nullptr &&
                 val_off != nullptr && bad != nullptr && out != nullptr,
             "ck_flow_leaf_categorical: null pointer");
  CK_REQUIRE(Q > 0 && Cout > 0 && B > 0 && root_fold >= 0 && root_ko > 0 && K_uniform >= 0,
             "ck_flow_leaf_categorical: non-positive size");
  if (int st = launch_logev(vals, val_off, root_fold, root_ko, bad, B, logev, stream)) return st;
  const LeafEntry* ent = reinterpret_cast<const LeafEntry*>(entries);
  if (K_uniform == 32 || K_uniform == 64) {
    const int64_t row_tiles = (B + 31) / 32;
    CK_REQUIRE(Q * row_tiles <= 0x7fffffff, "ck_flow_leaf_categorical: grid too large");
    const dim3 grid(static_cast<unsigned>(Q * row_tiles));
    return ck::dispatch(
        [=](hipStream_t s) {
          if (K_uniform == 32)
            hipLaunchKernelGGL(flow_leaf_cat_mfma<32>, grid, dim3(kThreads), 0, s, ent, qstart, Q, Cout, ntab, flow, vals, val_off,
                               root_fold, root_ko, bad, B, row_tiles, out);
          else
            hipLaunchKernelGGL(flow_leaf_cat_mfma<64>, grid, dim3(kThreads), 0, s, ent, qstart, Q, Cout, ntab, flow, vals, val_off,
                               root_fold, root_ko, bad, B, row_tiles, out);
          return hipGetLastError();
        },
        stream);
  }
  const int64_t blocks = blocks_of(B * Q * Cout, kThreads);
  CK_REQUIRE(blocks <= 0x7fffffff, "ck_flow_leaf_categorical: too many entries");
  return ck::dispatch(
      [=](hipStream_t s) {
        hipLaunchKernelGGL(flow_leaf_cat_generic, dim3(static_cast<unsigned>(blocks)), dim3(kThreads), 0, s, ent, qstart, Q, Cout,
                           ntab, flow, vals, val_off, root_fold, root_ko, bad, B, out);
        return hipGetLastError();
      },
      stream);
}

int ck_flow_leaf_gaussian(const int64_t* entries, const int32_t* qstart, int Q, const float* mean, const float* stddev,
                          const float* flow, const float* vals, const int64_t* val_off, int root_fold, int root_ko,
                          const int32_t* bad, int64_t B, float* out, float* logev, void* stream) {
  CK_REQUIRE(entries != nullptr && qstart != nullptr && mean != nullptr && stddev != nullptr && flow != nullptr &&
                 vals != nullptr && val_off != nullptr && bad != nullptr && out != nullptr,
             "ck_flow_leaf_gaussian: null pointer");
  CK_REQUIRE(Q > 0 && B > 0 && root_fold >= 0 && root_ko > 0, "ck_flow_leaf_gaussian: non-positive size");
  if (int st = launch_logev(vals, val_off, root_fold, root_ko, bad, B, logev, stream)) return st;
  const int64_t blocks = blocks_of(B * Q, kThreads);
  CK_REQUIRE(blocks <= 0x7fffffff, "ck_flow_leaf_gaussian: too many entries");
  return ck::dispatch(
      [=](hipStream_t s) {
        hipLaunchKernelGGL(flow_leaf_gauss_kernel, dim3(static_cast<unsigned>(blocks)), dim3(kThreads), 0, s,
                           reinterpret_cast<const LeafEntry*>(entries), qstart, Q, mean, stddev, flow, vals, val_off, root_fold,
                           root_ko, bad, B, out);
        return hipGetLastError();
      },
      stream);
}
