// Expected statistics ("Expected statistics"): the flow pass of ck_flow.hip reduced OVER THE BATCH,
// behind `HipCircuit.expected_statistics`.  With v the per-row log values of the evidence forward, f the flows and e_i the
// child value of entry i, a sum-type fold accumulates N[k, i] = sum_n f_k(n) w[k, i] exp(e_i(n) - v_k(n)) over the LIVE rows
// (live[n] != 0: evidence in range, finite root value); input folds accumulate their flows by observed state or moment, every
// fold its flows by unit.  No float atomics: every sum has a fixed order, so results are bit-identical from call to call.
//
// Every term is factored as a[n, k] w[k, i] g[n, i] with a per-row shift m (flow_down_sum's: the maximum of log f_k - v_k
// over the units of the row that carry flow): a = f_k exp(-v_k - m) <= 1, g = exp(e_i + m).  Nothing is exponentiated
// unshifted.  A row with an entry whose e_i + m reaches kSlowShift (only possible where the weights of the row's heaviest
// unit on that entry are <= e^-40, or zero) leaves the factored product: its terms are f_k exp(e_i - v_k) in fp64, no shift.
#include <math.h>

#include "ck_down.h"

namespace {

using ck::blocks_of;
using ck::f32x16;
using ck::kMaxLds;
using ck::kThreads;
using ck::kWaves;
constexpr int kTile = 1024;           // accumulators of one (MFMA tile | generic pair chunk)
constexpr int kPairs = kTile / kThreads;
constexpr float kSlowShift = 40.f;    // g <= e^40, so a >= e^-87 (the smallest normal fp32) loses nothing above e^-47
constexpr int64_t kTargetWaves = 1024;  // rows are split into slices until a launch has about this many waves
constexpr int64_t kMinSliceRows = 64;

// The shift and the factor a are the flow pass's (ck_down.h: flow_lg, flow_a); callers keep the exponent below kSlowShift, so
// the two-sum exponential is taken without its overflow branch (scaled_exp_core).
// One term without its weight, unfactored: f exp(e - v) in fp64 (the rows that left the factored product).
__device__ __forceinline__ float stats_term(float f, float v, float e) {
  if (!(f > 0.f && v > -INFINITY && v < INFINITY) || e == -INFINITY) return 0.f;
  return static_cast<float>(static_cast<double>(f) * exp(static_cast<double>(e) - static_cast<double>(v)));
}
// max over the 32 lanes of a wave half (the two halves hold two batch rows): wave_reduce without its last step
__device__ __forceinline__ float half_max(float v) {
  v = fmaxf(v, __uint_as_float(__builtin_amdgcn_mov_dpp(__float_as_uint(v), 0xB1, 0xF, 0xF, true)));
  v = fmaxf(v, __uint_as_float(__builtin_amdgcn_mov_dpp(__float_as_uint(v), 0x4E, 0xF, 0xF, true)));
  v = fmaxf(v, __uint_as_float(__builtin_amdgcn_mov_dpp(__float_as_uint(v), 0x141, 0xF, 0xF, true)));
  v = fmaxf(v, __uint_as_float(__builtin_amdgcn_mov_dpp(__float_as_uint(v), 0x140, 0xF, 0xF, true)));
  const auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  return fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1]));
}

// ---- the contraction on the fp32 matrix cores: sum and CP-T layers of KO = 32 / 64 units, M a multiple of 32 ---------
// One wave owns (fold, 32-unit block, 32-entry tile, row slice) and walks its rows two at a time:
// acc (32 units x 32 entries) += A (32 units x 2 rows) B (2 rows x 32 entries) on v_mfma_f32_32x32x2_f32.  Lane (b = lane & 31,
// hi = lane >> 5) holds a[row n0 + hi][unit k0 + b] and g[row n0 + hi][entry i0 + b]; the shift of a row is taken over the
// 32 units of the wave's own block.  S == 1: the wave adds w acc to edge itself; otherwise it stores its partial tile.
template <int KO>
__global__ void __launch_bounds__(kThreads)
    stats_edge_mfma(int type, const int32_t* __restrict__ child, const float* __restrict__ w, int64_t F, int H, int Ki, int M,
                    const float* __restrict__ vals, const float* __restrict__ flow, const int64_t* __restrict__ val_off,
                    int fold_off, const int32_t* __restrict__ live, int64_t B, int S, int64_t slice_rows,
                    float* __restrict__ edge, float* __restrict__ scratch) {
  constexpr int KB = KO / 32;
  const int MT = M / 32;
  const int lane = threadIdx.x & (ck::kWave - 1), wave = threadIdx.x / ck::kWave;
  const int b = lane & 31, hi = lane >> 5;
  const int64_t job = static_cast<int64_t>(blockIdx.x) * kWaves + wave;
  if (job >= F * KB * MT * S) return;
  const int slice = static_cast<int>(job % S);
  const int64_t tile = job / S;
  const int it = static_cast<int>(tile % MT), kb = static_cast<int>((tile / MT) % KB);
  const int64_t f = tile / (static_cast<int64_t>(MT) * KB);
  const int64_t n_begin = slice * slice_rows;
  const int64_t n_end = n_begin + slice_rows < B ? n_begin + slice_rows : B;
  const int64_t blk = val_off[fold_off + f];
  const int32_t* ch = child + f * H;
  const int k0 = kb * 32, i = it * 32 + b;
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  for (int64_t n0 = n_begin; n0 < n_end; n0 += 2) {
    const int64_t n = n0 + hi;
    const bool ok = n < n_end && live[n < n_end ? n : n0] != 0;
    const int64_t nn = n < n_end ? n : n0;  // (a row the loads may touch)
    const float fk = flow[blk + nn * KO + k0 + b], vk = vals[blk + nn * KO + k0 + b];
    const float m = half_max(ok ? ck::flow_lg(fk, vk) : -INFINITY);
    float a = 0.f, g = 0.f;
    bool slow = false;
    if (m > -INFINITY) {  // (uniform over the half: some unit of the row carries flow)
      const float e = ck::entry_value(type, ch, H, Ki, vals, val_off, nn, i);
      slow = e > -INFINITY && e + m >= kSlowShift;
      a = ck::flow_a<false>(fk, vk, m);
      g = (e > -INFINITY && !slow) ? ck::scaled_exp_core(1.f, e, m) : 0.f;
    }
    const uint64_t sl = __ballot(slow);
    if (__builtin_expect(sl != 0, 0)) {
      if ((hi ? sl >> 32 : sl & 0xffffffffu) != 0) a = 0.f;  // the whole row leaves the product
      for (int h = 0; h < 2; ++h) {
        if (((h ? sl >> 32 : sl & 0xffffffffu)) == 0) continue;
        const int64_t ns = n0 + h;
        const float e = ck::entry_value(type, ch, H, Ki, vals, val_off, ns, i);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int k = k0 + 8 * (r >> 2) + 4 * hi + (r & 3);
          acc[r] += stats_term(flow[blk + ns * KO + k], vals[blk + ns * KO + k], e);
        }
      }
    }
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, g, acc, 0, 0, 0);
  }
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int row = 8 * (r >> 2) + 4 * hi + (r & 3);
    if (S == 1) {
      const int64_t at = (f * KO + k0 + row) * M + i;
      const float wv = w[at];
      edge[at] += wv > 0.f ? wv * acc[r] : 0.f;
    } else {
      scratch[(tile * S + slice) * kTile + row * 32 + b] = acc[r];
    }
  }
}

// ---- the contraction, plain VALU path: any layer type, any unit counts ---------------------------------------------
// A workgroup owns (fold, chunk of kTile (unit, entry) pairs, row slice); a thread kPairs pairs p = chunk kTile + j kThreads
// + thread, unit p / M, entry p % M.  Rows are staged TR at a time: LDS sa[TR][Ko] = a, sg[TR][M] = g, ss[TR] whether the
// row left the factored product.
__global__ void __launch_bounds__(kThreads)
    stats_edge_generic(int type, int diag, const int32_t* __restrict__ child, const float* __restrict__ w, int64_t F, int H, int Ki,
                       int Ko, int M, const float* __restrict__ vals, const float* __restrict__ flow,
                       const int64_t* __restrict__ val_off, int fold_off, const int32_t* __restrict__ live, int64_t B, int S,
                       int64_t slice_rows, int TR, int PC, float* __restrict__ edge, float* __restrict__ scratch) {
  extern __shared__ float sh[];
  float* const sa = sh;
  float* const sg = sa + TR * Ko;
  int* const ss = reinterpret_cast<int*>(sg + TR * M);
  const int lane = threadIdx.x & (ck::kWave - 1), wave = threadIdx.x / ck::kWave;
  const int slice = static_cast<int>(blockIdx.x % S);
  const int64_t tile = blockIdx.x / S;
  const int pc = static_cast<int>(tile % PC);
  const int64_t f = tile / PC;
  const int64_t n_begin = slice * slice_rows;
  const int64_t n_end = n_begin + slice_rows < B ? n_begin + slice_rows : B;
  const int64_t blk = val_off[fold_off + f];
  const int32_t* ch = child + f * H;
  const int64_t pairs = static_cast<int64_t>(Ko) * M;
  float acc[kPairs];
  int pk[kPairs], pi[kPairs];
#pragma unroll
  for (int j = 0; j < kPairs; ++j) {
    const int64_t p = static_cast<int64_t>(pc) * kTile + j * kThreads + threadIdx.x;
    acc[j] = 0.f;
    pk[j] = p < pairs ? static_cast<int>(p / M) : -1;
    pi[j] = p < pairs ? static_cast<int>(p % M) : 0;
    if (diag && pk[j] >= 0 && pi[j] % Ki != pk[j]) pk[j] = -1;  // mixing: entry i only meets unit i % Ki
  }
  for (int64_t n0 = n_begin; n0 < n_end; n0 += TR) {
    for (int r = wave; r < TR; r += kWaves) {
      const int64_t n = n0 + r;
      const bool ok = n < n_end && live[n] != 0;
      float mx = -INFINITY;
      if (ok)
        for (int k = lane; k < Ko; k += ck::kWave) mx = fmaxf(mx, ck::flow_lg(flow[blk + n * Ko + k], vals[blk + n * Ko + k]));
      const float m = ck::wave_max(mx);
      bool slow = false;
      for (int i = lane; i < M; i += ck::kWave) {
        float g = 0.f;
        if (m > -INFINITY) {
          const float e = ck::entry_value(type, ch, H, Ki, vals, val_off, n, i);
          if (e > -INFINITY) {
            if (e + m >= kSlowShift) slow = true;
            else g = ck::scaled_exp_core(1.f, e, m);
          }
        }
        sg[r * M + i] = g;
      }
      const bool any_slow = __ballot(slow) != 0;
      for (int k = lane; k < Ko; k += ck::kWave)
        sa[r * Ko + k] = (m > -INFINITY && !any_slow) ? ck::flow_a<false>(flow[blk + n * Ko + k], vals[blk + n * Ko + k], m) : 0.f;
      if (lane == 0) ss[r] = any_slow ? 1 : 0;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < kPairs; ++j) {
      if (pk[j] < 0) continue;
      float s = acc[j];
      for (int r = 0; r < TR; ++r) {
        s = fmaf(sa[r * Ko + pk[j]], sg[r * M + pi[j]], s);
        if (__builtin_expect(ss[r] != 0, 0)) {
          const int64_t n = n0 + r;
          s += stats_term(flow[blk + n * Ko + pk[j]], vals[blk + n * Ko + pk[j]],
                          ck::entry_value(type, ch, H, Ki, vals, val_off, n, pi[j]));
        }
      }
      acc[j] = s;
    }
    __syncthreads();
  }
#pragma unroll
  for (int j = 0; j < kPairs; ++j) {
    const int64_t p = static_cast<int64_t>(pc) * kTile + j * kThreads + threadIdx.x;
    if (S == 1) {
      if (p >= pairs) continue;
      const float wv = w[f * pairs + p];
      edge[f * pairs + p] += wv > 0.f ? wv * acc[j] : 0.f;
    } else {
      scratch[(tile * S + slice) * kTile + j * kThreads + threadIdx.x] = acc[j];
    }
  }
}

// The partial tiles of the row slices, added in slice order, times the weight, onto edge.  mfma != 0: tile = (fold, unit
// block, entry tile) of 32 x 32; otherwise tile = (fold, pair chunk) of kTile consecutive pairs.
__global__ void __launch_bounds__(kThreads)
    stats_edge_reduce(int mfma, const float* __restrict__ w, int Ko, int M, int PC, int S, int64_t tiles,
                      const float* __restrict__ scratch, float* __restrict__ edge) {
  const int64_t idx = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (idx >= tiles * kTile) return;
  const int64_t tile = idx / kTile;
  const int el = static_cast<int>(idx % kTile);
  int64_t at;
  if (mfma) {
    const int MT = M / 32, KB = Ko / 32;
    const int it = static_cast<int>(tile % MT), kb = static_cast<int>((tile / MT) % KB);
    const int64_t f = tile / (static_cast<int64_t>(MT) * KB);
    at = (f * Ko + kb * 32 + el / 32) * M + it * 32 + el % 32;
  } else {
    const int64_t pairs = static_cast<int64_t>(Ko) * M;
    const int64_t p = (tile % PC) * kTile + el;
    if (p >= pairs) return;
    at = (tile / PC) * pairs + p;
  }
  float s = 0.f;
  for (int sl = 0; sl < S; ++sl) s += scratch[(tile * S + sl) * kTile + el];
  const float wv = w[at];
  edge[at] += wv > 0.f ? wv * s : 0.f;
}

// ---- input layers --------------------------------------------------------------------------------------------------
// Categorical / Binomial: a workgroup owns (fold, block of KU units) and keeps their (KU, C) histogram in LDS.  Thread
// (unit u = thread % KU, group g = thread / KU) walks ALL rows in order and adds f_u to the state the row observes if that
// state is in the group's range of CG states: no two threads share a cell, the order is the row order.  Group 0 also sums the
// flows of the rows that miss the variable; the epilogue adds hist + missing nt.
__global__ void __launch_bounds__(kThreads)
    stats_leaf_cat_kernel(const int64_t* __restrict__ scope, const float* __restrict__ ntab, int K, int C, int KU, int CG,
                          const void* __restrict__ ev, int x_float, int D, const float* __restrict__ flow,
                          const int64_t* __restrict__ val_off, int fold_off, const int32_t* __restrict__ live, int64_t B,
                          float* __restrict__ leaf) {
  extern __shared__ float sh[];
  float* const hist = sh;            // [KU][C]
  float* const miss = sh + KU * C;   // [KU]
  const int kblocks = (K + KU - 1) / KU;
  const int64_t f = blockIdx.x / kblocks;
  const int ku0 = static_cast<int>(blockIdx.x % kblocks) * KU;
  const int nu = K - ku0 < KU ? K - ku0 : KU;
  for (int t = threadIdx.x; t < KU * C + KU; t += kThreads) sh[t] = 0.f;
  __syncthreads();
  const int u = threadIdx.x % KU, g = threadIdx.x / KU;
  const int groups = kThreads / KU;
  const int64_t var = scope[f];
  const float* fr = flow + val_off[fold_off + f] + ku0 + u;
  if (g < groups && u < nu) {
    const int c_lo = g * CG, c_hi = c_lo + CG;
    float mine = 0.f;
    for (int64_t n = 0; n < B; ++n) {
      if (live[n] == 0) continue;
      float e = 0.f;
      int64_t c = 0;
      const bool obs = ck::observed(ev, n * D + var, x_float, false, e, c);
      if (obs) {
        if (x_float) c = static_cast<int64_t>(e);
        if (c >= c_lo && c < c_hi && c < C) hist[u * C + c] += fr[n * K];
      } else if (g == 0) {
        mine += fr[n * K];
      }
    }
    if (g == 0) miss[u] = mine;
  }
  __syncthreads();
  for (int t = threadIdx.x; t < nu * C; t += kThreads) {
    const int64_t at = (f * K + ku0) * C + t;
    leaf[at] += hist[t] + miss[t / C] * ntab[at];
  }
}

// Gaussian: one thread per (fold, unit) walks the rows in order: sum f, sum f m1, sum f m2 with (m1, m2) = (x, x^2) where the
// variable is observed, (mean, stddev^2 + mean^2) where it is missing (NaN).
__global__ void __launch_bounds__(kThreads)
    stats_leaf_gauss_kernel(const int64_t* __restrict__ scope, const float* __restrict__ mean, const float* __restrict__ stddev,
                            int64_t F, int K, const float* __restrict__ ev, int D, const float* __restrict__ flow,
                            const int64_t* __restrict__ val_off, int fold_off, const int32_t* __restrict__ live, int64_t B,
                            float* __restrict__ leaf) {
  const int64_t idx = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (idx >= F * K) return;
  const int64_t f = idx / K;
  const int k = static_cast<int>(idx % K);
  const int64_t var = scope[f];
  const float mu = mean[idx], sd = stddev[idx];
  const float mm2 = fmaf(sd, sd, mu * mu);
  const float* fr = flow + val_off[fold_off + f] + k;
  float s0 = 0.f, s1 = 0.f, s2 = 0.f;
  for (int64_t n = 0; n < B; ++n) {
    if (live[n] == 0) continue;
    const float fl = fr[n * K];
    const float x = ev[n * D + var];
    const bool obs = !isnan(x);
    s0 += fl;
    s1 = fmaf(fl, obs ? x : mu, s1);
    s2 = fmaf(fl, obs ? x * x : mm2, s2);
  }
  leaf[idx * 3] += s0;
  leaf[idx * 3 + 1] += s1;
  leaf[idx * 3 + 2] += s2;
}

// ---- flows by unit ---------------------------------------------------------------------------------------------------
// A workgroup owns one global fold g of Ko = fold_ko[g] units.  Ko <= kThreads: the first T = Ko (kThreads / Ko) threads walk
// the fold's (B, Ko) block T elements at a time (thread t stays on unit t % Ko), then unit k adds the T / Ko partial sums in
// thread order.  Wider folds: thread t sums unit k0 + t over all rows, k0 in steps of kThreads.
__global__ void __launch_bounds__(kThreads)
    stats_unit_kernel(const float* __restrict__ flow, const int64_t* __restrict__ val_off, const int32_t* __restrict__ fold_ko,
                      const int64_t* __restrict__ unit_off, const int32_t* __restrict__ live, int64_t B,
                      float* __restrict__ unit) {
  __shared__ float part[kThreads];
  const int64_t g = blockIdx.x;
  const int Ko = fold_ko[g];
  const float* fr = flow + val_off[g];
  float* out = unit + unit_off[g];
  if (Ko > kThreads) {
    for (int k = threadIdx.x; k < Ko; k += kThreads) {
      float s = 0.f;
      for (int64_t n = 0; n < B; ++n)
        if (live[n] != 0) s += fr[n * Ko + k];
      out[k] += s;
    }
    return;
  }
  const int R = kThreads / Ko, T = R * Ko;
  float s = 0.f;
  if (threadIdx.x < T) {
    const int k = threadIdx.x % Ko;
    for (int64_t n = threadIdx.x / Ko; n < B; n += R)
      if (live[n] != 0) s += fr[n * Ko + k];
  }
  part[threadIdx.x] = s;
  __syncthreads();
  if (threadIdx.x < Ko) {
    float t = 0.f;
    for (int r = 0; r < R; ++r) t += part[r * Ko + threadIdx.x];
    out[threadIdx.x] += t;
  }
}

// The number of row slices of a launch of `tiles` tiles over B rows: a function of (tiles, B) alone.
int slices_of(int64_t tiles, int64_t B) {
  if (tiles >= kTargetWaves) return 1;
  int64_t s = (kTargetWaves + tiles - 1) / tiles;
  const int64_t cap = (B + kMinSliceRows - 1) / kMinSliceRows;
  if (s > cap) s = cap;
  return static_cast<int>(s < 1 ? 1 : s);
}

}  // namespace

int ck_stats_edge_sum(int type, int diag, const int32_t* child, const float* w, int64_t F, int H, int Ki, int Ko, int M,
                      const float* vals, const float* flow, const int64_t* val_off, int fold_off, const int32_t* live,
                      int64_t B, float* edge, float* scratch, int64_t scratch_floats, void* stream) {
  CK_REQUIRE(type == CK_SAMPLE_SUM || type == CK_SAMPLE_CPT || type == CK_SAMPLE_TUCKER, "ck_stats_edge_sum: not a sum-type layer");
  CK_REQUIRE(child != nullptr && w != nullptr && vals != nullptr && flow != nullptr && val_off != nullptr && live != nullptr &&
                 edge != nullptr,
             "ck_stats_edge_sum: null pointer");
  CK_REQUIRE(F > 0 && H > 0 && Ki > 0 && Ko > 0 && M > 0 && B > 0 && fold_off >= 0 && scratch_floats >= 0,
             "ck_stats_edge_sum: non-positive size");
  CK_REQUIRE(M == (type == CK_SAMPLE_SUM ? H * Ki : type == CK_SAMPLE_CPT ? Ki : Ki * Ki) && (type != CK_SAMPLE_TUCKER || H == 2),
             "ck_stats_edge_sum: %d entries for type %d, arity %d, %d input units", M, type, H, Ki);
  CK_REQUIRE(!diag || (type == CK_SAMPLE_SUM && Ko == Ki), "ck_stats_edge_sum: a mixing layer is a sum layer with Ko = Ki");
  const bool mfma = !diag && type != CK_SAMPLE_TUCKER && (Ko == 32 || Ko == 64) && Ki % 32 == 0;
  const int PC = static_cast<int>(blocks_of(static_cast<int64_t>(Ko) * M, kTile));
  const int64_t tiles = mfma ? F * (Ko / 32) * (M / 32) : F * PC;
  const int S = slices_of(tiles, B);
  int64_t slice_rows = (B + S - 1) / S;
  slice_rows += slice_rows & 1;  // (whole row pairs)
  CK_REQUIRE(S == 1 || (scratch != nullptr && scratch_floats >= tiles * S * kTile),
             "ck_stats_edge_sum: %lld tiles in %d row slices need %lld floats of scratch, %lld given", static_cast<long long>(tiles),
             S, static_cast<long long>(tiles * S * kTile), static_cast<long long>(scratch_floats));
  const int64_t jobs = tiles * S;
  const int64_t rblocks = blocks_of(tiles * kTile, kThreads);
  CK_REQUIRE(jobs <= 0x7fffffff && rblocks <= 0x7fffffff, "ck_stats_edge_sum: grid too large");
  int TR = 0;
  size_t lds = 0;
  if (!mfma) {
    const int64_t per_row = (static_cast<int64_t>(Ko) + M + 1) * 4;
    TR = 16;
    while (TR > 1 && TR * per_row > kMaxLds) TR /= 2;
    CK_REQUIRE(TR * per_row <= kMaxLds, "ck_stats_edge_sum: %d units and %d entries exceed the LDS budget", Ko, M);
    lds = static_cast<size_t>(TR * per_row);
  }
  return ck::dispatch(
      [=](hipStream_t s) {
        if (mfma) {
          const dim3 grid(static_cast<unsigned>(blocks_of(jobs, kWaves)));
          if (Ko == 32)
            hipLaunchKernelGGL(stats_edge_mfma<32>, grid, dim3(kThreads), 0, s, type, child, w, F, H, Ki, M, vals, flow, val_off,
                               fold_off, live, B, S, slice_rows, edge, scratch);
          else
            hipLaunchKernelGGL(stats_edge_mfma<64>, grid, dim3(kThreads), 0, s, type, child, w, F, H, Ki, M, vals, flow, val_off,
                               fold_off, live, B, S, slice_rows, edge, scratch);
        } else {
          hipLaunchKernelGGL(stats_edge_generic, dim3(static_cast<unsigned>(jobs)), dim3(kThreads), lds, s, type, diag, child, w, F,
                             H, Ki, Ko, M, vals, flow, val_off, fold_off, live, B, S, slice_rows, TR, PC, edge, scratch);
        }
        if (S > 1)
          hipLaunchKernelGGL(stats_edge_reduce, dim3(static_cast<unsigned>(rblocks)), dim3(kThreads), 0, s, mfma ? 1 : 0, w, Ko, M,
                             PC, S, tiles, scratch, edge);
        return hipGetLastError();
      },
      stream);
}

int ck_stats_leaf_categorical(const int64_t* scope, const float* ntab, int64_t F, int K, int C, const void* ev, int x_float,
                              int D, const float* flow, const int64_t* val_off, int fold_off, const int32_t* live, int64_t B,
                              float* leaf, void* stream) {
  CK_REQUIRE(scope != nullptr && ntab != nullptr && ev != nullptr && flow != nullptr && val_off != nullptr && live != nullptr &&
                 leaf != nullptr,
             "ck_stats_leaf_categorical: null pointer");
  CK_REQUIRE(F > 0 && K > 0 && C > 0 && D > 0 && B > 0 && fold_off >= 0, "ck_stats_leaf_categorical: non-positive size");
  int KU = K < kThreads ? K : kThreads;
  while (KU > 1 && static_cast<int64_t>(KU) * (C + 1) * 4 > kMaxLds) KU = (KU + 1) / 2;
  CK_REQUIRE(static_cast<int64_t>(KU) * (C + 1) * 4 <= kMaxLds, "ck_stats_leaf_categorical: %d states exceed the LDS budget", C);
  const int groups = kThreads / KU;
  const int CG = (C + groups - 1) / groups;
  const int64_t blocks = F * ((K + KU - 1) / KU);
  CK_REQUIRE(blocks <= 0x7fffffff, "ck_stats_leaf_categorical: grid too large");
  const size_t lds = static_cast<size_t>(KU) * (C + 1) * 4;
  return ck::launch(stats_leaf_cat_kernel, dim3(static_cast<unsigned>(blocks)), dim3(kThreads), lds, stream, scope, ntab, K, C,
                    KU, CG, ev, x_float, D, flow, val_off, fold_off, live, B, leaf);
}

int ck_stats_leaf_gaussian(const int64_t* scope, const float* mean, const float* stddev, int64_t F, int K, const float* ev, int D,
                           const float* flow, const int64_t* val_off, int fold_off, const int32_t* live, int64_t B, float* leaf,
                           void* stream) {
  CK_REQUIRE(scope != nullptr && mean != nullptr && stddev != nullptr && ev != nullptr && flow != nullptr && val_off != nullptr &&
                 live != nullptr && leaf != nullptr,
             "ck_stats_leaf_gaussian: null pointer");
  CK_REQUIRE(F > 0 && K > 0 && D > 0 && B > 0 && fold_off >= 0, "ck_stats_leaf_gaussian: non-positive size");
  const int64_t blocks = blocks_of(F * K, kThreads);
  CK_REQUIRE(blocks <= 0x7fffffff, "ck_stats_leaf_gaussian: grid too large");
  return ck::launch(stats_leaf_gauss_kernel, dim3(static_cast<unsigned>(blocks)), dim3(kThreads), 0, stream, scope, mean, stddev,
                    F, K, ev, D, flow, val_off, fold_off, live, B, leaf);
}

int ck_stats_unit_sum(const float* flow, const int64_t* val_off, const int32_t* fold_ko, const int64_t* unit_off,
                      int64_t total_folds, const int32_t* live, int64_t B, float* unit, void* stream) {
  CK_REQUIRE(flow != nullptr && val_off != nullptr && fold_ko != nullptr && unit_off != nullptr && live != nullptr &&
                 unit != nullptr,
             "ck_stats_unit_sum: null pointer");
  CK_REQUIRE(total_folds > 0 && B > 0, "ck_stats_unit_sum: non-positive size");
  CK_REQUIRE(total_folds <= 0x7fffffff, "ck_stats_unit_sum: grid too large");
  return ck::launch(stats_unit_kernel, dim3(static_cast<unsigned>(total_folds)), dim3(kThreads), 0, stream, flow, val_off,
                    fold_ko, unit_off, live, B, unit);
}
