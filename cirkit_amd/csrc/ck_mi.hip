// Pairwise mutual information of categorical columns for Chow-Liu structure learning ("Structure
// learning").  The joint counts of every pair of columns,
//
//   counts[i, j, a, b] = #{n : x[n, i] = a, x[n, j] = b},
//
// are the Gram matrix of the one-hot encoding of the data: a product of 0/1 matrices, exact on the bf16 matrix pipe with fp32
// accumulation as long as a count stays below 2^24.  The reference (templates/region_graph/algorithms/chow_liu.py:107-151)
// materialises them as a (D, D, C^2) int64 tensor; here a 32 x 32 tile of the Gram matrix lives in the accumulators of one
// wave and is reduced to its mutual-information terms in fp64 before anything is written, so nothing of size (D C)^2 exists.
//
// Index space: (variable, state) -> variable * Cp + state, Cp = C padded to a power of two (C <= 32) or to a multiple of 32.
//   Cp <= 32: a wave takes one 64 x 64 block (2 x 2 tiles) of the upper triangle; a tile holds (32 / Cp)^2 whole pairs.
//   Cp >  32: a wave takes one pair i <= j and walks its (Cp / 32)^2 tiles in 64 x 64 blocks, in a fixed order.
// The one-hot fragments are built in registers from the staged codes (one variable's codes contiguous along n, uint8): lane
// (r, h) compares the 8 codes n0 + 8h .. n0 + 8h + 7 of its variable with its state -- the A operand for the tile's rows, the
// B operand for its columns, both in the same k order.  A fragment serves the two MFMAs of its block row / column.
// Rows n >= N of the staged copy are zero (a valid code: 256 states leave no spare byte value), so the A fragment of the last,
// ragged k step is masked instead.
#include <algorithm>
#include <cmath>

#include "ck_internal.h"

namespace {

typedef __bf16 mi_bf16x8 __attribute__((ext_vector_type(8)));
typedef uint32_t mi_u32x4 __attribute__((ext_vector_type(4)));
typedef float mi_f32x16 __attribute__((ext_vector_type(16)));

constexpr int kStageTile = 64;
constexpr int kMaxStates = 256;
constexpr int64_t kMaxRows = int64_t(1) << 24;  // fp32 accumulators count exactly up to here

// (N, D) row-major integers -> codes (D, ldn) uint8, x / div; an entry outside [0, c_in) raises *bad and is staged as 0
template <class T>
__global__ void __launch_bounds__(256)
    mi_stage_kernel(const T* __restrict__ x, int64_t N, int D, int64_t c_in, int div, uint8_t* __restrict__ codes, int64_t ldn,
                    int32_t* __restrict__ bad) {
  __shared__ uint8_t tile[kStageTile][kStageTile + 1];  // [variable][row]
  const int64_t n0 = static_cast<int64_t>(blockIdx.x) * kStageTile;
  const int d0 = blockIdx.y * kStageTile;
  const int lo = threadIdx.x & 63, hi = threadIdx.x >> 6;
#pragma unroll 4
  for (int k = 0; k < kStageTile / 4; ++k) {
    const int64_t n = n0 + hi + 4 * k;
    const int d = d0 + lo;
    uint8_t code = 0;
    if (n < N && d < D) {
      const int64_t v = static_cast<int64_t>(x[n * D + d]);
      const bool ok = v >= 0 && v < c_in;
      if (!ok) *bad = 1;
      code = ok ? static_cast<uint8_t>(v / div) : 0;
    }
    tile[lo][hi + 4 * k] = code;
  }
  __syncthreads();
#pragma unroll 4
  for (int k = 0; k < kStageTile / 4; ++k) {
    const int d = d0 + hi + 4 * k;
    const int64_t n = n0 + lo;
    if (n < N && d < D) codes[static_cast<int64_t>(d) * ldn + n] = tile[hi + 4 * k][lo];
  }
}

// one block per variable: histogram of its codes, and log of the reference's smoothed marginal
__global__ void __launch_bounds__(256)
    mi_marginal_kernel(const uint8_t* __restrict__ codes, int N, int64_t ldn, int C, double alpha, int64_t* __restrict__ hist,
                       double* __restrict__ logm) {
  __shared__ int h[kMaxStates];
  h[threadIdx.x] = 0;
  __syncthreads();
  const uint8_t* col = codes + static_cast<int64_t>(blockIdx.x) * ldn;
  for (int n = threadIdx.x; n < N; n += 256) atomicAdd(&h[col[n]], 1);
  __syncthreads();
  if (static_cast<int>(threadIdx.x) < C) {
    const int64_t o = static_cast<int64_t>(blockIdx.x) * C + threadIdx.x;
    const double c = static_cast<double>(C);
    if (hist != nullptr) hist[o] = h[threadIdx.x];
    logm[o] = log((static_cast<double>(h[threadIdx.x]) + c * alpha) / (static_cast<double>(N) + c * c * alpha));
  }
}

// 8 codes (one per byte of w, the lowest byte first) against `state`: 8 bf16 of 1.0 / 0.0, element 2d in the low half of dword d
__device__ __forceinline__ mi_u32x4 one_hot(uint64_t w, uint32_t state) {
  mi_u32x4 f;
#pragma unroll
  for (int d = 0; d < 4; ++d) {
    const uint32_t b0 = static_cast<uint32_t>(w >> (16 * d)) & 0xffu;
    const uint32_t b1 = static_cast<uint32_t>(w >> (16 * d + 8)) & 0xffu;
    f[d] = (b0 == state ? 0x3f80u : 0u) | (b1 == state ? 0x3f800000u : 0u);
  }
  return f;
}

struct PairsArgs {
  const uint8_t* codes;
  const double* logm;
  double* mi;
  int64_t* counts;
  int64_t ldn;
  double alpha;
  int N, D, C, Cp;
};

// The 64 x 64 block of the Gram matrix at (row0, col0) of the (variable, state) index space: acc[s][t] is its tile (s, t).
__device__ __forceinline__ void gram_block(const PairsArgs& p, int64_t row0, int64_t col0, int lane, mi_f32x16 (&acc)[2][2]) {
  const int r = lane & 31, h = lane >> 5;
  const uint8_t* pa[2];
  const uint8_t* pb[2];
  uint32_t sa[2], sb[2];
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    const int64_t ia = row0 + 32 * s + r, ib = col0 + 32 * s + r;
    // a variable >= D (the ragged end of the index space) reads the last real one; the epilogue masks its cells
    const int64_t va = std::min<int64_t>(ia / p.Cp, p.D - 1), vb = std::min<int64_t>(ib / p.Cp, p.D - 1);
    sa[s] = static_cast<uint32_t>(ia % p.Cp);
    sb[s] = static_cast<uint32_t>(ib % p.Cp);
    pa[s] = p.codes + va * p.ldn + 8 * h;
    pb[s] = p.codes + vb * p.ldn + 8 * h;
  }
#pragma unroll
  for (int s = 0; s < 2; ++s)
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int k = 0; k < 16; ++k) acc[s][t][k] = 0.f;

  auto step = [&](int n0, const mi_u32x4& keep) {
    mi_u32x4 fa[2], fb[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      fa[s] = one_hot(*reinterpret_cast<const uint64_t*>(pa[s] + n0), sa[s]) & keep;
      fb[s] = one_hot(*reinterpret_cast<const uint64_t*>(pb[s] + n0), sb[s]);
    }
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int t = 0; t < 2; ++t)
        acc[s][t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(mi_bf16x8, fa[s]), __builtin_bit_cast(mi_bf16x8, fb[t]),
                                                            acc[s][t], 0, 0, 0);
  };
  const int full = p.N / 16;
  const mi_u32x4 all = {~0u, ~0u, ~0u, ~0u};
  for (int k = 0; k < full; ++k) step(16 * k, all);
  if (p.N % 16 != 0) {  // rows n >= N contribute nothing: their elements of A are cleared (ldn covers the whole step)
    const int live = p.N - 16 * full - 8 * h;  // of this lane's 8 rows
    mi_u32x4 keep;
#pragma unroll
    for (int d = 0; d < 4; ++d) keep[d] = (2 * d < live ? 0xffffu : 0u) | (2 * d + 1 < live ? 0xffff0000u : 0u);
    step(16 * full, keep);
  }
}

// The epilogue of one 32 x 32 tile at (trow0, tcol0).  Row of the tile = (variable, state) of A, column = that of B:
// column = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5).
// COUNTS: stores the cells of the pairs i <= j, and their mirror images for i < j.
// otherwise: term[reg] <- joint (log joint - log m_i(a) - log m_j(b)) for the real cells of the pairs i < j, 0 elsewhere.
template <bool COUNTS>
__device__ __forceinline__ void tile_terms(const PairsArgs& p, const mi_f32x16& acc, int64_t trow0, int64_t tcol0, int lane,
                                           double (&term)[16]) {
  const int h = lane >> 5;
  const int64_t gc = tcol0 + (lane & 31);
  const int64_t vj = gc / p.Cp;
  const int b = static_cast<int>(gc % p.Cp);
  const double c = static_cast<double>(p.C);
  const double inv_denom = 1.0 / (static_cast<double>(p.N) + c * c * p.alpha);
  const bool col_ok = vj < p.D && b < p.C;
  const double lmj = (!COUNTS && col_ok) ? p.logm[vj * p.C + b] : 0.0;
#pragma unroll
  for (int reg = 0; reg < 16; ++reg) {
    const int64_t gr = trow0 + (reg & 3) + 8 * (reg >> 2) + 4 * h;
    const int64_t vi = gr / p.Cp;
    const int a = static_cast<int>(gr % p.Cp);
    const bool ok = col_ok && vi < p.D && a < p.C && (COUNTS ? vi <= vj : vi < vj);
    if constexpr (COUNTS) {
      if (ok) {
        const int64_t n = static_cast<int64_t>(acc[reg]);
        p.counts[((vi * p.D + vj) * p.C + a) * p.C + b] = n;
        if (vi < vj) p.counts[((vj * p.D + vi) * p.C + b) * p.C + a] = n;
      }
    } else {
      double t = 0.0;
      if (ok) {
        const double joint = (static_cast<double>(acc[reg]) + p.alpha) * inv_denom;
        t = joint * (log(joint) - p.logm[vi * p.C + a] - lmj);
      }
      term[reg] = t;
    }
  }
}

// Cp <= 32: block (blockIdx.y, blockIdx.x) of the upper triangle of 64 x 64 blocks
template <bool COUNTS>
__global__ void __launch_bounds__(64) mi_pairs_narrow_kernel(PairsArgs p) {
  if (blockIdx.y > blockIdx.x) return;
  const int lane = threadIdx.x;
  const int64_t row0 = static_cast<int64_t>(blockIdx.y) * 64, col0 = static_cast<int64_t>(blockIdx.x) * 64;
  mi_f32x16 acc[2][2];
  gram_block(p, row0, col0, lane, acc);
  const int Cp = p.Cp, segs = 32 / Cp;
#pragma unroll
  for (int s = 0; s < 2; ++s)
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int64_t trow0 = row0 + 32 * s, tcol0 = col0 + 32 * t;
      if (trow0 > tcol0) continue;  // (below the diagonal: every pair of the tile has i > j)
      double term[16];
      tile_terms<COUNTS>(p, acc[s][t], trow0, tcol0, lane, term);
      if constexpr (!COUNTS) {
        // segmented sum: the rows of variable trow0 / Cp + q are the registers with row / Cp == q (both lane halves), the
        // columns of a variable an aligned group of Cp lanes
        for (int q = 0; q < segs; ++q) {
          double v = 0.0;
#pragma unroll
          for (int reg = 0; reg < 16; ++reg) {
            const int row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5);
            if (row / Cp == q) v += term[reg];
          }
          for (int o = 1; o < Cp; o <<= 1) v += __shfl_xor(v, o, 64);
          v += __shfl_xor(v, 32, 64);
          const int64_t vi = trow0 / Cp + q, vj = (tcol0 + lane) / Cp;
          if (lane < 32 && (lane & (Cp - 1)) == 0 && vi < vj && vj < p.D) {
            p.mi[vi * p.D + vj] = v;
            p.mi[vj * p.D + vi] = v;
          }
        }
      }
    }
}

// Cp > 32: the pair (blockIdx.y, blockIdx.x), all its tiles; the fp64 sum runs per lane over the tiles in a fixed order and
// is folded over the wave once
template <bool COUNTS>
__global__ void __launch_bounds__(64) mi_pairs_wide_kernel(PairsArgs p) {
  const int64_t i = blockIdx.y, j = blockIdx.x;
  if (i > j || (!COUNTS && i == j)) return;
  const int lane = threadIdx.x;
  const int Cp = p.Cp;
  double total = 0.0;
  for (int u = 0; u < Cp; u += 64)
    for (int v = 0; v < Cp; v += 64) {
      mi_f32x16 acc[2][2];
      gram_block(p, i * Cp + u, j * Cp + v, lane, acc);  // (a state >= Cp of the block's second half matches no code)
#pragma unroll
      for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          if (u + 32 * s >= Cp || v + 32 * t >= Cp) continue;
          double term[16];
          tile_terms<COUNTS>(p, acc[s][t], i * Cp + u + 32 * s, j * Cp + v + 32 * t, lane, term);
          if constexpr (!COUNTS) {
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) total += term[reg];
          }
        }
    }
  if constexpr (!COUNTS) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) total += __shfl_xor(total, o, 64);
    if (lane == 0) {
      p.mi[i * p.D + j] = total;
      p.mi[j * p.D + i] = total;
    }
  }
}

int padded_states(int C) {
  if (C > 32) return (C + 31) / 32 * 32;
  int cp = 1;
  while (cp < C) cp <<= 1;
  return cp;
}

int check_shape(const char* who, int64_t N, int D, int C, int64_t ldn) {
  CK_REQUIRE(N >= 1 && N <= kMaxRows, "%s: %lld rows (1 .. 2^24: fp32 accumulators hold a count exactly up to 2^24)", who,
             static_cast<long long>(N));
  CK_REQUIRE(D >= 1, "%s: %d variables", who, D);
  CK_REQUIRE(C >= 1 && C <= kMaxStates, "%s: %d states (1 .. 256)", who, C);
  CK_REQUIRE(ldn >= N && ldn % 16 == 0, "%s: the staged row stride %lld must cover %lld rows and be a multiple of 16", who,
             static_cast<long long>(ldn), static_cast<long long>(N));
  return 0;
}

}  // namespace

extern "C" {

int ck_mi_stage(const void* x, int is_int64, int64_t N, int D, int num_categories, int divisor, uint8_t* codes, int64_t ldn,
                int32_t* bad_flag, void* stream) {
  CK_REQUIRE(x != nullptr && codes != nullptr && bad_flag != nullptr, "ck_mi_stage: null pointer");
  CK_REQUIRE(divisor >= 1, "ck_mi_stage: divisor %d", divisor);
  if (int st = check_shape("ck_mi_stage", N, D, num_categories, ldn)) return st;
  const dim3 grid(static_cast<unsigned>((N + kStageTile - 1) / kStageTile), static_cast<unsigned>((D + kStageTile - 1) / kStageTile));
  CK_REQUIRE(grid.y <= 65535u, "ck_mi_stage: %d variables (at most 65535 * 64)", D);
  if (is_int64)
    return ck::launch(mi_stage_kernel<int64_t>, grid, dim3(256), 0, stream, static_cast<const int64_t*>(x), N, D,
                      static_cast<int64_t>(num_categories), divisor, codes, ldn, bad_flag);
  return ck::launch(mi_stage_kernel<int32_t>, grid, dim3(256), 0, stream, static_cast<const int32_t*>(x), N, D,
                    static_cast<int64_t>(num_categories), divisor, codes, ldn, bad_flag);
}

int ck_mi_marginals(const uint8_t* codes, int64_t N, int D, int64_t ldn, int C, double alpha, int64_t* hist, double* logm,
                    void* stream) {
  CK_REQUIRE(codes != nullptr && logm != nullptr, "ck_mi_marginals: null pointer");
  CK_REQUIRE(alpha > 0.0 && std::isfinite(alpha), "ck_mi_marginals: smoothing %g (must be positive)", alpha);
  if (int st = check_shape("ck_mi_marginals", N, D, C, ldn)) return st;
  return ck::launch(mi_marginal_kernel, dim3(D), dim3(256), 0, stream, codes, static_cast<int>(N), ldn, C, alpha, hist, logm);
}

int ck_mi_pairs(const uint8_t* codes, int64_t N, int D, int64_t ldn, int C, double alpha, const double* logm, double* mi,
                int64_t* counts, void* stream) {
  CK_REQUIRE(codes != nullptr, "ck_mi_pairs: null codes");
  CK_REQUIRE((mi != nullptr) != (counts != nullptr), "ck_mi_pairs: exactly one of mi and counts");
  CK_REQUIRE(counts != nullptr || logm != nullptr, "ck_mi_pairs: the mutual information needs the marginal table");
  CK_REQUIRE(counts != nullptr || (alpha > 0.0 && std::isfinite(alpha)), "ck_mi_pairs: smoothing %g (must be positive)", alpha);
  if (int st = check_shape("ck_mi_pairs", N, D, C, ldn)) return st;
  if (counts != nullptr)
    CK_REQUIRE(static_cast<double>(D) * D * C * C <= static_cast<double>(CK_MI_MAX_COUNTS),
               "ck_mi_pairs: %d^2 x %d^2 counts exceed 2^28 elements", D, C);
  PairsArgs p{codes, logm, mi, counts, ldn, alpha, static_cast<int>(N), D, C, padded_states(C)};
  if (p.Cp <= 32) {
    const int64_t nb = (static_cast<int64_t>(D) * p.Cp + 63) / 64;
    CK_REQUIRE(nb <= 65535, "ck_mi_pairs: %d variables of %d states (at most 65535 * 64 (variable, state) pairs)", D, C);
    const dim3 grid(static_cast<unsigned>(nb), static_cast<unsigned>(nb));
    if (counts != nullptr) return ck::launch(mi_pairs_narrow_kernel<true>, grid, dim3(64), 0, stream, p);
    return ck::launch(mi_pairs_narrow_kernel<false>, grid, dim3(64), 0, stream, p);
  }
  CK_REQUIRE(D <= 65535, "ck_mi_pairs: %d variables (at most 65535 with more than 32 states)", D);
  const dim3 grid(static_cast<unsigned>(D), static_cast<unsigned>(D));
  if (counts != nullptr) return ck::launch(mi_pairs_wide_kernel<true>, grid, dim3(64), 0, stream, p);
  return ck::launch(mi_pairs_wide_kernel<false>, grid, dim3(64), 0, stream, p);
}

}  // extern "C"
