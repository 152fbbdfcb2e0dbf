// Soft and interval evidence of squared circuits p(x) = |c(x)|^2 / Z ("Soft and interval evidence of squared
// circuits").  Z(lambda)[b] = sum_x |c(x)|^2 prod_{v in S} lambda[b, v, x_v] is the product circuit c (x) conj(c) with one change at
// the leaves: the input fold of a soft variable emits, per row, the WEIGHTED Gram matrix of its table,
//     G_b[k][l] = sum_s lambda_b(s) e_k(s) conj(e_l(s)),
// K^2 values per row in the mixed arena's element format and unit order (unit k K + l, the unconjugated factor slow): a FULL child
// of `ck_squared_mixed_fwd` (ck_sqmar.hip).  The tables are real (real parameter tensors), so the Gram is real and symmetric; its
// logarithm is written as `float` under lse-sum and as c32 under complex-lse-sum (argument pi where the sum is negative, -inf
// where it is exactly 0: TdR / TdC::log_shift of ck_td.h).  The partition function's unweighted Gram at batch 1 is
// `functional._embedding_square_integral` / `_categorical_square_integral`; the reference has no weighted one.
//
// Stabilisation: the weights of a row are shifted by m_b = the clamped maximum of its log weights (an all -inf row gives -inf, not
// NaN), a table of logarithms by the clamped maximum mt_k of every unit's column (a side table of the caller); the result is
// log G + m_b (+ mt_k + mt_l).  A NaN or +inf among the read log weights of a row makes that row's block NaN.
// Interval evidence is the 0/1 case read from the bounds themselves: lambda_b(s) = [lo <= s <= hi], m_b = 0.
#include <algorithm>

#include "ck_tile.h"

namespace {

constexpr int kSsSlab = 128;             // states of a slab of the 32-unit form (even: a step takes two states)
constexpr int kSsRows = 4;               // rows of a wave of the 32-unit form: their accumulators live across the slabs
constexpr int kSsTile = 4 * kSsRows;     // rows of a workgroup per walk of the slabs
constexpr int kSsGenFloats = 8192;       // table values of a slab of the plain form
constexpr int kSsGenStates = 256;        // ... and its states at most
constexpr int kSsGenElems = 16;          // Gram elements of a thread of the plain form: K <= 64

struct SsArgs {
  const float* table;     // (F, C + 1, K); row C is the layer's integral row, not read
  const float* unit_max;  // (F, K) clamped column maxima of a table of logarithms, or null
  const int32_t* tab;     // [n][2]: fold of the table, column (of log_lik's S axis / of lo and hi)
  const float* ll;        // (B, S, Cl) log weights, or null: interval evidence
  const int64_t* lo;      // (B, D)
  const int64_t* hi;
  float* out;             // (n, B, K^2) values
  int n, B, C, K, S, Cl, D, R;
};

// the bounds of a row as states 0 .. C - 1 (the rule of ck_interval.hip: both negative is the full range, else clamped; l > h: empty)
__device__ __forceinline__ void ss_bounds(const SsArgs& a, int64_t b, int col, int& l, int& h) {
  int64_t l64 = a.lo[b * a.D + col], h64 = a.hi[b * a.D + col];
  if (l64 < 0 && h64 < 0) l64 = 0, h64 = a.C - 1;
  if (l64 < 0) l64 = 0;
  if (h64 > a.C - 1) h64 = a.C - 1;
  if (l64 > h64) l64 = 1, h64 = 0;
  l = static_cast<int>(l64), h = static_cast<int>(h64);
}

// m_b of a row over its C read log weights, by one wave (every lane gets it); NaN where a read entry is NaN or +inf
__device__ __forceinline__ float ss_row_shift(const float* __restrict__ row, int C, int lane) {
  float mx = -INFINITY, bad = 0.f;
  for (int s = lane; s < C; s += 64) {
    const float v = row[s];
    mx = fmaxf(mx, v);
    bad = (v != v || v == INFINITY) ? 1.f : bad;
  }
  mx = ck::clamp_finite(ck::wave_max(mx));
  return ck::wave_max(bad) != 0.f ? __builtin_nanf("") : mx;
}

// log of the REAL sum g plus the shift, in the element format: what TdR::log_shift / TdC::log_shift (ck_td.h) give for a value without
// imaginary part -- `float`: -inf for 0, NaN for a negative sum; c32: (log |g| + shift, pi where g < 0), (-inf, 0) for 0 -- without
// the library's hypot, log1p and atan2 of a complex argument: 16 elements per lane and row sit behind every Gram of the MFMA form
template <bool CPLX>
__device__ __forceinline__ void ss_store(float* out, int64_t elem, float g, float shift) {
  if constexpr (CPLX) {
    const float re = fmaf(__builtin_amdgcn_logf(fabsf(g)), kLN2, shift);  // (log 0 = -inf, and -inf + shift stays -inf)
    *reinterpret_cast<float2*>(out + 2 * elem) = make_float2(re, g < 0.f ? 3.14159265358979323846f : 0.f);
  } else {
    out[elem] = fmaf(__builtin_amdgcn_logf(g), kLN2, shift);
  }
}

// ---- 32 units: a wave takes kSsRows rows; per step of two states s = 2 step + lane / 32 the A and the B operand of
// v_mfma_f32_32x32x2_f32 are the same staged value a(s, lane % 32), A scaled by the row's weight w_b(s).  D[k][l] comes back in lane
// (l, hi) register r with k = 8 (r >> 2) + 4 hi + (r & 3) (ck_tile.h): a register is one row of the Gram, 32 lanes wide.  The
// workgroup stages a slab of the fold's table once for its kSsTile rows (once for all its rows when the table is one slab).  Under
// soft evidence every row takes every step: the wave reads a staged value once for its rows and interleaves their chains; under
// interval evidence a row takes only the steps that meet its bounds, one row after the other.  Either way a row's sum runs over
// the states in ascending order: its bits do not depend on its place.
template <bool CPLX, bool TLOG, bool SOFT>
__global__ void __launch_bounds__(256) ss_gram32_kernel(SsArgs a) {
  __shared__ __attribute__((aligned(16))) float a_s[kSsSlab * 32];
  __shared__ __attribute__((aligned(16))) float w_s[kSsTile * kSsSlab];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6, bl = lane & 31, kh = lane >> 5;
  const int Rb = (a.R + kSsTile - 1) / kSsTile * kSsTile;
  const int nb = (a.B + Rb - 1) / Rb;
  const int j = blockIdx.x / nb;
  const int fold = a.tab[2 * j], col = a.tab[2 * j + 1];
  const float* tf = a.table + static_cast<int64_t>(fold) * (a.C + 1) * 32;
  const int64_t b0 = static_cast<int64_t>(blockIdx.x - j * nb) * Rb;
  const int64_t b1 = b0 + Rb < a.B ? b0 + Rb : a.B;
  const bool one_slab = a.C <= kSsSlab;
  float mtk = 0.f;
  if constexpr (TLOG) mtk = a.unit_max[fold * 32 + (t & 31)];  // (the unit this thread stages)
  for (int64_t t0 = b0; t0 < b1; t0 += kSsTile) {
    float m[kSsRows];
    int l[kSsRows], h[kSsRows];
    f32x16 acc[kSsRows];
#pragma unroll
    for (int r = 0; r < kSsRows; ++r) {
      const int64_t b = t0 + wv * kSsRows + r;
      m[r] = 0.f, l[r] = 0, h[r] = a.C - 1;
      if (b < b1) {
        if constexpr (SOFT)
          m[r] = ss_row_shift(a.ll + (b * a.S + col) * a.Cl, a.C, lane);
        else
          ss_bounds(a, b, col, l[r], h[r]);
      }
#pragma unroll
      for (int q = 0; q < 16; ++q) acc[r][q] = 0.f;
    }
    for (int s0 = 0; s0 < a.C; s0 += kSsSlab) {
      const int ns = a.C - s0 < kSsSlab ? a.C - s0 : kSsSlab;
      const int ne = (ns + 1) & ~1;  // an odd count leaves the last step half empty: that state is staged as 0 with weight 0
      if (!one_slab || t0 == b0) {
        __syncthreads();  // (the steps of the slab before are done)
        for (int i = t; i < ne * 32; i += 256) {
          float v = 0.f;
          if (i < ns * 32) {
            v = tf[static_cast<int64_t>(s0) * 32 + i];
            if constexpr (TLOG) v = expf(v - mtk);
          }
          a_s[i] = v;
        }
      }
      const float* wr = w_s + wv * kSsRows * kSsSlab;
      if constexpr (SOFT) {  // (a wave stages and reads the weights of its own rows; a row past the batch weighs nothing)
#pragma unroll
        for (int r = 0; r < kSsRows; ++r) {
          const int64_t b = t0 + wv * kSsRows + r;
          const float* row = a.ll + (b * a.S + col) * a.Cl + s0;
          for (int s = lane; s < ne; s += 64) w_s[(wv * kSsRows + r) * kSsSlab + s] = (b < b1 && s < ns) ? expf(row[s] - m[r]) : 0.f;
        }
      }
      __syncthreads();
      if constexpr (SOFT) {  // every row takes every step: a staged value is read once for the wave's rows, whose chains interleave
        if (t0 + wv * kSsRows >= b1) continue;  // (uniform in the wave; the barriers of the next slab are at the top of the loop)
        for (int st = 0; st < ne / 2; ++st) {
          const int s = 2 * st + kh;
          const float av = a_s[s * 32 + bl];
#pragma unroll
          for (int r = 0; r < kSsRows; ++r) acc[r] = __builtin_amdgcn_mfma_f32_32x32x2f32(wr[r * kSsSlab + s] * av, av, acc[r], 0, 0, 0);
        }
      } else {  // a row takes the steps that meet its [l, h] alone: uniform in the wave
#pragma unroll
        for (int r = 0; r < kSsRows; ++r) {
          if (t0 + wv * kSsRows + r >= b1) continue;
          const int sl = l[r] - s0 > 0 ? l[r] - s0 : 0, sh = h[r] - s0 < ns - 1 ? h[r] - s0 : ns - 1;
          const int st1 = sl <= sh ? sh / 2 + 1 : 0;
          const int lr = l[r] - s0, hr = h[r] - s0;
          auto step = [&](int st) {
            const int s = 2 * st + kh;
            const float av = a_s[s * 32 + bl];
            acc[r] = __builtin_amdgcn_mfma_f32_32x32x2f32((s >= lr && s <= hr) ? av : 0.f, av, acc[r], 0, 0, 0);
          };
          int st = sl / 2;
          for (; st + 4 <= st1; st += 4) {
            step(st), step(st + 1), step(st + 2), step(st + 3);
          }
          for (; st < st1; ++st) step(st);
        }
      }
    }
    float mtl = 0.f;
    if constexpr (TLOG) mtl = a.unit_max[fold * 32 + bl];
#pragma unroll
    for (int r = 0; r < kSsRows; ++r) {
      const int64_t b = t0 + wv * kSsRows + r;
      if (b >= b1) continue;
      const int64_t base = (static_cast<int64_t>(j) * a.B + b) * 1024;
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int k = 8 * (q >> 2) + 4 * kh + (q & 3);
        float shift = m[r];
        if constexpr (TLOG) shift += a.unit_max[fold * 32 + k] + mtl;
        ss_store<CPLX>(a.out, base + k * 32 + bl, acc[r][q], shift);
      }
    }
  }
}

// ---- any other K (K^2 <= 256 kSsGenElems): one row at a time, thread t owns the elements i = t + 256 e of the Gram; a slab of the
// table and the row's weights in LDS, the sums on the VALU in the order of the states.
template <bool CPLX, bool TLOG>
__global__ void __launch_bounds__(256) ss_gram_kernel(SsArgs a, int slab) {
  extern __shared__ __attribute__((aligned(16))) char ss_smem[];
  float* a_s = reinterpret_cast<float*>(ss_smem);  // [slab][K]
  float* w_s = a_s + slab * a.K;                   // [slab]
  const int t = threadIdx.x, lane = t & 63, K = a.K, K2 = K * K;
  const int nb = (a.B + a.R - 1) / a.R;
  const int j = blockIdx.x / nb;
  const int fold = a.tab[2 * j], col = a.tab[2 * j + 1];
  const float* tf = a.table + static_cast<int64_t>(fold) * (a.C + 1) * K;
  const float* mt = TLOG ? a.unit_max + static_cast<int64_t>(fold) * K : nullptr;
  const int64_t b0 = static_cast<int64_t>(blockIdx.x - j * nb) * a.R;
  const int64_t b1 = b0 + a.R < a.B ? b0 + a.R : a.B;
  for (int64_t b = b0; b < b1; ++b) {
    float m = 0.f;
    int l = 0, h = a.C - 1;
    const float* row = nullptr;
    if (a.ll != nullptr) {
      row = a.ll + (b * a.S + col) * a.Cl;
      m = ss_row_shift(row, a.C, lane);  // (every wave the same value)
    } else {
      ss_bounds(a, b, col, l, h);
    }
    float acc[kSsGenElems];
#pragma unroll
    for (int e = 0; e < kSsGenElems; ++e) acc[e] = 0.f;
    for (int s0 = 0; s0 < a.C; s0 += slab) {
      const int ns = a.C - s0 < slab ? a.C - s0 : slab;
      if (s0 > h || s0 + ns <= l) continue;  // (uniform in the workgroup: no state of the slab is inside the bounds)
      __syncthreads();
      for (int i = t; i < ns * K; i += 256) {
        float v = tf[static_cast<int64_t>(s0) * K + i];
        if constexpr (TLOG) v = expf(v - mt[i % K]);
        a_s[i] = v;
      }
      for (int s = t; s < ns; s += 256)
        w_s[s] = row != nullptr ? expf(row[s0 + s] - m) : ((s0 + s >= l && s0 + s <= h) ? 1.f : 0.f);
      __syncthreads();
      const int sa = l - s0 > 0 ? l - s0 : 0, sb = h - s0 < ns - 1 ? h - s0 : ns - 1;
#pragma unroll
      for (int e = 0; e < kSsGenElems; ++e) {
        const int i = t + 256 * e;
        if (i >= K2) continue;
        const int k = i / K, q = i - k * K;
        float s_acc = acc[e];
        for (int s = sa; s <= sb; ++s) s_acc = fmaf(w_s[s] * a_s[s * K + k], a_s[s * K + q], s_acc);
        acc[e] = s_acc;
      }
    }
    const int64_t base = (static_cast<int64_t>(j) * a.B + b) * K2;
#pragma unroll
    for (int e = 0; e < kSsGenElems; ++e) {
      const int i = t + 256 * e;
      if (i >= K2) continue;
      float shift = m;
      if constexpr (TLOG) shift += mt[i / K] + mt[i % K];
      ss_store<CPLX>(a.out, base + i, acc[e], shift);
    }
  }
}

template <template <bool, bool> class Launcher, class... A>
int ss_pick(bool cplx, bool tlog, A... args) {
  if (cplx) return tlog ? Launcher<true, true>::run(args...) : Launcher<true, false>::run(args...);
  return tlog ? Launcher<false, true>::run(args...) : Launcher<false, false>::run(args...);
}
template <bool CPLX, bool TLOG>
struct SsMfma {
  static int run(const SsArgs& a, int64_t blocks, void* stream) {
    if (a.ll != nullptr) return ck::launch(ss_gram32_kernel<CPLX, TLOG, true>, dim3(static_cast<unsigned>(blocks)), dim3(256), 0, stream, a);
    return ck::launch(ss_gram32_kernel<CPLX, TLOG, false>, dim3(static_cast<unsigned>(blocks)), dim3(256), 0, stream, a);
  }
};
template <bool CPLX, bool TLOG>
struct SsPlain {
  static int run(const SsArgs& a, int64_t blocks, int slab, void* stream) {
    const size_t lds = static_cast<size_t>(slab) * (a.K + 1) * sizeof(float);  // (<= 32 KiB + 1 KiB: below the default limit)
    return ck::launch(ss_gram_kernel<CPLX, TLOG>, dim3(static_cast<unsigned>(blocks)), dim3(256), lds, stream, a, slab);
  }
};

}  // namespace

extern "C" int ck_squared_soft_leaf(const float* table, int num_folds, int C, int K, int table_log, const float* unit_max,
                                    const int32_t* tab_host, const int32_t* tab, int n, const float* log_lik, int S, int C_lik,
                                    const int64_t* lo, const int64_t* hi, int D, float* out, int B, int rows_per_block, int complex_values,
                                    int form, void* stream) {
  const char* who = "ck_squared_soft_leaf";
  CK_REQUIRE(table && tab_host && tab && out, "%s: null pointer", who);
  CK_REQUIRE(n > 0 && B > 0 && C > 0 && K > 0 && num_folds > 0 && rows_per_block > 0, "%s: bad sizes", who);
  CK_REQUIRE(!table_log || unit_max, "%s: a table of logarithms needs the units' column maxima", who);
  CK_REQUIRE(form == 0 || form == 1, "%s: form=%d", who, form);
  const bool soft = log_lik != nullptr;
  CK_REQUIRE(soft ? (!lo && !hi && S > 0 && C_lik >= C) : (lo && hi && D > 0),
             "%s: either log_lik (B, S, C_lik >= C = %d) or lo and hi (B, D)", who, C);
  for (int j = 0; j < n; ++j)  // the folds as the host knows them: every read inside the table, log_lik, lo and hi
    CK_REQUIRE(tab_host[2 * j] >= 0 && tab_host[2 * j] < num_folds && tab_host[2 * j + 1] >= 0 && tab_host[2 * j + 1] < (soft ? S : D),
               "%s: fold %d: table fold %d of %d, column %d of %d", who, j, tab_host[2 * j], num_folds, tab_host[2 * j + 1], soft ? S : D);
  const SsArgs a{table, table_log ? unit_max : nullptr, tab, log_lik, lo, hi, out, n, B, C, K, S, C_lik, D, rows_per_block};
  if (K == 32 && form == 0) {
    const int Rb = (rows_per_block + kSsTile - 1) / kSsTile * kSsTile;
    const int64_t blocks = static_cast<int64_t>(n) * ((B + Rb - 1) / Rb);
    CK_REQUIRE(blocks <= 0x7fffffffLL, "%s: %d folds x %d rows", who, n, B);
    return ss_pick<SsMfma>(complex_values != 0, table_log != 0, a, blocks, stream);
  }
  if (static_cast<int64_t>(K) * K > 256 * kSsGenElems)
    return ck::fail(CK_ERR_UNSUPPORTED, "%s: K=%d: the plain form holds at most %d x %d Gram elements per workgroup (K <= 64)", who, K, 256,
                    kSsGenElems);
  const int slab = std::max(1, std::min(std::min(kSsGenStates, kSsGenFloats / K), C));
  const int64_t blocks = static_cast<int64_t>(n) * ((B + rows_per_block - 1) / rows_per_block);
  CK_REQUIRE(blocks <= 0x7fffffffLL, "%s: %d folds x %d rows", who, n, B);
  return ss_pick<SsPlain>(complex_values != 0, table_log != 0, a, blocks, slab, stream);
}
