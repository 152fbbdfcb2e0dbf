// Soft (likelihood) evidence: the leaves of `HipCircuit.soft_evidence_log_prob` and `HipCircuit.soft_posterior_marginals`
// ("Soft evidence").
//
// A soft variable of a row carries a non-negative weight per state, log_lik[n, s, c] = log lambda; an input unit over it
// emits log sum_c lambda(c) t_k(c) and the inner layers run unchanged.  Kernels:
//   * soft_tables_kernel:   per parameter state, per (fold, unit): mt = max_c table (0 where every term is -inf) and the
//     table in linear space relative to it, lin (F, C, K) and its transpose linT (F, K, C);
//   * soft_leaf_mfma:       K = 32 / 64.  A workgroup owns (fold, 32 rows): the rows' log_lik go through LDS, are shifted by
//     their row maximum and exponentiated in place, and are contracted with lin on the fp32 matrix cores, the four waves
//     each a quarter of the states.  An entry whose sum stays below 2^-60 -- the evidence peaks where the table is in a far
//     tail, both shifted operands underflow -- is recomputed by the exact two-pass log-sum-exp;
//   * soft_leaf_generic:    any K and C, the exact two-pass log-sum-exp per (row, unit);
//   * soft_post_mfma / soft_post_generic: the posteriors p[n, s, c] = sum_k f_k exp(table[c, k] + log_lik[n, s, c] - v_k)
//     from the flows f and the leaf's own values v.  The matrix-core kernel factors a term as
//     (f_k exp(ml + mt_k - v_k)) lin[c, k] exp(log_lik - ml); a row with a unit whose shifted sum was below 2^-60 takes the
//     exact form instead, every exponent <= 0.
// A NaN or +inf in a read entry of log_lik marks the row in bad[] and gives NaN; -inf is weight 0.
#include <algorithm>

#include "ck_internal.h"
#include "ck_soft_entry.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
constexpr int kThreads = 256;
constexpr int kWaves = kThreads / ck::kWave;
constexpr int kRows = 32;               // rows of a matrix-core tile
constexpr float kTiny = 0x1p-60f;       // a shifted sum below this is recomputed exactly
constexpr float kTinyLog = -41.58883f;  // log(2^-60)
constexpr int kMaxStatesMfma = 256;     // the staged (32, C) tile, the partials and the factors stay below 48 KiB of LDS

__device__ __forceinline__ bool unusable(float v) { return v != v || v == INFINITY; }  // NaN or +inf: the row is NaN

// log sum_c exp(ll[c] + tab[c K]) over c < C, two passes, every term relative to the maximum.
__device__ __forceinline__ float exact_lse(const float* __restrict__ ll, const float* __restrict__ tab, int C, int K) {
  float m = -INFINITY;
  for (int c = 0; c < C; ++c) m = fmaxf(m, ll[c] + tab[static_cast<int64_t>(c) * K]);
  if (!(m > -INFINITY)) return -INFINITY;
  float s = 0.f;
  for (int c = 0; c < C; ++c) s += expf((ll[c] + tab[static_cast<int64_t>(c) * K]) - m);
  return m + logf(s);
}

__global__ void __launch_bounds__(kThreads)
    soft_tables_kernel(const float* __restrict__ table, float* __restrict__ lin, float* __restrict__ linT,
                       float* __restrict__ mt, int64_t n, int C, int K) {
  for (int64_t i = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x; i < n;
       i += static_cast<int64_t>(gridDim.x) * blockDim.x) {
    const int k = static_cast<int>(i % K);
    const int64_t f = i / K;
    const float* t = table + f * (C + 1) * K + k;
    float m = -INFINITY;
    for (int c = 0; c < C; ++c) m = fmaxf(m, t[static_cast<int64_t>(c) * K]);
    if (!(m > -INFINITY && m < INFINITY)) m = 0.f;
    mt[i] = m;
    for (int c = 0; c < C; ++c) {
      const float e = expf(t[static_cast<int64_t>(c) * K] - m);
      lin[(f * C + c) * K + k] = e;
      linT[(f * K + k) * C + c] = e;
    }
  }
}

// Rows n0 .. n0 + 31 of soft variable s into LDS tile L (32 rows of `stride` floats, columns C .. Cp - 1 weight 0; Cp <= 256):
// the row maximum (0 for a row of -inf) in sm, whether the row holds a NaN / +inf in snan, exp(ll - max) in the tile.  Wave w
// stages rows 8 w .. 8 w + 7, a lane four consecutive states of each: all eight loads are in flight before the first
// reduction (`vec`: as one 16-byte load; C and Cl multiples of 4, ll aligned).  The caller synchronises.
__device__ __forceinline__ void stage_rows(const float* __restrict__ ll, int64_t n0, int64_t B, int s, int S, int Cl, int C,
                                           int Cp, int stride, bool vec, float* L, float* sm, int* snan) {
  constexpr int R = kRows / kWaves;
  const int lane = threadIdx.x & (ck::kWave - 1), wave = threadIdx.x / ck::kWave;
  const int c4 = 4 * lane;
  float4 v[R];
#pragma unroll
  for (int i = 0; i < R; ++i) {
    const int64_t n = n0 + wave * R + i;
    const float* row = ll + (n * S + s) * static_cast<int64_t>(Cl) + c4;
    v[i] = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
    if (n < B) {
      if (vec) {
        if (c4 < C) v[i] = ck::gload4(row);
      } else {
        if (c4 < C) v[i].x = row[0];
        if (c4 + 1 < C) v[i].y = row[1];
        if (c4 + 2 < C) v[i].z = row[2];
        if (c4 + 3 < C) v[i].w = row[3];
      }
    }
  }
#pragma unroll
  for (int i = 0; i < R; ++i) {
    const int r = wave * R + i;
    const float4 t = v[i];
    const int nan = __any(unusable(t.x) || unusable(t.y) || unusable(t.z) || unusable(t.w)) ? 1 : 0;
    const float mx = ck::wave_max(fmaxf(fmaxf(t.x, t.y), fmaxf(t.z, t.w)));
    const float m0 = (mx > -INFINITY && !nan) ? mx : 0.f;
    if (c4 < Cp)
      *reinterpret_cast<float4*>(L + r * stride + c4) =
          nan ? make_float4(0.f, 0.f, 0.f, 0.f) : make_float4(expf(t.x - m0), expf(t.y - m0), expf(t.z - m0), expf(t.w - m0));
    if (lane == 0) sm[r] = m0, snan[r] = nan;
  }
}

template <int K>
__global__ void __launch_bounds__(kThreads)
    soft_leaf_mfma(const float* __restrict__ table, const float* __restrict__ lin, const float* __restrict__ mt,
                   const float* __restrict__ ll, const int32_t* __restrict__ spos, float* __restrict__ out,
                   int32_t* __restrict__ bad, int B, int C, int S, int Cl, int Cp, int big, int vec) {
  constexpr int NT = K / 32;
  extern __shared__ float sh[];
  float* const L = sh;  // the staged tile, then the waves' partial sums (4, 32, K)
  float* const sm = sh + big;
  int* const snan = reinterpret_cast<int*>(sm + kRows);
  const int f = blockIdx.y;
  const int s = spos[f];
  if (s < 0) return;  // a hard variable: the forward's own launch wrote this fold
  const int stride = Cp + 4;
  const int64_t n0 = static_cast<int64_t>(blockIdx.x) * kRows;
  stage_rows(ll, n0, B, s, S, Cl, C, Cp, stride, vec != 0, L, sm, snan);
  __syncthreads();
  const int lane = threadIdx.x & (ck::kWave - 1), wave = threadIdx.x / ck::kWave;
  const int b = lane & 31, hi = lane >> 5;
  const int Ch = Cp / (2 * kWaves);  // states per half wave, a multiple of 4
  const int cbase = (wave * 2 + hi) * Ch;
  f32x16 acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
  const float* lf = lin + static_cast<int64_t>(f) * C * K + b;
  for (int j = 0; j < Ch; j += 4) {
    const float4 a = *reinterpret_cast<const float4*>(L + b * stride + cbase + j);
    const float av[4] = {a.x, a.y, a.z, a.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int c = min(cbase + j + i, C - 1);  // (columns past C carry weight 0)
#pragma unroll
      for (int t = 0; t < NT; ++t)
        acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[i], lf[static_cast<int64_t>(c) * K + 32 * t], acc[t], 0, 0, 0);
    }
  }
  __syncthreads();  // every wave has read its part of the tile: the partial sums take its place
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = 8 * (r >> 2) + 4 * hi + (r & 3);
      L[(wave * kRows + row) * K + 32 * t + b] = acc[t][r];
    }
  __syncthreads();
  for (int o = threadIdx.x; o < kRows * K; o += kThreads) {
    const int row = o / K, k = o % K;
    const int64_t n = n0 + row;
    if (n >= B) continue;
    float sum = L[row * K + k];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) sum += L[(w * kRows + row) * K + k];
    float y;
    if (snan[row]) {
      y = NAN;
      if (k == 0) bad[n] = 1;
    } else if (sum < kTiny) {
      y = exact_lse(ll + (n * S + s) * static_cast<int64_t>(Cl), table + static_cast<int64_t>(f) * (C + 1) * K + k, C, K);
    } else {
      y = sm[row] + mt[static_cast<int64_t>(f) * K + k] + logf(sum);
    }
    out[(static_cast<int64_t>(f) * B + n) * K + k] = y;
  }
}

__global__ void __launch_bounds__(kThreads)
    soft_leaf_generic(const float* __restrict__ table, const float* __restrict__ ll, const int32_t* __restrict__ spos,
                      float* __restrict__ out, int32_t* __restrict__ bad, int B, int K, int C, int S, int Cl) {
  const int f = blockIdx.y;
  const int s = spos[f];
  if (s < 0) return;
  const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= static_cast<int64_t>(B) * K) return;
  const int64_t n = i / K;
  const int k = static_cast<int>(i % K);
  const float* row = ll + (n * S + s) * static_cast<int64_t>(Cl);
  bool nan = false;
  for (int c = 0; c < C; ++c) nan |= unusable(row[c]);
  float y = NAN;
  if (nan) {
    if (k == 0) bad[n] = 1;
  } else {
    y = exact_lse(row, table + static_cast<int64_t>(f) * (C + 1) * K + k, C, K);
  }
  out[static_cast<int64_t>(f) * B * K + i] = y;
}

// ---- posteriors --------------------------------------------------------------------------------------------------------
using ck::SoftEntry;  // (ck_soft_entry.h, shared with ck_soft_decode.hip)

__device__ __forceinline__ bool row_ok(const float* __restrict__ vals, const int64_t* __restrict__ val_off, int root_fold,
                                       int root_ko, const int32_t* __restrict__ bad, int64_t n) {
  const float r = vals[val_off[root_fold] + n * root_ko];
  return r > -INFINITY && r < INFINITY && bad[n] == 0;
}

__global__ void __launch_bounds__(kThreads)
    soft_logev_kernel(const float* __restrict__ vals, const int64_t* __restrict__ val_off, int root_fold, int root_ko,
                      const int32_t* __restrict__ bad, int64_t B, float* __restrict__ logev) {
  const int64_t n = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (n < B) logev[n] = bad[n] ? NAN : vals[val_off[root_fold] + n * root_ko];
}

// sum_k f_k exp((t[c, k] + l) - v_k) over the units that carry flow: every exponent <= 0 up to rounding.
__device__ __forceinline__ float exact_post(const SoftEntry& e, const float* __restrict__ fr, const float* __restrict__ vr,
                                            int c, float l) {
  if (!(l > -INFINITY)) return 0.f;
  const float* t = e.table + static_cast<int64_t>(c) * e.K;
  float acc = 0.f;
  for (int k = 0; k < e.K; ++k) {
    const float fk = fr[k], v = vr[k];
    if (fk > 0.f && v > -INFINITY && v < INFINITY) acc = fmaf(fk, expf(fminf((t[k] + l) - v, 0.f)), acc);
  }
  return acc;
}

__global__ void __launch_bounds__(kThreads)
    soft_post_generic(const SoftEntry* __restrict__ ent, const int32_t* __restrict__ qstart, int S, int Cl,
                      const float* __restrict__ ll, const float* __restrict__ flow, const float* __restrict__ vals,
                      const int64_t* __restrict__ val_off, int root_fold, int root_ko, const int32_t* __restrict__ bad,
                      int64_t B, float* __restrict__ out) {
  const int64_t idx = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (idx >= B * S * Cl) return;
  const int c = static_cast<int>(idx % Cl);
  const int s = static_cast<int>((idx / Cl) % S);
  const int64_t n = idx / (static_cast<int64_t>(Cl) * S);
  float acc = 0.f;
  if (!row_ok(vals, val_off, root_fold, root_ko, bad, n)) {
    acc = NAN;
  } else {
    for (int q = qstart[s]; q < qstart[s + 1]; ++q) {
      const SoftEntry e = ent[q];
      if (c >= e.C) continue;
      const int64_t at = val_off[e.g] + n * e.K;
      acc += exact_post(e, flow + at, vals + at, c, ll[idx]);
    }
  }
  out[idx] = acc;
}

// Every entry with K units and C states.  A workgroup owns (s, 32 rows): the rows' log_lik staged as in the evidence leaf;
// per entry the factors a[row, k] = f_k exp(ml + mt_k - v_k) in LDS; the waves own 32-state column tiles of
// (32 rows x K) a x (K x 32) linT; a result is scaled by its exp(log_lik - ml).  A row with a unit whose shifted sum
// exp(v_k - ml - mt_k) is below 2^-60 is left to the exact form after the tiles.
template <int K>
__global__ void __launch_bounds__(kThreads)
    soft_post_mfma(const SoftEntry* __restrict__ ent, const int32_t* __restrict__ qstart, int S, int Cl, int C, int Cp,
                   const float* __restrict__ ll, const float* __restrict__ linT, const float* __restrict__ mt,
                   const float* __restrict__ flow, const float* __restrict__ vals, const int64_t* __restrict__ val_off,
                   int root_fold, int root_ko, const int32_t* __restrict__ bad, int64_t B, int64_t row_tiles,
                   int vec, float* __restrict__ out) {
  constexpr int KH = K / 2, AS = K + 4;
  extern __shared__ float sh[];
  const int stride = Cp + 4;
  float* const L = sh;                     // (32, stride) exp(log_lik - ml)
  float* const sa = L + kRows * stride;    // (32, K + 4) the factors of one entry
  float* const sm = sa + kRows * AS;       // (32) ml
  int* const snan = reinterpret_cast<int*>(sm + kRows);
  int* const sflag = snan + kRows;         // 0: the tiles; 1: the exact form; 2: NaN
  const int lane = threadIdx.x & (ck::kWave - 1), wave = threadIdx.x / ck::kWave;
  const int b = lane & 31, hi = lane >> 5;
  const int s = static_cast<int>(blockIdx.x / row_tiles);
  const int64_t n0 = (blockIdx.x % row_tiles) * kRows;
  stage_rows(ll, n0, B, s, S, Cl, C, Cp, stride, vec != 0, L, sm, snan);
  if (threadIdx.x < kRows) {
    const int64_t n = n0 + threadIdx.x;
    sflag[threadIdx.x] = (n < B && row_ok(vals, val_off, root_fold, root_ko, bad, n)) ? 0 : 2;
  }
  __syncthreads();
  const int q0 = qstart[s], q1 = qstart[s + 1];
  for (int cg = 0; cg < Cp; cg += kWaves * 32) {
    const int c0 = cg + wave * 32;
    const int c = c0 + b;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    for (int q = q0; q < q1; ++q) {
      const SoftEntry e = ent[q];
      for (int o = threadIdx.x; o < kRows * K; o += kThreads) {
        const int row = o / K, k = o % K;
        const int64_t n = min(n0 + row, B - 1);
        const int64_t at = val_off[e.g] + n * K + k;
        const float fk = flow[at], v = vals[at];
        float a = 0.f;
        if (fk > 0.f && v > -INFINITY && v < INFINITY) {
          const float d = (v - sm[row]) - mt[e.mt_off + k];  // log of the unit's shifted sum
          if (d >= kTinyLog) {
            a = fk * expf(-d);
          } else if (sflag[row] == 0) {
            sflag[row] = 1;  // (every writer stores the same value)
          }
        }
        sa[row * AS + k] = a;
      }
      __syncthreads();
      if (c0 < C) {
        const float* t = linT + e.lin_off + static_cast<int64_t>(hi) * KH * C + min(c, C - 1);
#pragma unroll
        for (int j = 0; j < KH; j += 4) {
          const float4 a4 = *reinterpret_cast<const float4*>(sa + b * AS + hi * KH + j);
          const float av[4] = {a4.x, a4.y, a4.z, a4.w};
#pragma unroll
          for (int i = 0; i < 4; ++i)
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[i], t[static_cast<int64_t>(j + i) * C], acc, 0, 0, 0);
        }
      }
      __syncthreads();  // the next entry's factors take the place of these
    }
    if (c >= C) continue;  // (no barrier follows in this round for the lanes that leave: the loop's barriers are all above)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = 8 * (r >> 2) + 4 * hi + (r & 3);
      const int64_t n = n0 + row;
      if (n >= B || sflag[row] == 1) continue;
      out[(n * S + s) * static_cast<int64_t>(Cl) + c] = sflag[row] == 2 ? NAN : acc[r] * L[row * stride + c];
    }
  }
  // the exact form for the rows that asked for it, and the zeros past the variable's states
  for (int row = 0; row < kRows; ++row) {
    const int64_t n = n0 + row;
    if (n >= B) break;
    const int flag = sflag[row];
    float* orow = out + (n * S + s) * static_cast<int64_t>(Cl);
    for (int cc = C + threadIdx.x; cc < Cl; cc += kThreads) orow[cc] = flag == 2 ? NAN : 0.f;
    if (flag != 1) continue;
    const float* lrow = ll + (n * S + s) * static_cast<int64_t>(Cl);
    for (int cc = threadIdx.x; cc < C; cc += kThreads) {
      float acc = 0.f;
      for (int q = q0; q < q1; ++q) {
        const SoftEntry e = ent[q];
        const int64_t at = val_off[e.g] + n * K;
        acc += exact_post(e, flow + at, vals + at, cc, lrow[cc]);
      }
      orow[cc] = acc;
    }
  }
}

// whether a lane's four states of a row are one aligned 16-byte load
int vec_ok(const float* ll, int C, int Cl) { return (C % 4 == 0 && Cl % 4 == 0 && ck::aligned16(ll)) ? 1 : 0; }

int lds_floats_leaf(int Cp, int K) { return std::max(kRows * (Cp + 4), kWaves * kRows * K); }

}  // namespace

extern "C" {

int ck_soft_tables(const float* table, float* lin, float* linT, float* mt, int F, int C, int K, void* stream) {
  CK_REQUIRE(table && lin && linT && mt, "ck_soft_tables: null pointer");
  CK_REQUIRE(F > 0 && C > 0 && K > 0, "ck_soft_tables: non-positive size F=%d C=%d K=%d", F, C, K);
  const int64_t n = static_cast<int64_t>(F) * K;
  dim3 grid(static_cast<unsigned>(std::min<int64_t>((n + kThreads - 1) / kThreads, 8192))), block(kThreads);
  return ck::launch(soft_tables_kernel, grid, block, 0, stream, table, lin, linT, mt, n, C, K);
}

int ck_soft_leaf_fwd(const float* table, const float* lin, const float* mt, const float* log_lik, const int32_t* spos,
                     float* out, int32_t* bad, int F, int B, int K, int C, int S, int Cl, int exact, void* stream) {
  CK_REQUIRE(table && lin && mt && log_lik && spos && out && bad, "ck_soft_leaf_fwd: null pointer");
  CK_REQUIRE(F > 0 && B > 0 && K > 0 && C > 0 && S > 0 && Cl >= C,
             "ck_soft_leaf_fwd: bad size F=%d B=%d K=%d C=%d S=%d Cl=%d", F, B, K, C, S, Cl);
  if (F > ck::kMaxFoldsPerLaunch)
    return ck::chunk_folds(F, [&](int f0, int n) {
      return ck_soft_leaf_fwd(table + static_cast<int64_t>(f0) * (C + 1) * K, lin + static_cast<int64_t>(f0) * C * K,
                              mt + static_cast<int64_t>(f0) * K, log_lik, spos + f0, out + static_cast<int64_t>(f0) * B * K,
                              bad, n, B, K, C, S, Cl, exact, stream);
    });
  if (!exact && (K == 32 || K == 64) && C <= kMaxStatesMfma) {
    const int Cp = (C + 31) / 32 * 32;
    const int big = lds_floats_leaf(Cp, K);
    const size_t lds = (big + 2 * kRows) * sizeof(float);
    dim3 grid((B + kRows - 1) / kRows, F), block(kThreads);
    auto kern = K == 32 ? soft_leaf_mfma<32> : soft_leaf_mfma<64>;
    return ck::launch(kern, grid, block, lds, stream, table, lin, mt, log_lik, spos, out, bad, B, C, S, Cl, Cp, big,
                      vec_ok(log_lik, C, Cl));
  }
  const int64_t blocks = (static_cast<int64_t>(B) * K + kThreads - 1) / kThreads;
  CK_REQUIRE(blocks <= 0x7fffffff, "ck_soft_leaf_fwd: too many entries");
  dim3 grid(static_cast<unsigned>(blocks), F), block(kThreads);
  return ck::launch(soft_leaf_generic, grid, block, 0, stream, table, log_lik, spos, out, bad, B, K, C, S, Cl);
}

int ck_soft_posterior(const int64_t* entries, const int32_t* qstart, int S, int Cl, int K_uniform, int C_uniform,
                      const float* log_lik, const float* linT, const float* mt, const float* flow, const float* vals,
                      const int64_t* val_off, int root_fold, int root_ko, const int32_t* bad, int64_t B, float* out,
                      float* logev, void* stream) {
  CK_REQUIRE(entries && qstart && log_lik && linT && mt && flow && vals && val_off && bad && out,
             "ck_soft_posterior: null pointer");
  CK_REQUIRE(S > 0 && Cl > 0 && B > 0 && root_fold >= 0 && root_ko > 0 && K_uniform >= 0 && C_uniform >= 0 && C_uniform <= Cl,
             "ck_soft_posterior: bad size");
  static_assert(sizeof(SoftEntry) == 6 * sizeof(int64_t), "six int64 per entry");
  if (logev != nullptr) {
    const int64_t blocks = (B + kThreads - 1) / kThreads;
    if (int st = ck::launch(soft_logev_kernel, dim3(static_cast<unsigned>(blocks)), dim3(kThreads), 0, stream, vals, val_off,
                            root_fold, root_ko, bad, B, logev))
      return st;
  }
  const SoftEntry* ent = reinterpret_cast<const SoftEntry*>(entries);
  if ((K_uniform == 32 || K_uniform == 64) && C_uniform > 0 && C_uniform <= kMaxStatesMfma) {
    const int C = C_uniform, Cp = (C + 31) / 32 * 32;
    const int64_t row_tiles = (B + kRows - 1) / kRows;
    CK_REQUIRE(S * row_tiles <= 0x7fffffff, "ck_soft_posterior: grid too large");
    const size_t lds = (kRows * (Cp + 4) + kRows * (K_uniform + 4) + 3 * kRows) * sizeof(float);
    auto kern = K_uniform == 32 ? soft_post_mfma<32> : soft_post_mfma<64>;
    return ck::launch(kern, dim3(static_cast<unsigned>(S * row_tiles)), dim3(kThreads), lds, stream, ent, qstart, S, Cl, C, Cp,
                      log_lik, linT, mt, flow, vals, val_off, root_fold, root_ko, bad, B, row_tiles, vec_ok(log_lik, C, Cl), out);
  }
  const int64_t blocks = (B * S * Cl + kThreads - 1) / kThreads;
  CK_REQUIRE(blocks <= 0x7fffffff, "ck_soft_posterior: too many entries");
  return ck::launch(soft_post_generic, dim3(static_cast<unsigned>(blocks)), dim3(kThreads), 0, stream, ent, qstart, S, Cl,
                    log_lik, flow, vals, val_off, root_fold, root_ko, bad, B, out);
}

}  // extern "C"
