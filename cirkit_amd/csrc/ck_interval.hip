// Interval (box) evidence: the input layers of `HipCircuit.interval_log_prob` ("Interval evidence").
//
// Every variable of a row carries a closed interval [lo, hi] instead of a value; an input unit emits the log of the mass
// its distribution puts on the interval and the inner layers run unchanged.  Four kernels:
//   * stage_bounds_kernel: the two (B, D) bound tensors -> (D, B) staging copies with the contract's clamping and sentinel
//     rules applied once (the transposes of ck_input.hip, two tensors at a time);
//   * block_sums_kernel:   per parameter state, per (fold, unit): the sums of the aligned blocks of 16 table states, in
//     linear space relative to the block's own maximum;
//   * cat_interval_*:      the mass of a range as a sum of NON-NEGATIVE terms only -- at most 15 head states, whole blocks,
//     at most 15 tail states; no difference of cumulative sums anywhere (in fp32 a prefix difference loses narrow tail
//     intervals entirely);
//   * gauss_interval_kernel: log(Phi(b) - Phi(a)) in fp64 on the side where both tails are small, rounded once.
#include <algorithm>

#include "ck_internal.h"

namespace {

constexpr int kTile = 32;
constexpr int kBlk = 16;           // states per block of the side table
constexpr int kIntLimit = 1 << 30;  // floating-point bounds are clamped to +-2^30 before they become integers

struct IBounds {
  int32_t lo, hi;
};

// The contract's rule for a discrete variable of `ns` states (0: no discrete layer reads it) on integer bounds:
// both negative = integrated (-1, -1); else clamped into 0 .. ns - 1; an empty set is stored as (1, 0).
__device__ __forceinline__ IBounds discrete_rule(int64_t l, int64_t h, int ns) {
  if (l < 0 && h < 0) return {-1, -1};
  if (l < 0) l = 0;
  if (ns > 0 && h > ns - 1) h = ns - 1;
  if (h > kIntLimit) h = kIntLimit;
  if (l > h) return {1, 0};
  return {static_cast<int32_t>(l), static_cast<int32_t>(h)};
}

__device__ __forceinline__ void stage_one(int64_t l, int64_t h, int ns, IBounds& bi, float& fl, float& fh) {
  bi = discrete_rule(l, h, ns);
  fl = static_cast<float>(l), fh = static_cast<float>(h);
}
__device__ __forceinline__ void stage_one(float l, float h, int ns, IBounds& bi, float& fl, float& fh) {
  if (l != l || h != h) {  // a NaN in either bound integrates the variable
    bi = {-1, -1};
    fl = fh = __builtin_nanf("");
    return;
  }
  // the discrete layers read ceil(lo) and floor(hi)
  const float cl = fminf(fmaxf(ceilf(l), -static_cast<float>(kIntLimit)), static_cast<float>(kIntLimit));
  const float fh_ = fminf(fmaxf(floorf(h), -static_cast<float>(kIntLimit)), static_cast<float>(kIntLimit));
  bi = discrete_rule(static_cast<int64_t>(cl), static_cast<int64_t>(fh_), ns);
  fl = l, fh = h;
}

// (B, D) lo / hi -> (D, B) int32 pair (discrete layers) and / or fp32 pair (Gaussian layers); either pair may be NULL.
template <typename T>
__global__ void stage_bounds_kernel(const T* __restrict__ lo, const T* __restrict__ hi, int B, int D,
                                    const int32_t* __restrict__ num_states, int32_t* __restrict__ lo_i,
                                    int32_t* __restrict__ hi_i, float* __restrict__ lo_f, float* __restrict__ hi_f) {
  __shared__ int32_t ti[2][kTile][kTile + 1];
  __shared__ float tf[2][kTile][kTile + 1];
  const int d0 = blockIdx.x * kTile, b0 = blockIdx.y * kTile;
  const int tx = threadIdx.x, ty = threadIdx.y;  // (32, 8)
#pragma unroll
  for (int j = 0; j < kTile; j += 8) {
    const int b = b0 + ty + j, d = d0 + tx;
    if (b < B && d < D) {
      const int64_t i = static_cast<int64_t>(b) * D + d;
      IBounds bi;
      float fl, fh;
      stage_one(lo[i], hi[i], num_states != nullptr ? num_states[d] : 0, bi, fl, fh);
      ti[0][ty + j][tx] = bi.lo, ti[1][ty + j][tx] = bi.hi;
      tf[0][ty + j][tx] = fl, tf[1][ty + j][tx] = fh;
    }
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < kTile; j += 8) {
    const int d = d0 + ty + j, b = b0 + tx;
    if (b < B && d < D) {
      const int64_t o = static_cast<int64_t>(d) * B + b;
      if (lo_i != nullptr) lo_i[o] = ti[0][tx][ty + j], hi_i[o] = ti[1][tx][ty + j];
      if (lo_f != nullptr) lo_f[o] = tf[0][tx][ty + j], hi_f[o] = tf[1][tx][ty + j];
    }
  }
}

// side (F, nblk, 2, K): row 0 the maximum m of the block's log terms, row 1 sum_c exp(t_c - m) over the block's states
// (m = -inf: 0).  One thread per (fold, block, unit), K-minor like the table: the reads of a wave are contiguous.
__global__ void __launch_bounds__(256)
    block_sums_kernel(const float* __restrict__ table, float* __restrict__ side, int64_t n, int C, int K, int nblk) {
  for (int64_t i = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x; i < n; i += static_cast<int64_t>(gridDim.x) * blockDim.x) {
    const int k = static_cast<int>(i % K);
    const int64_t fj = i / K;
    const int j = static_cast<int>(fj % nblk);
    const int64_t f = fj / nblk;
    const float* t = table + (f * (C + 1) + static_cast<int64_t>(j) * kBlk) * K + k;
    const int cnt = min(kBlk, C - j * kBlk);
    float m = -INFINITY;
    for (int c = 0; c < cnt; ++c) m = fmaxf(m, t[static_cast<int64_t>(c) * K]);
    float s = 0.f;
    if (m > -INFINITY)
      for (int c = 0; c < cnt; ++c) s += expf(t[static_cast<int64_t>(c) * K] - m);
    side[(fj * 2) * K + k] = m;
    side[(fj * 2 + 1) * K + k] = s;
  }
}

// W consecutive units of one table / side row
template <int W>
__device__ __forceinline__ void load_units(const float* __restrict__ p, float (&v)[W]) {
  if constexpr (W == 4) {
    const float4 t = *reinterpret_cast<const float4*>(p);
    v[0] = t.x, v[1] = t.y, v[2] = t.z, v[3] = t.w;
  } else {
    v[0] = *p;
  }
}
template <int W>
__device__ __forceinline__ void store_units(float* __restrict__ p, const float (&v)[W]) {
  if constexpr (W == 4) {
    *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
    *p = v[0];
  }
}

// The pieces of the range l .. h (0 <= l < h < C): single states through `state(c)`, whole aligned blocks through `block(j)`.
template <class FS, class FB>
__device__ __forceinline__ void walk_range(int l, int h, FS&& state, FB&& block) {
  const int e = h + 1;
  const int hb = (l + kBlk - 1) / kBlk, tb = e / kBlk;  // whole blocks hb .. tb - 1
  if (hb >= tb) {
    for (int c = l; c < e; ++c) state(c);
    return;
  }
  for (int c = l; c < hb * kBlk; ++c) state(c);
  for (int j = hb; j < tb; ++j) block(j);
  for (int c = tb * kBlk; c < e; ++c) state(c);
}

// out[0..W) for W units of one (fold, row): tab / side point at the fold's block, already advanced to the units.
template <int W>
__device__ __forceinline__ void interval_units(const float* __restrict__ tab, const float* __restrict__ side, int K, int C,
                                               int l, int h, float (&out)[W]) {
  h = min(h, C - 1);  // (memory safety: the staging copy is clamped to the variable's state count already)
  if (l > h) {  // the empty set
#pragma unroll
    for (int i = 0; i < W; ++i) out[i] = -INFINITY;
    return;
  }
  if (l < 0 || (l == 0 && h == C - 1 && C > 1)) return load_units<W>(tab + static_cast<int64_t>(C) * K, out);  // integral row
  if (l == h) return load_units<W>(tab + static_cast<int64_t>(l) * K, out);                                    // a point
  float m[W], s[W], v[W], u[W];
#pragma unroll
  for (int i = 0; i < W; ++i) m[i] = -INFINITY, s[i] = 0.f;
  walk_range(
      l, h,
      [&](int c) {
        load_units<W>(tab + static_cast<int64_t>(c) * K, v);
#pragma unroll
        for (int i = 0; i < W; ++i) m[i] = fmaxf(m[i], v[i]);
      },
      [&](int j) {
        load_units<W>(side + static_cast<int64_t>(2 * j) * K, v);
#pragma unroll
        for (int i = 0; i < W; ++i) m[i] = fmaxf(m[i], v[i]);
      });
#pragma unroll
  for (int i = 0; i < W; ++i) m[i] = m[i] > -INFINITY ? m[i] : 0.f;  // (a range of -inf terms: exp(-inf - 0) = 0, log 0 = -inf)
  walk_range(
      l, h,
      [&](int c) {
        load_units<W>(tab + static_cast<int64_t>(c) * K, v);
#pragma unroll
        for (int i = 0; i < W; ++i) s[i] += expf(v[i] - m[i]);
      },
      [&](int j) {
        load_units<W>(side + static_cast<int64_t>(2 * j) * K, v);
        load_units<W>(side + static_cast<int64_t>(2 * j + 1) * K, u);
#pragma unroll
        for (int i = 0; i < W; ++i) s[i] = fmaf(u[i], expf(v[i] - m[i]), s[i]);
      });
#pragma unroll
  for (int i = 0; i < W; ++i) out[i] = m[i] + logf(s[i]);
}

// vector path: K % 4 == 0.  One lane = 4 consecutive units of one (f, b) row (the shape of gather_rows_vec).
__global__ void __launch_bounds__(256)
    cat_interval_vec(const float* __restrict__ table, const float* __restrict__ side, const int32_t* __restrict__ lo,
                     const int32_t* __restrict__ hi, const int64_t* __restrict__ scope, float* __restrict__ out, int B, int K,
                     int C, int nblk, int rows_per_block) {
  const int f = blockIdx.y;
  const int kv = K >> 2;
  const int lanes_rows = blockDim.x / kv;
  const int r_in = threadIdx.x / kv, q = threadIdx.x - r_in * kv;
  if (r_in >= lanes_rows) return;
  const int64_t var = scope[f];
  const int32_t* lrow = lo + var * B;
  const int32_t* hrow = hi + var * B;
  const float* tab = table + static_cast<int64_t>(f) * (C + 1) * K + 4 * q;
  const float* sd = side + static_cast<int64_t>(f) * nblk * 2 * K + 4 * q;
  const int b_begin = blockIdx.x * rows_per_block;
  const int b_end = min(B, b_begin + rows_per_block);
  for (int b = b_begin + r_in; b < b_end; b += lanes_rows) {
    float v[4];
    interval_units<4>(tab, sd, K, C, lrow[b], hrow[b], v);
    store_units<4>(out + (static_cast<int64_t>(f) * B + b) * K + 4 * q, v);
  }
}

// scalar path: any K.
__global__ void __launch_bounds__(256)
    cat_interval_scalar(const float* __restrict__ table, const float* __restrict__ side, const int32_t* __restrict__ lo,
                        const int32_t* __restrict__ hi, const int64_t* __restrict__ scope, float* __restrict__ out, int B, int K,
                        int C, int nblk) {
  const int f = blockIdx.y;
  const int64_t var = scope[f];
  const int64_t n = static_cast<int64_t>(B) * K;
  const float* tab = table + static_cast<int64_t>(f) * (C + 1) * K;
  const float* sd = side + static_cast<int64_t>(f) * nblk * 2 * K;
  for (int64_t i = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x; i < n;
       i += static_cast<int64_t>(gridDim.x) * blockDim.x) {
    const int b = static_cast<int>(i / K), k = static_cast<int>(i - static_cast<int64_t>(b) * K);
    float v[1];
    interval_units<1>(tab + k, sd + k, K, C, lo[var * B + b], hi[var * B + b], v);
    out[static_cast<int64_t>(f) * n + i] = v[0];
  }
}

// One thread per unit and a few rows (the shape of gaussian_kernel): mean, stddev and 1 / (stddev sqrt 2) once per unit,
// the mass of every (row, unit) in fp64.
__global__ void __launch_bounds__(256)
    gauss_interval_kernel(const float* __restrict__ mean, const float* __restrict__ stddev, const float* __restrict__ logz,
                          const float* __restrict__ lo, const float* __restrict__ hi, const int64_t* __restrict__ scope,
                          float* __restrict__ out, int B, int K, int rows_per_block) {
  const int f = blockIdx.y;
  const int kk = K <= 256 ? K : 256;
  const int lanes_rows = 256 / kk;
  const int r_in = threadIdx.x / kk, k0 = threadIdx.x - r_in * kk;
  if (r_in >= lanes_rows) return;
  const float* lrow = lo + scope[f] * B;
  const float* hrow = hi + scope[f] * B;
  const int b_begin = blockIdx.x * rows_per_block;
  const int b_end = min(B, b_begin + rows_per_block);
  for (int k = k0; k < K; k += kk) {
    const double mu = mean[static_cast<int64_t>(f) * K + k];
    const double inv = 1.0 / (static_cast<double>(stddev[static_cast<int64_t>(f) * K + k]) * 1.41421356237309504880);
    const float lz = logz != nullptr ? logz[static_cast<int64_t>(f) * K + k] : 0.f;
    for (int b = b_begin + r_in; b < b_end; b += lanes_rows) {
      const float l = lrow[b], h = hrow[b];
      float r;
      if (l != l || h != h) {
        r = lz;  // NaN = integrated: the layer's integral, log_partition or 0
      } else if (!(l < h)) {
        r = -INFINITY;  // lo > hi: the empty set; lo == hi: a point has mass 0
      } else {
        double a = (static_cast<double>(l) - mu) * inv, c = (static_cast<double>(h) - mu) * inv;  // z / sqrt 2
        if (a + c > 0.0) {  // to the side where both tails are small
          const double t = a;
          a = -c, c = -t;
        }
        const double mass = 0.5 * (erfc(-c) - erfc(-a));
        r = static_cast<float>(static_cast<double>(lz) + log(mass));  // (mass 0 past ~37 sigma: -inf)
      }
      out[(static_cast<int64_t>(f) * B + b) * K + k] = r;
    }
  }
}

}  // namespace

extern "C" {

int ck_interval_stage(const void* lo, const void* hi, int is_float, int B, int D, const int32_t* num_states, int32_t* lo_i,
                      int32_t* hi_i, float* lo_f, float* hi_f, void* stream) {
  CK_REQUIRE(lo && hi, "ck_interval_stage: null pointer");
  CK_REQUIRE(B > 0 && D > 0, "ck_interval_stage: B=%d D=%d must be positive", B, D);
  CK_REQUIRE((lo_i == nullptr) == (hi_i == nullptr) && (lo_f == nullptr) == (hi_f == nullptr) && (lo_i || lo_f),
             "ck_interval_stage: the staging copies come in pairs, at least one pair");
  dim3 grid((D + kTile - 1) / kTile, (B + kTile - 1) / kTile), block(kTile, 8);
  CK_REQUIRE(grid.y <= 65535, "ck_interval_stage: B=%d exceeds grid.y", B);
  return ck::dispatch(
      [=](hipStream_t s) {
        if (is_float)
          hipLaunchKernelGGL(stage_bounds_kernel<float>, grid, block, 0, s, static_cast<const float*>(lo),
                             static_cast<const float*>(hi), B, D, num_states, lo_i, hi_i, lo_f, hi_f);
        else
          hipLaunchKernelGGL(stage_bounds_kernel<int64_t>, grid, block, 0, s, static_cast<const int64_t*>(lo),
                             static_cast<const int64_t*>(hi), B, D, num_states, lo_i, hi_i, lo_f, hi_f);
        return hipGetLastError();
      },
      stream);
}

int ck_interval_block_sums(const float* table, float* side, int F, int C, int K, void* stream) {
  CK_REQUIRE(table && side, "ck_interval_block_sums: null pointer");
  CK_REQUIRE(F > 0 && C > 0 && K > 0, "ck_interval_block_sums: non-positive size F=%d C=%d K=%d", F, C, K);
  const int nblk = (C + kBlk - 1) / kBlk;
  const int64_t n = static_cast<int64_t>(F) * nblk * K;
  dim3 grid(static_cast<unsigned>(std::min<int64_t>((n + 255) / 256, 8192))), block(256);
  return ck::launch(block_sums_kernel, grid, block, 0, stream, table, side, n, C, K, nblk);
}

int ck_categorical_interval_fwd(const float* table, const float* side, const int32_t* lo, const int32_t* hi,
                                const int64_t* scope, float* out, int F, int B, int K, int C, int D, void* stream) {
  CK_REQUIRE(table && side && lo && hi && scope && out, "ck_categorical_interval_fwd: null pointer");
  CK_REQUIRE(F > 0 && B > 0 && K > 0 && C > 0 && D > 0, "ck_categorical_interval_fwd: non-positive size F=%d B=%d K=%d C=%d D=%d",
             F, B, K, C, D);
  const int nblk = (C + kBlk - 1) / kBlk;
  if (F > ck::kMaxFoldsPerLaunch)
    return ck::chunk_folds(F, [&](int f0, int n) {
      return ck_categorical_interval_fwd(table + static_cast<int64_t>(f0) * (C + 1) * K, side + static_cast<int64_t>(f0) * nblk * 2 * K,
                                         lo, hi, scope + f0, out + static_cast<int64_t>(f0) * B * K, n, B, K, C, D, stream);
    });
  const bool vec = (K % 4 == 0) && (K / 4 <= 256) && ck::aligned16(table) && ck::aligned16(side) && ck::aligned16(out);
  if (vec) {
    const int rows_per_block = 256;
    dim3 grid((B + rows_per_block - 1) / rows_per_block, F), block(256);
    return ck::launch(cat_interval_vec, grid, block, 0, stream, table, side, lo, hi, scope, out, B, K, C, nblk, rows_per_block);
  }
  const int64_t n = static_cast<int64_t>(B) * K;
  dim3 grid(static_cast<unsigned>(std::min<int64_t>((n + 255) / 256, 4096)), F), block(256);
  return ck::launch(cat_interval_scalar, grid, block, 0, stream, table, side, lo, hi, scope, out, B, K, C, nblk);
}

int ck_gaussian_interval_fwd(const float* mean, const float* stddev, const float* log_partition, const float* lo,
                             const float* hi, const int64_t* scope, float* out, int F, int B, int K, int D, void* stream) {
  CK_REQUIRE(mean && stddev && lo && hi && scope && out, "ck_gaussian_interval_fwd: null pointer");
  CK_REQUIRE(F > 0 && B > 0 && K > 0 && D > 0, "ck_gaussian_interval_fwd: non-positive size");
  if (F > ck::kMaxFoldsPerLaunch)
    return ck::chunk_folds(F, [&](int f0, int n) {
      const int64_t o = static_cast<int64_t>(f0) * K;
      return ck_gaussian_interval_fwd(mean + o, stddev + o, log_partition == nullptr ? nullptr : log_partition + o, lo, hi,
                                      scope + f0, out + static_cast<int64_t>(f0) * B * K, n, B, K, D, stream);
    });
  // (fp64 erfc and log per (row, unit): 32 rows per workgroup spread the work over more compute units than the 256 of
  //  the point kernel, whose rows cost a handful of fp32 instructions each)
  const int rows_per_block = std::max(32, 256 / std::min(K, 256));
  dim3 grid((B + rows_per_block - 1) / rows_per_block, F), block(256);
  return ck::launch(gauss_interval_kernel, grid, block, 0, stream, mean, stddev, log_partition, lo, hi, scope, out, B, K,
                    rows_per_block);
}

}  // extern "C"
