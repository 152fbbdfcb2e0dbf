// What the walks down a squared circuit share (ck_sqpath.hip: one path, root to one input fold, in one launch; ck_sqdown.hip: every
// fold above a set of query variables, one launch per layer; ck_sqar.hip: the paths of many steps of an order in one launch): the siblings of a fold read by kind (sp_siblings), one transposed
// TensorDot stage between two LDS blocks (sp_stage) and the leaf form over all states of a variable (sp_leaf), with their
// helpers.  Carved out of ck_sqpath.hip as ck_td.h was out of ck_backward_c.hip; every translation unit gets its own copy.
#pragma once
#include <algorithm>
#include <type_traits>

#include "ck_internal.h"
#include "ck_philox.h"
#include "ck_td.h"

namespace {

constexpr int kSpHead = CK_SQ_PATH_LEVEL_WORDS;  // int64 words of a level in front of its sibling (kind, offset) pairs
constexpr int kSpStates = 256;                   // states of the leaf evaluated at a time: one per thread

template <class T>
struct SpArgs {
  const T* full;
  const T* cst;
  const T* rank1;
  const int64_t* lev;  // [L][kSpHead + 2 S]
  int L, S;
  const float* table;  // the input fold's (C + 1, K) table
  int C, K, table_log;
  float* log_m;    // (B, C) or null
  int64_t* x;      // (B, D) the batch c's forward reads, or null: no draw
  int64_t* x_out;  // (B, D) the samples
  int32_t* dead;   // (B,) rows that draw -1
  int D, var;
  uint32_t node, seed_lo, seed_hi;
  int64_t row0;
  int B, R, maxK;
  const float* lam;  // log weights of the variable's states under soft evidence, row b at lam + b lam_row; null: none
  int64_t lam_row;
};

template <class T>
__device__ __forceinline__ T sp_log_real(float r);
template <>
__device__ __forceinline__ float sp_log_real<float>(float r) { return r; }
template <>
__device__ __forceinline__ c32 sp_log_real<c32>(float r) { return {r, 0.f}; }

__device__ __forceinline__ float sp_lift(float a, float b) { return a + b; }                  // y_k + y_l
__device__ __forceinline__ c32 sp_lift(c32 a, c32 b) { return {a.re + b.re, a.im - b.im}; }   // y_k + conj(y_l)

// v plus the values of the level's siblings at element i = k K + l of row b
template <class S>
__device__ __forceinline__ typename S::T sp_siblings(const SpArgs<typename S::T>& a, const int64_t* e, int64_t b, int K, int i, typename S::T v) {
  using T = typename S::T;
  const int n = static_cast<int>(e[6]);
  for (int h = 0; h < n; ++h) {
    const int64_t kd = e[kSpHead + 2 * h], o = e[kSpHead + 2 * h + 1];
    T c;
    if (kd == CK_SQ_FULL) {
      c = a.full[o + b * K * K + i];
    } else if (kd == CK_SQ_CONST) {
      c = a.cst[o + i];
    } else {
      const T* y = a.rank1 + o + b * K;
      c = sp_lift(y[i / K], y[i % K]);
    }
    v = S::add(v, c);
  }
  return v;
}

// the maximum over the workgroup (NaN ignored); `red`: 4 floats nobody else is reading
__device__ __forceinline__ float sp_block_max(float v, float* red, int t) {
#pragma unroll
  for (int s = 1; s < 64; s <<= 1) v = fmaxf(v, __shfl_xor(v, s, 64));
  __syncthreads();
  if ((t & 63) == 0) red[t >> 6] = v;
  __syncthreads();
  return fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

// a row that draws nothing: -1 in the samples, NaN marginals
template <class T>
__device__ __forceinline__ void sp_dead_row(const SpArgs<T>& a, int64_t b, int t) {
  if (a.log_m)
    for (int s = t; s < a.C; s += 256) a.log_m[b * a.C + s] = __int_as_float(0x7fc00000);
  if (a.x_out && t == 0) {
    a.x_out[b * a.D + a.var] = -1;
    a.x[b * a.D + a.var] = 0;
    a.dead[b] = 1;
  }
}

// The leaf: log m_b(s) = log max(0, sum_kl e[k][l] a_k(s) a_l(s)) + gmax for every state s, e = Re exp(G - gmax) in LDS (real
// parameters: a is real and only the real part of the quadratic form is left); a table of logarithms is shifted by its
// maximum over the units state by state.  Under soft evidence (`lam`) the state's own log weight is added.  Then, with a batch to
// draw into, the inverse CDF over the states.
template <class T>
__device__ __forceinline__ void sp_leaf(const SpArgs<T>& a, int64_t b, const float* e, float* av, float* lm, float* red, float gmax, int t) {
  const int K = a.K, C = a.C;
  const float* lam = a.lam ? a.lam + b * a.lam_row : nullptr;
  for (int s0 = 0; s0 < C; s0 += kSpStates) {
    const int n = C - s0 < kSpStates ? C - s0 : kSpStates;
    __syncthreads();  // (e is written, av is free)
    for (int i = t; i < n * K; i += 256) {
      const int s = i / K, k = i - s * K;
      av[s * (K + 1) + k] = a.table[static_cast<int64_t>(s0) * K + i];
    }
    __syncthreads();
    if (t < n) {
      float* r = av + t * (K + 1);  // (this thread's row: nobody else touches it)
      float tm = 0.f;
      if (a.table_log) {
        tm = -INFINITY;
        for (int k = 0; k < K; ++k) tm = fmaxf(tm, r[k]);
        tm = ck::clamp_finite(tm);
        for (int k = 0; k < K; ++k) r[k] = expf(r[k] - tm);
      }
      float acc = 0.f;
      for (int k = 0; k < K; ++k) {
        float in = 0.f;
        for (int l2 = 0; l2 < K; ++l2) in = fmaf(e[k * K + l2], r[l2], in);
        acc = fmaf(r[k], in, acc);
      }
      acc = acc < 0.f ? 0.f : acc;  // (cancellation can leave -1e-9: that is a zero, not a NaN; a NaN stays one)
      lm[s0 + t] = logf(acc) + gmax + 2.f * tm;
      if (lam) lm[s0 + t] += lam[s0 + t];
    }
  }
  __syncthreads();
  if (a.log_m)
    for (int s = t; s < C; s += 256) a.log_m[b * C + s] = lm[s];
  if (!a.x_out) return;
  float mx = -INFINITY;
  for (int s = t; s < C; s += 256) mx = fmaxf(mx, lm[s]);
  mx = ck::clamp_finite(sp_block_max(mx, red, t));
  for (int s = t; s < C; s += 256) lm[s] = expf(lm[s] - mx);
  __syncthreads();
  if (t != 0) return;
  float tot = 0.f;
  for (int s = 0; s < C; ++s) tot += lm[s];
  int64_t state = -1;
  if (tot > 0.f && tot < INFINITY) {  // (all zero, or a NaN among them: no draw)
    const ck::Philox4 p = ck::philox4x32_10(static_cast<uint32_t>(a.row0 + b), a.node, 0u, 0u, a.seed_lo, a.seed_hi);
    const float target = ck::philox_uniform(p.x[0]) * tot;
    float cum = 0.f;
    int last = -1;
    for (int s = 0; s < C; ++s) {  // the smallest s with u T < CDF_s; rounding at the top: the last state with any mass
      if (lm[s] > 0.f) last = s;
      cum += lm[s];
      if (cum > target) {
        state = s;
        break;
      }
    }
    if (state < 0) state = last;
  }
  a.x_out[b * a.D + a.var] = state;
  a.x[b * a.D + a.var] = state < 0 ? 0 : state;
  if (state < 0) a.dead[b] = 1;
}

// one TensorDot stage of the way down between two LDS blocks: y[q][k] = log(sum_j W[j][k] exp(x[j][q] - m_q)) + m_q, x (Kj, Kq),
// W (Kj, Kk) the FORWARD's row-major weight matrix (Ko = Kj, Ki = Kk) read transposed; the sums in td_fwd_body's order
template <class S>
__device__ __forceinline__ void sp_stage(const typename S::T* x, typename S::T* y, typename S::T* a_s, float* w_s, float* m_s,
                                         const float* __restrict__ w, int Kj, int Kq, int Kk) {
  using T = typename S::T;
  for (int i = threadIdx.x; i < Kj * Kk; i += 256) {
    const int j = i / Kk, k = i - j * Kk;
    w_s[k * (Kj + 1) + j] = w[i];
  }
  for (int i = threadIdx.x; i < Kj * Kq; i += 256) {
    const int j = i / Kq, q = i - j * Kq;
    a_s[q * (Kj + 1) + j] = x[i];
  }
  __syncthreads();
  for (int q = threadIdx.x; q < Kq; q += 256) {
    float mx = -INFINITY;
    for (int j = 0; j < Kj; ++j) mx = fmaxf(mx, S::re(a_s[q * (Kj + 1) + j]));
    m_s[q] = ck::clamp_finite(mx);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < Kq * Kj; i += 256) {
    const int q = i / Kj, j = i - q * Kj;
    a_s[q * (Kj + 1) + j] = S::exp_shift(a_s[q * (Kj + 1) + j], m_s[q]);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < Kq * Kk; i += 256) {
    const int q = i / Kk, k = i - q * Kk;
    T acc = S::zero();
    for (int j = 0; j < Kj; ++j) acc = S::fma_w(w_s[k * (Kj + 1) + j], a_s[q * (Kj + 1) + j], acc);
    y[i] = S::log_shift(acc, m_s[q]);
  }
  __syncthreads();
}

template <class T>
__host__ __device__ constexpr size_t sp_value_words(int maxK) {  // the two gradient blocks and a stage's a
  return static_cast<size_t>(2) * maxK * maxK + static_cast<size_t>(maxK) * (maxK + 1);
}
__host__ __device__ constexpr size_t sp_leaf_floats(int C, int K) {  // av, lm
  return static_cast<size_t>(C < kSpStates ? C : kSpStates) * (K + 1) + C;
}

// `Kernel` needs its dynamic-LDS limit raised once per device, not once per step of a 784-step sample
template <auto Kernel>
hipError_t sp_raise_lds(size_t lds, size_t fixed) {
  static size_t raised[64] = {};  // per device: the largest dynamic size the limit was raised to
  if (lds + fixed <= 48 * 1024) return hipSuccess;
  int dev = 0;
  hipError_t er = hipGetDevice(&dev);
  if (er != hipSuccess) return er;
  if (dev < 0 || dev >= 64 || lds > raised[dev]) {
    er = hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds));
    if (er != hipSuccess) return er;
    if (dev >= 0 && dev < 64) raised[dev] = lds;
  }
  return hipSuccess;
}

}  // namespace
