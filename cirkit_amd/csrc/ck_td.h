// The arithmetic of the TensorDot launches (ck_backward_c.hip) shared with the mixed folds of a squared circuit's marginals
// (ck_sqmar.hip): the complex helpers, the semiring traits TdR / TdC, the shape-generic stage (td_stage, td_fwd_body) and the
// 32-unit forms (TdR32 / TdC32, Td32Lds, td32_stage_w, td32_exp, td32_fwd_stage).  Every translation unit gets its own copy.
#pragma once
#include "ck_internal.h"

namespace {

using ck::c32;

__device__ __forceinline__ c32 cmul(c32 a, c32 b) { return {a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re}; }
__device__ __forceinline__ c32 cconj(c32 a) { return {a.re, -a.im}; }
__device__ __forceinline__ c32 cexp(c32 z) {
  const float r = expf(z.re);
  float s, c;
  sincosf(z.im, &s, &c);
  return {r * c, r * s};
}

#ifdef CK_TD_STAMPS  // lab build (scripts/ubench/td_stamps.hip): wall-clock stamps of workgroup (0, 0)
__device__ long long* g_td_stamps = nullptr;
__device__ int g_td_n = 0;
#define TD_STAMP()                                                                                             \
  do {                                                                                                         \
    if (g_td_stamps != nullptr && threadIdx.x == 0 && blockIdx.x == 0 && blockIdx.y == 0 && g_td_n < 32)        \
      g_td_stamps[g_td_n++] = static_cast<long long>(wall_clock64());                                          \
  } while (0)
#else
#define TD_STAMP() do {} while (0)
#endif

struct TdC {
  using T = c32;
  static __device__ __forceinline__ float re(c32 a) { return a.re; }
  static __device__ __forceinline__ c32 add(c32 a, c32 b) { return ck::c_add(a, b); }
  static __device__ __forceinline__ c32 exp_shift(c32 v, float m) { return cexp({v.re - m, v.im}); }                 // a
  static __device__ __forceinline__ c32 log_shift(c32 y, float m) { return ck::c_log_shift(y, m); }
  static __device__ __forceinline__ c32 tee(c32 y, c32 g, float m) {                                                 // t
    return (g.re == 0.f && g.im == 0.f) ? c32{0.f, 0.f} : cmul(cconj(cexp({m - y.re, -y.im})), g);
  }
  static __device__ __forceinline__ c32 zero() { return {0.f, 0.f}; }
  static __device__ __forceinline__ c32 fma_w(float w, c32 t, c32 acc) { return {fmaf(w, t.re, acc.re), fmaf(w, t.im, acc.im)}; }
  static __device__ __forceinline__ c32 child(c32 a, c32 acc) { return cmul(cconj(a), acc); }
  static __device__ __forceinline__ float dw(c32 a, c32 t) { return a.re * t.re + a.im * t.im; }  // Re(conj(a) t)
};
struct TdR {
  using T = float;
  static __device__ __forceinline__ float re(float a) { return a; }
  static __device__ __forceinline__ float add(float a, float b) { return a + b; }
  static __device__ __forceinline__ float exp_shift(float v, float m) { return expf(v - m); }
  static __device__ __forceinline__ float log_shift(float y, float m) { return logf(y) + m; }
  static __device__ __forceinline__ float tee(float y, float g, float m) { return g == 0.f ? 0.f : expf(m - y) * g; }
  static __device__ __forceinline__ float zero() { return 0.f; }
  static __device__ __forceinline__ float fma_w(float w, float t, float acc) { return fmaf(w, t, acc); }
  static __device__ __forceinline__ float child(float a, float acc) { return a * acc; }
  static __device__ __forceinline__ float dw(float a, float t) { return a * t; }
};

// LDS of a stage: a [Kq][Kj + 1] values, (backward) t [Kq][Kk + 1] values, W [Kk][Kj + 1] floats, m [Kq] floats
template <class S>
__host__ __device__ constexpr size_t td_lds(int Kj, int Kq, int Kk, bool bwd) {
  return (static_cast<size_t>(Kq) * (Kj + 1) + (bwd ? static_cast<size_t>(Kq) * (Kk + 1) : 0)) * sizeof(typename S::T) +
         (static_cast<size_t>(Kk) * (Kj + 1) + Kq) * sizeof(float);
}

// a <- exp(x - m_q) with x[j][q] = load(j Kq + q), W staged: the common first half of both directions
template <class S, class Load>
__device__ __forceinline__ void td_stage(typename S::T* a_s, float* w_s, float* m_s, Load&& load, const float* __restrict__ wf, int Kj, int Kq,
                                         int Kk) {
  for (int i = threadIdx.x; i < Kk * Kj; i += 256) w_s[(i / Kj) * (Kj + 1) + i % Kj] = wf[i];
  for (int i = threadIdx.x; i < Kj * Kq; i += 256) {  // coalesced read of x[j][q]
    const int j = i / Kq, q = i - j * Kq;
    a_s[q * (Kj + 1) + j] = load(i);
  }
  __syncthreads();
  TD_STAMP();
  for (int q = threadIdx.x; q < Kq; q += 256) {
    float mx = -INFINITY;
    for (int j = 0; j < Kj; ++j) mx = fmaxf(mx, S::re(a_s[q * (Kj + 1) + j]));
    m_s[q] = ck::clamp_finite(mx);
  }
  __syncthreads();
  TD_STAMP();
  for (int i = threadIdx.x; i < Kq * Kj; i += 256) {
    const int q = i / Kj, j = i - q * Kj;
    a_s[q * (Kj + 1) + j] = S::exp_shift(a_s[q * (Kj + 1) + j], m_s[q]);
  }
  TD_STAMP();
}

template <class S, class Load>
__device__ __forceinline__ void td_fwd_body(char* smem, Load&& load, const float* __restrict__ wf, typename S::T* __restrict__ dst, int Kj, int Kq,
                                            int Kk) {
  using T = typename S::T;
  T* a_s = reinterpret_cast<T*>(smem);
  float* w_s = reinterpret_cast<float*>(a_s + static_cast<size_t>(Kq) * (Kj + 1));
  float* m_s = w_s + static_cast<size_t>(Kk) * (Kj + 1);
  td_stage<S>(a_s, w_s, m_s, load, wf, Kj, Kq, Kk);
  __syncthreads();
  TD_STAMP();
  for (int i = threadIdx.x; i < Kq * Kk; i += 256) {
    const int q = i / Kk, k = i - q * Kk;
    T acc = S::zero();
    for (int j = 0; j < Kj; ++j) acc = S::fma_w(w_s[k * (Kj + 1) + j], a_s[q * (Kj + 1) + j], acc);
    dst[i] = S::log_shift(acc, m_s[q]);
  }
  TD_STAMP();
}

// ---- 32 units everywhere (the partition function of BASELINE config 5: M' = W M W^T per fold, (32, 32) blocks) ---------------------
// The shape-generic bodies above are chains of phases of 1 - 4 us each on ONE row (scripts/ubench/td_stamps.hip: per stage 1.7 us of
// loads, 1.8 a serial maximum per column, 1.2 library exponentials, 3.9 a contraction whose 4 x 32 dependent LDS reads the
// compiler cannot unroll for run-time sizes + library logarithms; the second stage reloads from memory what the workgroup has
// just stored: 17 us forward, 28 us backward for ONE fold).  With the sizes fixed thread t owns the elements i = t + 256 r of every
// (32, 32) block in play -- the same four for the stage's input x[j][q] (i = 32 j + q), its output / the tee (i = 32 q + k), the
// child gradient (i = 32 j + q) and the weight gradient (i = 32 k + j) -- so the column maxima are four registers + one shuffle +
// four LDS words, the second stage's input and the gradient between the stages never leave the registers, and every LDS loop is
// unrolled over 16-byte reads.  The order of every sum is the generic kernels' (bit-identical contractions); exp / log / sincos /
// atan are the polynomial forms of the complex tile kernels (ck_internal.h, <= 2 ulp).
struct TdC32 : TdC {
  static constexpr int kA = 34;  // values per LDS row of a (32, 32) block: rows start on 16 bytes
  static __device__ __forceinline__ c32 exp_shift(c32 v, float m) { return ck::c_exp_shift_tile(v, m); }
  static __device__ __forceinline__ c32 log_shift(c32 y, float m) { return ck::c_log_shift_tile(y, m); }
  static __device__ __forceinline__ c32 tee(c32 y, c32 g, float m) {
    return (g.re == 0.f && g.im == 0.f) ? c32{0.f, 0.f} : cmul(cconj(ck::c_exp_shift_tile({-y.re, -y.im}, -m)), g);
  }
  static __device__ __forceinline__ void read4(const c32* p, c32 (&v)[4]) {
    const float4 a = *reinterpret_cast<const float4*>(p), b = *reinterpret_cast<const float4*>(p + 2);
    v[0] = {a.x, a.y};
    v[1] = {a.z, a.w};
    v[2] = {b.x, b.y};
    v[3] = {b.z, b.w};
  }
};
struct TdR32 : TdR {
  static constexpr int kA = 36;
  static __device__ __forceinline__ void read4(const float* p, float (&v)[4]) {
    const float4 a = *reinterpret_cast<const float4*>(p);
    v[0] = a.x;
    v[1] = a.y;
    v[2] = a.z;
    v[3] = a.w;
  }
};
constexpr int kTdW = 36;  // floats per LDS row of a (32, 32) weight matrix

template <class S>
struct Td32Lds {
  typename S::T a[32 * S::kA];   // a[q][j] = exp(x[j][q] - m_q)
  typename S::T t[32 * S::kA];   // (backward) t[q][k]
  typename S::T tt[32 * S::kA];  // (backward) t[q][k] at [k][q]
  float w[2][32 * kTdW];         // W[k][j] of the two stages
  float wt[2][32 * kTdW];        // (backward) W[k][j] at [j][k]
  float m[32];
  float red[4][32];
};

// the weights of a stage into LDS (visible after the stage's first barrier)
template <bool BWD>
__device__ __forceinline__ void td32_stage_w(const float* __restrict__ wf, float* w_s, float* wt_s, int t) {
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int i = t + 256 * r;
    const float v = wf[i];
    w_s[(i >> 5) * kTdW + (i & 31)] = v;
    if (BWD) wt_s[(i & 31) * kTdW + (i >> 5)] = v;
  }
}

// m_q = the clamped maximum of column q = t & 31 (this thread's four values are rows j = (t >> 5) + 8 r of it), a = exp(x - m_q):
// into `a` and, transposed, into LDS; m into LDS.  Ends with a barrier.
template <class S, class L>
__device__ __forceinline__ void td32_exp(L& l, const typename S::T (&x)[4], typename S::T (&a)[4], int t) {
  float pm = fmaxf(fmaxf(S::re(x[0]), S::re(x[1])), fmaxf(S::re(x[2]), S::re(x[3])));
  pm = fmaxf(pm, __shfl_xor(pm, 32, 64));
  if ((t & 63) < 32) l.red[t >> 6][t & 31] = pm;
  __syncthreads();
  const int q = t & 31;
  const float m = ck::clamp_finite(fmaxf(fmaxf(l.red[0][q], l.red[1][q]), fmaxf(l.red[2][q], l.red[3][q])));
  if (t < 32) l.m[t] = m;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    a[r] = S::exp_shift(x[r], m);
    l.a[q * S::kA + (t >> 5) + 8 * r] = a[r];
  }
  __syncthreads();
}

// y[q'][k] = log(sum_j W[k][j] a[q'][j]) + m_q' for this thread's elements i = 32 q' + k
template <class S, class L>
__device__ __forceinline__ void td32_fwd_stage(L& l, const float* w_s, const typename S::T (&x)[4], typename S::T (&y)[4], int t) {
  using T = typename S::T;
  T a[4];
  td32_exp<S>(l, x, a, t);
  const int k = t & 31, q0 = t >> 5;
  T acc[4] = {S::zero(), S::zero(), S::zero(), S::zero()};
#pragma unroll 2
  for (int j = 0; j < 32; j += 4) {
    const float4 w4 = *reinterpret_cast<const float4*>(w_s + k * kTdW + j);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      T av[4];
      S::read4(l.a + (q0 + 8 * r) * S::kA + j, av);
      acc[r] = S::fma_w(w4.x, av[0], acc[r]);
      acc[r] = S::fma_w(w4.y, av[1], acc[r]);
      acc[r] = S::fma_w(w4.z, av[2], acc[r]);
      acc[r] = S::fma_w(w4.w, av[3], acc[r]);
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) y[r] = S::log_shift(acc[r], l.m[q0 + 8 * r]);
}
}  // namespace
