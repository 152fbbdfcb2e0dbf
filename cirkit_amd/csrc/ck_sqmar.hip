// Marginals of a squared circuit p(x) = |c(x)|^2 / Z: the MIXED folds of the product circuit c (x) conj(c) -- the folds of c whose
// scope holds observed AND integrated variables ("Marginals of squared circuits").  What the reference
// evaluates as integrate(multiply(c, conjugate(c)), scope=M) followed by a forward (symbolic/functional.py:161-258 integrate,
// :259-593 multiply; the Kronecker-weighted sum split into two TensorDot layers, optimization/layers.py:90-127), with every
// fold of the product circuit at K^2 units per row.  Here a fold of c whose scope misses M is never squared (its K^2 values are
// the outer product of the K values c's own forward left in its arena: RANK-1, lifted while it is read), a fold inside M is a
// constant of the partition-function circuit (CONST, evaluated once at batch 1) and only the folds in between are evaluated
// here, K^2 units per row (FULL), from children of all three kinds:
//     out[f, b, :] = TD2(TD1(sum_h lift(child_h)))            (log space: the sum is the Hadamard product)
// TD1 / TD2 are the two TensorDot stages of a squared sum layer (ck_backward_c.hip: td32_fwd_kernel<S, true>, the arithmetic of
// ck_td.h): unit k K + l of a block pairs unit k of c (slow) with unit l of conj(c).
#include <algorithm>

#include "ck_internal.h"
#include "ck_td.h"

namespace {

__device__ __forceinline__ float sq_lift(float a, float b) { return a + b; }                       // y_k + y_l
__device__ __forceinline__ c32 sq_lift(c32 a, c32 b) { return {a.re + b.re, a.im - b.im}; }        // y_k + conj(y_l)

// the children of one mixed fold: element i = k K + l of row b of child h
template <class S>
struct SqChildren {
  using T = typename S::T;
  const T* full;
  const T* cst;
  const T* rank1;
  const int32_t* kind;  // [H]
  const int64_t* off;   // [H]
  int H, K;
  __device__ __forceinline__ T one(int h, int64_t b, int i) const {
    const int64_t o = off[h];
    const int kd = kind[h];
    if (kd == CK_SQ_FULL) return full[o + b * K * K + i];
    if (kd == CK_SQ_CONST) return cst[o + i];
    const T* y = rank1 + o + b * K;
    return sq_lift(y[i / K], y[i % K]);
  }
  __device__ __forceinline__ T load(int64_t b, int i) const {
    T v = one(0, b, i);
    for (int h = 1; h < H; ++h) v = S::add(v, one(h, b, i));
    return v;
  }
};

template <class S>
__device__ __forceinline__ SqChildren<S> sq_children(const typename S::T* full, const typename S::T* cst, const typename S::T* rank1,
                                                     const int32_t* kind, const int64_t* off, int H, int K, int f) {
  return {full, cst, rank1, kind + static_cast<int64_t>(f) * H, off + static_cast<int64_t>(f) * H, H, K};
}

// a Hadamard layer of c: the K^2 product itself, any K.  One workgroup per (fold, row).
template <class S>
__global__ void __launch_bounds__(256)
    sq_hadamard_kernel(const typename S::T* full, const typename S::T* __restrict__ cst, const typename S::T* __restrict__ rank1,
                       const int32_t* __restrict__ kind, const int64_t* __restrict__ off, int H, typename S::T* out, int B, int K) {
  const int f = blockIdx.y;
  const int64_t b = blockIdx.x;
  const auto ch = sq_children<S>(full, cst, rank1, kind, off, H, K, f);
  typename S::T* o = out + (static_cast<int64_t>(f) * B + b) * K * K;
  for (int i = threadIdx.x; i < K * K; i += 256) o[i] = ch.load(b, i);
}

// 32 units everywhere: td32_fwd_kernel<S, true> with the children read by kind.  A workgroup stages the fold's two weight
// matrices once and walks R rows.
template <class S>
__global__ void __launch_bounds__(256, 2)
    sq_mixed32_kernel(const typename S::T* full, const typename S::T* __restrict__ cst, const typename S::T* __restrict__ rank1,
                      const int32_t* __restrict__ kind, const int64_t* __restrict__ off, int H, const float* __restrict__ w1,
                      const float* __restrict__ w2, const int32_t* __restrict__ wfold, typename S::T* out, int B, int R) {
  using T = typename S::T;
  __shared__ __attribute__((aligned(16))) Td32Lds<S> l;
  const int t = threadIdx.x, f = blockIdx.y;
  const auto ch = sq_children<S>(full, cst, rank1, kind, off, H, 32, f);
  const int64_t wf = static_cast<int64_t>(wfold[f]) * 1024;
  td32_stage_w<false>(w1 + wf, l.w[0], nullptr, t);
  td32_stage_w<false>(w2 + wf, l.w[1], nullptr, t);
  const int64_t b0 = static_cast<int64_t>(blockIdx.x) * R;
  const int64_t b1 = b0 + R < B ? b0 + R : B;
  for (int64_t b = b0; b < b1; ++b) {
    T x[4], y[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) x[r] = ch.load(b, t + 256 * r);
    td32_fwd_stage<S>(l, l.w[0], x, y, t);
    td32_fwd_stage<S>(l, l.w[1], y, x, t);  // (stage 1's (Kq, Kk1) block is stage 2's (Kj, Kq): element i of the one is element i of the other)
    T* o = out + (static_cast<int64_t>(f) * B + b) * 1024;
#pragma unroll
    for (int r = 0; r < 4; ++r) o[t + 256 * r] = x[r];
  }
}

// the root: 32 x 32 input units, ONE output unit in both stages (td32_root_fwd_kernel; the block between the stages stays in LDS)
template <class S>
__global__ void __launch_bounds__(256)
    sq_root32_kernel(const typename S::T* full, const typename S::T* __restrict__ cst, const typename S::T* __restrict__ rank1,
                     const int32_t* __restrict__ kind, const int64_t* __restrict__ off, int H, const float* __restrict__ w1,
                     const float* __restrict__ w2, const int32_t* __restrict__ wfold, typename S::T* out, int B) {
  using T = typename S::T;
  __shared__ __attribute__((aligned(16))) Td32Lds<S> l;
  const int t = threadIdx.x, f = blockIdx.y;
  const int64_t b = blockIdx.x;
  const auto ch = sq_children<S>(full, cst, rank1, kind, off, H, 32, f);
  T x[4], a[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) x[r] = ch.load(b, t + 256 * r);
  if (t < 32) {
    l.w[0][t] = w1[static_cast<int64_t>(wfold[f]) * 32 + t];
    l.w[1][t] = w2[static_cast<int64_t>(wfold[f]) * 32 + t];
  }
  td32_exp<S>(l, x, a, t);
  if (t >= 32) return;  // (no barrier below: wave 0 alone)
  T acc = S::zero();
#pragma unroll 8
  for (int j = 0; j < 32; ++j) acc = S::fma_w(l.w[0][j], l.a[t * S::kA + j], acc);
  const T o1 = S::log_shift(acc, l.m[t]);
  float m2 = S::re(o1);
#pragma unroll
  for (int s2 = 1; s2 < 32; s2 <<= 1) m2 = fmaxf(m2, __shfl_xor(m2, s2, 64));
  m2 = ck::clamp_finite(m2);
  l.t[t] = S::exp_shift(o1, m2);
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0): the wave's own LDS writes have landed
  __builtin_amdgcn_wave_barrier();
  if (t == 0) {
    T y2 = S::zero();
    for (int q = 0; q < 32; ++q) y2 = S::fma_w(l.w[1][q], l.t[q], y2);
    out[static_cast<int64_t>(f) * B + b] = S::log_shift(y2, m2);
  }
}

// any other shape: the two stages of td_fwd_kernel<S, true>, the block between them through `mid` (n, B, Ki Ko)
template <class S>
__global__ void __launch_bounds__(256)
    sq_mixed_kernel(const typename S::T* full, const typename S::T* __restrict__ cst, const typename S::T* __restrict__ rank1,
                    const int32_t* __restrict__ kind, const int64_t* __restrict__ off, int H, const float* __restrict__ w1,
                    const float* __restrict__ w2, const int32_t* __restrict__ wfold, typename S::T* mid, typename S::T* out, int B, int Ki,
                    int Ko) {
  using T = typename S::T;
  extern __shared__ __attribute__((aligned(16))) char sq_smem[];
  const int f = blockIdx.y;
  const int64_t b = blockIdx.x;
  const auto ch = sq_children<S>(full, cst, rank1, kind, off, H, Ki, f);
  const int64_t wf = static_cast<int64_t>(wfold[f]) * Ko * Ki;
  T* m1 = mid + (static_cast<int64_t>(f) * B + b) * Ki * Ko;
  td_fwd_body<S>(sq_smem, [&](int i) { return ch.load(b, i); }, w1 + wf, m1, Ki, Ki, Ko);
  __syncthreads();  // (the block between the stages: written and read by this workgroup only)
  const T* m1c = m1;
  td_fwd_body<S>(sq_smem, [&](int i) { return m1c[i]; }, w2 + wf, out + (static_cast<int64_t>(f) * B + b) * Ko * Ko, Ki, Ko, Ko);
}

template <class S, class S32>
int sq_launch(const typename S::T* full, const typename S::T* cst, const typename S::T* rank1, const int32_t* kind, const int64_t* off, int H,
              const float* w1, const float* w2, const int32_t* wfold, typename S::T* mid, typename S::T* out, int n, int B, int Ki, int Ko,
              int stages, int R, void* stream) {
  const char* who = "ck_squared_mixed_fwd";
  if (stages == 0)
    return ck::launch(sq_hadamard_kernel<S>, dim3(B, n), dim3(256), 0, stream, full, cst, rank1, kind, off, H, out, B, Ki);
  if (Ki == 32 && Ko == 32)
    return ck::launch(sq_mixed32_kernel<S32>, dim3((B + R - 1) / R, n), dim3(256), 0, stream, full, cst, rank1, kind, off, H, w1, w2, wfold, out,
                      B, R);
  if (Ki == 32 && Ko == 1)
    return ck::launch(sq_root32_kernel<S32>, dim3(B, n), dim3(256), 0, stream, full, cst, rank1, kind, off, H, w1, w2, wfold, out, B);
  CK_REQUIRE(mid, "%s: null pointer (mid: Ki=%d, Ko=%d take the shape-generic form)", who, Ki, Ko);
  const size_t lds = std::max(td_lds<S>(Ki, Ki, Ko, false), td_lds<S>(Ki, Ko, Ko, false));
  if (lds > 160 * 1024) return ck::fail(CK_ERR_UNSUPPORTED, "%s: Ki=%d, Ko=%d do not fit in LDS", who, Ki, Ko);
  const dim3 grid(B, n), block(256);
  return ck::dispatch(
      [=](hipStream_t s) {
        if (lds > 48 * 1024) {
          hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(sq_mixed_kernel<S>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                             static_cast<int>(lds));
          if (e != hipSuccess) return e;
        }
        hipLaunchKernelGGL(sq_mixed_kernel<S>, grid, block, lds, s, full, cst, rank1, kind, off, H, w1, w2, wfold, mid, out, B, Ki, Ko);
        return hipGetLastError();
      },
      stream);
}

}  // namespace

extern "C" int ck_squared_mixed_fwd(const float* full, const float* cst, const float* rank1, const int32_t* kind, const int64_t* off, int H,
                                    const float* w1, const float* w2, const int32_t* wfold, float* mid, float* out, int n, int B, int Ki,
                                    int Ko, int stages, int rows_per_block, int complex_values, void* stream) {
  const char* who = "ck_squared_mixed_fwd";
  CK_REQUIRE(kind && off && out, "%s: null pointer", who);
  CK_REQUIRE(stages == 0 || stages == 2, "%s: stages=%d (0: a Hadamard layer, 2: a sum / CP-T layer)", who, stages);
  CK_REQUIRE(stages == 0 || (w1 && w2 && wfold), "%s: null pointer", who);
  CK_REQUIRE(n > 0 && n <= 65535 && H > 0 && B > 0 && Ki > 0 && (stages == 0 || Ko > 0) && rows_per_block > 0, "%s: bad sizes", who);
  CK_REQUIRE(Ki <= 1024, "%s: Ki=%d", who, Ki);  // (Ki^2 element indices are 32-bit)
  if (complex_values)
    return sq_launch<TdC, TdC32>(reinterpret_cast<const c32*>(full), reinterpret_cast<const c32*>(cst), reinterpret_cast<const c32*>(rank1), kind,
                                 off, H, w1, w2, wfold, reinterpret_cast<c32*>(mid), reinterpret_cast<c32*>(out), n, B, Ki, Ko, stages,
                                 rows_per_block, stream);
  return sq_launch<TdR, TdR32>(full, cst, rank1, kind, off, H, w1, w2, wfold, mid, out, n, B, Ki, Ko, stages, rows_per_block, stream);
}
