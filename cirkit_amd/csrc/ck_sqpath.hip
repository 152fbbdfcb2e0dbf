// Sampling squared circuits p(x) = |c(x)|^2 / Z ("Sampling squared circuits"): the derivative of the root of
// the product circuit c (x) conj(c) with respect to the K^2 squared units of ONE input fold, walked from the root down the
// ancestors of that fold's variable v, then the marginal of v over ALL its states and, on request, a draw from it.
//
// The product circuit is multilinear in those K^2 units, so with every other variable observed or integrated out
//     m_b(s) = sum_kl G_b[k][l] a_k(s) conj(a_l(s)),
// a_k(s) the linear value of unit k of the input fold at state s (its table) and G_b the derivative for row b.  At a sum / CP-T
// fold the forward is O = W P W^T in linear space (ck_sqmar.hip: the two TensorDot stages, ck_td.h), so dP = W^T G W: the SAME
// two log-space stages with the weight matrix read transposed; the gradient of the child on the path is dP plus (log space) the
// values of the fold's other children, read by kind as ck_squared_mixed_fwd reads them (RANK-1 lifted from c's arena, CONST from
// the partition-function circuit's, FULL from this query's mixed arena).  The gradient block never goes to memory: registers
// between the levels of the 32-unit form, LDS in the shape-generic form.  The reference has no such query: it would evaluate
// integrate(multiply(c, conjugate(c)), scope=M) (symbolic/functional.py:161-258, :259-593) once per state.
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
// maximum over the units state by state.  Then, with a batch to draw into, the inverse CDF over the states.
template <class T>
__device__ __forceinline__ void sp_leaf(const SpArgs<T>& a, int64_t b, const float* e, float* av, float* lm, float* red, float gmax, int t) {
  const int K = a.K, C = a.C;
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

// any shape that fits in LDS: the gradient block lives in LDS, a workgroup walks R rows one after the other
template <class S>
__global__ void __launch_bounds__(256) sp_path_kernel(SpArgs<typename S::T> a) {
  using T = typename S::T;
  extern __shared__ __attribute__((aligned(16))) char sp_smem[];
  const int t = threadIdx.x, mk = a.maxK;
  T* ga = reinterpret_cast<T*>(sp_smem);
  T* gb = ga + mk * mk;
  T* a_s = gb + mk * mk;
  float* w_s = reinterpret_cast<float*>(a_s + mk * (mk + 1));
  float* m_s = w_s + mk * (mk + 1);
  float* red = m_s + mk;
  float* e = red + 4;
  float* av = e + a.K * a.K;
  float* lm = av + (a.C < kSpStates ? a.C : kSpStates) * (a.K + 1);
  const int stride = kSpHead + 2 * a.S;
  const int64_t b0 = static_cast<int64_t>(blockIdx.x) * a.R;
  const int64_t b1 = b0 + a.R < a.B ? b0 + a.R : a.B;
  for (int64_t b = b0; b < b1; ++b) {
    __syncthreads();  // (the previous row has left LDS)
    if (a.dead && a.dead[b]) {
      sp_dead_row(a, b, t);
      continue;
    }
    int Kc = a.L ? static_cast<int>(a.lev[3]) : a.K;
    for (int i = t; i < Kc * Kc; i += 256) ga[i] = sp_log_real<T>(i == 0 ? 0.f : -INFINITY);  // the root reads unit 0: G = log 1 there
    __syncthreads();
    for (int lv = 0; lv < a.L; ++lv) {
      const int64_t* le = a.lev + static_cast<int64_t>(lv) * stride;
      const int Ki = static_cast<int>(le[2]), Ko = static_cast<int>(le[3]);
      if (le[0] & CK_SQ_PATH_STAGES) {
        const int64_t wf = le[1] * Ko * Ki;
        sp_stage<S>(ga, gb, a_s, w_s, m_s, reinterpret_cast<const float*>(le[4]) + wf, Ko, Ko, Ki);
        sp_stage<S>(gb, ga, a_s, w_s, m_s, reinterpret_cast<const float*>(le[5]) + wf, Ko, Ki, Ki);
      }
      if (le[6])
        for (int i = t; i < Ki * Ki; i += 256) ga[i] = sp_siblings<S>(a, le, b, Ki, i, ga[i]);
      __syncthreads();
    }
    const int K2 = a.K * a.K;
    float gm = -INFINITY;
    for (int i = t; i < K2; i += 256) gm = fmaxf(gm, S::re(ga[i]));
    gm = ck::clamp_finite(sp_block_max(gm, red, t));
    for (int i = t; i < K2; i += 256) e[i] = S::re(S::exp_shift(ga[i], gm));
    sp_leaf(a, b, e, av, lm, red, gm, t);
  }
}

// 32 units on the whole path, ONE output unit at the root: thread t owns elements t + 256 r of every (32, 32) block, as in
// td32_fwd_stage; the weights of a level are staged transposed (td32_stage_w<true>) and the gradient stays in registers.
// A workgroup walks its R rows one after the other, root to leaf each, and stages every level's weights again for every row
// (8 KiB per level from L2, as much as one FULL sibling): R only changes the grid, it buys no reuse of the staged weights.
template <class S>
__global__ void __launch_bounds__(256) sp_path32_kernel(SpArgs<typename S::T> a) {
  using T = typename S::T;
  __shared__ __attribute__((aligned(16))) Td32Lds<S> l;
  extern __shared__ __attribute__((aligned(16))) char sp_smem[];
  const int t = threadIdx.x;
  float* e = reinterpret_cast<float*>(l.t);  // (the forward stages leave t / tt alone: 32 * kA values >= 1024 floats)
  float* av = reinterpret_cast<float*>(sp_smem);
  float* lm = av + (a.C < kSpStates ? a.C : kSpStates) * 33;
  const int stride = kSpHead + 2 * a.S;
  const int64_t b0 = static_cast<int64_t>(blockIdx.x) * a.R;
  const int64_t b1 = b0 + a.R < a.B ? b0 + a.R : a.B;
  for (int64_t b = b0; b < b1; ++b) {
    __syncthreads();  // (the previous row has left LDS)
    if (a.dead && a.dead[b]) {
      sp_dead_row(a, b, t);
      continue;
    }
    T x[4], y[4];
    {  // the root: G = log 1, dP[j][q] = log W1[0][j] + log W2[0][q]
      const int64_t wf = a.lev[1] * 32;
      if (t < 32) {
        l.w[0][t] = reinterpret_cast<const float*>(a.lev[4])[wf + t];
        l.w[1][t] = reinterpret_cast<const float*>(a.lev[5])[wf + t];
      }
      __syncthreads();
      const T one = S::exp_shift(sp_log_real<T>(0.f), 0.f);
      const T lq = S::log_shift(S::fma_w(l.w[1][t & 31], one, S::zero()), 0.f);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        x[r] = S::add(S::log_shift(S::fma_w(l.w[0][(t >> 5) + 8 * r], one, S::zero()), 0.f), lq);
        if (a.lev[6]) x[r] = sp_siblings<S>(a, a.lev, b, 32, t + 256 * r, x[r]);
      }
    }
    for (int lv = 1; lv < a.L; ++lv) {
      const int64_t* le = a.lev + static_cast<int64_t>(lv) * stride;
      if (le[0] & CK_SQ_PATH_STAGES) {
        __syncthreads();  // (the level above has read its weights)
        const int64_t wf = le[1] * 1024;
        td32_stage_w<true>(reinterpret_cast<const float*>(le[4]) + wf, l.w[0], l.wt[0], t);
        td32_stage_w<true>(reinterpret_cast<const float*>(le[5]) + wf, l.w[1], l.wt[1], t);
        td32_fwd_stage<S>(l, l.wt[0], x, y, t);
        td32_fwd_stage<S>(l, l.wt[1], y, x, t);
      }
      if (le[6]) {
#pragma unroll
        for (int r = 0; r < 4; ++r) x[r] = sp_siblings<S>(a, le, b, 32, t + 256 * r, x[r]);
      }
    }
    float gm = fmaxf(fmaxf(S::re(x[0]), S::re(x[1])), fmaxf(S::re(x[2]), S::re(x[3])));
    gm = ck::clamp_finite(sp_block_max(gm, l.red[0], t));
#pragma unroll
    for (int r = 0; r < 4; ++r) e[t + 256 * r] = S::re(S::exp_shift(x[r], gm));
    sp_leaf(a, b, e, av, lm, l.red[1], gm, t);
  }
}

// `Kernel` needs its dynamic-LDS limit raised once per device, not once per step of a 784-step sample
template <auto Kernel, class A>
int sp_dispatch(const A& a, size_t lds, size_t fixed, void* stream) {
  static size_t raised[64] = {};  // per device: the largest dynamic size the limit was raised to
  const dim3 grid((a.B + a.R - 1) / a.R), block(256);
  return ck::dispatch(
      [=](hipStream_t s) {
        if (lds + fixed > 48 * 1024) {
          int dev = 0;
          hipError_t er = hipGetDevice(&dev);
          if (er != hipSuccess) return er;
          if (dev < 0 || dev >= 64 || lds > raised[dev]) {
            er = hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds));
            if (er != hipSuccess) return er;
            if (dev >= 0 && dev < 64) raised[dev] = lds;
          }
        }
        hipLaunchKernelGGL(Kernel, grid, block, lds, s, a);
        return hipGetLastError();
      },
      stream);
}

template <class S, class S32>
int sp_launch(const SpArgs<typename S::T>& a, bool all32, void* stream) {
  using T = typename S::T;
  const char* who = "ck_squared_path_bwd";
  if (all32) {
    const size_t lds = sp_leaf_floats(a.C, 32) * sizeof(float);
    if (lds + sizeof(Td32Lds<S32>) > 160 * 1024) return ck::fail(CK_ERR_UNSUPPORTED, "%s: C=%d states do not fit in LDS", who, a.C);
    return sp_dispatch<sp_path32_kernel<S32>>(a, lds, sizeof(Td32Lds<S32>), stream);
  }
  const int mk = a.maxK;
  const size_t lds = sp_value_words<T>(mk) * sizeof(T) +
                     (static_cast<size_t>(mk) * (mk + 1) + mk + 4 + static_cast<size_t>(a.K) * a.K + sp_leaf_floats(a.C, a.K)) * sizeof(float);
  if (lds > 160 * 1024) return ck::fail(CK_ERR_UNSUPPORTED, "%s: %d units, C=%d states do not fit in LDS", who, mk, a.C);
  return sp_dispatch<sp_path_kernel<S>>(a, lds, 0, stream);
}

}  // namespace

extern "C" int ck_squared_path_bwd(const float* full, const float* cst, const float* rank1, const int64_t* levels_host, const int64_t* levels,
                                   int L, int max_siblings, const float* table, int64_t leaf_fold, int C, int K, int table_log, float* log_m,
                                   int64_t* x, int64_t* x_out, int32_t* dead, int D, int var, int node, uint64_t seed, int64_t row0, int B,
                                   int rows_per_block, int complex_values, void* stream) {
  const char* who = "ck_squared_path_bwd";
  CK_REQUIRE(table && (log_m || x_out), "%s: null pointer", who);
  CK_REQUIRE(L == 0 || (levels_host && levels), "%s: null pointer (levels)", who);
  CK_REQUIRE(!x_out || (x && dead), "%s: null pointer (a draw needs x, x_out and dead)", who);
  CK_REQUIRE(L >= 0 && max_siblings >= 0 && B > 0 && C > 0 && K > 0 && rows_per_block > 0 && leaf_fold >= 0, "%s: bad sizes", who);
  CK_REQUIRE(K <= 1024, "%s: K=%d", who, K);  // (K^2 element indices are 32-bit)
  CK_REQUIRE(!x_out || (D > 0 && var >= 0 && var < D && node >= 0), "%s: var=%d, D=%d, node=%d", who, var, D, node);
  // the path as the host knows it: shapes chain from the root's units to the leaf's, every child kind is one of the three
  const int stride = kSpHead + 2 * max_siblings;
  int Kc = L ? static_cast<int>(levels_host[3]) : K, maxK = std::max(K, Kc);
  bool all32 = K == 32 && L >= 1;
  for (int lv = 0; lv < L; ++lv) {
    const int64_t* le = levels_host + static_cast<int64_t>(lv) * stride;
    const bool st = (le[0] & CK_SQ_PATH_STAGES) != 0;
    CK_REQUIRE(le[2] > 0 && le[2] <= 1024 && le[3] == Kc && (st || le[2] == le[3]), "%s: level %d: Ki=%lld, Ko=%lld under %d units", who, lv,
               static_cast<long long>(le[2]), static_cast<long long>(le[3]), Kc);
    CK_REQUIRE(!st || (le[1] >= 0 && le[4] && le[5]), "%s: level %d: weights", who, lv);
    CK_REQUIRE(le[6] >= 0 && le[6] <= max_siblings, "%s: level %d: %lld siblings, room for %d", who, lv, static_cast<long long>(le[6]),
               max_siblings);
    for (int h = 0; h < le[6]; ++h) {
      const int64_t kd = le[kSpHead + 2 * h];
      CK_REQUIRE(kd == CK_SQ_FULL || kd == CK_SQ_CONST || kd == CK_SQ_RANK1, "%s: level %d: child kind %lld", who, lv, static_cast<long long>(kd));
      CK_REQUIRE(le[kSpHead + 2 * h + 1] >= 0 && (kd == CK_SQ_FULL ? full : kd == CK_SQ_CONST ? cst : rank1) != nullptr,
                 "%s: level %d: null pointer or negative offset of a child", who, lv);
    }
    Kc = static_cast<int>(le[2]);
    maxK = std::max(maxK, Kc);
    all32 = all32 && Kc == 32 && (lv > 0 || (st && le[3] == 1));
  }
  CK_REQUIRE(Kc == K, "%s: the path ends on %d units, the input fold has %d", who, Kc, K);
  const float* tab = table + leaf_fold * (static_cast<int64_t>(C) + 1) * K;
  const auto args = [&](auto* f, auto* c, auto* r) {
    using T = std::remove_cv_t<std::remove_pointer_t<decltype(f)>>;
    return SpArgs<T>{f, c, r, levels, L, max_siblings, tab, C, K, table_log, log_m, x_out ? x : nullptr, x_out, dead, D, var,
                     static_cast<uint32_t>(node), static_cast<uint32_t>(seed), static_cast<uint32_t>(seed >> 32), row0, B, rows_per_block, maxK};
  };
  if (complex_values)
    return sp_launch<TdC, TdC32>(args(reinterpret_cast<const c32*>(full), reinterpret_cast<const c32*>(cst), reinterpret_cast<const c32*>(rank1)),
                                 all32, stream);
  return sp_launch<TdR, TdR32>(args(full, cst, rank1), all32, stream);
}
