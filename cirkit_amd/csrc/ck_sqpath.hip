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
#include "ck_sqpath.h"

namespace {

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

template <auto Kernel, class A>
int sp_dispatch(const A& a, size_t lds, size_t fixed, void* stream) {
  const dim3 grid((a.B + a.R - 1) / a.R), block(256);
  return ck::dispatch(
      [=](hipStream_t s) {
        const hipError_t er = sp_raise_lds<Kernel>(lds, fixed);
        if (er != hipSuccess) return er;
        hipLaunchKernelGGL(Kernel, grid, block, lds, s, a);
        return hipGetLastError();
      },
      stream);
}

template <class S, class S32>
int sp_launch(const SpArgs<typename S::T>& a, bool all32, const char* who, void* stream) {
  using T = typename S::T;
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

// what both entries do; lam: the log weights of the variable's own states, row b at lam + b lam_row, or null
int sp_entry(const char* who, const float* full, const float* cst, const float* rank1, const int64_t* levels_host, const int64_t* levels,
             int L, int max_siblings, const float* table, int64_t leaf_fold, int C, int K, int table_log, const float* lam,
             int64_t lam_row, float* log_m, int64_t* x, int64_t* x_out, int32_t* dead, int D, int var, int node, uint64_t seed,
             int64_t row0, int B, int rows_per_block, int complex_values, void* stream) {
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
                     static_cast<uint32_t>(node), static_cast<uint32_t>(seed), static_cast<uint32_t>(seed >> 32), row0, B, rows_per_block, maxK,
                     lam, lam_row};
  };
  if (complex_values)
    return sp_launch<TdC, TdC32>(args(reinterpret_cast<const c32*>(full), reinterpret_cast<const c32*>(cst), reinterpret_cast<const c32*>(rank1)),
                                 all32, who, stream);
  return sp_launch<TdR, TdR32>(args(full, cst, rank1), all32, who, stream);
}

}  // namespace

extern "C" int ck_squared_path_bwd(const float* full, const float* cst, const float* rank1, const int64_t* levels_host, const int64_t* levels,
                                   int L, int max_siblings, const float* table, int64_t leaf_fold, int C, int K, int table_log, float* log_m,
                                   int64_t* x, int64_t* x_out, int32_t* dead, int D, int var, int node, uint64_t seed, int64_t row0, int B,
                                   int rows_per_block, int complex_values, void* stream) {
  return sp_entry("ck_squared_path_bwd", full, cst, rank1, levels_host, levels, L, max_siblings, table, leaf_fold, C, K, table_log, nullptr, 0,
                  log_m, x, x_out, dead, D, var, node, seed, row0, B, rows_per_block, complex_values, stream);
}

// the same walk under soft evidence: the variable's own log weights log_lik[b, pos, :] are added to log m before it is written and drawn from
extern "C" int ck_squared_path_soft_bwd(const float* full, const float* cst, const float* rank1, const int64_t* levels_host,
                                        const int64_t* levels, int L, int max_siblings, const float* table, int64_t leaf_fold, int C, int K,
                                        int table_log, const float* log_lik, int S, int C_lik, int pos, float* log_m, int64_t* x,
                                        int64_t* x_out, int32_t* dead, int D, int var, int node, uint64_t seed, int64_t row0, int B,
                                        int rows_per_block, int complex_values, void* stream) {
  const char* who = "ck_squared_path_soft_bwd";
  CK_REQUIRE(log_lik, "%s: null pointer (log_lik)", who);
  CK_REQUIRE(S > 0 && pos >= 0 && pos < S && C_lik >= C, "%s: position %d of %d, log_lik has %d states, the variable %d", who, pos, S, C_lik, C);
  return sp_entry(who, full, cst, rank1, levels_host, levels, L, max_siblings, table, leaf_fold, C, K, table_log,
                  log_lik + static_cast<int64_t>(pos) * C_lik, static_cast<int64_t>(S) * C_lik, log_m, x, x_out, dead, D, var, node, seed, row0,
                  B, rows_per_block, complex_values, stream);
}
