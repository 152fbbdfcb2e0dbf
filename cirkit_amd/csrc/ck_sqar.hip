// Autoregressive conditionals of squared circuits p(x) = |c(x)|^2 / Z ("Autoregressive conditionals and
// coding of squared circuits"): log p(X_{o_i} = s | x_{o_0 .. o_{i-1}}) for MANY steps i of an order o of the variables, on rows
// that are known in full (teacher forcing, encoding, a bits-per-dimension map).  Step i is the walk of ck_sqpath.hip down the
// ancestors of o_i with the earlier variables observed and the later ones integrated out.  Where every sibling of the path is
// entirely before or entirely after o_i (tree_order: RANK-1 from c's arena on the COMPLETE row, CONST from the partition-function
// circuit) nothing a step reads depends on the step, so ONE forward of c serves all of them and all (row, step) pairs go into one
// launch: blockIdx.y is the step, blockIdx.x a tile of rows.  A workgroup reads its step's level table and leaf words and then
// walks exactly as sp_path_kernel / sp_path32_kernel do, with the same device functions in the same order: log m is theirs bit
// for bit.  The leaf epilogue adds what the chain rule needs: the normalisation over the states and the pick at x[b, var].
#include "ck_sqpath.h"

namespace {

constexpr int kSsLeaf = CK_SQ_STEP_LEAF_WORDS;

template <class T>
struct SsArgs {
  const T* full;
  const T* cst;
  const T* rank1;
  const int64_t* lev;   // [steps][step_stride] words: the level tables of ck_squared_path_bwd, stacked
  const int64_t* leaf;  // [steps][kSsLeaf]
  int64_t step_stride;
  int S, step0;
  const int64_t* x;  // (B, D), read only
  int D;
  const int32_t* bad;  // (B,) rows that are NaN throughout, or null
  float* log_m;        // [b lm_row + j lm_step + s], s < Cmax; or null
  float* cond;
  float* log_prob;  // [b lp_row + j lp_step]; or null
  int64_t lm_row, lm_step, cd_row, cd_step, lp_row, lp_step;
  int Cmax, B, R, maxK;  // maxK: the most units of any level of any step of the launch
};

// the sum over the workgroup in a fixed order; `red`: 4 floats nobody else is reading
__device__ __forceinline__ float ss_block_sum(float v, float* red, int t) {
#pragma unroll
  for (int s = 1; s < 64; s <<= 1) v += __shfl_xor(v, s, 64);
  __syncthreads();
  if ((t & 63) == 0) red[t >> 6] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

// the step of this workgroup as the path kernels see one launch; whether it takes the 32-unit form (sp_entry's rule)
template <class T>
__device__ __forceinline__ SpArgs<T> ss_step(const SsArgs<T>& a, int step, bool* all32) {
  const int64_t* lf = a.leaf + static_cast<int64_t>(step) * kSsLeaf;
  const int64_t* lev = a.lev + static_cast<int64_t>(step) * a.step_stride;
  const int C = static_cast<int>(lf[2]), K = static_cast<int>(lf[3]), L = static_cast<int>(lf[6]);
  const int stride = kSpHead + 2 * a.S;
  bool f = K == 32 && L >= 1;
  for (int lv = 0; lv < L && f; ++lv) {
    const int64_t* le = lev + static_cast<int64_t>(lv) * stride;
    f = le[2] == 32 && (lv > 0 || ((le[0] & CK_SQ_PATH_STAGES) && le[3] == 1));
  }
  *all32 = f;
  return SpArgs<T>{a.full, a.cst, a.rank1, lev, L, a.S,
                   reinterpret_cast<const float*>(lf[0]) + lf[1] * (static_cast<int64_t>(C) + 1) * K, C, K, static_cast<int>(lf[4]),
                   nullptr, nullptr, nullptr, nullptr, a.D, static_cast<int>(lf[5]), 0u, 0u, 0u, 0, a.B, a.R, a.maxK, nullptr, 0};
}

// a row that is NaN throughout
template <class T>
__device__ __forceinline__ void ss_bad_row(const SsArgs<T>& a, int64_t b, int j, int t) {
  const float nan = __int_as_float(0x7fc00000);
  for (int s = t; s < a.Cmax; s += 256) {
    if (a.log_m) a.log_m[b * a.lm_row + j * a.lm_step + s] = nan;
    if (a.cond) a.cond[b * a.cd_row + j * a.cd_step + s] = nan;
  }
  if (a.log_prob && t == 0) a.log_prob[b * a.lp_row + j * a.lp_step] = nan;
}

// behind sp_leaf: lm holds log m of the C states.  log m as it is, log m - lse_s log m, and that at the row's own state; the
// columns past C are -inf.  A row without mass (every state -inf) is NaN where it is normalised.
template <class T>
__device__ __forceinline__ void ss_epilogue(const SsArgs<T>& a, const SpArgs<T>& sa, int64_t b, int j, const float* lm, float* red, int t) {
  const int C = sa.C;
  if (a.log_m)
    for (int s = t; s < a.Cmax; s += 256) a.log_m[b * a.lm_row + j * a.lm_step + s] = s < C ? lm[s] : -INFINITY;
  if (!a.cond && !a.log_prob) return;
  float mx = -INFINITY;
  for (int s = t; s < C; s += 256) mx = fmaxf(mx, lm[s]);
  mx = ck::clamp_finite(sp_block_max(mx, red, t));
  float sum = 0.f;
  for (int s = t; s < C; s += 256) sum += expf(lm[s] - mx);
  const float lse = logf(ss_block_sum(sum, red, t)) + mx;
  if (a.cond)
    for (int s = t; s < a.Cmax; s += 256) a.cond[b * a.cd_row + j * a.cd_step + s] = s < C ? lm[s] - lse : -INFINITY;
  if (a.log_prob && t == 0) {
    const int64_t xv = a.x[b * a.D + sa.var];
    a.log_prob[b * a.lp_row + j * a.lp_step] = (xv >= 0 && xv < C) ? lm[xv] - lse : __int_as_float(0x7fc00000);
  }
}

// the steps of any shape that fits in LDS: sp_path_kernel's walk, the LDS carved for the largest step of the launch
template <class S>
__global__ void __launch_bounds__(256) ss_steps_kernel(SsArgs<typename S::T> a) {
  using T = typename S::T;
  extern __shared__ __attribute__((aligned(16))) char sp_smem[];
  const int t = threadIdx.x, mk = a.maxK, j = blockIdx.y;
  bool all32;
  const SpArgs<T> sa = ss_step(a, a.step0 + j, &all32);
  if (all32) return;  // (the 32-unit launch has this step)
  T* ga = reinterpret_cast<T*>(sp_smem);
  T* gb = ga + mk * mk;
  T* a_s = gb + mk * mk;
  float* w_s = reinterpret_cast<float*>(a_s + mk * (mk + 1));
  float* m_s = w_s + mk * (mk + 1);
  float* red = m_s + mk;
  float* e = red + 4;
  float* av = e + mk * mk;
  float* lm = av + (a.Cmax < kSpStates ? a.Cmax : kSpStates) * (mk + 1);
  const int stride = kSpHead + 2 * sa.S;
  const int64_t b0 = static_cast<int64_t>(blockIdx.x) * a.R;
  const int64_t b1 = b0 + a.R < a.B ? b0 + a.R : a.B;
  for (int64_t b = b0; b < b1; ++b) {
    __syncthreads();  // (the previous row has left LDS)
    if (a.bad && a.bad[b]) {
      ss_bad_row(a, b, j, t);
      continue;
    }
    int Kc = sa.L ? static_cast<int>(sa.lev[3]) : sa.K;
    for (int i = t; i < Kc * Kc; i += 256) ga[i] = sp_log_real<T>(i == 0 ? 0.f : -INFINITY);  // the root reads unit 0: G = log 1 there
    __syncthreads();
    for (int lv = 0; lv < sa.L; ++lv) {
      const int64_t* le = sa.lev + static_cast<int64_t>(lv) * stride;
      const int Ki = static_cast<int>(le[2]), Ko = static_cast<int>(le[3]);
      if (le[0] & CK_SQ_PATH_STAGES) {
        const int64_t wf = le[1] * Ko * Ki;
        sp_stage<S>(ga, gb, a_s, w_s, m_s, reinterpret_cast<const float*>(le[4]) + wf, Ko, Ko, Ki);
        sp_stage<S>(gb, ga, a_s, w_s, m_s, reinterpret_cast<const float*>(le[5]) + wf, Ko, Ki, Ki);
      }
      if (le[6])
        for (int i = t; i < Ki * Ki; i += 256) ga[i] = sp_siblings<S>(sa, le, b, Ki, i, ga[i]);
      __syncthreads();
    }
    const int K2 = sa.K * sa.K;
    float gm = -INFINITY;
    for (int i = t; i < K2; i += 256) gm = fmaxf(gm, S::re(ga[i]));
    gm = ck::clamp_finite(sp_block_max(gm, red, t));
    for (int i = t; i < K2; i += 256) e[i] = S::re(S::exp_shift(ga[i], gm));
    sp_leaf(sa, b, e, av, lm, red, gm, t);
    ss_epilogue(a, sa, b, j, lm, red, t);
  }
}

// the steps with 32 units on the whole path and ONE output unit at the root: sp_path32_kernel's walk, the gradient in registers
template <class S>
__global__ void __launch_bounds__(256) ss_steps32_kernel(SsArgs<typename S::T> a) {
  using T = typename S::T;
  __shared__ __attribute__((aligned(16))) Td32Lds<S> l;
  extern __shared__ __attribute__((aligned(16))) char sp_smem[];
  const int t = threadIdx.x, j = blockIdx.y;
  bool all32;
  const SpArgs<T> sa = ss_step(a, a.step0 + j, &all32);
  if (!all32) return;  // (the shape-generic launch has this step)
  float* e = reinterpret_cast<float*>(l.t);  // (the forward stages leave t / tt alone: 32 * kA values >= 1024 floats)
  float* av = reinterpret_cast<float*>(sp_smem);
  float* lm = av + (a.Cmax < kSpStates ? a.Cmax : kSpStates) * 33;
  const int stride = kSpHead + 2 * sa.S;
  const int64_t b0 = static_cast<int64_t>(blockIdx.x) * a.R;
  const int64_t b1 = b0 + a.R < a.B ? b0 + a.R : a.B;
  for (int64_t b = b0; b < b1; ++b) {
    __syncthreads();  // (the previous row has left LDS)
    if (a.bad && a.bad[b]) {
      ss_bad_row(a, b, j, t);
      continue;
    }
    T x[4], y[4];
    {  // the root: G = log 1, dP[j][q] = log W1[0][j] + log W2[0][q]
      const int64_t wf = sa.lev[1] * 32;
      if (t < 32) {
        l.w[0][t] = reinterpret_cast<const float*>(sa.lev[4])[wf + t];
        l.w[1][t] = reinterpret_cast<const float*>(sa.lev[5])[wf + t];
      }
      __syncthreads();
      const T one = S::exp_shift(sp_log_real<T>(0.f), 0.f);
      const T lq = S::log_shift(S::fma_w(l.w[1][t & 31], one, S::zero()), 0.f);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        x[r] = S::add(S::log_shift(S::fma_w(l.w[0][(t >> 5) + 8 * r], one, S::zero()), 0.f), lq);
        if (sa.lev[6]) x[r] = sp_siblings<S>(sa, sa.lev, b, 32, t + 256 * r, x[r]);
      }
    }
    for (int lv = 1; lv < sa.L; ++lv) {
      const int64_t* le = sa.lev + static_cast<int64_t>(lv) * stride;
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
        for (int r = 0; r < 4; ++r) x[r] = sp_siblings<S>(sa, le, b, 32, t + 256 * r, x[r]);
      }
    }
    float gm = fmaxf(fmaxf(S::re(x[0]), S::re(x[1])), fmaxf(S::re(x[2]), S::re(x[3])));
    gm = ck::clamp_finite(sp_block_max(gm, l.red[0], t));
#pragma unroll
    for (int r = 0; r < 4; ++r) e[t + 256 * r] = S::re(S::exp_shift(x[r], gm));
    sp_leaf(sa, b, e, av, lm, l.red[1], gm, t);
    ss_epilogue(a, sa, b, j, lm, l.red[1], t);
  }
}

template <auto Kernel, class A>
int ss_dispatch(const A& a, int steps, size_t lds, size_t fixed, void* stream) {
  const dim3 grid((a.B + a.R - 1) / a.R, steps), block(256);
  return ck::dispatch(
      [=](hipStream_t s) {
        const hipError_t er = sp_raise_lds<Kernel>(lds, fixed);
        if (er != hipSuccess) return er;
        hipLaunchKernelGGL(Kernel, grid, block, lds, s, a);
        return hipGetLastError();
      },
      stream);
}

// one launch per form that any step of the range takes; a workgroup whose step takes the other form returns at once
template <class S, class S32>
int ss_launch(const SsArgs<typename S::T>& a, int steps, bool any32, bool any_generic, int maxK_generic, const char* who, void* stream) {
  using T = typename S::T;
  if (any32) {
    const size_t lds = sp_leaf_floats(a.Cmax, 32) * sizeof(float);
    if (lds + sizeof(Td32Lds<S32>) > 160 * 1024) return ck::fail(CK_ERR_UNSUPPORTED, "%s: C=%d states do not fit in LDS", who, a.Cmax);
    const int st = ss_dispatch<ss_steps32_kernel<S32>>(a, steps, lds, sizeof(Td32Lds<S32>), stream);
    if (st != 0) return st;
  }
  if (any_generic) {
    SsArgs<T> g = a;
    const int mk = g.maxK = maxK_generic;
    const size_t lds = sp_value_words<T>(mk) * sizeof(T) +
                       (static_cast<size_t>(mk) * (mk + 1) + mk + 4 + static_cast<size_t>(mk) * mk + sp_leaf_floats(a.Cmax, mk)) * sizeof(float);
    if (lds > 160 * 1024) return ck::fail(CK_ERR_UNSUPPORTED, "%s: %d units, C=%d states do not fit in LDS", who, mk, a.Cmax);
    return ss_dispatch<ss_steps_kernel<S>>(g, steps, lds, 0, stream);
  }
  return 0;
}

}  // namespace

extern "C" int ck_squared_path_steps(const float* full, const float* cst, const float* rank1, const int64_t* levels_host, const int64_t* levels,
                                     int64_t step_stride, int max_siblings, const int64_t* leaf_host, const int64_t* leaf, int step0,
                                     int num_steps, const int64_t* x, int D, const int32_t* bad, float* log_m, int64_t lm_row,
                                     int64_t lm_step, float* cond, int64_t cd_row, int64_t cd_step, float* log_prob, int64_t lp_row,
                                     int64_t lp_step, int C_max, int B, int rows_per_block, int complex_values, void* stream) {
  const char* who = "ck_squared_path_steps";
  CK_REQUIRE(levels_host && levels && leaf_host && leaf && x, "%s: null pointer", who);
  CK_REQUIRE(log_m || cond || log_prob, "%s: null pointer (no output)", who);
  CK_REQUIRE(step0 >= 0 && num_steps > 0 && num_steps <= 65535 && max_siblings >= 0 && B > 0 && D > 0 && C_max > 0 && rows_per_block > 0,
             "%s: bad sizes", who);
  const int stride = kSpHead + 2 * max_siblings;
  CK_REQUIRE(step_stride >= stride, "%s: a step of %lld words, a level of %d", who, static_cast<long long>(step_stride), stride);
  CK_REQUIRE((!log_m || (lm_step >= C_max && lm_row >= lm_step * num_steps)) && (!cond || (cd_step >= C_max && cd_row >= cd_step * num_steps)) &&
                 (!log_prob || (lp_step >= 1 && lp_row >= lp_step * num_steps)),
             "%s: output strides", who);
  // every step's path as the host knows it, checked as ck_squared_path_bwd checks its one path
  bool any32 = false, any_generic = false;
  int maxK_generic = 1;
  for (int j = 0; j < num_steps; ++j) {
    const int64_t si = static_cast<int64_t>(step0) + j;
    const int64_t* lf = leaf_host + si * kSsLeaf;
    const int64_t* lev = levels_host + si * step_stride;
    CK_REQUIRE(lf[0] != 0 && lf[1] >= 0 && lf[2] > 0 && lf[2] <= C_max && lf[3] > 0 && lf[3] <= 1024 && (lf[4] == 0 || lf[4] == 1) &&
                   lf[5] >= 0 && lf[5] < D && lf[6] >= 0 && lf[6] * stride <= step_stride,
               "%s: step %lld: leaf words", who, static_cast<long long>(si));
    const int K = static_cast<int>(lf[3]), L = static_cast<int>(lf[6]);
    int Kc = L ? static_cast<int>(lev[3]) : K, maxK = std::max(K, Kc);
    bool all32 = K == 32 && L >= 1;
    for (int lv = 0; lv < L; ++lv) {
      const int64_t* le = lev + static_cast<int64_t>(lv) * stride;
      const bool st = (le[0] & CK_SQ_PATH_STAGES) != 0;
      CK_REQUIRE(le[2] > 0 && le[2] <= 1024 && le[3] == Kc && (st || le[2] == le[3]), "%s: step %lld, level %d: Ki=%lld, Ko=%lld under %d units",
                 who, static_cast<long long>(si), lv, static_cast<long long>(le[2]), static_cast<long long>(le[3]), Kc);
      CK_REQUIRE(!st || (le[1] >= 0 && le[4] && le[5]), "%s: step %lld, level %d: weights", who, static_cast<long long>(si), lv);
      CK_REQUIRE(le[6] >= 0 && le[6] <= max_siblings, "%s: step %lld, level %d: %lld siblings, room for %d", who, static_cast<long long>(si), lv,
                 static_cast<long long>(le[6]), max_siblings);
      for (int h = 0; h < le[6]; ++h) {
        const int64_t kd = le[kSpHead + 2 * h];
        CK_REQUIRE(kd == CK_SQ_FULL || kd == CK_SQ_CONST || kd == CK_SQ_RANK1, "%s: step %lld, level %d: child kind %lld", who,
                   static_cast<long long>(si), lv, static_cast<long long>(kd));
        CK_REQUIRE(le[kSpHead + 2 * h + 1] >= 0 && (kd == CK_SQ_FULL ? full : kd == CK_SQ_CONST ? cst : rank1) != nullptr,
                   "%s: step %lld, level %d: null pointer or negative offset of a child", who, static_cast<long long>(si), lv);
      }
      Kc = static_cast<int>(le[2]);
      maxK = std::max(maxK, Kc);
      all32 = all32 && Kc == 32 && (lv > 0 || (st && le[3] == 1));
    }
    CK_REQUIRE(Kc == K, "%s: step %lld: the path ends on %d units, the input fold has %d", who, static_cast<long long>(si), Kc, K);
    if (all32) {
      any32 = true;
    } else {
      any_generic = true;
      maxK_generic = std::max(maxK_generic, maxK);
    }
  }
  const auto args = [&](auto* f, auto* c, auto* r) {
    using T = std::remove_cv_t<std::remove_pointer_t<decltype(f)>>;
    return SsArgs<T>{f, c, r, levels, leaf, step_stride, max_siblings, step0, x, D, bad, log_m, cond, log_prob,
                     lm_row, lm_step, cd_row, cd_step, lp_row, lp_step, C_max, B, rows_per_block, 32};
  };
  if (complex_values)
    return ss_launch<TdC, TdC32>(args(reinterpret_cast<const c32*>(full), reinterpret_cast<const c32*>(cst), reinterpret_cast<const c32*>(rank1)),
                                 num_steps, any32, any_generic, maxK_generic, who, stream);
  return ss_launch<TdR, TdR32>(args(full, cst, rank1), num_steps, any32, any_generic, maxK_generic, who, stream);
}
