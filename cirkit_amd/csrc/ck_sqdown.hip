// Posterior marginals of squared circuits p(x) = |c(x)|^2 / Z ("Posterior marginals of squared circuits"):
// the walk of ck_sqpath.hip in its layer-wise form.  For a set Q of query variables the derivative G of the root of the product
// circuit c (x) conj(c) is kept for EVERY fold whose scope meets Q (the down folds): one launch per layer of c that has any, from
// the output layer downwards, reads a fold's G (Ko^2 values per row in the down arena; the output fold: log 1 at unit 0), applies
// the two transposed log-space stages where the layer has them (dP = W^T G W, sp_stage / td32_fwd_stage as the path kernels do)
// and writes, for every child slot h that is a down fold itself,
//     G_child = dP (+) sum over h' != h of value(h')        (log space; the OTHER children read by kind, sp_siblings),
// never the total minus the child's own value: -inf and signed cancellation break that.  A last launch evaluates all C states
// of every query variable from the G of its input fold (sp_leaf).  Every sibling is read at its value with Q and the other
// integrated variables integrated out, so column s of variable v is log_marginal of the row with x_v = s and the rest of Q
// integrated: what ck_squared_path_bwd gives for one variable, here for all of them with the ancestors shared.
#include "ck_sqpath.h"

namespace {

constexpr int kSdHead = CK_SQ_DOWN_FOLD_WORDS;  // int64 words of a fold in front of its child (gout, kind, offset) triples
constexpr int kSdMaxH = 8;                      // children of a fold
constexpr int kSdLeaf = CK_SQ_DOWN_LEAF_WORDS;

template <class T>
struct SdArgs {
  SpArgs<T> sp;        // full, cst, rank1: what sp_siblings reads
  T* down;             // the down arena
  const int64_t* tab;  // [n][kSdHead + 3 H]
  const float* w1;
  const float* w2;
  int n, H, Ki, Ko, stages, B, R, maxK;
};

// the level row sp_siblings reads, for the child in slot h: every other slot's (kind, offset), in slot order
__device__ __forceinline__ void sd_others(int64_t* lev_s, const int64_t* row, int H, int h, int t) {
  __syncthreads();  // (the previous slot's readers are done)
  if (t == 0) {
    int n = 0;
    for (int g = 0; g < H; ++g) {
      if (g == h) continue;
      lev_s[kSpHead + 2 * n] = row[kSdHead + 3 * g + 1];
      lev_s[kSpHead + 2 * n + 1] = row[kSdHead + 3 * g + 2];
      ++n;
    }
    lev_s[6] = n;
  }
  __syncthreads();
}

// any shape that fits in LDS: the blocks live in LDS as in sp_path_kernel; a workgroup takes one fold and R rows one after the other
template <class S>
__global__ void __launch_bounds__(256) sd_down_kernel(SdArgs<typename S::T> a) {
  using T = typename S::T;
  extern __shared__ __attribute__((aligned(16))) char sd_smem[];
  __shared__ int64_t lev_s[kSpHead + 2 * kSdMaxH];
  const int t = threadIdx.x, mk = a.maxK, Ki = a.Ki, Ko = a.Ko;
  T* ga = reinterpret_cast<T*>(sd_smem);
  T* gb = ga + mk * mk;
  T* a_s = gb + mk * mk;
  float* w_s = reinterpret_cast<float*>(a_s + mk * (mk + 1));
  float* m_s = w_s + mk * (mk + 1);
  const int nb = (a.B + a.R - 1) / a.R;
  const int f = blockIdx.x / nb;
  const int64_t* row = a.tab + static_cast<int64_t>(f) * (kSdHead + 3 * a.H);
  const int64_t wf = row[0] * Ko * Ki, gin = row[1];
  const int64_t b0 = static_cast<int64_t>(blockIdx.x - f * nb) * a.R;
  const int64_t b1 = b0 + a.R < a.B ? b0 + a.R : a.B;
  for (int64_t b = b0; b < b1; ++b) {
    __syncthreads();  // (the previous row has left LDS)
    for (int i = t; i < Ko * Ko; i += 256)  // the output fold is read at unit 0: G = log 1 there
      ga[i] = gin < 0 ? sp_log_real<T>(i == 0 ? 0.f : -INFINITY) : a.down[gin + b * Ko * Ko + i];
    __syncthreads();
    if (a.stages) {
      sp_stage<S>(ga, gb, a_s, w_s, m_s, a.w1 + wf, Ko, Ko, Ki);
      sp_stage<S>(gb, ga, a_s, w_s, m_s, a.w2 + wf, Ko, Ki, Ki);
    }
    for (int h = 0; h < a.H; ++h) {
      const int64_t gout = row[kSdHead + 3 * h];
      if (gout < 0) continue;
      sd_others(lev_s, row, a.H, h, t);
      T* dst = a.down + gout + b * Ki * Ki;
      for (int i = t; i < Ki * Ki; i += 256) dst[i] = lev_s[6] ? sp_siblings<S>(a.sp, lev_s, b, Ki, i, ga[i]) : ga[i];
    }
  }
}

// 32 input units, and 32 output units or the ONE of the root: thread t owns elements t + 256 r of every (32, 32) block, the
// weights staged transposed (td32_stage_w<true>), the block between the stages in registers: sp_path32_kernel, one level of it
template <class S>
__global__ void __launch_bounds__(256) sd_down32_kernel(SdArgs<typename S::T> a) {
  using T = typename S::T;
  __shared__ __attribute__((aligned(16))) Td32Lds<S> l;
  __shared__ int64_t lev_s[kSpHead + 2 * kSdMaxH];
  const int t = threadIdx.x;
  const int nb = (a.B + a.R - 1) / a.R;
  const int f = blockIdx.x / nb;
  const int64_t* row = a.tab + static_cast<int64_t>(f) * (kSdHead + 3 * a.H);
  const int64_t gin = row[1];
  const int64_t b0 = static_cast<int64_t>(blockIdx.x - f * nb) * a.R;
  const int64_t b1 = b0 + a.R < a.B ? b0 + a.R : a.B;
  for (int64_t b = b0; b < b1; ++b) {
    __syncthreads();  // (the previous row has read its weights)
    T x[4], y[4];
    if (a.stages && a.Ko == 1) {  // the root: G = log 1, dP[j][q] = log W1[0][j] + log W2[0][q]
      const int64_t wf = row[0] * 32;
      if (t < 32) {
        l.w[0][t] = a.w1[wf + t];
        l.w[1][t] = a.w2[wf + t];
      }
      __syncthreads();
      const T one = S::exp_shift(sp_log_real<T>(0.f), 0.f);
      const T lq = S::log_shift(S::fma_w(l.w[1][t & 31], one, S::zero()), 0.f);
#pragma unroll
      for (int r = 0; r < 4; ++r) x[r] = S::add(S::log_shift(S::fma_w(l.w[0][(t >> 5) + 8 * r], one, S::zero()), 0.f), lq);
    } else {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = t + 256 * r;
        x[r] = gin < 0 ? sp_log_real<T>(i == 0 ? 0.f : -INFINITY) : a.down[gin + b * 1024 + i];
      }
      if (a.stages) {
        const int64_t wf = row[0] * 1024;
        td32_stage_w<true>(a.w1 + wf, l.w[0], l.wt[0], t);
        td32_stage_w<true>(a.w2 + wf, l.w[1], l.wt[1], t);
        td32_fwd_stage<S>(l, l.wt[0], x, y, t);
        td32_fwd_stage<S>(l, l.wt[1], y, x, t);
      }
    }
    for (int h = 0; h < a.H; ++h) {
      const int64_t gout = row[kSdHead + 3 * h];
      if (gout < 0) continue;
      sd_others(lev_s, row, a.H, h, t);
      T* dst = a.down + gout + b * 1024;
      const bool any = lev_s[6] != 0;
#pragma unroll
      for (int r = 0; r < 4; ++r) dst[t + 256 * r] = any ? sp_siblings<S>(a.sp, lev_s, b, 32, t + 256 * r, x[r]) : x[r];
    }
  }
}

template <class T>
struct SdLeafArgs {
  const T* down;
  const int64_t* tab;  // [nq][kSdLeaf]
  float* log_m;        // (B, nq, Cmax)
  int nq, Cmax, B, maxC, maxK;
};

// one workgroup per (query variable, row): e = Re exp(G - max) and sp_leaf over the variable's own table
template <class S>
__global__ void __launch_bounds__(256) sd_leaf_kernel(SdLeafArgs<typename S::T> a) {
  using T = typename S::T;
  extern __shared__ __attribute__((aligned(16))) char sd_smem[];
  const int t = threadIdx.x;
  const int q = blockIdx.x / a.B;
  const int64_t b = blockIdx.x - q * a.B;
  const int64_t* row = a.tab + static_cast<int64_t>(q) * kSdLeaf;
  const int C = static_cast<int>(row[1]), K = static_cast<int>(row[2]), K2 = K * K;
  const int64_t goff = row[4];
  float* e = reinterpret_cast<float*>(sd_smem);
  float* av = e + a.maxK * a.maxK;
  float* lm = av + (a.maxC < kSpStates ? a.maxC : kSpStates) * (a.maxK + 1);
  float* red = lm + a.maxC;
  const T* g = a.down + goff + b * K2;
  float gm = -INFINITY;
  for (int i = t; i < K2; i += 256) gm = fmaxf(gm, goff < 0 ? (i == 0 ? 0.f : -INFINITY) : S::re(g[i]));
  gm = ck::clamp_finite(sp_block_max(gm, red, t));
  for (int i = t; i < K2; i += 256) e[i] = S::re(S::exp_shift(goff < 0 ? sp_log_real<T>(i == 0 ? 0.f : -INFINITY) : g[i], gm));
  float* out = a.log_m + (b * a.nq + q) * a.Cmax;
  SpArgs<T> sa{};
  sa.table = reinterpret_cast<const float*>(row[0]);
  sa.C = C;
  sa.K = K;
  sa.table_log = static_cast<int>(row[3]);
  sa.log_m = out;
  sp_leaf(sa, 0, e, av, lm, red, gm, t);
  for (int s = C + t; s < a.Cmax; s += 256) out[s] = -INFINITY;  // (columns past the variable's own states)
}

template <auto Kernel, class A>
int sd_dispatch(const A& a, int64_t blocks, size_t lds, size_t fixed, void* stream) {
  const dim3 grid(static_cast<unsigned>(blocks)), block(256);
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
int sd_launch(const SdArgs<typename S::T>& a, bool form32, void* stream) {
  using T = typename S::T;
  const int64_t blocks = static_cast<int64_t>(a.n) * ((a.B + a.R - 1) / a.R);
  const size_t lev = sizeof(int64_t) * (kSpHead + 2 * kSdMaxH);
  if (form32) return sd_dispatch<sd_down32_kernel<S32>>(a, blocks, 0, sizeof(Td32Lds<S32>) + lev, stream);
  const int mk = a.maxK;
  const size_t lds = sp_value_words<T>(mk) * sizeof(T) + (static_cast<size_t>(mk) * (mk + 1) + mk) * sizeof(float);
  if (lds + lev > 160 * 1024) return ck::fail(CK_ERR_UNSUPPORTED, "ck_squared_down_bwd: %d units do not fit in LDS", mk);
  return sd_dispatch<sd_down_kernel<S>>(a, blocks, lds, lev, stream);
}

template <class S, class S32>
int sd_leaf_launch(const SdLeafArgs<typename S::T>& a, bool all32, void* stream) {
  const size_t lds = (static_cast<size_t>(a.maxK) * a.maxK + sp_leaf_floats(a.maxC, a.maxK) + 4) * sizeof(float);
  if (lds > 160 * 1024) return ck::fail(CK_ERR_UNSUPPORTED, "ck_squared_down_leaf: %d units, C=%d states do not fit in LDS", a.maxK, a.maxC);
  const int64_t blocks = static_cast<int64_t>(a.nq) * a.B;
  if (all32) return sd_dispatch<sd_leaf_kernel<S32>>(a, blocks, lds, 0, stream);
  return sd_dispatch<sd_leaf_kernel<S>>(a, blocks, lds, 0, stream);
}

}  // namespace

extern "C" int ck_squared_down_bwd(const float* full, const float* cst, const float* rank1, float* down, int64_t down_elems,
                                   const int64_t* folds_host, const int64_t* folds, int n, int H, const float* w1, const float* w2,
                                   int num_weight_folds, int Ki, int Ko, int stages, int B, int rows_per_block, int complex_values,
                                   void* stream) {
  const char* who = "ck_squared_down_bwd";
  CK_REQUIRE(down && folds_host && folds, "%s: null pointer", who);
  CK_REQUIRE(n > 0 && B > 0 && rows_per_block > 0 && down_elems > 0, "%s: bad sizes", who);
  CK_REQUIRE(H >= 1 && H <= kSdMaxH, "%s: %d children per fold, at most %d", who, H, kSdMaxH);
  CK_REQUIRE(Ki > 0 && Ki <= 1024 && Ko > 0 && Ko <= 1024, "%s: Ki=%d, Ko=%d", who, Ki, Ko);  // (K^2 element indices are 32-bit)
  CK_REQUIRE(stages == 0 || stages == 2, "%s: stages=%d", who, stages);
  CK_REQUIRE(stages ? (w1 && w2 && num_weight_folds > 0) : Ki == Ko, "%s: %s", who, stages ? "weights" : "a Hadamard layer has Ki = Ko");
  const int64_t nb = (static_cast<int64_t>(B) + rows_per_block - 1) / rows_per_block;
  CK_REQUIRE(n * nb <= 0x7fffffffLL, "%s: %d folds x %lld row blocks", who, n, static_cast<long long>(nb));
  const int64_t in_words = static_cast<int64_t>(B) * Ko * Ko, out_words = static_cast<int64_t>(B) * Ki * Ki;
  bool all_top = true, any_down = false;
  for (int f = 0; f < n; ++f) {  // the folds as the host knows them: every G inside the arena, every child kind one of the three
    const int64_t* row = folds_host + static_cast<int64_t>(f) * (kSdHead + 3 * H);
    CK_REQUIRE(!stages || (row[0] >= 0 && row[0] < num_weight_folds), "%s: fold %d: weight fold %lld of %d", who, f,
               static_cast<long long>(row[0]), num_weight_folds);
    CK_REQUIRE(row[1] == -1 || (row[1] >= 0 && row[1] + in_words <= down_elems), "%s: fold %d: G at %lld of %lld", who, f,
               static_cast<long long>(row[1]), static_cast<long long>(down_elems));
    all_top = all_top && row[1] == -1;
    int nd = 0;
    for (int h = 0; h < H; ++h) nd += row[kSdHead + 3 * h] >= 0;
    for (int h = 0; h < H; ++h) {
      const int64_t go = row[kSdHead + 3 * h], kd = row[kSdHead + 3 * h + 1], o = row[kSdHead + 3 * h + 2];
      CK_REQUIRE(go == -1 || (go >= 0 && go + out_words <= down_elems), "%s: fold %d: child %d: G at %lld of %lld", who, f, h,
                 static_cast<long long>(go), static_cast<long long>(down_elems));
      CK_REQUIRE(kd == CK_SQ_FULL || kd == CK_SQ_CONST || kd == CK_SQ_RANK1, "%s: fold %d: child kind %lld", who, f, static_cast<long long>(kd));
      const bool is_read = nd - (go >= 0 ? 1 : 0) > 0;  // (some OTHER slot is a down fold)
      CK_REQUIRE(o >= 0 && (!is_read || (kd == CK_SQ_FULL ? full : kd == CK_SQ_CONST ? cst : rank1) != nullptr),
                 "%s: fold %d: null pointer or negative offset of a child", who, f);
      any_down = any_down || go >= 0;
    }
  }
  CK_REQUIRE(any_down, "%s: no child is a down fold", who);
  const bool form32 = Ki == 32 && (stages ? (Ko == 32 || (Ko == 1 && all_top)) : true);
  const int maxK = std::max(Ki, Ko);
  const auto args = [&](auto* fu, auto* c, auto* r, auto* d) {
    using T = std::remove_cv_t<std::remove_pointer_t<decltype(fu)>>;
    SdArgs<T> a{};
    a.sp.full = fu;
    a.sp.cst = c;
    a.sp.rank1 = r;
    a.down = d;
    a.tab = folds;
    a.w1 = w1;
    a.w2 = w2;
    a.n = n, a.H = H, a.Ki = Ki, a.Ko = Ko, a.stages = stages, a.B = B, a.R = rows_per_block, a.maxK = maxK;
    return a;
  };
  if (complex_values)
    return sd_launch<TdC, TdC32>(args(reinterpret_cast<const c32*>(full), reinterpret_cast<const c32*>(cst),
                                      reinterpret_cast<const c32*>(rank1), reinterpret_cast<c32*>(down)),
                                 form32, stream);
  return sd_launch<TdR, TdR32>(args(full, cst, rank1, down), form32, stream);
}

extern "C" int ck_squared_down_leaf(const float* down, int64_t down_elems, const int64_t* vars_host, const int64_t* vars, int nq, int C_max,
                                    float* log_m, int B, int complex_values, void* stream) {
  const char* who = "ck_squared_down_leaf";
  CK_REQUIRE(vars_host && vars && log_m, "%s: null pointer", who);
  CK_REQUIRE(nq > 0 && B > 0 && C_max > 0 && down_elems >= 0, "%s: bad sizes", who);
  CK_REQUIRE(static_cast<int64_t>(nq) * B <= 0x7fffffffLL, "%s: %d variables x %d rows", who, nq, B);
  int maxC = 1, maxK = 1;
  bool all32 = true;
  for (int q = 0; q < nq; ++q) {
    const int64_t* row = vars_host + static_cast<int64_t>(q) * kSdLeaf;
    CK_REQUIRE(row[0] != 0 && row[1] > 0 && row[1] <= C_max && row[2] > 0 && row[2] <= 1024, "%s: variable %d: table, C=%lld, K=%lld", who, q,
               static_cast<long long>(row[1]), static_cast<long long>(row[2]));
    CK_REQUIRE(row[4] == -1 || (down && row[4] >= 0 && row[4] + static_cast<int64_t>(B) * row[2] * row[2] <= down_elems),
               "%s: variable %d: G at %lld of %lld", who, q, static_cast<long long>(row[4]), static_cast<long long>(down_elems));
    maxC = std::max(maxC, static_cast<int>(row[1]));
    maxK = std::max(maxK, static_cast<int>(row[2]));
    all32 = all32 && row[2] == 32;
  }
  if (complex_values) {
    SdLeafArgs<c32> a{reinterpret_cast<const c32*>(down), vars, log_m, nq, C_max, B, maxC, maxK};
    return sd_leaf_launch<TdC, TdC32>(a, all32, stream);
  }
  SdLeafArgs<float> a{down, vars, log_m, nq, C_max, B, maxC, maxK};
  return sd_leaf_launch<TdR, TdR32>(a, all32, stream);
}
