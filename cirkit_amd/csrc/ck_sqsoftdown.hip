// Posteriors under soft evidence of squared circuits p(x) = |c(x)|^2 / Z ("Posteriors and sampling under soft
// evidence of squared circuits"): the leaves of ck_sqdown.hip's walk over a SOFT bottom-up pass (ck_sqsoft.hip).  The derivative G
// that reaches the input fold of a soft variable v holds "all children but this one" at every ancestor, so it carries the weights
// of every OTHER variable and not lambda_v:
//     log_m[b, q, s] = log_lik[b, pos_q, s] + log max(0, sum_kl e[k][l] a_k(s) a_l(s)) + gmax (+ 2 tm_s),   e = Re exp(G - gmax).
// Two forms.  The plain form is sp_leaf (ck_sqpath.h) with the weight added: one thread per state, K^2 FMAs each, the table staged
// again for every row.  The 32-unit form contracts on v_mfma_f32_32x32x2_f32 in exact fp32: the table is staged once per workgroup
// and slab, a wave holds a row's e in registers as the A operands and walks the tiles of 32 states.
#include "ck_sqpath.h"
#include "ck_tile.h"

namespace {

constexpr int kQlLeaf = CK_SQ_DOWN_LEAF_WORDS;
constexpr int kQlSlab = 128;           // states of a slab of the 32-unit form: four tiles, one accumulator each
constexpr int kQlTiles = kQlSlab / 32;
constexpr int kQlRows = 16;             // the rows of a workgroup of the 32-unit form come in multiples of 16: four per wave share a staged slab
constexpr int kQlStride = kQlSlab + 1;  // floats of a unit's row of the slab: the staging writes walk the units, an odd stride spreads them over the banks

template <class T>
struct QlArgs {
  const T* down;
  const int64_t* tab;  // [nq][kQlLeaf]
  const float* ll;     // (B, S, Cl)
  float* log_m;        // (B, nq, Cmax)
  int nq, Cmax, B, R, S, Cl, maxC, maxK;
};

// the plain form: a workgroup takes one variable and R rows one after the other; sd_leaf_kernel of ck_sqdown.hip with `lam` set
template <class S>
__global__ void __launch_bounds__(256) ql_plain_kernel(QlArgs<typename S::T> a) {
  using T = typename S::T;
  extern __shared__ __attribute__((aligned(16))) char ql_smem[];
  const int t = threadIdx.x;
  const int nb = (a.B + a.R - 1) / a.R;
  const int q = blockIdx.x / nb;
  const int64_t* row = a.tab + static_cast<int64_t>(q) * kQlLeaf;
  const int C = static_cast<int>(row[1]), K = static_cast<int>(row[2]), K2 = K * K;
  const int64_t goff = row[4], pos = row[5];
  float* e = reinterpret_cast<float*>(ql_smem);
  float* av = e + a.maxK * a.maxK;
  float* lm = av + (a.maxC < kSpStates ? a.maxC : kSpStates) * (a.maxK + 1);
  float* red = lm + a.maxC;
  const int64_t b0 = static_cast<int64_t>(blockIdx.x - q * nb) * a.R;
  const int64_t b1 = b0 + a.R < a.B ? b0 + a.R : a.B;
  for (int64_t b = b0; b < b1; ++b) {
    __syncthreads();  // (the previous row has left LDS)
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
    sa.lam = a.ll + (b * a.S + pos) * a.Cl;
    sp_leaf(sa, 0, e, av, lm, red, gm, t);
    for (int s = C + t; s < a.Cmax; s += 256) out[s] = -INFINITY;  // (columns past the variable's own states)
  }
}

// the sum of a value with its partner in the other 32-lane half (v_permlane32_swap: no LDS round trip)
__device__ __forceinline__ float ql_xhalf_sum(float v) {
  const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}

// The 32-unit form.  Step st of the 16 contracts the two units k = ql_unit(st, half): the A operand of lane (l, half) is
// e[l][k], the B operand of lane (s, half) is a_k(s), and D[l][s] = sum_k e[l][k] a_k(s) comes back in lane (s, half), register r,
// with l = 8 (r >> 2) + 4 half + (r & 3) (ck_tile.h).  The order in which the steps take the units is free, and taking them in the
// accumulator's own order, k = ql_unit(st, half) = 8 (st >> 2) + 4 half + (st & 3), makes the B operand of step r the very a_l(s)
// that register r of the result is multiplied with: m(s) = sum_l a_l(s) D[l][s] needs no second read of the table.
__device__ __forceinline__ int ql_unit(int st, int half) { return 8 * (st >> 2) + 4 * half + (st & 3); }

template <class S, bool TLOG>
__global__ void __launch_bounds__(256) ql_mfma_kernel(QlArgs<typename S::T> a) {
  using T = typename S::T;
  __shared__ float a_s[32 * kQlStride];  // a_s[k][s]: a lane half reads 32 consecutive states of one unit
  __shared__ float tm_s[kQlSlab];        // the per-state shift of a table of logarithms
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6, sl = lane & 31, half = lane >> 5;
  const int Rb = (a.R + kQlRows - 1) / kQlRows * kQlRows;  // (as ck_sqsoft.hip rounds: rows_per_block only changes the grid)
  const int nb = (a.B + Rb - 1) / Rb;
  const int q = blockIdx.x / nb;
  const int64_t* row = a.tab + static_cast<int64_t>(q) * kQlLeaf;
  const float* table = reinterpret_cast<const float*>(row[0]);
  const int C = static_cast<int>(row[1]);
  const int64_t goff = row[4], pos = row[5];
  const int64_t b0 = static_cast<int64_t>(blockIdx.x - q * nb) * Rb;
  const int64_t b1 = b0 + Rb < a.B ? b0 + Rb : a.B;
  for (int s0 = 0; s0 < C; s0 += kQlSlab) {
    const int ns = C - s0 < kQlSlab ? C - s0 : kQlSlab;
    const int nt = (ns + 31) / 32;
    __syncthreads();  // (the rows of the slab before are done)
    for (int i = t; i < nt * 1024; i += 256) {  // thread i: state i / 32, unit i % 32 -- the 32 lanes of a half share a state
      const int s = i >> 5, k = i & 31;
      float v = 0.f, tm = 0.f;
      if (s < ns) v = table[static_cast<int64_t>(s0) * 32 + i];
      if constexpr (TLOG) {
        tm = s < ns ? v : -INFINITY;
#pragma unroll
        for (int d = 1; d < 32; d <<= 1) tm = fmaxf(tm, __shfl_xor(tm, d, 64));
        tm = ck::clamp_finite(tm);
        v = s < ns ? expf(v - tm) : 0.f;
        if (s >= ns) tm = 0.f;
      }
      a_s[k * kQlStride + s] = v;
      if (k == 0) tm_s[s] = tm;
    }
    __syncthreads();
    for (int64_t b = b0 + wv; b < b1; b += 4) {  // a wave takes a row: nothing below leaves the wave
      float ea[16];
      float gm = -INFINITY;
#pragma unroll
      for (int st = 0; st < 16; ++st) {
        const int i = sl * 32 + ql_unit(st, half);
        const T g = goff < 0 ? sp_log_real<T>(i == 0 ? 0.f : -INFINITY) : a.down[goff + b * 1024 + i];
        gm = fmaxf(gm, S::re(g));
      }
      gm = ck::clamp_finite(ck::wave_max(gm));
#pragma unroll
      for (int st = 0; st < 16; ++st) {
        const int i = sl * 32 + ql_unit(st, half);
        const T g = goff < 0 ? sp_log_real<T>(i == 0 ? 0.f : -INFINITY) : a.down[goff + b * 1024 + i];
        ea[st] = S::re(S::exp_shift(g, gm));
      }
      f32x16 acc[kQlTiles];
      float bv[kQlTiles][16];
#pragma unroll
      for (int j = 0; j < kQlTiles; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
#pragma unroll
      for (int st = 0; st < 16; ++st) {
        const float* ar = a_s + ql_unit(st, half) * kQlStride + sl;
#pragma unroll
        for (int j = 0; j < kQlTiles; ++j) {
          if (j < nt) {  // (uniform in the workgroup)
            bv[j][st] = ar[32 * j];
            acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(ea[st], bv[j][st], acc[j], 0, 0, 0);
          }
        }
      }
      const float* lam = a.ll + (b * a.S + pos) * a.Cl + s0;
      float* out = a.log_m + (b * a.nq + q) * a.Cmax + s0;
#pragma unroll
      for (int j = 0; j < kQlTiles; ++j) {
        if (j >= nt) continue;
        float m = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) m = fmaf(bv[j][r], acc[j][r], m);
        m = ql_xhalf_sum(m);
        m = m < 0.f ? 0.f : m;  // (cancellation can leave -1e-9: that is a zero, not a NaN; a NaN stays one)
        const int s = 32 * j + sl;
        if (half == 0 && s < ns) {
          float v = logf(m) + gm;
          if constexpr (TLOG) v += 2.f * tm_s[s];
          out[s] = v + lam[s];
        }
      }
    }
  }
  for (int64_t b = b0 + wv; b < b1; b += 4)  // (columns past the variable's own states)
    for (int s = C + lane; s < a.Cmax; s += 64) a.log_m[(b * a.nq + q) * a.Cmax + s] = -INFINITY;
}

template <auto Kernel, class A>
int ql_dispatch(const A& a, int rows, size_t lds, void* stream) {  // rows: of a workgroup
  const dim3 grid(static_cast<unsigned>(static_cast<int64_t>(a.nq) * ((a.B + rows - 1) / rows))), block(256);
  return ck::dispatch(
      [=](hipStream_t s) {
        const hipError_t er = sp_raise_lds<Kernel>(lds, 0);
        if (er != hipSuccess) return er;
        hipLaunchKernelGGL(Kernel, grid, block, lds, s, a);
        return hipGetLastError();
      },
      stream);
}

template <class S, class S32>
int ql_launch(const QlArgs<typename S::T>& a, bool all32, bool all_log, bool none_log, int form, void* stream) {
  if (form == 0 && all32 && (all_log || none_log)) {  // (the kind of table is a template argument: a launch that mixes them is plain)
    const int Rb = (a.R + kQlRows - 1) / kQlRows * kQlRows;
    if (all_log) return ql_dispatch<ql_mfma_kernel<S32, true>>(a, Rb, 0, stream);
    return ql_dispatch<ql_mfma_kernel<S32, false>>(a, Rb, 0, stream);
  }
  const size_t lds = (static_cast<size_t>(a.maxK) * a.maxK + sp_leaf_floats(a.maxC, a.maxK) + 4) * sizeof(float);
  if (lds > 160 * 1024)
    return ck::fail(CK_ERR_UNSUPPORTED, "ck_squared_soft_down_leaf: %d units, C=%d states do not fit in LDS", a.maxK, a.maxC);
  if (all32) return ql_dispatch<ql_plain_kernel<S32>>(a, a.R, lds, stream);
  return ql_dispatch<ql_plain_kernel<S>>(a, a.R, lds, stream);
}

}  // namespace

extern "C" int ck_squared_soft_down_leaf(const float* down, int64_t down_elems, const int64_t* vars_host, const int64_t* vars, int nq,
                                         int C_max, const float* log_lik, int S, int C_lik, float* log_m, int B, int rows_per_block,
                                         int complex_values, int form, void* stream) {
  const char* who = "ck_squared_soft_down_leaf";
  CK_REQUIRE(vars_host && vars && log_m && log_lik, "%s: null pointer", who);
  CK_REQUIRE(nq > 0 && B > 0 && C_max > 0 && down_elems >= 0 && S > 0 && C_lik > 0 && rows_per_block > 0, "%s: bad sizes", who);
  CK_REQUIRE(form == 0 || form == 1, "%s: form=%d", who, form);
  const int64_t nb = (static_cast<int64_t>(B) + rows_per_block - 1) / rows_per_block;
  CK_REQUIRE(nq * nb <= 0x7fffffffLL, "%s: %d variables x %lld row blocks", who, nq, static_cast<long long>(nb));
  int maxC = 1, maxK = 1;
  bool all32 = true, all_log = true, none_log = true;
  for (int q = 0; q < nq; ++q) {  // the variables as the host knows them: every read inside the arena and log_lik, every write inside log_m
    const int64_t* row = vars_host + static_cast<int64_t>(q) * kQlLeaf;
    CK_REQUIRE(row[0] != 0 && row[1] > 0 && row[1] <= C_max && row[2] > 0 && row[2] <= 1024, "%s: variable %d: table, C=%lld, K=%lld", who, q,
               static_cast<long long>(row[1]), static_cast<long long>(row[2]));
    CK_REQUIRE(row[1] <= C_lik, "%s: variable %d: C=%lld states, log_lik has %d", who, q, static_cast<long long>(row[1]), C_lik);
    CK_REQUIRE(row[4] == -1 || (down && row[4] >= 0 && row[4] + static_cast<int64_t>(B) * row[2] * row[2] <= down_elems),
               "%s: variable %d: G at %lld of %lld", who, q, static_cast<long long>(row[4]), static_cast<long long>(down_elems));
    CK_REQUIRE(row[5] >= 0 && row[5] < S, "%s: variable %d: position %lld of %d", who, q, static_cast<long long>(row[5]), S);
    maxC = std::max(maxC, static_cast<int>(row[1]));
    maxK = std::max(maxK, static_cast<int>(row[2]));
    all32 = all32 && row[2] == 32;
    all_log = all_log && row[3] != 0;
    none_log = none_log && row[3] == 0;
  }
  if (complex_values) {
    QlArgs<c32> a{reinterpret_cast<const c32*>(down), vars, log_lik, log_m, nq, C_max, B, rows_per_block, S, C_lik, maxC, maxK};
    return ql_launch<TdC, TdC32>(a, all32, all_log, none_log, form, stream);
  }
  QlArgs<float> a{down, vars, log_lik, log_m, nq, C_max, B, rows_per_block, S, C_lik, maxC, maxK};
  return ql_launch<TdR, TdR32>(a, all32, all_log, none_log, form, stream);
}
