// Autoregressive conditionals and coding tables ("Autoregressive conditionals and coding"): the kernels
// behind `HipCircuit.autoregressive_conditionals`, `autoregressive_log_probs` and `coding_tables`.  Expanded row r = b P + j
// of a (B, D) batch is row b with every variable at step >= positions[j] of the order set to the sentinel; its one query
// variable is the variable AT that step.  ck_ar_expand writes a chunk of expanded rows, the evidence forward and the
// derivative pass of ck_loo.hip run on it unchanged, and the leaves below are ck_loo.hip's with one query variable per row
// (rowvar[n]) instead of Q per row -- the same arithmetic in the same order, so that the conditionals are bit for bit those
// `leave_one_out` gives for the host-expanded batch.  ck_ar_quantise turns conditionals into the integer cumulative
// frequency tables an entropy coder reads.
#include <math.h>

#include "ck_loo_leaf.h"

namespace {

using ck::blocks_of;
using ck::entries_max;
using ck::finite_d;
using ck::kMaxLds;
using ck::kThreads;
using ck::kWaves;
using ck::LooEntry;
using ck::shifted_exp;

// One thread per (expanded row n of the chunk, variable v).  order_pos[v]: the step of v, -1 for a variable outside the
// order (kept as it is).  The thread of the row's query variable also writes rowvar[n] and rowobs[n], the row's own value
// there (the dtype of x).  A value the range check would refuse (states[v] > 0 and value >= states[v]) marks the WHOLE row b
// bad, hidden behind the sentinel or not: bad[n] = 1 for every expanded row of b, *flag |= 1 (flag may be NULL).
__global__ void __launch_bounds__(kThreads)
    ar_expand_kernel(const void* __restrict__ x, int x_float, int D, const int32_t* __restrict__ order_pos,
                     const int32_t* __restrict__ positions, int P, const int32_t* __restrict__ states, int64_t r0, int64_t nb,
                     void* __restrict__ xe, int32_t* __restrict__ rowvar, void* __restrict__ rowobs, int32_t* __restrict__ bad,
                     int32_t* flag) {
  const int64_t o = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (o >= nb * D) return;
  const int64_t n = o / D;
  const int v = static_cast<int>(o % D);
  const int64_t r = r0 + n;
  const int64_t b = r / P;
  const int step = positions[r % P], at = order_pos[v];
  const bool hide = at >= step;
  const int S = states[v];
  bool out_of_range;
  if (x_float) {
    const float e = static_cast<const float*>(x)[b * D + v];
    out_of_range = S > 0 && e > -1.f && e >= static_cast<float>(S);
    static_cast<float*>(xe)[o] = hide ? NAN : e;
    if (at == step) static_cast<float*>(rowobs)[n] = e;
  } else {
    const int64_t c = static_cast<const int64_t*>(x)[b * D + v];
    out_of_range = S > 0 && c >= S;
    static_cast<int64_t*>(xe)[o] = hide ? -1 : c;
    if (at == step) static_cast<int64_t*>(rowobs)[n] = c;
  }
  if (at == step) rowvar[n] = v;
  if (out_of_range) {
    bad[n] = 1;
    if (flag != nullptr) atomicOr(flag, 1);
  }
}

// Categorical / Binomial query variables: loo_leaf_cat_generic (ck_loo.hip) with one wave per ROW and q = rowvar[n].  The
// weights pi_k = exp((D_k - mD) + log Z_k - m2) are staged in the wave's own LDS row, a_c = sum_k pi_k ntab[k, c] is formed
// twice, once for the total over c and once for the single store of a_c / total.  sw: max_units floats per wave.
__global__ void __launch_bounds__(kThreads)
    ar_leaf_cat_kernel(const LooEntry* __restrict__ ent, const int32_t* __restrict__ vstart, const int32_t* __restrict__ rowvar,
                       int Cout, int max_units, const float* __restrict__ ntab, const float* __restrict__ lz,
                       const float* __restrict__ der, const int64_t* __restrict__ val_off, const int32_t* __restrict__ bad,
                       int64_t B, float* __restrict__ out) {
  extern __shared__ float sh[];
  const int lane = threadIdx.x & (ck::kWave - 1), wave = threadIdx.x / ck::kWave;
  float* const sw = sh + static_cast<int64_t>(wave) * max_units;
  const int64_t n = static_cast<int64_t>(blockIdx.x) * kWaves + wave;
  if (n >= B) return;  // (no workgroup barrier below: the LDS rows are the wave's own)
  float* o = out + n * Cout;
  if (bad[n] != 0) {
    for (int c = lane; c < Cout; c += ck::kWave) o[c] = NAN;
    return;
  }
  const int q = rowvar[n];
  const int s0 = vstart[q], s1 = vstart[q + 1];
  const float mD = ck::wave_max(entries_max(ent, s0, s1, der, val_off, n, lane, ck::kWave));
  float mx = -INFINITY;
  int u0 = 0;
  for (int s = s0; s < s1; ++s) {
    const LooEntry e = ent[s];
    const float* dr = der + val_off[e.g] + n * e.K;
    for (int k = lane; k < e.K; k += ck::kWave) {
      const float d = dr[k], z = lz[e.zoff + k];
      const float t = (finite_d(d) && z > -INFINITY) ? (d - mD) + z : -INFINITY;
      sw[u0 + k] = t;
      mx = fmaxf(mx, t);
    }
    u0 += static_cast<int>(e.K);
  }
  const float m2 = ck::wave_max(mx);
  for (int k = lane; k < u0; k += ck::kWave) sw[k] = sw[k] > -INFINITY ? expf(sw[k] - m2) : 0.f;
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  float total = 0.f;
  for (int pass = 0; pass < 2; ++pass) {
    for (int c = lane; c < Cout; c += ck::kWave) {
      float acc = 0.f;
      int u = 0;
      for (int s = s0; s < s1; ++s) {
        const LooEntry e = ent[s];
        if (c < e.C) {
          const float* t = ntab + e.off + c;
          for (int k = 0; k < e.K; ++k)
            if (sw[u + k] > 0.f) acc = fmaf(sw[u + k], t[k * e.C], acc);
        }
        u += static_cast<int>(e.K);
      }
      if (pass == 0) total += acc;
      else o[c] = total > 0.f ? acc / total : NAN;
    }
    if (pass == 0) total = ck::wave_sum(total);
  }
}

// Gaussian query variables: loo_leaf_gauss_kernel (ck_loo.hip) with one thread per row and q = rowvar[n].
__global__ void __launch_bounds__(kThreads)
    ar_leaf_gauss_kernel(const LooEntry* __restrict__ ent, const int32_t* __restrict__ vstart, const int32_t* __restrict__ rowvar,
                         const float* __restrict__ mean, const float* __restrict__ stddev, const float* __restrict__ der,
                         const int64_t* __restrict__ val_off, const int32_t* __restrict__ bad, int64_t B,
                         float* __restrict__ out) {
  const int64_t n = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (n >= B) return;
  const int q = rowvar[n];
  float s1 = NAN, s2 = NAN;
  const int a = vstart[q], b = vstart[q + 1];
  const float mD = bad[n] != 0 ? -INFINITY : entries_max(ent, a, b, der, val_off, n, 0, 1);
  if (finite_d(mD)) {
    float t0 = 0.f, t1 = 0.f, t2 = 0.f;
    for (int s = a; s < b; ++s) {
      const LooEntry e = ent[s];
      const float* dr = der + val_off[e.g] + n * e.K;
      for (int k = 0; k < e.K; ++k) {
        const float p = shifted_exp(dr[k], mD);
        const float mu = mean[e.off + k], sd = stddev[e.off + k];
        t0 += p;
        t1 = fmaf(p, mu, t1);
        t2 = fmaf(p, fmaf(sd, sd, mu * mu), t2);
      }
    }
    s1 = t1 / t0;
    s2 = t2 / t0;
  }
  out[n * 2] = s1;
  out[n * 2 + 1] = s2 - s1 * s1;
}

// out (B): log p(x_q | the row's prefix) = lse_k(d_k + v_k) - lse_k(d_k + log Z_k), d_k = D_k - max_k D_k, as
// loo_log_probs_kernel (ck_loo.hip) -- but the value v_k of the row's OWN observation rowobs[n] is formed here, because the
// expanded row hides it from the evidence forward: the entry ltab[k, c] of the unit's LOG table for a discrete unit (what the
// forward reads; a normalised linear table would lose every state below 1e-45 of its row), -inf for a state outside the
// table; log N(x; mean_k, stddev_k) for a Gaussian unit (log Z_k = 0).  One thread per row.
__global__ void __launch_bounds__(kThreads)
    ar_log_probs_kernel(const LooEntry* __restrict__ ent, const int32_t* __restrict__ vstart, const int32_t* __restrict__ vkind,
                        const int32_t* __restrict__ rowvar, const void* __restrict__ rowobs, int x_float,
                        const float* __restrict__ ltab, const float* __restrict__ lz, const float* __restrict__ mean,
                        const float* __restrict__ stddev, const float* __restrict__ der, const int64_t* __restrict__ val_off,
                        const int32_t* __restrict__ bad, int64_t B, float* __restrict__ out) {
  const int64_t n = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (n >= B) return;
  const int v = rowvar[n];
  const int a = vstart[v], b = vstart[v + 1];
  const bool gauss = vkind[v] == 2;
  float e = 0.f;
  int64_t c = 0;
  float res = 0.f;
  if (bad[n] != 0) {
    res = NAN;
  } else if (a < b && ck::observed(rowobs, n, x_float, gauss, e, c)) {
    if (x_float && !gauss) c = static_cast<int64_t>(e);  // (a float batch is truncated, as the forward does)
    const float mD = entries_max(ent, a, b, der, val_off, n, 0, 1);
    float mn = -INFINITY, md = -INFINITY, sn = 0.f, sd = 0.f;
    for (int pass = 0; pass < 2 && finite_d(mD); ++pass)
      for (int s = a; s < b; ++s) {
        const LooEntry en = ent[s];
        const int64_t at = val_off[en.g] + n * en.K;
        for (int k = 0; k < en.K; ++k) {
          const float d = der[at + k];
          if (!finite_d(d)) continue;
          const float z = lz[en.zoff + k];
          float val;
          if (gauss) {
            val = ck::mpe_gauss(e, mean[en.off + k], stddev[en.off + k], nullptr, 0);
          } else {
            val = c < en.C ? ltab[en.off + k * en.C + c] : -INFINITY;
          }
          const float tn = (d - mD) + val, td = (d - mD) + z;
          if (pass == 0) {
            mn = fmaxf(mn, tn);
            md = fmaxf(md, td);
          } else {
            if (tn > -INFINITY) sn += expf(tn - mn);
            if (td > -INFINITY) sd += expf(td - md);
          }
        }
      }
    if (!finite_d(md)) res = NAN;
    else if (!finite_d(mn)) res = mn;  // (-inf: the observed value has no mass)
    else res = (mn + logf(sn)) - (md + logf(sd));
  }
  out[n] = res;
}

// ---- the quantiser ---------------------------------------------------------------------------------------------------
// sum / max / inclusive scan over the 64 lanes of a wave, integers: every lane gets the result
__device__ __forceinline__ int wave_sum_i(int v) {
  for (int o = 1; o < ck::kWave; o <<= 1) v += __shfl_xor(v, o, ck::kWave);
  return v;
}
__device__ __forceinline__ long long wave_max_ll(long long v) {
  for (int o = 1; o < ck::kWave; o <<= 1) {
    const long long w = __shfl_xor(v, o, ck::kWave);
    v = w > v ? w : v;
  }
  return v;
}
__device__ __forceinline__ int wave_scan_i(int v, int lane) {
  for (int o = 1; o < ck::kWave; o <<= 1) {
    const int w = __shfl_up(v, o, ck::kWave);
    if (lane >= o) v += w;
  }
  return v;
}

// The count of state c before the slack: 1 + floor(p (T - S)), the product rounded ONCE to fp32 (no contraction with
// anything else), so that the rule is an integer function of the fp32 vector that numpy restates exactly.
__device__ __forceinline__ int ar_count(float p, float scale) { return 1 + static_cast<int>(__fmul_rn(p, scale)); }

// One wave per row.  p (rows, C) fp32 conditionals, S = states[rowvar[n]] <= C states of the row's variable, T = 2^precision.
// count_c = 1 + floor(p_c (T - S)) for c < S and 0 past S; the slack T - sum_c count_c, of either sign, goes to the first
// state with the largest count.  A row holding a value outside [0, 1] (NaN included), or whose slack would leave its largest
// count below 1, becomes uniform: floor(T / S) each, the remainder to state 0.  out (rows, C + 1): the exclusive cumulative
// counts, out[n, 0] = 0 and out[n, c] = T for every c >= S.
__global__ void __launch_bounds__(kThreads)
    ar_quantise_kernel(const float* __restrict__ p, const int32_t* __restrict__ rowvar, const int32_t* __restrict__ states,
                       int64_t rows, int C, int precision, int32_t* __restrict__ out) {
  const int lane = threadIdx.x & (ck::kWave - 1), wave = threadIdx.x / ck::kWave;
  const int64_t n = static_cast<int64_t>(blockIdx.x) * kWaves + wave;
  if (n >= rows) return;
  const float* pr = p + n * C;
  int32_t* o = out + n * (static_cast<int64_t>(C) + 1);
  const int T = 1 << precision;
  const int S = min(max(states[rowvar[n]], 1), C);
  const float scale = static_cast<float>(T - S);
  int sum = 0, invalid = 0;
  long long best = -1;  // (count << 32) | (2^32 - 1 - c): the maximum is the FIRST state with the largest count
  for (int c = lane; c < S; c += ck::kWave) {
    const float x = pr[c];
    if (!(x >= 0.f && x <= 1.f)) {
      invalid = 1;
      continue;
    }
    const int k = ar_count(x, scale);
    sum += k;
    const long long key = (static_cast<long long>(k) << 32) | static_cast<long long>(0xffffffffu - static_cast<unsigned>(c));
    best = key > best ? key : best;
  }
  invalid = wave_sum_i(invalid);
  sum = wave_sum_i(sum);
  best = wave_max_ll(best);
  int slack = T - sum;
  int top = static_cast<int>(0xffffffffu - static_cast<unsigned>(best & 0xffffffffll));
  const bool uniform = invalid != 0 || best < 0 || static_cast<int>(best >> 32) + slack < 1;
  if (uniform) {
    slack = T - (T / S) * S;
    top = 0;
  }
  int carry = 0;
  if (lane == 0) o[0] = 0;
  for (int c0 = 0; c0 < C; c0 += ck::kWave) {  // (every lane takes every turn: the scan is over the whole wave)
    const int c = c0 + lane;
    int k = 0;
    if (c < S) {
      k = uniform ? T / S : ar_count(pr[c], scale);
      if (c == top) k += slack;
    }
    const int inc = wave_scan_i(k, lane);
    if (c < C) o[c + 1] = carry + inc;
    carry += __shfl(inc, ck::kWave - 1, ck::kWave);
  }
}

}  // namespace

int ck_ar_expand(const void* x, int x_float, int64_t B, int D, const int32_t* order_pos, const int32_t* positions, int P,
                 const int32_t* states, int64_t r0, int64_t nb, void* xe, int32_t* rowvar, void* rowobs, int32_t* bad,
                 int32_t* flag, void* stream) {
  CK_REQUIRE(x != nullptr && order_pos != nullptr && positions != nullptr && states != nullptr && xe != nullptr &&
                 rowvar != nullptr && rowobs != nullptr && bad != nullptr,
             "ck_ar_expand: null pointer");
  CK_REQUIRE(B > 0 && D > 0 && P > 0 && nb > 0, "ck_ar_expand: non-positive size");
  CK_REQUIRE(r0 >= 0 && r0 + nb <= B * P, "ck_ar_expand: rows %lld .. %lld outside the %lld expanded rows",
             static_cast<long long>(r0), static_cast<long long>(r0 + nb), static_cast<long long>(B * P));
  const int64_t blocks = blocks_of(nb * D, kThreads);
  CK_REQUIRE(blocks <= 0x7fffffff, "ck_ar_expand: too many entries");
  return ck::launch(ar_expand_kernel, dim3(static_cast<unsigned>(blocks)), dim3(kThreads), 0, stream, x, x_float, D, order_pos,
                    positions, P, states, r0, nb, xe, rowvar, rowobs, bad, flag);
}

int ck_ar_leaf_categorical(const int64_t* entries, const int32_t* vstart, const int32_t* rowvar, int Cout, int max_units,
                           const float* ntab, const float* lz, const float* der, const int64_t* val_off, const int32_t* bad,
                           int64_t B, float* out, void* stream) {
  CK_REQUIRE(entries != nullptr && vstart != nullptr && rowvar != nullptr && ntab != nullptr && lz != nullptr &&
                 der != nullptr && val_off != nullptr && bad != nullptr && out != nullptr,
             "ck_ar_leaf_categorical: null pointer");
  CK_REQUIRE(Cout > 0 && B > 0 && max_units > 0, "ck_ar_leaf_categorical: non-positive size");
  const int64_t lds = static_cast<int64_t>(kWaves) * max_units * 4;
  CK_REQUIRE(lds <= kMaxLds, "ck_ar_leaf_categorical: %d input units over one variable exceed the LDS budget", max_units);
  const int64_t blocks = blocks_of(B, kWaves);
  CK_REQUIRE(blocks <= 0x7fffffff, "ck_ar_leaf_categorical: too many rows");
  return ck::launch(ar_leaf_cat_kernel, dim3(static_cast<unsigned>(blocks)), dim3(kThreads), static_cast<size_t>(lds), stream,
                    reinterpret_cast<const LooEntry*>(entries), vstart, rowvar, Cout, max_units, ntab, lz, der, val_off, bad, B,
                    out);
}

int ck_ar_leaf_gaussian(const int64_t* entries, const int32_t* vstart, const int32_t* rowvar, const float* mean,
                        const float* stddev, const float* der, const int64_t* val_off, const int32_t* bad, int64_t B,
                        float* out, void* stream) {
  CK_REQUIRE(entries != nullptr && vstart != nullptr && rowvar != nullptr && mean != nullptr && stddev != nullptr &&
                 der != nullptr && val_off != nullptr && bad != nullptr && out != nullptr,
             "ck_ar_leaf_gaussian: null pointer");
  CK_REQUIRE(B > 0, "ck_ar_leaf_gaussian: non-positive size");
  const int64_t blocks = blocks_of(B, kThreads);
  CK_REQUIRE(blocks <= 0x7fffffff, "ck_ar_leaf_gaussian: too many rows");
  return ck::launch(ar_leaf_gauss_kernel, dim3(static_cast<unsigned>(blocks)), dim3(kThreads), 0, stream,
                    reinterpret_cast<const LooEntry*>(entries), vstart, rowvar, mean, stddev, der, val_off, bad, B, out);
}

int ck_ar_log_probs(const int64_t* entries, const int32_t* vstart, const int32_t* vkind, const int32_t* rowvar,
                    const void* rowobs, int x_float, int has_discrete, int has_gaussian, const float* ltab, const float* lz,
                    const float* mean, const float* stddev, const float* der, const int64_t* val_off, const int32_t* bad,
                    int64_t B, float* out, void* stream) {
  CK_REQUIRE(entries != nullptr && vstart != nullptr && vkind != nullptr && rowvar != nullptr && rowobs != nullptr &&
                 lz != nullptr && der != nullptr && val_off != nullptr && bad != nullptr && out != nullptr,
             "ck_ar_log_probs: null pointer");
  CK_REQUIRE(!has_discrete || ltab != nullptr, "ck_ar_log_probs: discrete variables without their log tables");
  CK_REQUIRE(!has_gaussian || (mean != nullptr && stddev != nullptr), "ck_ar_log_probs: Gaussian variables without their moments");
  CK_REQUIRE(B > 0, "ck_ar_log_probs: non-positive size");
  const int64_t blocks = blocks_of(B, kThreads);
  CK_REQUIRE(blocks <= 0x7fffffff, "ck_ar_log_probs: too many rows");
  return ck::launch(ar_log_probs_kernel, dim3(static_cast<unsigned>(blocks)), dim3(kThreads), 0, stream,
                    reinterpret_cast<const LooEntry*>(entries), vstart, vkind, rowvar, rowobs, x_float, ltab, lz, mean, stddev,
                    der, val_off, bad, B, out);
}

int ck_ar_quantise(const float* p, const int32_t* rowvar, const int32_t* states, int64_t rows, int C, int precision,
                   int32_t* out, void* stream) {
  CK_REQUIRE(p != nullptr && rowvar != nullptr && states != nullptr && out != nullptr, "ck_ar_quantise: null pointer");
  CK_REQUIRE(rows > 0 && C > 0, "ck_ar_quantise: non-positive size");
  CK_REQUIRE(precision >= 8 && precision <= 24, "ck_ar_quantise: precision %d outside 8 .. 24", precision);
  CK_REQUIRE(static_cast<int64_t>(C) * 4 <= (int64_t{1} << precision), "ck_ar_quantise: %d states exceed 2^(precision - 2) at precision %d",
             C, precision);
  const int64_t blocks = blocks_of(rows, kWaves);
  CK_REQUIRE(blocks <= 0x7fffffff, "ck_ar_quantise: too many rows");
  return ck::launch(ar_quantise_kernel, dim3(static_cast<unsigned>(blocks)), dim3(kThreads), 0, stream, p, rowvar, states, rows,
                    C, precision, out);
}
