// Leave-one-out conditionals ("Leave-one-out conditionals"): the top-down DERIVATIVE pass behind
// `HipCircuit.leave_one_out` and `HipCircuit.conditional_log_probs`.  With v the per-row log values of the layer-wise marginal
// forward of the evidence, D(u) = log (dc(x_O) / du) in LOG space, 0 at the root unit and -inf where the derivative is 0.
// Unlike the flow of ck_flow.hip, f = (dc/du) u / c, nothing here divides by a value or multiplies by the child's own value:
// a unit that gives the observed state probability 0 keeps its derivative, which is what the conditional of THAT variable
// needs.  The arena is laid out as the value arena (global fold g's (B, Ko) block at val_off[g]).  The pass itself --
// contraction, message blocks, segment combine by logaddexp -- is ck_down.h's, instantiated with DerivativePass below; this
// file adds the product kernel and the leaves.
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

// m + log T, -inf where T = 0
__device__ __forceinline__ float lift(float T, float m) { return T > 0.f ? m + logf(T) : -INFINITY; }
__device__ __forceinline__ float logaddexp(float a, float b) {
  const float hi = fmaxf(a, b), lo = fminf(a, b);
  if (!(hi > -INFINITY)) return -INFINITY;
  return hi + log1pf(expf(lo - hi));
}

// The messages of entry i of fold f at row n, from base = m + log T_i.  Sum / mixing: slot f H + i / Ki, unit i % Ki, the
// base itself.  CP-T: slot f H + h, unit i, for every input h the base plus the values of the OTHER inputs at unit i, added
// in input order (a loop over the siblings, never total - v_h: one -inf sibling gives -inf, not NaN).
__device__ __forceinline__ void store_messages(int type, const int32_t* __restrict__ ch, int64_t f, int H, int Ki, int64_t B,
                                               int64_t n, int i, float base, const float* __restrict__ vals,
                                               const int64_t* __restrict__ val_off, float* __restrict__ msg) {
  if (type == CK_SAMPLE_SUM) {
    msg[((f * H + i / Ki) * B + n) * Ki + i % Ki] = base;
    return;
  }
  for (int h = 0; h < H; ++h) {
    float acc = base;
    for (int h2 = 0; h2 < H; ++h2)
      if (h2 != h) acc += vals[val_off[ch[h2]] + n * Ki + i];
    msg[((f * H + h) * B + n) * Ki + i] = acc;
  }
}

// The derivative pass as a policy of ck_down.h: the factor of a unit is a = exp(D - m), the base of entry i is m + log T_i
// and every input of the entry receives it with its SIBLINGS' values, a child combines what its consumers send by logaddexp.
struct DerivativePass {
  static __device__ __forceinline__ float key(float d, float) { return finite_d(d) ? d : -INFINITY; }
  static __device__ __forceinline__ float factor(float d, float, float m) { return shifted_exp(d, m); }
  static __device__ __forceinline__ float emit(bool tucker, int type, const int32_t* __restrict__ ch, int64_t f, int H, int Ki,
                                               int64_t B, int64_t n, int i, float T, float m, const float* __restrict__ vals,
                                               const int64_t* __restrict__ val_off, float* __restrict__ msg) {
    const float base = lift(T, m);
    if (!tucker) store_messages(type, ch, f, H, Ki, B, n, i, base, vals, val_off, msg);
    return base;
  }
  // Tucker: input 0 unit a receives lse_b(base[a, b] + v1[b]), input 1 unit b receives lse_a(base[a, b] + v0[a])
  static __device__ __forceinline__ float tucker(const float* row, int Ki, int s, int u, const int32_t* __restrict__ ch,
                                                 const float* __restrict__ vals, const int64_t* __restrict__ val_off, int64_t n) {
    const float* other = vals + val_off[ch[1 - s]] + n * Ki;
    const int at = s == 0 ? u * Ki : u, step = s == 0 ? 1 : Ki;
    float mx = -INFINITY;
    for (int j = 0; j < Ki; ++j) mx = fmaxf(mx, row[at + j * step] + other[j]);
    float out = -INFINITY;
    if (finite_d(mx)) {
      float acc = 0.f;
      for (int j = 0; j < Ki; ++j) acc += expf(row[at + j * step] + other[j] - mx);
      out = mx + logf(acc);
    }
    return out;
  }
  static __device__ __forceinline__ float identity() { return -INFINITY; }
  static __device__ __forceinline__ float combine(float a, float b) { return logaddexp(a, b); }
};

// Product layers, read from the derivative arena itself.  An item is the pair (consumer's global fold g, input position h);
// child holds the (F, H) global child folds of the layer whose first global fold is layer_fold.  Hadamard: unit i receives
// D_g[i] plus the values of the consumer's other inputs at unit i.  Kronecker: the log-sum-exp, over the outputs o whose digit
// h (base Ki, input 0 most significant) is i, in ascending output order, of D_g[o] plus the other inputs' values at their
// digits of o.
__global__ void __launch_bounds__(kThreads)
    loo_product_kernel(int type, const int32_t* __restrict__ cstart, const int32_t* __restrict__ cfold,
                       const int32_t* __restrict__ cfirst, const int32_t* __restrict__ items, const int32_t* __restrict__ child,
                       int layer_fold, const float* __restrict__ vals, float* der, const int64_t* __restrict__ val_off,
                       int64_t n_child, int H, int Ki, int Ko, int64_t B) {
  const int64_t idx = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  const int64_t per = B * Ki;
  if (idx >= n_child * per) return;
  const int64_t c = idx / per, rem = idx % per;
  const int64_t n = rem / Ki;
  const int i = static_cast<int>(rem % Ki);
  float* dst = der + val_off[cfold[c]] + rem;
  float acc = cfirst[c] ? -INFINITY : *dst;
  for (int s = cstart[c]; s < cstart[c + 1]; ++s) {
    const int g = items[2 * s], h = items[2 * s + 1];
    const int32_t* ch = child + static_cast<int64_t>(g - layer_fold) * H;
    const float* p = der + val_off[g] + n * Ko;
    if (type == CK_SAMPLE_HADAMARD) {
      float t = p[i];
      for (int h2 = 0; h2 < H; ++h2)
        if (h2 != h) t += vals[val_off[ch[h2]] + n * Ki + i];
      acc = logaddexp(acc, t);
      continue;
    }
    int stride = 1;
    for (int q = H - 1; q > h; --q) stride *= Ki;
    const int tops = Ko / (stride * Ki);
    float mx = -INFINITY, sum = 0.f;
    for (int pass = 0; pass < 2; ++pass) {
      if (pass == 1 && !finite_d(mx)) break;
      for (int top = 0; top < tops; ++top)
        for (int lo = 0; lo < stride; ++lo) {
          const int o = (top * Ki + i) * stride + lo;
          float t = p[o];
          int rest = o;
          for (int h2 = H - 1; h2 >= 0; --h2) {  // digits of o, least significant (input H - 1) first
            if (h2 != h) t += vals[val_off[ch[h2]] + n * Ki + rest % Ki];
            rest /= Ki;
          }
          if (pass == 0) mx = fmaxf(mx, t);
          else sum += expf(t - mx);
        }
    }
    if (finite_d(mx)) acc = logaddexp(acc, mx + logf(sum));
  }
  *dst = acc;
}

// ---- leaves --------------------------------------------------------------------------------------------------------
// The leaf-entry table (LooEntry) and entries_max: ck_loo_leaf.h, shared with ck_ar.hip.
// Categorical / Binomial query variables.  One wave owns (row, query variable).  With mD = max_k D_k, the weight of unit k is
// pi_k = exp((D_k - mD) + log Z_k - m2) (m2 the maximum of the exponent's first two terms: nothing is exponentiated
// unshifted, and the sum with log Z_k is taken at the size of log Z_k, not of D), staged in LDS; a_c = sum_k pi_k ntab[k, c]
// is formed twice, once for the total over c and once for the single store of a_c / total.  sw: max_units floats per wave.
__global__ void __launch_bounds__(kThreads)
    loo_leaf_cat_generic(const LooEntry* __restrict__ ent, const int32_t* __restrict__ qstart, int Q, int Cout, int max_units,
                         const float* __restrict__ ntab, const float* __restrict__ lz, const float* __restrict__ der,
                         const int64_t* __restrict__ val_off, const int32_t* __restrict__ bad, int64_t B,
                         float* __restrict__ out) {
  extern __shared__ float sh[];
  const int lane = threadIdx.x & (ck::kWave - 1), wave = threadIdx.x / ck::kWave;
  float* const sw = sh + static_cast<int64_t>(wave) * max_units;
  const int64_t item = static_cast<int64_t>(blockIdx.x) * kWaves + wave;
  if (item >= B * Q) return;  // (no workgroup barrier below: the LDS rows are the wave's own)
  const int q = static_cast<int>(item % Q);
  const int64_t n = item / Q;
  float* o = out + item * Cout;
  if (bad[n] != 0) {
    for (int c = lane; c < Cout; c += ck::kWave) o[c] = NAN;
    return;
  }
  const int s0 = qstart[q], s1 = qstart[q + 1];
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

// Gaussian query variables: out[n, q] = (S1, S2 - S1^2) with pi_k = softmax_k(D_k) over the units of the variable's input
// folds (the leaves are normalised densities), S1 = sum pi_k mean_k, S2 = sum pi_k (stddev_k^2 + mean_k^2).
__global__ void __launch_bounds__(kThreads)
    loo_leaf_gauss_kernel(const LooEntry* __restrict__ ent, const int32_t* __restrict__ qstart, int Q,
                          const float* __restrict__ mean, const float* __restrict__ stddev, const float* __restrict__ der,
                          const int64_t* __restrict__ val_off, const int32_t* __restrict__ bad, int64_t B,
                          float* __restrict__ out) {
  const int64_t idx = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (idx >= B * Q) return;
  const int q = static_cast<int>(idx % Q);
  const int64_t n = idx / Q;
  float s1 = NAN, s2 = NAN;
  const int a = qstart[q], b = qstart[q + 1];
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
  out[idx * 2] = s1;
  out[idx * 2 + 1] = s2 - s1 * s1;
}

// out (B, D): log p(x_v | x_{O \ v}) = lse_k(d_k + v_k) - lse_k(d_k + log Z_k) with d_k = D_k - max_k D_k, so that both sums
// are taken at the size of the leaf values, not of D.  0 for a variable the row misses or no input layer covers, NaN where
// the leave-one-out mass is 0 or the row's evidence was out of range, -inf where only the observed value has no mass.
// vkind[v]: 2 for a Gaussian variable (NaN is its sentinel in an fp32 batch), anything else discrete.
__global__ void __launch_bounds__(kThreads)
    loo_log_probs_kernel(const LooEntry* __restrict__ ent, const int32_t* __restrict__ vstart, const int32_t* __restrict__ vkind,
                         int D, const float* __restrict__ lz, const float* __restrict__ der, const float* __restrict__ vals,
                         const int64_t* __restrict__ val_off, const void* __restrict__ ev, int x_float,
                         const int32_t* __restrict__ bad, int64_t B, float* __restrict__ out) {
  const int64_t idx = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (idx >= B * D) return;
  const int v = static_cast<int>(idx % D);
  const int64_t n = idx / D;
  const int a = vstart[v], b = vstart[v + 1];
  float e;
  int64_t c;
  float res = 0.f;
  if (bad[n] != 0) {
    res = NAN;
  } else if (a < b && ck::observed(ev, idx, x_float, vkind[v] == 2, e, c)) {
    const float mD = entries_max(ent, a, b, der, val_off, n, 0, 1);
    float mn = -INFINITY, md = -INFINITY, sn = 0.f, sd = 0.f;
    for (int pass = 0; pass < 2 && finite_d(mD); ++pass)
      for (int s = a; s < b; ++s) {
        const LooEntry en = ent[s];
        const int64_t at = val_off[en.g] + n * en.K;
        for (int k = 0; k < en.K; ++k) {
          const float d = der[at + k];
          if (!finite_d(d)) continue;
          const float tn = (d - mD) + vals[at + k], td = (d - mD) + lz[en.zoff + k];
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
  out[idx] = res;
}

}  // namespace

int ck_loo_down_sum(int type, int diag, const int32_t* child, const float* w, int64_t F, int H, int Ki, int Ko, int M,
                    const float* vals, const float* der, const int64_t* val_off, int fold_off, int64_t B, float* msg,
                    void* stream) {
  return ck::launch_down_sum<DerivativePass>("ck_loo_down_sum", type, diag, child, w, F, H, Ki, Ko, M, vals, der, val_off,
                                             fold_off, B, msg, stream);
}

int ck_loo_segment_lse(const float* msg, const int32_t* cstart, const int32_t* cfold, const int32_t* cfirst,
                       const int32_t* items, float* der, const int64_t* val_off, int64_t n_child, int Ki, int64_t B,
                       void* stream) {
  return ck::launch_segment<DerivativePass>("ck_loo_segment_lse", msg, 0, cstart, cfold, cfirst, items, der, val_off, n_child, Ki,
                                            B, stream);
}

int ck_loo_down_product(int type, const int32_t* cstart, const int32_t* cfold, const int32_t* cfirst, const int32_t* items,
                        const int32_t* child, int layer_fold, const float* vals, float* der, const int64_t* val_off,
                        int64_t n_child, int H, int Ki, int Ko, int64_t B, void* stream) {
  CK_REQUIRE(type == CK_SAMPLE_HADAMARD || type == CK_SAMPLE_KRONECKER, "ck_loo_down_product: not a product layer");
  CK_REQUIRE(cstart != nullptr && cfold != nullptr && cfirst != nullptr && items != nullptr && child != nullptr &&
                 vals != nullptr && der != nullptr && val_off != nullptr,
             "ck_loo_down_product: null pointer");
  CK_REQUIRE(n_child > 0 && H > 0 && Ki > 0 && Ko > 0 && B > 0 && layer_fold >= 0, "ck_loo_down_product: non-positive size");
  if (int st = ck::check_product_shape("ck_loo_down_product", type, H, Ki, Ko)) return st;
  const int64_t blocks = blocks_of(n_child * B * Ki, kThreads);
  CK_REQUIRE(blocks <= 0x7fffffff, "ck_loo_down_product: too many entries");
  return ck::launch(loo_product_kernel, dim3(static_cast<unsigned>(blocks)), dim3(kThreads), 0, stream, type, cstart, cfold,
                    cfirst, items, child, layer_fold, vals, der, val_off, n_child, H, Ki, Ko, B);
}

int ck_loo_leaf_categorical(const int64_t* entries, const int32_t* qstart, int Q, int Cout, int max_units, const float* ntab,
                            const float* lz, const float* der, const int64_t* val_off, const int32_t* bad, int64_t B,
                            float* out, void* stream) {
  CK_REQUIRE(entries != nullptr && qstart != nullptr && ntab != nullptr && lz != nullptr && der != nullptr &&
                 val_off != nullptr && bad != nullptr && out != nullptr,
             "ck_loo_leaf_categorical: null pointer");
  CK_REQUIRE(Q > 0 && Cout > 0 && B > 0 && max_units > 0, "ck_loo_leaf_categorical: non-positive size");
  const int64_t lds = static_cast<int64_t>(kWaves) * max_units * 4;
  CK_REQUIRE(lds <= kMaxLds, "ck_loo_leaf_categorical: %d input units over one variable exceed the LDS budget", max_units);
  const int64_t blocks = blocks_of(B * Q, kWaves);
  CK_REQUIRE(blocks <= 0x7fffffff, "ck_loo_leaf_categorical: too many entries");
  return ck::launch(loo_leaf_cat_generic, dim3(static_cast<unsigned>(blocks)), dim3(kThreads), static_cast<size_t>(lds), stream,
                    reinterpret_cast<const LooEntry*>(entries), qstart, Q, Cout, max_units, ntab, lz, der, val_off, bad, B, out);
}

int ck_loo_leaf_gaussian(const int64_t* entries, const int32_t* qstart, int Q, const float* mean, const float* stddev,
                         const float* der, const int64_t* val_off, const int32_t* bad, int64_t B, float* out, void* stream) {
  CK_REQUIRE(entries != nullptr && qstart != nullptr && mean != nullptr && stddev != nullptr && der != nullptr &&
                 val_off != nullptr && bad != nullptr && out != nullptr,
             "ck_loo_leaf_gaussian: null pointer");
  CK_REQUIRE(Q > 0 && B > 0, "ck_loo_leaf_gaussian: non-positive size");
  const int64_t blocks = blocks_of(B * Q, kThreads);
  CK_REQUIRE(blocks <= 0x7fffffff, "ck_loo_leaf_gaussian: too many entries");
  return ck::launch(loo_leaf_gauss_kernel, dim3(static_cast<unsigned>(blocks)), dim3(kThreads), 0, stream,
                    reinterpret_cast<const LooEntry*>(entries), qstart, Q, mean, stddev, der, val_off, bad, B, out);
}

int ck_loo_log_probs(const int64_t* entries, const int32_t* vstart, const int32_t* vkind, int D, const float* lz,
                     const float* der, const float* vals, const int64_t* val_off, const void* ev, int x_float,
                     const int32_t* bad, int64_t B, float* out, void* stream) {
  CK_REQUIRE(entries != nullptr && vstart != nullptr && vkind != nullptr && lz != nullptr && der != nullptr && vals != nullptr &&
                 val_off != nullptr && ev != nullptr && bad != nullptr && out != nullptr,
             "ck_loo_log_probs: null pointer");
  CK_REQUIRE(D > 0 && B > 0, "ck_loo_log_probs: non-positive size");
  const int64_t blocks = blocks_of(B * D, kThreads);
  CK_REQUIRE(blocks <= 0x7fffffff, "ck_loo_log_probs: too many entries");
  return ck::launch(loo_log_probs_kernel, dim3(static_cast<unsigned>(blocks)), dim3(kThreads), 0, stream,
                    reinterpret_cast<const LooEntry*>(entries), vstart, vkind, D, lz, der, vals, val_off, ev, x_float, bad, B,
                    out);
}
