// Posterior marginals ("Posterior marginals"): the top-down FLOW pass behind
// `HipCircuit.posterior_marginals`.  With v the per-row log values of the layer-wise marginal forward of the evidence, the
// flow of a unit is f(u) = d log c(x_O) / d log u, in LINEAR space, f(root) = 1.  Flows live in an fp32 arena laid out as the
// value arena (global fold g's (B, Ko) block at val_off[g]).  The pass itself -- contraction, message blocks, segment add --
// is ck_down.h's, instantiated with FlowPass below; this file adds the Kronecker kernel and the leaves.
#include <math.h>

#include "ck_down.h"

namespace {

using ck::blocks_of;
using ck::f32x16;
using ck::kThreads;
using ck::kWaves;

// T exp(m + e) with nothing exponentiated unshifted; T = 0 gives exactly 0, e = -inf gives 0.
__device__ __forceinline__ float flow_out(float T, float m, float e) {
  if (!(T > 0.f)) return 0.f;
  if (e == -INFINITY) return 0.f;
  return ck::scaled_exp(T, m, e);
}

// Where the flow of entry i of fold f at row n goes: sum / mixing slot f H + i / Ki unit i % Ki; CP-T slot f unit i.
__device__ __forceinline__ int64_t msg_index(int type, int64_t f, int H, int Ki, int64_t B, int64_t n, int i) {
  const int64_t slot = type == CK_SAMPLE_SUM ? f * H + i / Ki : f;
  const int unit = type == CK_SAMPLE_SUM ? i % Ki : i;
  return (slot * B + n) * Ki + unit;
}

// The flow pass as a policy of ck_down.h: the factor of a unit is a = f exp(-v - m), entry i receives the flow
// T exp(m + e_i), a child adds what its consumers send.
struct FlowPass {
  static __device__ __forceinline__ float key(float f, float v) { return ck::flow_lg(f, v); }
  static __device__ __forceinline__ float factor(float f, float v, float m) { return ck::flow_a(f, v, m); }
  static __device__ __forceinline__ float emit(bool tucker, int type, const int32_t* __restrict__ ch, int64_t f, int H, int Ki,
                                               int64_t B, int64_t n, int i, float T, float m, const float* __restrict__ vals,
                                               const int64_t* __restrict__ val_off, float* __restrict__ msg) {
    float fl = 0.f;
    if (T > 0.f) fl = flow_out(T, m, ck::entry_value(type, ch, H, Ki, vals, val_off, n, i));
    if (!tucker) msg[msg_index(type, f, H, Ki, B, n, i)] = fl;
    return fl;
  }
  // Tucker: input 0 unit a receives the sum over b, input 1 unit b the sum over a
  static __device__ __forceinline__ float tucker(const float* row, int Ki, int s, int u, const int32_t* __restrict__,
                                                 const float* __restrict__, const int64_t* __restrict__, int64_t) {
    float acc = 0.f;
    if (s == 0) {
      for (int b = 0; b < Ki; ++b) acc += row[u * Ki + b];
    } else {
      for (int a = 0; a < Ki; ++a) acc += row[a * Ki + u];
    }
    return acc;
  }
  static __device__ __forceinline__ float identity() { return 0.f; }
  static __device__ __forceinline__ float combine(float a, float b) { return a + b; }
};

// Kronecker: item (parent global fold g, input position h); unit i of the child receives the sum of the parent's flow over
// the outputs whose digit h (base Ki, input 0 most significant) is i, in ascending output order.
__global__ void __launch_bounds__(kThreads)
    flow_kron_kernel(const int32_t* __restrict__ cstart, const int32_t* __restrict__ cfold, const int32_t* __restrict__ cfirst,
                     const int32_t* __restrict__ items, float* flow, const int64_t* __restrict__ val_off, int64_t n_child,
                     int H, int Ki, int Ko, int64_t B) {
  const int64_t idx = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  const int64_t per = B * Ki;
  if (idx >= n_child * per) return;
  const int64_t c = idx / per, rem = idx % per;
  const int64_t n = rem / Ki;
  const int i = static_cast<int>(rem % Ki);
  float* dst = flow + val_off[cfold[c]] + rem;
  float acc = cfirst[c] ? 0.f : *dst;
  for (int s = cstart[c]; s < cstart[c + 1]; ++s) {
    const float* p = flow + val_off[items[2 * s]] + n * Ko;
    int stride = 1;
    for (int h = H - 1; h > items[2 * s + 1]; --h) stride *= Ki;
    for (int top = 0; top < Ko / (stride * Ki); ++top)
      for (int lo = 0; lo < stride; ++lo) acc += p[(top * Ki + i) * stride + lo];
  }
  *dst = acc;
}

// ---- leaves --------------------------------------------------------------------------------------------------------
// Per query variable q the entries qstart[q] .. qstart[q + 1] - 1, one per input fold over that variable, four int64 each:
// (global fold, units K, states C of the fold's table, element offset of its (K, C) block in `ntab` -- or of its K means /
// standard deviations for the Gaussian kernel).
struct LeafEntry {
  int64_t g, K, C, off;
};

// A row has a posterior when its root value is finite and its evidence was in range (bad[n] == 0, ck_flow_check_evidence).
__device__ __forceinline__ bool row_ok(const float* __restrict__ vals, const int64_t* __restrict__ val_off, int root_fold,
                                       int root_ko, const int32_t* __restrict__ bad, int64_t n) {
  const float r = vals[val_off[root_fold] + n * root_ko];
  return r > -INFINITY && r < INFINITY && bad[n] == 0;
}

// logev[n]: the root value of the row, NaN where its evidence was out of range.
__global__ void __launch_bounds__(kThreads)
    flow_logev_kernel(const float* __restrict__ vals, const int64_t* __restrict__ val_off, int root_fold, int root_ko,
                      const int32_t* __restrict__ bad, int64_t B, float* __restrict__ logev) {
  const int64_t n = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (n < B) logev[n] = bad[n] ? NAN : vals[val_off[root_fold] + n * root_ko];
}

// The range check of a chunk of masked evidence ev (B, D), int64 or fp32 (x_float), against states[d], the number of states
// the discrete input layers index variable d with (0: none does).  clean gets the evidence with every out-of-range observed
// category replaced by 0, so that the evidence forward stays finite for the other rows; bad[n] = 1 and *flag |= 1 (flag may be
// NULL) for a row that held one.  Sentinels as the forward reads them: a negative int64; in fp32 NaN or a value <= -1 (a float
// batch is truncated).
__global__ void __launch_bounds__(kThreads)
    flow_check_evidence_kernel(const void* __restrict__ ev, int x_float, const int32_t* __restrict__ states, int64_t B, int D,
                               void* __restrict__ clean, int32_t* __restrict__ bad, int32_t* flag) {
  const int64_t o = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (o >= B * D) return;
  const int S = states[o % D];
  bool out_of_range = false;
  if (x_float) {
    const float e = static_cast<const float*>(ev)[o];
    out_of_range = S > 0 && e > -1.f && e >= static_cast<float>(S);
    static_cast<float*>(clean)[o] = out_of_range ? 0.f : e;
  } else {
    const int64_t c = static_cast<const int64_t*>(ev)[o];
    out_of_range = S > 0 && c >= S;
    static_cast<int64_t*>(clean)[o] = out_of_range ? 0 : c;
  }
  if (out_of_range) {
    bad[o / D] = 1;
    if (flag != nullptr) atomicOr(flag, 1);
  }
}

__global__ void __launch_bounds__(kThreads)
    flow_leaf_cat_generic(const LeafEntry* __restrict__ ent, const int32_t* __restrict__ qstart, int Q, int Cout,
                          const float* __restrict__ ntab, const float* __restrict__ flow, const float* __restrict__ vals,
                          const int64_t* __restrict__ val_off, int root_fold, int root_ko, const int32_t* __restrict__ bad, int64_t B,
                          float* __restrict__ out) {
  const int64_t idx = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (idx >= B * Q * Cout) return;
  const int c = static_cast<int>(idx % Cout);
  const int q = static_cast<int>((idx / Cout) % Q);
  const int64_t n = idx / (static_cast<int64_t>(Cout) * Q);
  float acc = 0.f;
  if (!row_ok(vals, val_off, root_fold, root_ko, bad, n)) {
    acc = NAN;
  } else {
    for (int s = qstart[q]; s < qstart[q + 1]; ++s) {
      const LeafEntry e = ent[s];
      if (c >= e.C) continue;
      const float* fr = flow + val_off[e.g] + n * e.K;
      const float* t = ntab + e.off + c;
      for (int k = 0; k < e.K; ++k) acc = fmaf(fr[k], t[k * e.C], acc);
    }
  }
  out[idx] = acc;
}

// The same on the fp32 matrix cores, every entry with K units: a workgroup owns (q, 32 rows), its waves the 32-state column
// tiles; (32 rows x K) flows x (K x 32) normalised table rows per entry, the unit order of down_sum_mfma.  A wave
// stores, per accumulator register, two rows of 32 consecutive states: whole 128-byte lines.
template <int K>
__global__ void __launch_bounds__(kThreads)
    flow_leaf_cat_mfma(const LeafEntry* __restrict__ ent, const int32_t* __restrict__ qstart, int Q, int Cout,
                       const float* __restrict__ ntab, const float* __restrict__ flow, const float* __restrict__ vals,
                       const int64_t* __restrict__ val_off, int root_fold, int root_ko, const int32_t* __restrict__ bad, int64_t B,
                       int64_t row_tiles, float* __restrict__ out) {
  constexpr int KH = K / 2;
  __shared__ float sok[kWaves][32];
  const int lane = threadIdx.x & (ck::kWave - 1), wave = threadIdx.x / ck::kWave;
  const int b = lane & 31, hi = lane >> 5;
  const int q = static_cast<int>(blockIdx.x / row_tiles);
  const int64_t n0 = (blockIdx.x % row_tiles) * 32;
  const int64_t nb = n0 + b < B ? n0 + b : B - 1;
  if (hi == 0) sok[wave][b] = row_ok(vals, val_off, root_fold, root_ko, bad, nb) ? 0.f : NAN;
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  const int s0 = qstart[q], s1 = qstart[q + 1];
  for (int c0 = wave * 32; c0 < Cout; c0 += kWaves * 32) {
    const int c = c0 + b;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    for (int s = s0; s < s1; ++s) {
      const LeafEntry e = ent[s];
      const int C = static_cast<int>(e.C);
      const float* fr = flow + val_off[e.g] + nb * K + hi * KH;
      const float* t = ntab + e.off + static_cast<int64_t>(hi) * KH * C + (c < C ? c : C - 1);
      const float keep = c < C ? 1.f : 0.f;
#pragma unroll
      for (int kk = 0; kk < KH; ++kk)
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(fr[kk], keep * t[static_cast<int64_t>(kk) * C], acc, 0, 0, 0);
    }
    if (c >= Cout) continue;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = 8 * (r >> 2) + 4 * hi + (r & 3);
      const int64_t n = n0 + row;
      if (n < B) out[(n * Q + q) * Cout + c] = acc[r] + sok[wave][row];
    }
  }
}

// Gaussian query variables: out[n, q] = (S1, S2 - S1^2) with S1 = sum f_k mean_k and S2 = sum f_k (stddev_k^2 + mean_k^2)
// over the units of the variable's input folds: the mean and the variance of the mixture sum_k f_k N(mean_k, stddev_k^2).
__global__ void __launch_bounds__(kThreads)
    flow_leaf_gauss_kernel(const LeafEntry* __restrict__ ent, const int32_t* __restrict__ qstart, int Q,
                           const float* __restrict__ mean, const float* __restrict__ stddev, const float* __restrict__ flow,
                           const float* __restrict__ vals, const int64_t* __restrict__ val_off, int root_fold, int root_ko,
                           const int32_t* __restrict__ bad, int64_t B, float* __restrict__ out) {
  const int64_t idx = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (idx >= B * Q) return;
  const int q = static_cast<int>(idx % Q);
  const int64_t n = idx / Q;
  float s1 = 0.f, s2 = 0.f;
  if (!row_ok(vals, val_off, root_fold, root_ko, bad, n)) {
    s1 = s2 = NAN;
  } else {
    for (int s = qstart[q]; s < qstart[q + 1]; ++s) {
      const LeafEntry e = ent[s];
      const float* fr = flow + val_off[e.g] + n * e.K;
      for (int k = 0; k < e.K; ++k) {
        const float mu = mean[e.off + k], sd = stddev[e.off + k];
        s1 = fmaf(fr[k], mu, s1);
        s2 = fmaf(fr[k], fmaf(sd, sd, mu * mu), s2);
      }
    }
  }
  out[idx * 2] = s1;
  out[idx * 2 + 1] = s2 - s1 * s1;
}

}  // namespace

int ck_flow_down_sum(int type, int diag, const int32_t* child, const float* w, int64_t F, int H, int Ki, int Ko, int M,
                     const float* vals, const float* flow, const int64_t* val_off, int fold_off, int64_t B, float* msg,
                     void* stream) {
  return ck::launch_down_sum<FlowPass>("ck_flow_down_sum", type, diag, child, w, F, H, Ki, Ko, M, vals, flow, val_off, fold_off, B,
                                       msg, stream);
}

int ck_flow_segment_add(const float* msg, const int32_t* cstart, const int32_t* cfold, const int32_t* cfirst,
                        const int32_t* items, float* flow, const int64_t* val_off, int64_t n_child, int Ki, int64_t B,
                        void* stream) {
  return ck::launch_segment<FlowPass>("ck_flow_segment_add", msg, 0, cstart, cfold, cfirst, items, flow, val_off, n_child, Ki, B,
                                      stream);
}

int ck_flow_down_product(int type, const int32_t* cstart, const int32_t* cfold, const int32_t* cfirst, const int32_t* items,
                         float* flow, const int64_t* val_off, int64_t n_child, int H, int Ki, int Ko, int64_t B,
                         void* stream) {
  CK_REQUIRE(type == CK_SAMPLE_HADAMARD || type == CK_SAMPLE_KRONECKER, "ck_flow_down_product: not a product layer");
  CK_REQUIRE(cstart != nullptr && cfold != nullptr && cfirst != nullptr && items != nullptr && flow != nullptr &&
                 val_off != nullptr,
             "ck_flow_down_product: null pointer");
  CK_REQUIRE(n_child > 0 && H > 0 && Ki > 0 && Ko > 0 && B > 0, "ck_flow_down_product: non-positive size");
  if (int st = ck::check_product_shape("ck_flow_down_product", type, H, Ki, Ko)) return st;
  if (type == CK_SAMPLE_HADAMARD)  // unit k of every input receives f_k: the items are folds of the flow arena itself
    return ck::launch_segment<FlowPass>("ck_flow_down_product", flow, 1, cstart, cfold, cfirst, items, flow, val_off, n_child, Ki,
                                        B, stream);
  const int64_t blocks = blocks_of(n_child * B * Ki, kThreads);
  CK_REQUIRE(blocks <= 0x7fffffff, "ck_flow_down_product: too many entries");
  return ck::launch(flow_kron_kernel, dim3(static_cast<unsigned>(blocks)), dim3(kThreads), 0, stream, cstart, cfold, cfirst,
                    items, flow, val_off, n_child, H, Ki, Ko, B);
}

// The (B,) log evidence behind a leaf launch (logev may be NULL).
static int launch_logev(const float* vals, const int64_t* val_off, int root_fold, int root_ko, const int32_t* bad, int64_t B,
                        float* logev, void* stream) {
  if (logev == nullptr) return 0;
  const int64_t blocks = blocks_of(B, kThreads);
  return ck::launch(flow_logev_kernel, dim3(static_cast<unsigned>(blocks)), dim3(kThreads), 0, stream, vals, val_off, root_fold,
                    root_ko, bad, B, logev);
}

int ck_flow_check_evidence(const void* ev, int x_float, const int32_t* states, int64_t B, int D, void* clean, int32_t* bad,
                           int32_t* flag, void* stream) {
  CK_REQUIRE(ev != nullptr && states != nullptr && clean != nullptr && bad != nullptr, "ck_flow_check_evidence: null pointer");
  CK_REQUIRE(B > 0 && D > 0, "ck_flow_check_evidence: non-positive size");
  const int64_t blocks = blocks_of(B * D, kThreads);
  CK_REQUIRE(blocks <= 0x7fffffff, "ck_flow_check_evidence: too many entries");
  return ck::launch(flow_check_evidence_kernel, dim3(static_cast<unsigned>(blocks)), dim3(kThreads), 0, stream, ev, x_float,
                    states, B, D, clean, bad, flag);
}

int ck_flow_leaf_categorical(const int64_t* entries, const int32_t* qstart, int Q, int Cout, int K_uniform, const float* ntab,
                             const float* flow, const float* vals, const int64_t* val_off, int root_fold, int root_ko,
                             const int32_t* bad, int64_t B, float* out, float* logev, void* stream) {
  CK_REQUIRE(entries != nullptr && qstart != nullptr && ntab != nullptr && flow != nullptr && vals != nullptr &&
                 val_off != nullptr && bad != nullptr && out != nullptr,
             "ck_flow_leaf_categorical: null pointer");
  CK_REQUIRE(Q > 0 && Cout > 0 && B > 0 && root_fold >= 0 && root_ko > 0 && K_uniform >= 0,
             "ck_flow_leaf_categorical: non-positive size");
  if (int st = launch_logev(vals, val_off, root_fold, root_ko, bad, B, logev, stream)) return st;
  const LeafEntry* ent = reinterpret_cast<const LeafEntry*>(entries);
  if (K_uniform == 32 || K_uniform == 64) {
    const int64_t row_tiles = (B + 31) / 32;
    CK_REQUIRE(Q * row_tiles <= 0x7fffffff, "ck_flow_leaf_categorical: grid too large");
    const dim3 grid(static_cast<unsigned>(Q * row_tiles));
    auto kern = K_uniform == 32 ? flow_leaf_cat_mfma<32> : flow_leaf_cat_mfma<64>;
    return ck::launch(kern, grid, dim3(kThreads), 0, stream, ent, qstart, Q, Cout, ntab, flow, vals, val_off, root_fold, root_ko,
                      bad, B, row_tiles, out);
  }
  const int64_t blocks = blocks_of(B * Q * Cout, kThreads);
  CK_REQUIRE(blocks <= 0x7fffffff, "ck_flow_leaf_categorical: too many entries");
  return ck::launch(flow_leaf_cat_generic, dim3(static_cast<unsigned>(blocks)), dim3(kThreads), 0, stream, ent, qstart, Q, Cout,
                    ntab, flow, vals, val_off, root_fold, root_ko, bad, B, out);
}

int ck_flow_leaf_gaussian(const int64_t* entries, const int32_t* qstart, int Q, const float* mean, const float* stddev,
                          const float* flow, const float* vals, const int64_t* val_off, int root_fold, int root_ko,
                          const int32_t* bad, int64_t B, float* out, float* logev, void* stream) {
  CK_REQUIRE(entries != nullptr && qstart != nullptr && mean != nullptr && stddev != nullptr && flow != nullptr &&
                 vals != nullptr && val_off != nullptr && bad != nullptr && out != nullptr,
             "ck_flow_leaf_gaussian: null pointer");
  CK_REQUIRE(Q > 0 && B > 0 && root_fold >= 0 && root_ko > 0, "ck_flow_leaf_gaussian: non-positive size");
  if (int st = launch_logev(vals, val_off, root_fold, root_ko, bad, B, logev, stream)) return st;
  const int64_t blocks = blocks_of(B * Q, kThreads);
  CK_REQUIRE(blocks <= 0x7fffffff, "ck_flow_leaf_gaussian: too many entries");
  return ck::launch(flow_leaf_gauss_kernel, dim3(static_cast<unsigned>(blocks)), dim3(kThreads), 0, stream,
                    reinterpret_cast<const LeafEntry*>(entries), qstart, Q, mean, stddev, flow, vals, val_off, root_fold, root_ko,
                    bad, B, out);
}
