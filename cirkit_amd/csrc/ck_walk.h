// The top-down walk shared by ancestral sampling (ck_sample.hip), conditional sampling (ck_sample_cond.hip) and the MPE
// argmax walk (ck_mpe.hip), DESIGN.md section 11.  Every walk gives a workgroup S consecutive rows and keeps sel[g * S + s] in
// LDS: the unit of global fold g on row s's induced tree, -1 if g is not on it.  Layers are walked from the last to the
// first; a fold writes the units of its children, which belong to earlier layers, so one barrier per layer orders the walk.
#pragma once

#include <math.h>

#include "ck_internal.h"
#include "ck_philox.h"

namespace ck {

// ---- entry values: the MPE upward pass and the evidence walks ------------------------------------------------------
// One v_add_f32 / v_max3_f32 each.  A plain -O3 build may SLP-pack neighbouring f32 adds into v_pk_add_f32 (register
// pairs, extra moves) and put canonicalising v_max_f32 around fmaxf; the max-plus loop is exactly these two instructions.
__device__ __forceinline__ float mpe_add(float a, float b) {
  float r;
  asm("v_add_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}
__device__ __forceinline__ float mpe_max3(float a, float b, float c) {
  float r;
  asm("v_max3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
  return r;
}

// Child value of entry i of a sum-type unit at chunk row nl.  ch: the fold's (H) global child fold ids; val_off[g] + nl Ki
// is the start of child fold g's Ki values at that row.  Sum / mixing: unit i % Ki of input i / Ki; CP-T: unit i of every
// input, added in input order; Tucker (arity 2): v0[i / Ki] + v1[i % Ki].  The MPE walk recomputes the entries of a unit
// with the same instructions on the same operands as the upward pass, so the maximum it finds is bit for bit the unit value
// the upward pass stored, and the argmax is exact.
__device__ __forceinline__ float entry_value(int type, const int32_t* __restrict__ ch, int H, int Ki,
                                             const float* __restrict__ vals, const int64_t* __restrict__ val_off, int64_t nl,
                                             int i) {
  const int64_t r = nl * Ki;
  if (type == CK_SAMPLE_SUM) return vals[val_off[ch[i / Ki]] + r + i % Ki];
  if (type == CK_SAMPLE_CPT) {
    float v = vals[val_off[ch[0]] + r + i];
    for (int h = 1; h < H; ++h) v = mpe_add(v, vals[val_off[ch[h]] + r + i]);
    return v;
  }
  return mpe_add(vals[val_off[ch[0]] + r + i / Ki], vals[val_off[ch[1]] + r + i % Ki]);  // CK_SAMPLE_TUCKER
}

// Value of the entry under its log weight: log w + entry (log w = -inf for w <= 0).
__device__ __forceinline__ float mpe_term(float lw, float e) { return mpe_add(lw, e); }

// log N(x; mu, sd) (+ log_partition), as the Gaussian forward computes it; at x = mu it is the unit's maximum.
__device__ __forceinline__ float mpe_gauss(float x, float mu, float sd, const float* lz, int64_t o) {
  const float inv_two_var = 1.f / (2.f * (sd * sd));
  const float d = x - mu;
  float lp = -(d * d) * inv_two_var - __logf(sd) - 0.91893853320467274178f;
  if (lz != nullptr) lp += lz[o];
  return lp;
}

// Whether entry o of a masked (B, D) batch is observed; the entry is read once, into e (fp32 batch, x_float) or c (int64).
// Sentinels: a negative int64; in fp32 NaN, or for a discrete layer a value <= -1 (a float batch is truncated, as the
// forward does).
__device__ __forceinline__ bool observed(const void* __restrict__ ev, int64_t o, int x_float, bool gaussian, float& e,
                                         int64_t& c) {
  if (!x_float) {
    c = static_cast<const int64_t*>(ev)[o];
    return c >= 0;
  }
  e = static_cast<const float*>(ev)[o];
  return gaussian ? !isnan(e) : e > -1.f;
}

// ---- draws ---------------------------------------------------------------------------------------------------------
// The one Philox call of the node of global fold g for row n (counter layout: ck_philox.h).
__device__ __forceinline__ Philox4 walk_philox(int64_t n, int g, uint32_t key0, uint32_t key1) {
  return philox4x32_10(static_cast<uint32_t>(n), static_cast<uint32_t>(g), 0u, 0u, key0, key1);
}

// smallest i with t < cdf[i]: an entry whose own mass is positive (t < T is guaranteed by the caller)
__device__ __forceinline__ int cdf_search(const float* __restrict__ row, int M, float t) {
  int lo = 0, hi = M - 1;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (t < row[mid]) hi = mid;
    else lo = mid + 1;
  }
  return lo;
}

// The categorical draw from a CDF row of unnormalised masses.
__device__ __forceinline__ int cdf_draw(const float* __restrict__ row, int M, float u) {
  const float T = row[M - 1];
  if (!(T > 0.f)) return 0;  // (a row with no mass is never reached from a root of positive mass)
  float t = u * T;
  if (t >= T) t = __int_as_float(__float_as_int(T) - 1);  // the float below T (T > 0)
  return cdf_search(row, M, t);
}

// x[o] of the (B, D) output: int64, or fp32 when x_float.  A Gaussian value is only written to an fp32 output (a Gaussian
// layer makes the output fp32: DESIGN.md section 11).
__device__ __forceinline__ void store_category(void* __restrict__ x, int x_float, int64_t o, int c) {
  if (x_float) static_cast<float*>(x)[o] = static_cast<float>(c);
  else static_cast<int64_t*>(x)[o] = c;
}
__device__ __forceinline__ void store_value(void* __restrict__ x, int x_float, int64_t o, float v) {
  if (x_float) static_cast<float*>(x)[o] = v;
}

// The draw of unit k of input fold f into x[o]: Categorical / Binomial from its CDF row, Gaussian mean + stddev z with z
// from Box-Muller on (x0, x1) of the node's Philox call.
__device__ __forceinline__ void draw_input(const ck_sample_layer& L, int f, int k, const Philox4& p, void* __restrict__ x,
                                           int x_float, int64_t o) {
  const int64_t u = static_cast<int64_t>(f) * L.Ko + k;
  if (L.type == CK_SAMPLE_GAUSSIAN) {
    const float u1 = static_cast<float>((p.x[0] >> 8) + 1u) * 5.9604644775390625e-8f;
    const float u2 = philox_uniform(p.x[1]);
    const float z = sqrtf(-2.f * logf(u1)) * cospif(2.f * u2);
    store_value(x, x_float, o, L.mean[u] + L.stddev[u] * z);
  } else {
    store_category(x, x_float, o, cdf_draw(L.cdf + u * L.M, L.M, philox_uniform(p.x[0])));
  }
}

// ---- the walk ------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool is_input(int type) { return type == CK_SAMPLE_CATEGORICAL || type == CK_SAMPLE_GAUSSIAN; }

// Every fold off the tree; the root unit's Ko is returned for the evidence walks, which read the root's value.
__device__ __forceinline__ int walk_init(int16_t* sel, int total_folds, int S, const ck_sample_layer* __restrict__ layers,
                                         int n_layers, int root_fold) {
  for (int i = threadIdx.x; i < total_folds * S; i += blockDim.x) sel[i] = -1;
  int root_ko = 0;
  for (int j = 0; j < n_layers; ++j) {
    if (root_fold >= layers[j].fold_off && root_fold < layers[j].fold_off + layers[j].F) root_ko = layers[j].Ko;
  }
  return root_ko;
}

// A product unit k on the tree of row s passes through: Hadamard, unit k of every input; Kronecker, unit k = (u_0, ...,
// u_{H-1}) in base Ki, input 0 most significant.
__device__ __forceinline__ void walk_product(const ck_sample_layer& L, const int32_t* ch, int16_t* sel, int S, int s, int k) {
  if (L.type == CK_SAMPLE_HADAMARD) {
    for (int h = 0; h < L.H; ++h) sel[ch[h] * S + s] = static_cast<int16_t>(k);
    return;
  }
  int r = k;
  for (int h = L.H - 1; h >= 0; --h) {
    sel[ch[h] * S + s] = static_cast<int16_t>(r % L.Ki);
    r /= L.Ki;
  }
}

// The children of chosen entry i of a sum-type unit: sum / mixing, unit i % Ki of input i / Ki; CP-T, unit i of every input;
// Tucker (arity 2), unit i / Ki of input 0 and unit i % Ki of input 1.
__device__ __forceinline__ void walk_child(const ck_sample_layer& L, const int32_t* ch, int16_t* sel, int S, int s, int i) {
  if (L.type == CK_SAMPLE_SUM) {
    sel[ch[i / L.Ki] * S + s] = static_cast<int16_t>(i % L.Ki);
  } else if (L.type == CK_SAMPLE_CPT) {
    for (int h = 0; h < L.H; ++h) sel[ch[h] * S + s] = static_cast<int16_t>(i);
  } else {
    sel[ch[0] * S + s] = static_cast<int16_t>(i / L.Ki);
    sel[ch[1] * S + s] = static_cast<int16_t>(i % L.Ki);
  }
}

// choices[f, n] when recorded: entry i in the user's unit numbering, -1 for no choice (off the tree, or nothing drawn).
__device__ __forceinline__ void walk_record(const ck_sample_layer& L, int f, int64_t N, int64_t n, int i) {
  if (L.choices != nullptr) L.choices[static_cast<int64_t>(f) * N + n] = i < 0 ? -1 : (L.cmap != nullptr ? L.cmap[i] : i);
}

// One thread per item (fold f, row s) of layer L.  Inner layers: consecutive threads = consecutive rows of one fold (one
// CDF row region, coalesced `choices`); input layers: consecutive threads = consecutive folds of one row (neighbouring
// variables of one output row).  A product unit on the tree passes through; visit(f, s, g, k) gets every other item, with
// k = -1 off the tree.
template <class Visit>
__device__ __forceinline__ void walk_items(const ck_sample_layer& L, int16_t* sel, int S, int ns, Visit&& visit) {
  const bool input = is_input(L.type);
  for (int it = threadIdx.x; it < L.F * ns; it += blockDim.x) {
    const int f = input ? it % L.F : it / ns;
    const int s = input ? it / L.F : it % ns;
    const int g = L.fold_off + f;
    const int k = sel[g * S + s];
    const bool on = k >= 0 && k < L.Ko;
    if (on && (L.type == CK_SAMPLE_HADAMARD || L.type == CK_SAMPLE_KRONECKER))
      walk_product(L, L.child + static_cast<int64_t>(f) * L.H, sel, S, s, k);
    else
      visit(f, s, g, on ? k : -1);
  }
}

// The checks and the grid of every walk launch: `rows` rows, S per workgroup, total_folds * S int16 of LDS.
inline int walk_grid(const char* fn, int n_layers, int root_fold, int root_unit, int total_folds, int S, int64_t rows, int D,
                     size_t& lds, unsigned& blocks) {
  CK_REQUIRE(n_layers > 0 && total_folds > 0 && rows > 0 && D > 0 && S > 0, "%s: non-positive size", fn);
  CK_REQUIRE(root_fold >= 0 && root_fold < total_folds && root_unit >= 0 && root_unit < 32768, "%s: root out of range", fn);
  const int64_t bytes = static_cast<int64_t>(total_folds) * S * 2;
  CK_REQUIRE(bytes <= CK_SAMPLE_MAX_LDS, "%s: %d folds x %d rows exceed the LDS budget", fn, total_folds, S);
  const int64_t b = (rows + S - 1) / S;
  CK_REQUIRE(b <= 0x7fffffff, "%s: too many rows", fn);
  lds = static_cast<size_t>(bytes);
  blocks = static_cast<unsigned>(b);
  return 0;
}

// ---- the evidence walk: conditional sampling and MPE ---------------------------------------------------------------
constexpr int kEvidenceWalkThreads = 1024;  // 16 waves: the walk is latency-bound, a workgroup's LDS table limits residency
constexpr int kEvidenceWalkWaves = kEvidenceWalkThreads / kWave;

// Rows row0 + b0 .. of a chunk of B rows, each with its own evidence ev (B, D).  vals / val_off: the chunk's per-row unit
// values, global fold g's (B, Ko) block at vals + val_off[g].  tabs[li]: the (F, Ko, M) weight table of sum-type layer li
// that the walk policy P reads.  P supplies:
//   root(n, r)         whether row n, of root value r, has a tree;
//   choose(L, wr, ...) the entry a sum-type unit on the tree takes, wave-uniform, or -1 (wr: the unit's weight row);
//   fill(L, li, ...)   the value of an unobserved variable of input unit k.
// Sum-type layers take one wave per (fold, row); product and input layers one thread per item (walk_items).
template <class P>
__global__ void __launch_bounds__(kEvidenceWalkThreads)
    evidence_walk_kernel(const ck_sample_layer* __restrict__ layers, const float* const* __restrict__ tabs, int n_layers,
                         int root_fold, int root_unit, int total_folds, int S, const float* __restrict__ vals,
                         const int64_t* __restrict__ val_off, int64_t row0, int64_t B, int64_t N, int D,
                         const void* __restrict__ ev, void* __restrict__ x, int x_float, P p) {
  extern __shared__ int16_t sel[];
  const int64_t b0 = static_cast<int64_t>(blockIdx.x) * S;  // chunk row of the workgroup's row 0
  const int ns = static_cast<int>(B - b0 < S ? B - b0 : S);
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = threadIdx.x / kWave;
  const int root_ko = walk_init(sel, total_folds, S, layers, n_layers, root_fold);
  __syncthreads();
  for (int s = threadIdx.x; s < ns; s += blockDim.x) {
    if (p.root(row0 + b0 + s, vals[val_off[root_fold] + (b0 + s) * root_ko + root_unit]))
      sel[root_fold * S + s] = static_cast<int16_t>(root_unit);
  }
  __syncthreads();
  for (int li = n_layers - 1; li >= 0; --li) {
    const ck_sample_layer& L = layers[li];
    if (L.type == CK_SAMPLE_SUM || L.type == CK_SAMPLE_CPT || L.type == CK_SAMPLE_TUCKER) {
      const float* __restrict__ W = tabs[li];
      for (int it = wave; it < L.F * ns; it += kEvidenceWalkWaves) {  // (wave-uniform: every lane of a wave has the same item)
        const int f = it / ns, s = it % ns;
        const int64_t nl = b0 + s, n = row0 + nl;
        const int g = L.fold_off + f;
        const int k = sel[g * S + s];
        const int32_t* ch = L.child + static_cast<int64_t>(f) * L.H;
        int choice = -1;
        if (k >= 0 && k < L.Ko)
          choice = p.choose(L, W + (static_cast<int64_t>(f) * L.Ko + k) * L.M, ch, vals, val_off, nl, n, g, lane);
        if (lane == 0) {
          if (choice >= 0) walk_child(L, ch, sel, S, s, choice);
          walk_record(L, f, N, n, choice);
        }
      }
      __syncthreads();
      continue;
    }
    walk_items(L, sel, S, ns, [&](int f, int s, int g, int k) {
      if (k < 0) return;
      // input layers write only unobserved entries (the output starts as a copy of the masked evidence)
      const int64_t nl = b0 + s, o = nl * D + L.scope[f];
      float e;
      int64_t c;
      if (!observed(ev, o, x_float, L.type == CK_SAMPLE_GAUSSIAN, e, c)) p.fill(L, li, f, k, row0 + nl, g, x, x_float, o);
    });
    __syncthreads();
  }
}

// One launch of evidence_walk_kernel<P> over rows row0 .. row0 + B - 1 of a batch of N rows.
template <class P>
int evidence_walk(const char* fn, const ck_sample_layer* layers, const float* const* tabs, int n_layers, int root_fold,
                  int root_unit, int total_folds, int S, const float* vals, const int64_t* val_off, int64_t row0, int64_t B,
                  int64_t N, int D, const void* ev, void* x, int x_float, const P& p, void* stream) {
  CK_REQUIRE(layers != nullptr && tabs != nullptr && vals != nullptr && val_off != nullptr && ev != nullptr && x != nullptr,
             "%s: null pointer", fn);
  CK_REQUIRE(row0 >= 0 && row0 + B <= N, "%s: rows %lld .. %lld outside the %lld rows of the batch", fn,
             static_cast<long long>(row0), static_cast<long long>(row0 + B), static_cast<long long>(N));
  size_t lds;
  unsigned blocks;
  if (int st = walk_grid(fn, n_layers, root_fold, root_unit, total_folds, S, B, D, lds, blocks)) return st;
  return launch(evidence_walk_kernel<P>, dim3(blocks), dim3(kEvidenceWalkThreads), lds, stream, layers, tabs, n_layers, root_fold,
                root_unit, total_folds, S, vals, val_off, row0, B, N, D, ev, x, x_float, p);
}

}  // namespace ck
