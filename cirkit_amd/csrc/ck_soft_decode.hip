// Decoding under soft evidence: the kernels of `HipCircuit.soft_mpe` and `HipCircuit.sample_soft` (DESIGN.md section 11,
// "Decoding under soft evidence").  The reference has no such query.
//
//   * soft_max_leaf_kernel: the max-product value of the input units over a soft variable,
//     out[n, k] = max_c (table[f, c, k] + log_lik[n, spos[f], c]), into the fold's (B, K) block of the MPE arena: a max-plus
//     contraction built like mpe_up_sum_kernel (ck_mpe.hip) -- a workgroup owns (fold, row tile, unit tile), the rows'
//     log_lik and the fold's log table go through LDS in slices of kSC states, every thread keeps a kRM x kKM micro-tile of
//     maxima, two states per 3-way max, each after its add (ck::mpe_add / ck::mpe_max3);
//   * the walk policies SoftSampleWalk / SoftMpeWalk: CondDraw / MpeArgmax with a `fill` that, at an input fold over a soft
//     variable, records the node the row's tree reached instead of writing a value;
//   * soft_decode_leaf_kernel: per (row, soft variable) with a recorded node (fold g, unit k), a group of W lanes along the
//     states, reading the unit's row of the transposed log table, takes argmax_c (table[c, k] + log_lik[n, s, c]) (smallest
//     index among equal maxima; the maximum is bit for bit the value the max leaf stored) or draws c in proportion to
//     exp(table[c, k] + log_lik[n, s, c]), the exact two-pass form relative to the maximum.  Everything stays in log space:
//     a table in a far tail under peaked evidence (the soft leaf's trap) loses nothing here.
#include <limits.h>
#include <math.h>

#include "ck_cond_policy.h"
#include "ck_mpe_policy.h"
#include "ck_soft_entry.h"

namespace {

using ck::kKM;
using ck::kRM;
using ck::kUpThreads;
using ck::SoftEntry;

constexpr int kSC = 32;          // states staged in LDS per step: one 128-byte line of every row
constexpr int kNodeUnits = 32768;  // a recorded node is g * kNodeUnits + k (units < 32768, folds <= 32768: cirkit_amd/sampling.py)

__device__ __forceinline__ bool unusable(float v) { return v != v || v == INFINITY; }  // NaN or +inf: the row gets nothing

// ---- the max leaf --------------------------------------------------------------------------------------------------
// A thread stages NL 16-byte pieces of the rows per step (`vec`: one load each; C and Cl multiples of 4, log_lik aligned): all
// of them are in flight before the first is written to LDS.  A NaN / +inf in a read entry sets bad[n].
template <int TK>
__global__ void __launch_bounds__(kUpThreads)
    soft_max_leaf_kernel(const float* __restrict__ table, const float* __restrict__ ll, const int32_t* __restrict__ spos,
                         float* __restrict__ vals, const int64_t* __restrict__ val_off, int fold_off,
                         int32_t* __restrict__ bad, int64_t B, int K, int C, int S, int Cl, int64_t row_tiles, int vec) {
  constexpr int TKT = TK / kKM;          // threads along the units
  constexpr int TRT = kUpThreads / TKT;  // threads along the rows
  constexpr int TR = TRT * kRM;          // rows of the tile
  constexpr int EP = TR + 4;             // (padded LDS row)
  constexpr int LPR = kSC / 4;           // 16-byte pieces of a row per step
  constexpr int NL = TR * LPR / kUpThreads;
  __shared__ float4 sE[kSC * EP / 4];  // sE[m][r]: log_lik of state c0 + m, tile row r
  __shared__ float4 sW[kSC * TK / 4];  // sW[m][k]: table of state c0 + m, unit k0 + k
  float* const sEf = reinterpret_cast<float*>(sE);
  float* const sWf = reinterpret_cast<float*>(sW);
  const int64_t f = blockIdx.x / row_tiles;
  const int s = spos[f];
  if (s < 0) return;  // a hard variable: ck_mpe_up_input wrote this fold
  const int64_t n0 = (blockIdx.x % row_tiles) * TR;
  const int k0 = blockIdx.y * TK;
  const int tk = threadIdx.x % TKT, tr = threadIdx.x / TKT;
  const float* tf = table + f * (C + 1) * K;
  float acc[kRM][kKM];
#pragma unroll
  for (int i = 0; i < kRM; ++i)
#pragma unroll
    for (int j = 0; j < kKM; ++j) acc[i][j] = -INFINITY;
  for (int c0 = 0; c0 < C; c0 += kSC) {
    float4 v[NL];
#pragma unroll
    for (int i = 0; i < NL; ++i) {
      const int t = threadIdx.x + i * kUpThreads;
      const int r = t / LPR, c = c0 + 4 * (t % LPR);
      const int64_t n = n0 + r;
      v[i] = make_float4(0.f, 0.f, 0.f, 0.f);  // (states past C, rows past B: 0 under a table entry of -inf, or not stored)
      if (n < B && c < C) {
        const float* row = ll + (n * S + s) * static_cast<int64_t>(Cl) + c;
        if (vec) {
          v[i] = ck::gload4(row);
        } else {
          v[i].x = row[0];
          if (c + 1 < C) v[i].y = row[1];
          if (c + 2 < C) v[i].z = row[2];
          if (c + 3 < C) v[i].w = row[3];
        }
      }
    }
#pragma unroll
    for (int i = 0; i < NL; ++i) {
      const int t = threadIdx.x + i * kUpThreads;
      const int r = t / LPR, m = 4 * (t % LPR);
      const float4 a = v[i];
      if (unusable(a.x) || unusable(a.y) || unusable(a.z) || unusable(a.w)) bad[n0 + r] = 1;  // (only read entries can be)
      sEf[m * EP + r] = a.x;
      sEf[(m + 1) * EP + r] = a.y;
      sEf[(m + 2) * EP + r] = a.z;
      sEf[(m + 3) * EP + r] = a.w;
    }
    for (int t = threadIdx.x; t < TK * kSC; t += kUpThreads) {
      const int k = t % TK, m = t / TK;
      sWf[m * TK + k] = (c0 + m < C && k0 + k < K) ? tf[static_cast<int64_t>(c0 + m) * K + k0 + k] : -INFINITY;
    }
    __syncthreads();
#pragma unroll
    for (int m = 0; m < kSC; m += 2) {
      const float4 e0 = sE[(m * EP) / 4 + tr], e1 = sE[((m + 1) * EP) / 4 + tr];
      const float4 w0 = sW[(m * TK) / 4 + tk], w1 = sW[((m + 1) * TK) / 4 + tk];
      const float ea[kRM] = {e0.x, e0.y, e0.z, e0.w}, eb[kRM] = {e1.x, e1.y, e1.z, e1.w};
      const float wa[kKM] = {w0.x, w0.y, w0.z, w0.w}, wb[kKM] = {w1.x, w1.y, w1.z, w1.w};
#pragma unroll
      for (int i = 0; i < kRM; ++i)
#pragma unroll
        for (int j = 0; j < kKM; ++j)
          acc[i][j] = ck::mpe_max3(acc[i][j], ck::mpe_add(wa[j], ea[i]), ck::mpe_add(wb[j], eb[i]));
    }
    __syncthreads();
  }
  float* out = vals + val_off[fold_off + f];
#pragma unroll
  for (int i = 0; i < kRM; ++i) {
    const int64_t n = n0 + tr * kRM + i;
    if (n >= B) continue;
#pragma unroll
    for (int j = 0; j < kKM; ++j) {
      const int k = k0 + tk * kKM + j;
      if (k < K) out[n * K + k] = acc[i][j];
    }
  }
}

// ---- the walk policies ---------------------------------------------------------------------------------------------
// node (N, S) int32, -1 on entry: the input node the tree of row n reached over soft variable s.  spos[li]: layer li's (F)
// positions of its folds' variables among the soft variables (-1: hard), NULL for a layer without a soft fold.
struct SoftNodes {
  const int32_t* const* spos;
  int32_t* node;
  int S;

  __device__ bool record(int li, int f, int k, int64_t n, int g) const {
    const int32_t* sp = spos[li];
    const int s = sp != nullptr ? sp[f] : -1;
    if (s < 0) return false;
    node[n * S + s] = g * kNodeUnits + k;
    return true;
  }
};

// CondDraw over the values of the soft bottom-up pass; a row with bad evidence draws nothing; logev[n] gets the root value
// (NaN where bad[n]).
struct SoftSampleWalk {
  ck::CondDraw draw;
  SoftNodes nodes;
  const int32_t* bad;
  float* logev;

  __device__ bool root(int64_t n, float r) const {
    const bool b = bad[n] != 0;
    logev[n] = b ? NAN : r;
    return !b && draw.root(n, r);
  }
  __device__ int choose(const ck_sample_layer& L, const float* __restrict__ wr, const int32_t* __restrict__ ch,
                        const float* __restrict__ vals, const int64_t* __restrict__ val_off, int64_t nl, int64_t n, int g,
                        int lane) const {
    return draw.choose(L, wr, ch, vals, val_off, nl, n, g, lane);
  }
  __device__ void fill(const ck_sample_layer& L, int li, int f, int k, int64_t n, int g, void* __restrict__ x, int x_float,
                       int64_t o) const {
    if (!nodes.record(li, f, k, n, g)) draw.fill(L, li, f, k, n, g, x, x_float, o);
  }
};

struct SoftMpeWalk {
  ck::MpeArgmax arg;
  SoftNodes nodes;

  __device__ bool root(int64_t n, float r) const { return arg.root(n, r); }
  __device__ int choose(const ck_sample_layer& L, const float* __restrict__ wr, const int32_t* __restrict__ ch,
                        const float* __restrict__ vals, const int64_t* __restrict__ val_off, int64_t nl, int64_t n, int g,
                        int lane) const {
    return arg.choose(L, wr, ch, vals, val_off, nl, n, g, lane);
  }
  __device__ void fill(const ck_sample_layer& L, int li, int f, int k, int64_t n, int g, void* __restrict__ x, int x_float,
                       int64_t o) const {
    if (!nodes.record(li, f, k, n, g)) arg.fill(L, li, f, k, n, g, x, x_float, o);
  }
};

// ---- the decode leaf -----------------------------------------------------------------------------------------------
template <int W>
__device__ __forceinline__ float group_max(float v) {
#pragma unroll
  for (int d = W / 2; d > 0; d >>= 1) v = fmaxf(v, __shfl_xor(v, d, W));
  return v;
}
template <int W>
__device__ __forceinline__ int group_min(int v) {
#pragma unroll
  for (int d = W / 2; d > 0; d >>= 1) v = min(v, __shfl_xor(v, d, W));
  return v;
}
template <int W>
__device__ __forceinline__ int group_imax(int v) {
#pragma unroll
  for (int d = W / 2; d > 0; d >>= 1) v = max(v, __shfl_xor(v, d, W));
  return v;
}

// One group of W consecutive lanes per (chunk row nl, soft variable s); lane l of the group owns the states l, l + W, ...
// The entry's table is the TRANSPOSED log table, (K, C): the unit's row is read along the states, as log_lik is.  The first
// kNV * W states stay in registers (every state when C <= 256 at W = 64): one pass over memory.  mode 0: argmax; mode 1: the
// draw of the node's one Philox call (n = row0 + nl, g).
constexpr int kNV = 4;

template <int W>
__global__ void __launch_bounds__(256)
    soft_decode_leaf_kernel(int mode, const SoftEntry* __restrict__ ent, const int32_t* __restrict__ qstart,
                            const int64_t* __restrict__ vars, int S, int Cl, const float* __restrict__ ll,
                            const int32_t* __restrict__ node, int64_t row0, int64_t B, int D, uint32_t key0, uint32_t key1,
                            void* __restrict__ x, int x_float) {
  const int64_t item = (static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x) / W;
  const int lane = threadIdx.x % W;
  if (item >= B * S) return;  // (group-uniform, as every exit below: the shuffles stay inside a group)
  const int64_t nl = item / S;
  const int s = static_cast<int>(item % S);
  const int nd = node[(row0 + nl) * S + s];
  if (nd < 0) return;
  const int g = nd / kNodeUnits, k = nd % kNodeUnits;
  int q = qstart[s];
  const int q1 = qstart[s + 1];
  while (q < q1 && ent[q].g != g) ++q;
  if (q == q1) return;
  const int C = static_cast<int>(ent[q].C);
  const float* __restrict__ t = ent[q].table + static_cast<int64_t>(k) * C;
  const float* __restrict__ row = ll + (nl * S + s) * static_cast<int64_t>(Cl);
  const int64_t o = nl * D + vars[s];
  // v(c) = table[k, c] + log_lik[n, s, c] by the max leaf's add; NaN (-inf under +inf: no live row has one) counts as -inf
  auto value = [&](int c) -> float {
    if (c >= C) return -INFINITY;
    const float v = ck::mpe_add(t[c], row[c]);
    return v != v ? -INFINITY : v;
  };
  float v[kNV];
#pragma unroll
  for (int i = 0; i < kNV; ++i) v[i] = value(i * W + lane);
  float best = -INFINITY;
  int arg = INT_MAX;
#pragma unroll
  for (int i = 0; i < kNV; ++i) {
    if (v[i] > best) {  // strict: the smallest index of the lane's equal maxima
      best = v[i];
      arg = i * W + lane;
    }
  }
  for (int c = kNV * W + lane; c < C; c += W) {
    const float vc = value(c);
    if (vc > best) {
      best = vc;
      arg = c;
    }
  }
  const float m = group_max<W>(best);
  if (!(m > -INFINITY)) return;  // (a unit without mass is never reached from a root of finite value)
  if (mode == 0) {
    const int a = group_min<W>(best == m ? arg : INT_MAX);
    if (lane == 0) ck::store_category(x, x_float, o, a);
    return;
  }
  // inclusive scan of exp(v - m) over the W states of a step; the same arithmetic in both passes, so the total T of the
  // first is bit for bit the last CDF value of the second (CondDraw::choose)
  auto scan = [&](float vc) -> float {
    float e = expf(vc - m);  // (exp(-inf) = 0: a state of weight 0, or past C)
#pragma unroll
    for (int d = 1; d < W; d <<= 1) {
      const float up = __shfl_up(e, d, W);
      if (lane >= d) e += up;
    }
    return e;
  };
  float e[kNV];
  float T = 0.f;
#pragma unroll
  for (int i = 0; i < kNV; ++i) {
    e[i] = 0.f;
    if (i * W < C) {
      e[i] = scan(v[i]);
      T += __shfl(e[i], W - 1, W);
    }
  }
  for (int c0 = kNV * W; c0 < C; c0 += W) T += __shfl(scan(value(c0 + lane)), W - 1, W);
  const int64_t n = row0 + nl;
  float u = ck::philox_uniform(ck::walk_philox(n, g, key0, key1).x[0]) * T;
  if (u >= T) u = __int_as_float(__float_as_int(T) - 1);  // the float below T (T >= 1: the maximum's own term)
  float carry = 0.f;
  int last = -1;  // the last state that raised the CDF
  // one step of the search over the scanned masses ec of the states from c0; true when the draw is made
  auto step = [&](float ec, int c0) -> bool {
    const int c = c0 + lane;
    const int hit = group_min<W>((c < C && u < carry + ec) ? c : INT_MAX);
    if (hit != INT_MAX) {
      if (lane == 0) ck::store_category(x, x_float, o, hit);
      return true;
    }
    const float prev = __shfl_up(ec, 1, W);
    last = max(last, group_imax<W>((c < C && ec > (lane == 0 ? 0.f : prev)) ? c : -1));
    carry += __shfl(ec, W - 1, W);
    return false;
  };
#pragma unroll
  for (int i = 0; i < kNV; ++i) {
    if (i * W < C && step(e[i], i * W)) return;
  }
  for (int c0 = kNV * W; c0 < C; c0 += W) {
    if (step(scan(value(c0 + lane)), c0)) return;
  }
  if (lane == 0 && last >= 0) ck::store_category(x, x_float, o, last);  // (u < T always hits; see CondDraw::choose)
}

int check_nodes(const char* fn, const int32_t* const* spos, const int32_t* node, int S_soft) {
  CK_REQUIRE(spos != nullptr && node != nullptr && S_soft > 0, "%s: no soft variables", fn);
  return 0;
}

}  // namespace

int ck_soft_max_leaf(const float* table, const float* log_lik, const int32_t* spos, float* vals, const int64_t* val_off,
                     int fold_off, int32_t* bad, int64_t F, int64_t B, int K, int C, int S, int Cl, void* stream) {
  CK_REQUIRE(table && log_lik && spos && vals && val_off && bad, "ck_soft_max_leaf: null pointer");
  CK_REQUIRE(F > 0 && B > 0 && K > 0 && C > 0 && S > 0 && Cl >= C && fold_off >= 0,
             "ck_soft_max_leaf: bad size F=%lld B=%lld K=%d C=%d S=%d Cl=%d", static_cast<long long>(F),
             static_cast<long long>(B), K, C, S, Cl);
  const int tk = K <= 16 ? 16 : K <= 32 ? 32 : 64;
  const int tr = kUpThreads / (tk / kKM) * kRM;
  const int64_t row_tiles = (B + tr - 1) / tr, unit_tiles = (K + tk - 1) / tk;
  CK_REQUIRE(F * row_tiles <= 0x7fffffff && unit_tiles <= 65535, "ck_soft_max_leaf: grid too large");
  const dim3 grid(static_cast<unsigned>(F * row_tiles), static_cast<unsigned>(unit_tiles));
  const int vec = (C % 4 == 0 && Cl % 4 == 0 && ck::aligned16(log_lik)) ? 1 : 0;
  decltype(&soft_max_leaf_kernel<16>) kern;
  if (tk == 16) kern = soft_max_leaf_kernel<16>;
  else if (tk == 32) kern = soft_max_leaf_kernel<32>;
  else kern = soft_max_leaf_kernel<64>;
  return ck::launch(kern, grid, dim3(kUpThreads), 0, stream, table, log_lik, spos, vals, val_off, fold_off, bad, B, K, C, S, Cl,
                    row_tiles, vec);
}

int ck_soft_sample_walk(const ck_sample_layer* layers, const float* const* weights, const int32_t* const* spos, int n_layers,
                        int root_fold, int root_unit, int total_folds, int S, const float* vals, const int64_t* val_off,
                        const int32_t* bad, int64_t row0, int64_t B, int64_t N, int D, uint64_t seed, int S_soft,
                        int32_t* node, const void* ev, void* x, int x_float, float* logev, void* stream) {
  CK_REQUIRE(bad != nullptr && logev != nullptr, "ck_soft_sample_walk: null pointer");
  if (int st = check_nodes("ck_soft_sample_walk", spos, node, S_soft)) return st;
  const SoftSampleWalk p{ck::CondDraw{static_cast<uint32_t>(seed), static_cast<uint32_t>(seed >> 32)},
                         SoftNodes{spos, node, S_soft}, bad, logev};
  return ck::evidence_walk("ck_soft_sample_walk", layers, weights, n_layers, root_fold, root_unit, total_folds, S, vals,
                           val_off, row0, B, N, D, ev, x, x_float, p, stream);
}

int ck_soft_mpe_walk(const ck_sample_layer* layers, const float* const* logw, const int32_t* const* amax,
                     const int32_t* const* spos, int n_layers, int root_fold, int root_unit, int total_folds, int S,
                     const float* vals, const int64_t* val_off, const int32_t* bad, int64_t row0, int64_t B, int64_t N, int D,
                     int S_soft, int32_t* node, const void* ev, void* x, int x_float, float* logv, void* stream) {
  CK_REQUIRE(amax != nullptr && bad != nullptr && logv != nullptr, "ck_soft_mpe_walk: null pointer");
  if (int st = check_nodes("ck_soft_mpe_walk", spos, node, S_soft)) return st;
  const SoftMpeWalk p{ck::MpeArgmax{amax, bad, logv}, SoftNodes{spos, node, S_soft}};
  return ck::evidence_walk("ck_soft_mpe_walk", layers, logw, n_layers, root_fold, root_unit, total_folds, S, vals, val_off,
                           row0, B, N, D, ev, x, x_float, p, stream);
}

int ck_soft_decode_leaf(int mode, const int64_t* entries, const int32_t* qstart, const int64_t* vars, int S, int Cl,
                        int C_max, const float* log_lik, const int32_t* node, int64_t row0, int64_t B, int D, uint64_t seed,
                        void* x, int x_float, void* stream) {
  CK_REQUIRE(entries && qstart && vars && log_lik && node && x, "ck_soft_decode_leaf: null pointer");
  CK_REQUIRE((mode == 0 || mode == 1) && S > 0 && Cl > 0 && C_max > 0 && C_max <= Cl && row0 >= 0 && B > 0 && D > 0,
             "ck_soft_decode_leaf: bad argument");
  const SoftEntry* ent = reinterpret_cast<const SoftEntry*>(entries);
  const int W = C_max <= 4 ? 4 : C_max <= 16 ? 16 : C_max <= 32 ? 32 : 64;
  const int64_t blocks = ck::blocks_of(B * S * W, 256);
  CK_REQUIRE(blocks <= 0x7fffffff, "ck_soft_decode_leaf: too many items");
  decltype(&soft_decode_leaf_kernel<4>) kern;
  if (W == 4) kern = soft_decode_leaf_kernel<4>;
  else if (W == 16) kern = soft_decode_leaf_kernel<16>;
  else if (W == 32) kern = soft_decode_leaf_kernel<32>;
  else kern = soft_decode_leaf_kernel<64>;
  return ck::launch(kern, dim3(static_cast<unsigned>(blocks)), dim3(256), 0, stream, mode, ent, qstart, vars, S, Cl, log_lik, node,
                    row0, B, D, static_cast<uint32_t>(seed), static_cast<uint32_t>(seed >> 32), x, x_float);
}
