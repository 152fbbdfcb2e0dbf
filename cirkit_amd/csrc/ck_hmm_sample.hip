// Posterior path sampling of a hidden Markov model ("Sampling paths"): forward-filter-backward-sample.
//
// After ck_hmm_forward_keep (ck_hmm.hip) left t_s = v_{s-1} + e_s, relative to the row, in keep[b, var_s, :], a path is drawn from
// the last step down:
//     p(z_s = i | z_{s+1} = o, evidence) ~ exp(t_s[i]) W_s[o, i]             (o = 0 above the last step)
// and a missing entry of step s from the emission p(c | z_s) of its fold.  That is the Viterbi walk back (ck_hmm_viterbi.hip) with
// a draw where it takes a maximum: one (sample, step) is served from the hand-off and ONE contiguous weight row, O(K).
//
// hmm_sample_paths_kernel<G, NCH>.  A (row, sample) pair belongs to a GROUP of G lanes, not to a wave: G = 8 lanes at K = 32, 16 at
// 64, 32 up to 128, 64 above, lane l of the group holding elements 4 l + 4 G e + (0 .. 3) of chunk e < NCH (NCH > 1 from K > 256 on).
// A wave walks 64 / G samples at once -- 8 at K = 32, where the step is pure latency and a wave a sample would idle 56 lanes.
// Samples are numbered row-major, n = row S + j, so the groups of a wave mostly share a row: their reads of t_s are the same cache
// lines, and t_s needs no LDS.  Per step and group:
//   1  t_{s-1} and x[b, var_{s-1}] are requested before z_s is known (their addresses do not depend on it);
//   2  the weight row W_s[z_{s+1}] is gathered, 16 bytes a lane and chunk -- per group, since the groups diverge;
//   3  q_i = 2^96 exp(t_s[i] - m) W_s[z, i], m the group maximum of t_s over the real states: linear in W as the parameter graph
//      leaves it (no K^2 logarithms), with the headroom of the forward (kHmmHead) so that a state 154 nats below the best survives;
//   4  an inclusive prefix sum in index order: the lane's four, then the lane totals across the group -- DPP row_shr 1, 2, 4, 8
//      inside a row of 16; where G > 16 the odd rows add the total of the even row below and the upper half that of the lower
//      half, each fetched by one permlane swap -- chunk after chunk with the running total carried;
//   5  the draw is the smallest i < num_states with q_i > 0 and u Total < CDF_i, a minimum over the group.  (The contract's count
//      of CDF_i <= u Total assumes a CDF that never decreases; a tree of partial sums may step back by an ulp between two lanes,
//      and a count would then name a unit WITHOUT mass.  The minimum over units with mass cannot.)  If rounding leaves none it is
//      the last unit with mass -- both travel in one key, so one reduction;
//   6  every lane of the group holds the key: z needs no broadcast.
// Units >= num_states never compete, and z < num_states whatever the values were: it never indexes past the weights.
// Missing entries.  The emission is drawn from ck_hmm_emission_cdf's table by the SAME search, the group reading the contiguous
// row [fold, z, :] cooperatively (16 bytes a lane where C is a multiple of 4): all its loads are independent and are issued with
// the next step's weight row, one memory latency.  A bisection by one lane is log2 C DEPENDENT loads -- 8 latencies at C = 256
// against the one of the step itself, on every step on which any group of the wave misses its entry.
// Philox4x32-10 (ck_philox.h): key the halves of the seed, counter (n, s, 0, 0), ONE call per (sample, step); word x0 draws the
// state, word x1 the emission.  A sample depends on (seed, global row, j) only.
// A row whose score is not > -inf (no mass, or NaN) gets -1 in every state and at every missing entry.
//
// hmm_emission_cdf_kernel: (F, K, C) inclusive sums of exp(table[f, c, k]) over c, one contiguous row per (fold, state) -- the
// table of logarithms has a state's categories K floats apart, C cache lines a draw.  A wave owns 64 states of a fold; it sums
// down the categories (reads contiguous over the states) and transposes 64 x 64 tiles through LDS (writes contiguous over c).
#include "ck_hmm.h"
#include "ck_philox.h"

namespace {

struct SampleArgs {
  const float* const* w;  // (T) the steps' evaluated weights, row-major (Ko, K)
  const int32_t* fold;    // (T) input fold of each step
  const int32_t* var;     // (T) its variable
  const float* cdf;       // (F, K, C) emission table of hmm_emission_cdf_kernel
  const int64_t* x;       // (B, D)
  const int32_t* integ;   // (D) != 0: the variable is missing in every row; or nullptr
  const float* score;     // (B) log_prob of the keeping forward
  const float* keep;      // (B, D, K) its hand-off
  int64_t* states;        // (B, S, D)
  int64_t* completed;     // (B, S, D)
  int64_t row0;           // global index of row 0 (the Philox counter counts rows of the whole batch)
  uint32_t k0, k1;        // Philox key
  int T, K, num_states, D, C, B, S;
};

template <int CTRL, class V>
__device__ __forceinline__ V dpp_mov(V v) {
  return __builtin_bit_cast(V, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), CTRL, 0xF, 0xF, true));
}
// the lanes that have no source get 0
template <int CTRL>
__device__ __forceinline__ float dpp_or_zero(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xF, 0xF, false));
}

// the value of the lane's partner in the other row of its pair of rows (HALVES = false) or in the other half of the wave
template <bool HALVES, class V>
__device__ __forceinline__ V partner(V v) {
  const uint32_t own = __builtin_bit_cast(uint32_t, v);
  const auto r = HALVES ? __builtin_amdgcn_permlane32_swap(own, own, false, false) : __builtin_amdgcn_permlane16_swap(own, own, false, false);
  return __builtin_bit_cast(V, r[0] != own ? r[0] : r[1]);  // (one of the two is the lane's own)
}
// over the G lanes of a group (G-aligned in the wave), every lane gets the result: the exchange pattern of ck::wave_reduce
template <int G, class V, class Op>
__device__ __forceinline__ V group_reduce(V v, Op op) {
  v = op(v, dpp_mov<0xB1>(v));   // quad_perm [1,0,3,2]
  v = op(v, dpp_mov<0x4E>(v));   // quad_perm [2,3,0,1]
  v = op(v, dpp_mov<0x141>(v));  // row_half_mirror
  if constexpr (G >= 16) v = op(v, dpp_mov<0x140>(v));  // row_mirror
  if constexpr (G >= 32) v = op(v, partner<false>(v));
  if constexpr (G >= 64) v = op(v, partner<true>(v));
  return v;
}
template <int G>
__device__ __forceinline__ float group_max(float v) {
  return group_reduce<G>(v, [](float a, float b) { return fmaxf(a, b); });
}
template <int G>
__device__ __forceinline__ int group_min(int v) {
  return group_reduce<G>(v, [](int a, int b) { return a < b ? a : b; });
}

// inclusive prefix sum over the G lanes of a group in lane order; l: the lane's index in its group
template <int G, int N, int CTRL>
__device__ __forceinline__ void scan_step(float& v, int l) {
  float o = dpp_or_zero<CTRL>(v);  // row_shr:N
  if constexpr (G < 16) o = l >= N ? o : 0.f;  // (two groups share a row of 16)
  v += o;
}
// The sums never decrease along the lanes (no term is negative), so the total of a row of 16, or of the lower 32 lanes, is the
// MAXIMUM over it -- exact, and every lane of the partner row gets it by one swap, where the total itself sits in one lane.
template <int G>
__device__ __forceinline__ float group_scan(float v, int l) {
  scan_step<G, 1, 0x111>(v, l);
  scan_step<G, 2, 0x112>(v, l);
  scan_step<G, 4, 0x114>(v, l);
  if constexpr (G >= 16) scan_step<G, 8, 0x118>(v, l);
  if constexpr (G >= 32) {
    const float below = partner<false>(group_max<16>(v));
    v += (threadIdx.x & 16) ? below : 0.f;  // the odd rows: the total of the even row below
  }
  if constexpr (G >= 64) {
    const float below = partner<true>(group_max<32>(v));
    v += (threadIdx.x & 32) ? below : 0.f;  // the upper half: the total of the lower one
  }
  return v;
}

constexpr int kNoUnit = 0x7fffffff;
constexpr int kFallback = 1 << 16;  // keys from here on: no CDF entry above the threshold, the last entry with mass instead

template <int G, int NCH>
__global__ void __launch_bounds__(256) hmm_sample_paths_kernel(const SampleArgs a) {
  const int64_t tid = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  const int64_t n = tid / G;  // the sample of this chunk of rows, row-major
  const int l = static_cast<int>(threadIdx.x) & (G - 1);
  if (n >= static_cast<int64_t>(a.B) * a.S) return;
  const int K = a.K, T = a.T, C = a.C;
  const int b = static_cast<int>(n / a.S);
  const uint32_t ctr = static_cast<uint32_t>((a.row0 + b) * a.S + (n - static_cast<int64_t>(b) * a.S));
  const auto var = ck::as_global(a.var);
  const auto xrow = ck::as_global(a.x) + static_cast<int64_t>(b) * a.D;
  const auto sout = ck::as_global(a.states) + n * a.D;
  const auto cout = ck::as_global(a.completed) + n * a.D;
  auto missing = [&](int v, int64_t xv) { return xv < 0 || (a.integ != nullptr && ck::as_global(a.integ)[v] != 0); };

  if (!(ck::as_global(a.score)[b] > -INFINITY)) {  // no path of positive mass, or NaN
    if (l == 0)
      for (int s = 0; s < T; ++s) {
        const int v = var[s];
        const int64_t xv = xrow[v];
        sout[v] = -1;
        cout[v] = missing(v, xv) ? -1 : xv;
      }
    return;
  }

  const float* const base = a.keep + static_cast<int64_t>(b) * a.D * K + 4 * l;
  const float4 none = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
  float4 t[NCH], tn[NCH];  // the hand-off of this step, and of the one below it
  auto load_t = [&](int s, float4 (&v)[NCH]) {
    const float* src = base + static_cast<int64_t>(var[s]) * K;
#pragma unroll
    for (int e = 0; e < NCH; ++e) v[e] = 4 * l + 4 * G * e < K ? ck::gload4(src + 4 * G * e) : none;
  };
  load_t(T - 1, t);
  int64_t xv = xrow[var[T - 1]], xn = 0;
  int z = 0;  // the row of W_s that the step above chose: unit 0 above the last step
  for (int s = T - 1; s >= 0; --s) {
    const int v = var[s];
    if (s > 0) {
      load_t(s - 1, tn);
      xn = xrow[var[s - 1]];
    }
    const float* wr = ck::as_global(a.w)[s] + static_cast<int64_t>(z) * K + 4 * l;
    float4 w4[NCH];
#pragma unroll
    for (int e = 0; e < NCH; ++e) w4[e] = 4 * l + 4 * G * e < K ? ck::gload4(wr + 4 * G * e) : make_float4(0.f, 0.f, 0.f, 0.f);
    const bool miss = missing(v, xv);
    const ck::Philox4 rnd = ck::philox4x32_10(ctr, static_cast<uint32_t>(s), 0u, 0u, a.k0, a.k1);

    // m: the largest t_s of a real state
    float m = -INFINITY;
#pragma unroll
    for (int e = 0; e < NCH; ++e) {
      const int i0 = 4 * l + 4 * G * e;
      const float tv[4] = {t[e].x, t[e].y, t[e].z, t[e].w};
#pragma unroll
      for (int c = 0; c < 4; ++c) m = i0 + c < a.num_states ? fmaxf(m, tv[c]) : m;
    }
    m = ck::clamp_finite(group_max<G>(m));

    // CDF in index order; an entry without mass is marked -1: it is never above a threshold
    float cdf[NCH][4];
    float total = 0.f;
    int last = -1;  // the lane's last unit with mass
#pragma unroll
    for (int e = 0; e < NCH; ++e) {
      const int i0 = 4 * l + 4 * G * e;
      const float tv[4] = {t[e].x, t[e].y, t[e].z, t[e].w}, wv[4] = {w4[e].x, w4[e].y, w4[e].z, w4[e].w};
      float q[4], p[4];
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        // 2^96 exp(t - m): the headroom goes into the exponent only where exp2 alone would flush (below 2^-64 of the best);
        // adding 96 to the argument of a state that carries mass would round it at 2^-18, 2.6e-6 of its q
        const float xe = (tv[c] - m) * kL2E;
        const bool deep = xe < -64.f;
        const float ex = __builtin_amdgcn_exp2f(deep ? xe + kHmmHead : xe) * (deep ? 1.f : 0x1p96f);
        q[c] = i0 + c < a.num_states ? ex * wv[c] : 0.f;
        q[c] = q[c] > 0.f ? q[c] : 0.f;  // (NaN of 0 x inf included)
        p[c] = c ? p[c - 1] + q[c] : q[c];
        last = q[c] > 0.f ? i0 + c : last;
      }
      const float incl = group_scan<G>(p[3], l);
      const float before = total + (incl - p[3]);  // the lanes below in the group, to an ulp of the total
#pragma unroll
      for (int c = 0; c < 4; ++c) cdf[e][c] = q[c] > 0.f ? before + p[c] : -1.f;
      total = group_max<G>(before + p[3]);
    }
    const float th = ck::philox_uniform(rnd.x[0]) * total;
    int key = last >= 0 ? kFallback + (1023 - last) : kNoUnit;
#pragma unroll
    for (int e = NCH - 1; e >= 0; --e)
#pragma unroll
      for (int c = 3; c >= 0; --c) key = th < cdf[e][c] ? 4 * l + 4 * G * e + c : key;
    key = group_min<G>(key);
    z = key < kFallback ? key : (key != kNoUnit ? 1023 - (key - kFallback) : 0);  // (< num_states in every case)

    // the emission of a missing entry, from row [fold, z, :] of the table: the same search over c < C
    int cat = kNoUnit;
    if (miss) {
      const float* row = a.cdf + (static_cast<int64_t>(ck::as_global(a.fold)[s]) * K + z) * C;
      const float te = *ck::as_global(row + C - 1);
      const float the = ck::philox_uniform(rnd.x[1]) * te;
      auto take = [&](float cv, int c) {
        const int k = the < cv ? c : (cv >= te ? kFallback + c : kNoUnit);
        cat = k < cat ? k : cat;
      };
      if ((C & 3) == 0) {
        for (int c0 = 4 * l; c0 < C; c0 += 4 * G) {
          const float4 r4 = ck::gload4(row + c0);
          take(r4.x, c0), take(r4.y, c0 + 1), take(r4.z, c0 + 2), take(r4.w, c0 + 3);
        }
      } else {
        for (int c = l; c < C; c += G) take(*ck::as_global(row + c), c);
      }
    }
    cat = group_min<G>(cat);
    cat = cat < kFallback ? cat : (cat != kNoUnit ? cat - kFallback : 0);
    if (l == 0) {
      sout[v] = z;
      cout[v] = miss ? cat : xv;
    }
#pragma unroll
    for (int e = 0; e < NCH; ++e) t[e] = tn[e];
    xv = xn;
  }
}

constexpr int kCdfTile = 64;

__global__ void __launch_bounds__(64) hmm_emission_cdf_kernel(const float* table, int K, int C, float* cdf) {
  __shared__ float tile[kCdfTile][kCdfTile + 1];
  const int lane = threadIdx.x, f = blockIdx.y, k0 = blockIdx.x * kCdfTile;
  const int k = k0 + lane;
  const float* src = table + static_cast<int64_t>(f) * (C + 1) * K + k;  // (the layer's table has one more row: the integral)
  float* dst = cdf + (static_cast<int64_t>(f) * K + k0) * C;
  const int nk = K - k0 < kCdfTile ? K - k0 : kCdfTile;
  float sum = 0.f;
  for (int c0 = 0; c0 < C; c0 += kCdfTile) {
    const int nc = C - c0 < kCdfTile ? C - c0 : kCdfTile;
    if (k < K)
      for (int c = 0; c < nc; ++c) {
        sum += expf(*ck::as_global(src + static_cast<int64_t>(c0 + c) * K));
        tile[lane][c] = sum;
      }
    __syncthreads();
    if (lane < nc)
      for (int r = 0; r < nk; ++r) *ck::as_global(dst + static_cast<int64_t>(r) * C + c0 + lane) = tile[r][lane];
    __syncthreads();
  }
}

template <int G>
int sample_launch_chunks(const SampleArgs& a, void* stream) {
  const int64_t threads = static_cast<int64_t>(a.B) * a.S * G;
  const dim3 grid(static_cast<unsigned>((threads + 255) / 256)), block(256);
  if constexpr (G < 64) {
    return ck::launch(hmm_sample_paths_kernel<G, 1>, grid, block, 0, stream, a);
  } else {
    switch ((a.K + 255) / 256) {
      case 1: return ck::launch(hmm_sample_paths_kernel<64, 1>, grid, block, 0, stream, a);
      case 2: return ck::launch(hmm_sample_paths_kernel<64, 2>, grid, block, 0, stream, a);
      case 3: return ck::launch(hmm_sample_paths_kernel<64, 3>, grid, block, 0, stream, a);
      default: return ck::launch(hmm_sample_paths_kernel<64, 4>, grid, block, 0, stream, a);
    }
  }
}

}  // namespace

extern "C" int ck_hmm_emission_cdf(const float* table, int F, int K, int C, float* cdf, void* stream) {
  const char* name = "ck_hmm_emission_cdf";
  CK_REQUIRE(table && cdf, "%s: null operand", name);
  CK_REQUIRE(F >= 1 && F <= ck::kMaxFoldsPerLaunch && K >= 1 && C >= 1, "%s: F = %d, K = %d, C = %d", name, F, K, C);
  const dim3 grid((K + kCdfTile - 1) / kCdfTile, F), block(kCdfTile);
  return ck::launch(hmm_emission_cdf_kernel, grid, block, 0, stream, table, K, C, cdf);
}

extern "C" int ck_hmm_sample_paths(const void* const* w_steps, const int32_t* step_fold, const int32_t* step_var, int T, int K,
                                   int num_states, const float* cdf, const int64_t* x, int D, int C, const int32_t* integrate, int B,
                                   int S, int64_t row0, uint64_t seed, const float* log_prob, const float* keep, int64_t* states,
                                   int64_t* completed, void* stream) {
  const char* name = "ck_hmm_sample_paths";
  CK_REQUIRE(w_steps && step_fold && step_var && cdf && x && log_prob && keep && states && completed, "%s: null operand", name);
  CK_REQUIRE(T >= 1 && B >= 1 && D >= T && C >= 1, "%s: T = %d, B = %d, D = %d, C = %d", name, T, B, D, C);
  CK_REQUIRE(K >= 32 && K <= 1024 && K % 32 == 0, "%s: K = %d is not a multiple of 32 in 32 .. 1024", name, K);
  CK_REQUIRE(num_states >= 1 && num_states <= K, "%s: %d states of %d units", name, num_states, K);
  CK_REQUIRE(S >= 1 && row0 >= 0 && (row0 + B) * static_cast<int64_t>(S) <= (int64_t{1} << 32),
             "%s: S = %d, row0 = %lld: the sample index is the 32-bit word of the counter", name, S, static_cast<long long>(row0));
  CK_REQUIRE(ck::aligned16(cdf) && ck::aligned16(keep), "%s: the table and the hand-off are read 16 bytes at a time", name);
  const SampleArgs a{reinterpret_cast<const float* const*>(w_steps), step_fold, step_var, cdf, x, integrate, log_prob, keep, states,
                     completed, row0, static_cast<uint32_t>(seed), static_cast<uint32_t>(seed >> 32), T, K, num_states, D, C, B, S};
  if (K == 32) return sample_launch_chunks<8>(a, stream);
  if (K == 64) return sample_launch_chunks<16>(a, stream);
  if (K <= 128) return sample_launch_chunks<32>(a, stream);
  return sample_launch_chunks<64>(a, stream);
}
