// The forward algorithm of a hidden Markov model in ONE launch ("Hidden Markov models").
//
// A chain plan (cirkit_amd/hmm.py: chain_of) is T dependent layers of one fold each, K units wide:
//     v_s[b, o] = log sum_i W_s[o, i] exp(v_{s-1}[b, i] + e_s[b, i]),   v_{-1} = 0,   result v_{T-1}[b, 0]
// with e_s[b, :] the row of K log emissions of step s at x[b, var_s] (zeros where that entry is missing).  Layer by layer
// that is T launches that each write a (B, K) block and read it back; here a workgroup owns 32 rows for the whole chain
// and the state never leaves the chip.
//
// Decomposition.  A workgroup = min(K / 32, 4) waves x 32 rows.  The waves split the UNITS into blocks of 32: wave w
// owns blocks w, w + waves, ... (NOB of them at most) -- as OUTPUT blocks of a step's contraction and, because the output
// layout of v_mfma_f32_32x32x2_f32 is the input layout of the next one (ck_tile.h), as the blocks whose hand-off it
// prepares for the next step, in registers:
//   A  t = log y_{s-1} + e_s on the wave's blocks (registers); row maximum M over ALL units: per wave in registers, across
//      the waves through LDS; p = exp(t - M) goes to the activation tile in LDS in operand layout (block q, register group
//      g, lane: one ds_read_b128 per MFMA operand quad, no bank conflict); the row's log scale gains M.  (p carries a factor
//      2^96 that the logarithm takes off again: kHmmHead.)
//   B  y = W_s p on v_mfma_f32_32x32x2_f32 (exact fp32; weights as operand A, activations as B): every wave contracts
//      ALL K inputs from the shared tile against the weight rows of its own output blocks, then takes log y.
// This is LSESumSemiring's arithmetic (semiring.py:383-408) step for step -- the maximum is clamped to finite values, so a
// row without mass ends as -inf, never NaN -- and needs no fallback: nothing is renormalised in linear space, so nothing can
// underflow that the reference's own fp32 evaluation keeps (LAB_NOTES has the cost of the two transcendentals per unit).
//
// Weights.  W_s is K^2 floats (4 MiB at K = 1024) and every workgroup reads all of it at about the same time, from L2.  A
// wave streams the rows of its output blocks in UNITS of 32 outputs x 16 inputs (2 KiB: two global_load_lds_dwordx4 per
// lane land them in operand layout) through a private ring of NBUF units in LDS; no other wave reads them, so a unit needs
// no barrier, only the wave's own vmcnt: loads complete in order, so "at most 2 (NBUF - 1) requests outstanding" means unit
// u has landed once NBUF - 1 younger units are in flight, whatever else (emission rows) was requested around them; the last
// NBUF - 1 units of a step wait for everything.  The first NBUF - 1 units of a step are requested before its phase A.
// NBUF = 8 up to K = 512; 3 above, where the activation tile alone takes up to 128 of the 160 KiB.
//
// Emissions.  The K-row of step s + 1 is requested before step s contracts (its address depends on x only, and x of step
// s + 2 is read then too).  Two sources, one kernel: a table addressed by (fold, category) -- the Categorical layer's
// (F, C + 1, K) table of logarithms -- or a (F, B, K) block that the input layer's own launch wrote.
// The last step only needs output unit 0: a dot product with row 0 of its weights.
#include "ck_hmm.h"

namespace {

// KEEP: every step also stores t = log y + e, relative to the row's scale BEFORE the step, into keep[b, var_s, :] -- each wave its
// own blocks straight from the registers of phase A, 16 bytes a lane and register group -- for hmm_backward_kernel below.
template <int NOB, bool KEEP = false>
__global__ void __launch_bounds__(256) hmm_forward_kernel(const HmmArgs a) {
  constexpr int NBUF = NOB > 4 ? 3 : 8;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int K = a.K, NQ = K >> 5, T = a.T;
  const int nwaves = blockDim.x >> 6;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int kh = lane >> 5, row = lane & 31;
  const int b = blockIdx.x * 32 + row;
  const bool live = b < a.B;
  const int bl = live ? b : a.B - 1;  // (rows past B repeat the last one and store nothing)
  int nob = 0;                        // units blocks of this wave
#pragma unroll
  for (int j = 0; j < NOB; ++j) nob += wave + nwaves * j < NQ ? 1 : 0;

  // LDS: activation tile [NQ][4][64] float4 | row maxima [4][32] | weight rings [waves][NBUF][2][64] float4
  const uint32_t act = static_cast<uint32_t>(reinterpret_cast<uintptr_t>(smem));
  const uint32_t red = act + NQ * 4096;
  float* const ring_p = smem + NQ * 1024 + kHmmWaves * 32 + wave * (NBUF * kHmmUnit);
  const uint32_t ring = red + kHmmWaves * 128 + wave * (NBUF * kHmmUnit * 4) + lane * 16;

  bool bad = false;
  auto load_x = [&](int s) -> int64_t { return (a.x != nullptr && s < T) ? a.x[static_cast<int64_t>(bl) * a.D + a.var[s]] : 0; };
  auto row_of = [&](int s, int64_t xv) -> const float* {  // nullptr: the entry is missing
    const int64_t f = a.fold[s];
    if (a.x == nullptr) return a.rows + (f * a.B + bl) * K;
    if (xv < 0 || (a.integ != nullptr && a.integ[a.var[s]] != 0)) return nullptr;
    if (xv >= a.C) {
      bad = true;
      return nullptr;
    }
    return a.rows + (f * (a.C + 1) + xv) * K;
  };
  float e[NOB][16], la[NOB][16];
  auto load_e = [&](const float* r) {
#pragma unroll
    for (int j = 0; j < NOB; ++j) {
      const int q = wave + nwaves * j;
      if (q < NQ && r != nullptr) {
        tile_load(r + 32 * q + 4 * kh, e[j]);
      } else {
#pragma unroll
        for (int i = 0; i < 16; ++i) e[j][i] = 0.f;
      }
    }
  };
  // unit u of a step = (owned block j, input block q, half h): rows 32 ob .. of W, inputs 32 q + 16 h ..
  auto issue = [&](const float* w, int u) {
    const int j = u / (2 * NQ), r = u - j * 2 * NQ;
    const int ob = wave + nwaves * j;
    const float* src = w + static_cast<int64_t>(32 * ob + row) * K + 16 * r + 4 * kh;
    float* dst = ring_p + (u % NBUF) * kHmmUnit;
    __builtin_amdgcn_global_load_lds((ck::gptr_t)src, (ck::lptr_t)dst, 16, 0, 0);
    __builtin_amdgcn_global_load_lds((ck::gptr_t)(src + 8), (ck::lptr_t)(dst + 256), 16, 0, 0);
  };

#pragma unroll
  for (int j = 0; j < NOB; ++j)
#pragma unroll
    for (int i = 0; i < 16; ++i) la[j][i] = 0.f;
  float scale = 0.f;
  load_e(row_of(0, load_x(0)));
  int64_t xn = load_x(1);

  for (int s = 0; s < T; ++s) {
    const bool last = s + 1 == T;
    const float* w = a.w[s];
    const int U = last ? 0 : nob * NQ * 2;
    for (int u = 0; u < NBUF - 1 && u < U; ++u) issue(w, u);

    // ---- A: t = log y + e, its row maximum, p = exp(t - M) into the shared tile
    float m = -INFINITY;
#pragma unroll
    for (int j = 0; j < NOB; ++j)
      if (j < nob) {
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          e[j][i] += la[j][i];
          m = fmaxf(m, e[j][i]);
        }
      }
    if constexpr (KEEP) {
      if (live) {
        float* dst = a.keep + (static_cast<int64_t>(b) * a.D + a.var[s]) * K + 4 * kh;
#pragma unroll
        for (int j = 0; j < NOB; ++j)
          if (j < nob) keep_store(dst + 32 * (wave + nwaves * j), e[j]);
      }
    }
    m = ck::xhalf_max(m);
    asm volatile("ds_write_b32 %0, %1" ::"v"(red + (wave * 32 + row) * 4), "v"(m) : "memory");
    sync_lds();
    for (int k = 0; k < nwaves; ++k) {
      float o;
      asm volatile("ds_read_b32 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=v"(o) : "v"(red + (k * 32 + row) * 4) : "memory");
      m = fmaxf(m, o);
    }
    m = ck::clamp_finite(m);
    const float nml = exp_offset(m, kHmmHead);
    scale += m;
#pragma unroll
    for (int j = 0; j < NOB; ++j)
      if (j < nob) {
        const uint32_t dst = act + (wave + nwaves * j) * 4096 + lane * 16;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          float p[4];
#pragma unroll
          for (int t = 0; t < 4; ++t) p[t] = __builtin_amdgcn_exp2f(fmaf(e[j][4 * g + t], kL2E, nml));
          lds_w4(dst + g * 1024, p[0], p[1], p[2], p[3]);
        }
      }
    sync_lds();
    if (last) break;

    // the emission row of step s + 1 travels while this step contracts
    load_e(row_of(s + 1, xn));
    xn = load_x(s + 2);

    // ---- B: y = W p on the wave's output blocks, log y stays in registers
    int u = 0;
    static_for<0, NOB>([&](auto jc) {
      constexpr int j = decltype(jc)::value;
      if (j >= nob) return;
      f32x16 acc;
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[r] = 0.f;
      for (int r = 0; r < 2 * NQ; ++r, ++u) {
        if (u + NBUF - 1 < U) {
          issue(w, u + NBUF - 1);
          asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * (NBUF - 1)) : "memory");
        } else {
          asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        f32x4v w0, w1, p0, p1;
        const uint32_t wa = ring + (u % NBUF) * (kHmmUnit * 4), pa = act + r * 2048 + lane * 16;
        lds_read4(w0, w1, p0, p1, wa, wa + 1024, pa, pa + 1024);
#pragma unroll
        for (int t = 0; t < 4; ++t) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(w0[t], p0[t], acc, 0, 0, 0);
#pragma unroll
        for (int t = 0; t < 4; ++t) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(w1[t], p1[t], acc, 0, 0, 0);
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) la[j][r] = log_unscaled(acc[r]);
    });
  }

  // the last step: output unit 0 only
  if (wave == 0) {
    const float* wl = a.w[T - 1];
    float d = 0.f;
    for (int q = 0; q < NQ; ++q) {
      f32x4v p0, p1, p2, p3;
      const uint32_t pa = act + q * 4096 + lane * 16;
      lds_read4(p0, p1, p2, p3, pa, pa + 1024, pa + 2048, pa + 3072);
      const f32x4v* pg[4] = {&p0, &p1, &p2, &p3};
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const float4 w4 = ck::gload4(wl + 32 * q + 8 * g + 4 * kh);
        d = fmaf(w4.x, (*pg[g])[0], d);
        d = fmaf(w4.y, (*pg[g])[1], d);
        d = fmaf(w4.z, (*pg[g])[2], d);
        d = fmaf(w4.w, (*pg[g])[3], d);
      }
    }
    const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(d), __float_as_uint(d), false, false);
    d = __uint_as_float(sw[0]) + __uint_as_float(sw[1]);
    if (live && kh == 0) a.out[b] = bad ? __builtin_nanf("") : scale + log_unscaled(d);
  }
}

// ---- the backward pass: smoothing posteriors in place ("Smoothing posteriors") ------------------------
// With t_s = v_{s-1} + e_s what the KEEP forward left in keep[b, var_s, :] (relative to a per-row, per-step constant):
//     beta_{T-1}[i] = log W_{T-1}[0, i],   beta_{s-1}[i] = log sum_o W_{s-1}[o, i] exp(e_s[o] + beta_s[o])
//     gamma_s[i]    = exp(t_s[i] + beta_s[i]) / sum_j exp(t_s[j] + beta_s[j])      -> keep[b, var_s, :]
// Every (row, step) is normalised by its own sum, so neither t nor beta carries the row's scale: beta is kept relative as
// well (the row maximum that the forward adds to its scale is simply dropped), and a posterior is formed from small numbers.
//
// The forward's decomposition, mirrored: the same workgroup of min(K / 32, 4) waves owns the same 32 rows from step T - 1 down
// to 0, a wave the same blocks of units -- as the blocks of t it reads back with the lane mapping they were written with, and as
// the OUTPUT blocks i of the transposed contraction, so beta stays in registers in MFMA output = input layout.  Per step:
//   A  q = e + beta and u = t + beta on the wave's blocks; both row maxima in ONE exchange between the waves; g = exp(u - Mu)
//      and its row sum in a second exchange, which is also the barrier behind p = 2^96 exp(q - Mq) in the shared tile;
//      gamma = g / sum goes to keep[b, var_s, :] in place.
//   B  beta_{s-1} = log_unscaled(W_{s-1}^T p) on v_mfma_f32_32x32x2_f32.  Operand A is now W^T: lane (i, kh) needs
//      W[o][32 ib + i] for the 8 values o = 16 r + 8 h + 4 kh + t of a unit of 16 o-rows x 32 i-columns -- for a fixed o, 32 lanes
//      read one contiguous 128-byte row segment.  Eight global_load_lds_dword per lane land the unit as [slot 4 h + t][lane] in the
//      wave's private ring (same 2 KiB units, depth and LDS as the forward; 8 requests a unit, so unit u has landed once
//      8 (NBUF - 1) younger LOADS are in flight: the gamma stores also count on vmcnt but only ever make the wait longer);
//      four ds_read2st64_b32 (stride 64 dwords = one slot) fetch a lane's 8 values, conflict-free.
// The emission row of step s - 1 (and x of s - 2) and, where the registers allow it (NOB <= 4), the hand-off of step s - 1 are
// requested while step s contracts.  A row the forward marked NaN (a category >= C) is NaN in every entry; a row without mass
// is 0 / 0 = NaN.  T = 1 has no contraction.
__device__ __forceinline__ float xhalf_sum(float v) {
  const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}
// a lane's 8 values of a transposed weight unit (slots 0 .. 7, one dword each at stride 64 dwords) and the two operand quads of
// the activation tile that meet them
__device__ __forceinline__ void lds_read_wt(f32x2v& w01, f32x2v& w23, f32x2v& w45, f32x2v& w67, f32x4v& p0, f32x4v& p1, uint32_t wa,
                                            uint32_t pa) {
  asm volatile(
      "ds_read2st64_b32 %0, %6 offset1:1\n\tds_read2st64_b32 %1, %6 offset0:2 offset1:3\n\t"
      "ds_read2st64_b32 %2, %6 offset0:4 offset1:5\n\tds_read2st64_b32 %3, %6 offset0:6 offset1:7\n\t"
      "ds_read_b128 %4, %7\n\tds_read_b128 %5, %7 offset:1024\n\ts_waitcnt lgkmcnt(0)"
      : "=&v"(w01), "=&v"(w23), "=&v"(w45), "=&v"(w67), "=&v"(p0), "=&v"(p1)
      : "v"(wa), "v"(pa)
      : "memory");
}

//
// STATS (ck_hmm_backward_stats, DESIGN.md section 11, "Expected statistics (Baum-Welch E-step)"): the same pass also leaves,
// per (row, step), the two operand rows of the pair sum  N_s = W_s o (R_{s+1}^T A_s)  of ck_hmm_stats.hip:
//     a_s = exp(t_s - M_s)  (M_s the forward's clamped row maximum of t_s: a third maximum in the first exchange)
//     r_s = exp(q_s - Mu_s) / z_s = exp(q_s - Mq_s) c_s,   c_s = exp(Mq_s - Mu_s) / z_s
// Since exp(t_{s+1}[o]) = exp(e_{s+1}[o]) sum_i W_s[o, i] a_s[i], sum_{o,i} r_{s+1}[o] W_s[o, i] a_s[i] = 1 for a live row, log p
// never subtracted.  c reaches e^154 where y is tiny (peaked parameters), so its power of two 2^lc is SPLIT: r' = 2^h exp(q - Mq)
// with h = floor(lc / 2) goes to pair_r[b, var_s, :] and a'_{s-1} = 2^(lc - h) exp(t_{s-1} - M_{s-1}) to pair_a[b, var_{s-1}, :] one step
// later, both folded into the offset of the exponential: operands of a pair that counts stay within 2^+-111.  A DEAD row (log p not
// finite) is zeros in gamma and in both operands.  The STATS = false instantiation is the code it was.
template <int NOB, bool STATS = false>
__global__ void __launch_bounds__(256) hmm_backward_kernel(const HmmArgs a) {
  constexpr int NBUF = NOB > 4 ? 3 : 8;
  constexpr int NMAX = STATS ? 3 : 2;  // row maxima of the first exchange
  constexpr bool EARLY = NOB <= 4;  // three register tiles a block (e, t, beta): above, t is read back after the contraction
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int K = a.K, NQ = K >> 5, T = a.T;
  const int nwaves = blockDim.x >> 6;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int kh = lane >> 5, row = lane & 31;
  const int b = blockIdx.x * 32 + row;
  const bool live = b < a.B;
  const int bl = live ? b : a.B - 1;  // (rows past B repeat the last one's emissions, read no hand-off and store nothing)
  int nob = 0;
#pragma unroll
  for (int j = 0; j < NOB; ++j) nob += wave + nwaves * j < NQ ? 1 : 0;

  // LDS: activation tile [NQ][4][64] float4 | row maxima [NMAX][4][32] | row sums [4][32] | weight rings [waves][NBUF][8][64] float
  const uint32_t act = static_cast<uint32_t>(reinterpret_cast<uintptr_t>(smem));
  const uint32_t red = act + NQ * 4096;
  const uint32_t rsum = red + NMAX * kHmmWaves * 128;
  float* const ring_p = smem + NQ * 1024 + (NMAX + 1) * kHmmWaves * 32 + wave * (NBUF * kHmmUnit);
  const uint32_t ring = rsum + kHmmWaves * 128 + wave * (NBUF * kHmmUnit * 4) + lane * 4;

  const bool bad = a.out[bl] != a.out[bl];  // the forward's verdict on the row
  const bool dead = STATS && !(fabsf(a.out[bl]) < INFINITY);  // (NaN, or no mass)
  float ca = 0.f;  // STATS: lc - h of the step above, the exponent that a' of this step carries
  auto load_x = [&](int s) -> int64_t { return (a.x != nullptr && s >= 0) ? a.x[static_cast<int64_t>(bl) * a.D + a.var[s]] : 0; };
  auto row_of = [&](int s, int64_t xv) -> const float* {  // nullptr: the entry is missing (or out of range: the row is NaN)
    const int64_t f = a.fold[s];
    if (a.x == nullptr) return a.rows + (f * a.B + bl) * K;
    if (xv < 0 || xv >= a.C || (a.integ != nullptr && a.integ[a.var[s]] != 0)) return nullptr;
    return a.rows + (f * (a.C + 1) + xv) * K;
  };
  float e[NOB][16], t[NOB][16], be[NOB][16];
  auto load_e = [&](const float* r) {
#pragma unroll
    for (int j = 0; j < NOB; ++j) {
      const int q = wave + nwaves * j;
      if (q < NQ && r != nullptr) {
        tile_load(r + 32 * q + 4 * kh, e[j]);
      } else {
#pragma unroll
        for (int i = 0; i < 16; ++i) e[j][i] = 0.f;
      }
    }
  };
  auto keep_row = [&](int s) -> float* { return a.keep + (static_cast<int64_t>(bl) * a.D + a.var[s]) * K + 4 * kh; };
  auto load_t = [&](int s) {
    const float* src = keep_row(s);
#pragma unroll
    for (int j = 0; j < NOB; ++j) {
      const int q = wave + nwaves * j;
      if (q < NQ && live) {
        keep_load(src + 32 * q, t[j]);
      } else {
#pragma unroll
        for (int i = 0; i < 16; ++i) t[j][i] = 0.f;
      }
    }
  };
  // unit u of a step = (owned block j of COLUMNS, r): rows 16 r .. 16 r + 15 of W, columns 32 ib .. 32 ib + 31
  auto issue = [&](const float* w, int u) {
    const int j = u / (2 * NQ), r = u - j * 2 * NQ;
    const int ib = wave + nwaves * j;
    const float* src = w + static_cast<int64_t>(16 * r + 4 * kh) * K + 32 * ib + row;
    float* dst = ring_p + (u % NBUF) * kHmmUnit;
#pragma unroll
    for (int c = 0; c < 8; ++c)
      __builtin_amdgcn_global_load_lds((ck::gptr_t)(src + static_cast<int64_t>(8 * (c >> 2) + (c & 3)) * K), (ck::lptr_t)(dst + 64 * c), 4, 0,
                                       0);
  };

  {  // beta_{T-1} = log of row 0 of the last weight
    const float* wl = a.w[T - 1];
#pragma unroll
    for (int j = 0; j < NOB; ++j) {
      const int q = wave + nwaves * j;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const float4 w4 = q < NQ ? ck::gload4(wl + 32 * q + 8 * g + 4 * kh) : make_float4(1.f, 1.f, 1.f, 1.f);
        be[j][4 * g] = logf(w4.x), be[j][4 * g + 1] = logf(w4.y), be[j][4 * g + 2] = logf(w4.z), be[j][4 * g + 3] = logf(w4.w);
      }
    }
  }
  load_e(row_of(T - 1, load_x(T - 1)));
  load_t(T - 1);
  int64_t xn = load_x(T - 2);

  for (int s = T - 1; s >= 0; --s) {
    const bool first = s == 0;
    const float* w = first ? nullptr : a.w[s - 1];
    const int U = first ? 0 : nob * NQ * 2;
    for (int u = 0; u < NBUF - 1 && u < U; ++u) issue(w, u);

    // ---- A: q = e + beta, u = t + beta, their row maxima in one exchange
    float mq = -INFINITY, mu = -INFINITY, mt = -INFINITY;
#pragma unroll
    for (int j = 0; j < NOB; ++j)
      if (j < nob) {
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          e[j][i] += be[j][i];
          mq = fmaxf(mq, e[j][i]);
          if constexpr (STATS) {  // (t itself stays until a' is formed from it)
            mt = fmaxf(mt, t[j][i]);
            mu = fmaxf(mu, t[j][i] + be[j][i]);
          } else {
            t[j][i] += be[j][i];
            mu = fmaxf(mu, t[j][i]);
          }
        }
      }
    mq = ck::xhalf_max(mq);
    mu = ck::xhalf_max(mu);
    asm volatile("ds_write_b32 %0, %1\n\tds_write_b32 %0, %2 offset:512" ::"v"(red + (wave * 32 + row) * 4), "v"(mq), "v"(mu) : "memory");
    if constexpr (STATS) {
      mt = ck::xhalf_max(mt);
      asm volatile("ds_write_b32 %0, %1 offset:1024" ::"v"(red + (wave * 32 + row) * 4), "v"(mt) : "memory");
    }
    sync_lds();
    for (int k = 0; k < nwaves; ++k) {
      float o0, o1;
      asm volatile("ds_read_b32 %0, %2\n\tds_read_b32 %1, %2 offset:512\n\ts_waitcnt lgkmcnt(0)"
                   : "=&v"(o0), "=&v"(o1)
                   : "v"(red + (k * 32 + row) * 4)
                   : "memory");
      mq = fmaxf(mq, o0);
      mu = fmaxf(mu, o1);
      if constexpr (STATS) {
        float o2;
        asm volatile("ds_read_b32 %0, %1 offset:1024\n\ts_waitcnt lgkmcnt(0)" : "=v"(o2) : "v"(red + (k * 32 + row) * 4) : "memory");
        mt = fmaxf(mt, o2);
      }
    }
    mq = ck::clamp_finite(mq);
    mu = ck::clamp_finite(mu);
    if constexpr (STATS) {
      // a'_s = 2^ca exp(t_s - M_s) for the pair sum of step s (none above the last step), then u = t + beta as before
      if (s + 1 < T && live) {
        const float nma = exp_offset(ck::clamp_finite(mt), ca);
        float* dst = a.pair_a + (static_cast<int64_t>(b) * a.D + a.var[s]) * K + 4 * kh;
#pragma unroll
        for (int j = 0; j < NOB; ++j)
          if (j < nob) {
            float p[16];
#pragma unroll
            for (int i = 0; i < 16; ++i) p[i] = dead ? 0.f : __builtin_amdgcn_exp2f(fmaf(t[j][i], kL2E, nma));
            keep_store(dst + 32 * (wave + nwaves * j), p);
          }
      }
#pragma unroll
      for (int j = 0; j < NOB; ++j)
        if (j < nob) {
#pragma unroll
          for (int i = 0; i < 16; ++i) t[j][i] += be[j][i];
        }
    }
    // g = exp(u - Mu) and the wave's share of its row sum; p = 2^96 exp(q - Mq) into the shared tile
    const float nmu = exp_offset(mu, 0.f);
    float z = 0.f;
#pragma unroll
    for (int j = 0; j < NOB; ++j)
      if (j < nob) {
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          t[j][i] = __builtin_amdgcn_exp2f(fmaf(t[j][i], kL2E, nmu));
          z += t[j][i];
        }
      }
    z = xhalf_sum(z);
    asm volatile("ds_write_b32 %0, %1" ::"v"(rsum + (wave * 32 + row) * 4), "v"(z) : "memory");
    if (!first) {
      const float nmq = exp_offset(mq, kHmmHead);
#pragma unroll
      for (int j = 0; j < NOB; ++j)
        if (j < nob) {
          const uint32_t dst = act + (wave + nwaves * j) * 4096 + lane * 16;
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            float p[4];
#pragma unroll
            for (int c = 0; c < 4; ++c) p[c] = __builtin_amdgcn_exp2f(fmaf(e[j][4 * g + c], kL2E, nmq));
            lds_w4(dst + g * 1024, p[0], p[1], p[2], p[3]);
          }
        }
    }
    sync_lds();
    z = 0.f;
    for (int k = 0; k < nwaves; ++k) {  // (every wave adds the shares in the same order)
      float o;
      asm volatile("ds_read_b32 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=v"(o) : "v"(rsum + (k * 32 + row) * 4) : "memory");
      z += o;
    }
    const float inv = bad ? __builtin_nanf("") : 1.f / z;  // (no mass: 0 * inf = NaN)
    if (live) {
      float* dst = keep_row(s);
#pragma unroll
      for (int j = 0; j < NOB; ++j)
        if (j < nob) {
#pragma unroll
          for (int i = 0; i < 16; ++i) t[j][i] = STATS && dead ? 0.f : t[j][i] * inv;
          keep_store(dst + 32 * (wave + nwaves * j), t[j]);
        }
    }
    if constexpr (STATS) {
      // r'_s = 2^h exp(q_s - Mq_s) for the pair sum of step s - 1; the rest of c_s = 2^lc travels with a'_{s-1}
      const float lc = (mq - mu) * kL2E - __builtin_amdgcn_logf(z);
      const float h = floorf(0.5f * lc);
      ca = lc - h;
      if (!first && live) {
        const float nmr = exp_offset(mq, h);
        float* dst = a.pair_r + (static_cast<int64_t>(b) * a.D + a.var[s]) * K + 4 * kh;
#pragma unroll
        for (int j = 0; j < NOB; ++j)
          if (j < nob) {
            float p[16];
#pragma unroll
            for (int i = 0; i < 16; ++i) p[i] = dead ? 0.f : __builtin_amdgcn_exp2f(fmaf(e[j][i], kL2E, nmr));
            keep_store(dst + 32 * (wave + nwaves * j), p);
          }
      }
    }
    if (first) break;

    // the emission row (and, registers allowing, the hand-off) of step s - 1 travels while this step contracts
    load_e(row_of(s - 1, xn));
    xn = load_x(s - 2);
    if constexpr (EARLY) load_t(s - 1);

    // ---- B: beta_{s-1} = log(W_{s-1}^T p) on the wave's blocks of columns, in registers
    int u = 0;
    static_for<0, NOB>([&](auto jc) {
      constexpr int j = decltype(jc)::value;
      if (j >= nob) return;
      f32x16 acc;
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[r] = 0.f;
      for (int r = 0; r < 2 * NQ; ++r, ++u) {
        if (u + NBUF - 1 < U) {
          issue(w, u + NBUF - 1);
          asm volatile("s_waitcnt vmcnt(%0)" ::"n"(8 * (NBUF - 1)) : "memory");
        } else {
          asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        f32x2v w01, w23, w45, w67;
        f32x4v p0, p1;
        lds_read_wt(w01, w23, w45, w67, p0, p1, ring + (u % NBUF) * (kHmmUnit * 4), act + r * 2048 + lane * 16);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(w01[0], p0[0], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(w01[1], p0[1], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(w23[0], p0[2], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(w23[1], p0[3], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(w45[0], p1[0], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(w45[1], p1[1], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(w67[0], p1[2], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(w67[1], p1[3], acc, 0, 0, 0);
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) be[j][r] = log_unscaled(acc[r]);
    });
    if constexpr (!EARLY) load_t(s - 1);
  }
}

enum class HmmPass { kForward, kForwardKeep, kBackward, kBackwardStats };
template <int NOB>
int hmm_launch_pass(HmmPass pass, const HmmArgs& a, void* stream) {
  constexpr int NBUF = NOB > 4 ? 3 : 8;
  switch (pass) {
    case HmmPass::kForward: return hmm_launch(hmm_forward_kernel<NOB>, NBUF, kHmmWaves * 32, a, stream);
    case HmmPass::kForwardKeep: return hmm_launch(hmm_forward_kernel<NOB, true>, NBUF, kHmmWaves * 32, a, stream);
    case HmmPass::kBackward: return hmm_launch(hmm_backward_kernel<NOB>, NBUF, 3 * kHmmWaves * 32, a, stream);
    default: return hmm_launch(hmm_backward_kernel<NOB, true>, NBUF, 4 * kHmmWaves * 32, a, stream);
  }
}

int hmm_run(const char* name, HmmPass pass, const void* const* w_steps, const int32_t* step_fold, const int32_t* step_var, int T,
            int K, const float* rows, const int64_t* x, int D, int C, const int32_t* integrate, int B, float* out, float* keep,
            void* stream, float* pair_a = nullptr, float* pair_r = nullptr) {
  CK_REQUIRE(w_steps && step_fold && step_var && rows && out, "%s: null operand", name);
  CK_REQUIRE(T >= 1 && B >= 1, "%s: T = %d, B = %d", name, T, B);
  CK_REQUIRE(K >= 32 && K <= 1024 && K % 32 == 0, "%s: K = %d is not a multiple of 32 in 32 .. 1024", name, K);
  CK_REQUIRE(x == nullptr || (C >= 1 && D >= 1), "%s: a table source needs C >= 1 and D >= 1", name);
  CK_REQUIRE(x != nullptr || integrate == nullptr, "%s: a block source has its missing entries in the block", name);
  CK_REQUIRE(pass == HmmPass::kForward || (keep != nullptr && D >= T), "%s: needs the (B, D, K) hand-off buffer and D >= T", name);
  CK_REQUIRE(pass != HmmPass::kBackwardStats || (pair_a != nullptr && pair_r != nullptr), "%s: needs both operand buffers", name);
  const HmmArgs a{reinterpret_cast<const float* const*>(w_steps), step_fold, step_var, rows, x, integrate, out, C, D, T, B, K, keep,
                  pair_a, pair_r};
  const int NQ = K / 32, waves = NQ < kHmmWaves ? NQ : kHmmWaves;
  switch ((NQ + waves - 1) / waves) {
    case 1: return hmm_launch_pass<1>(pass, a, stream);
    case 2: return hmm_launch_pass<2>(pass, a, stream);
    case 3: return hmm_launch_pass<3>(pass, a, stream);
    case 4: return hmm_launch_pass<4>(pass, a, stream);
    case 5: return hmm_launch_pass<5>(pass, a, stream);
    case 6: return hmm_launch_pass<6>(pass, a, stream);
    case 7: return hmm_launch_pass<7>(pass, a, stream);
    default: return hmm_launch_pass<8>(pass, a, stream);
  }
}

}  // namespace

extern "C" int ck_hmm_forward(const void* const* w_steps, const int32_t* step_fold, const int32_t* step_var, int T, int K,
                              const float* rows, const int64_t* x, int D, int C, const int32_t* integrate, int B, float* out,
                              void* stream) {
  return hmm_run("ck_hmm_forward", HmmPass::kForward, w_steps, step_fold, step_var, T, K, rows, x, D, C, integrate, B, out, nullptr,
                 stream);
}

extern "C" int ck_hmm_forward_keep(const void* const* w_steps, const int32_t* step_fold, const int32_t* step_var, int T, int K,
                                   const float* rows, const int64_t* x, int D, int C, const int32_t* integrate, int B, float* log_prob,
                                   float* keep, void* stream) {
  return hmm_run("ck_hmm_forward_keep", HmmPass::kForwardKeep, w_steps, step_fold, step_var, T, K, rows, x, D, C, integrate, B,
                 log_prob, keep, stream);
}

extern "C" int ck_hmm_backward(const void* const* w_steps, const int32_t* step_fold, const int32_t* step_var, int T, int K,
                               const float* rows, const int64_t* x, int D, int C, const int32_t* integrate, int B,
                               const float* log_prob, float* keep, void* stream) {
  return hmm_run("ck_hmm_backward", HmmPass::kBackward, w_steps, step_fold, step_var, T, K, rows, x, D, C, integrate, B,
                 const_cast<float*>(log_prob), keep, stream);
}

extern "C" int ck_hmm_backward_stats(const void* const* w_steps, const int32_t* step_fold, const int32_t* step_var, int T, int K,
                                     const float* rows, const int64_t* x, int D, int C, const int32_t* integrate, int B,
                                     const float* log_prob, float* keep, float* pair_a, float* pair_r, void* stream) {
  return hmm_run("ck_hmm_backward_stats", HmmPass::kBackwardStats, w_steps, step_fold, step_var, T, K, rows, x, D, C, integrate, B,
                 const_cast<float*>(log_prob), keep, stream, pair_a, pair_r);
}
