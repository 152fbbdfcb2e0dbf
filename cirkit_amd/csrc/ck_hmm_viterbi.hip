// Viterbi decoding of a hidden Markov model in TWO launches ("Viterbi decoding").
//
//     delta_s[b, o] = log max_i W_s[o, i] exp(delta_{s-1}[b, i] + e_s[b, i]),   delta_{-1} = 0,   score delta_{T-1}[b, 0]
// is the chain of ck_hmm.hip with the sum replaced by a maximum, and the most probable path is read off it backwards.
//
// Launch 1, hmm_viterbi_forward_kernel: the ownership, the hand-off (phase A), the emission prefetch, the weight rings and the
// LDS layout of hmm_forward_kernel<NOB, KEEP = true> -- a workgroup of min(K / 32, 4) waves keeps 32 rows on chip for the whole
// chain, a wave owns blocks of 32 units, every step stores t_s = delta_{s-1} + e_s (relative to the row's scale) into
// keep[b, var_s, :] -- with a contraction of its own (phase B): max-times has no matrix instruction, its 32 K^2 products a
// workgroup and step go to the vector ALU.
//   Who owns what.  Lane l: row b = l & 31, half kh = l >> 5.  For an output block the lane keeps 16 running maxima, of units
//   8 g + 4 kh + t in register 4 g + t: the register tile of ck_tile.h, so delta never leaves registers between steps and
//   phase A writes p = 2^96 exp(t - M) straight from it.  The halves split the OUTPUTS, so nothing is combined across them.
//   Activations.  The tile [input quad K / 4][row 32] float4 is the forward's tile, byte for byte; a lane reads its own row's
//   quad with one ds_read_b128, 512 contiguous bytes a half-wave (both halves the same ones), for 64 products.
//   Weights.  One weight serves one product in a lane, since a lane owns one row.  What makes a weight read serve more is the
//   QUAD of lanes: the four lanes of a quad are four rows that need the same 16 outputs x 4 inputs, so lane k = l & 3 reads
//   only output k of each group of four -- one ds_read_b128, W[8 g + 4 kh + k][4 inputs] -- and the multiply takes its weight
//   from lane k' of the quad through DPP (quad_perm [k', k', k', k'], free in v_mul_f32).  A wave reads 128 distinct bytes per
//   instruction (8 quads of a half the same ones: a broadcast) for 16 products a lane: 5 LDS reads per 64 products, 96 vector
//   instructions -- the vector ALU, not LDS, bounds the loop.
//   The ring.  A unit is 32 outputs x 16 inputs as in the forward (2 KiB, two global_load_lds_dwordx4 a lane, the same ring
//   depths and the same vmcnt accounting), laid out for the reads above: instruction d of a unit, lane L -> W[16 d + (L & 15)]
//   [16 r + 4 (L >> 4) ..], so that byte 1024 d + 256 c + 128 (g & 1) + 64 kh + 16 k of the unit is what lane (kh, k) reads
//   for input quad c and output group g = 2 d + (g & 1).  16 rows x 64 contiguous bytes per request.
//   The inner loop per unit: 20 ds_read_b128 in one batch, then 256 v_mul_f32_dpp and 128 v_max3_f32 -- 1.5 vector instructions
//   a product, the minimum without packed multiplies (this file is built without them, like ck_hmm.hip).
// Linear-times-max, not log-plus-max: W is used as the parameter graph leaves it (no K^2 table of logarithms per step, which
// would be a third launch or K^2 v_log_f32 per workgroup and step), a product costs the same 1.5 instructions either way,
// and with the forward's headroom (kHmmHead) a state up to 154 nats below its row's best survives the flush of denormals:
// the range the forward already relies on under peaked parameters.  No backpointers are tracked.
//
// Launch 2, hmm_viterbi_backtrack_kernel: one wave a row, from step T - 1 down: z_s = argmax_i t_s[i] + log W_s[z_{s+1} or 0, i]
// from the kept hand-off and ONE contiguous weight row, O(K) a (row, step).  Lane l holds elements 4 l + 256 e + (0 .. 3); the
// arg-max crosses the wave by DPP and permlane swaps, the lowest index winning ties; units >= num_states never compete.
// t_{s-1} is requested before z_s is known (its address does not depend on it).  A row whose score is -inf or NaN gets -1.
#include "ck_hmm.h"

namespace {

// the weight of lane k' of the quad times the lane's own activation: v_mul_f32 with a DPP source
template <int KQ>
__device__ __forceinline__ float quad_mul(float w, float p) {
  return __uint_as_float(__builtin_amdgcn_mov_dpp(__float_as_uint(w), KQ * 0x55, 0xF, 0xF, true)) * p;
}
// the four outputs of a group against one input quad: acc[k'] = max(acc[k'], W[k'][t] p[t], t = 0 .. 3)
__device__ __forceinline__ void group_max(float* acc, const f32x4v& w, const f32x4v& p) {
  static_for<0, 4>([&](auto kc) {
    constexpr int k = decltype(kc)::value;
    acc[k] = __builtin_fmaxf(__builtin_fmaxf(acc[k], quad_mul<k>(w[0], p[0])), quad_mul<k>(w[1], p[1]));
    acc[k] = __builtin_fmaxf(__builtin_fmaxf(acc[k], quad_mul<k>(w[2], p[2])), quad_mul<k>(w[3], p[3]));
  });
}
// everything a lane reads of one unit: its row's 4 input quads and, per quad, its output's weights in the 4 groups
__device__ __forceinline__ void lds_read_unit(f32x4v (&p)[4], f32x4v (&w)[4][4], uint32_t pa, uint32_t wa) {
  asm volatile(
      "ds_read_b128 %0, %20\n\tds_read_b128 %4, %21\n\tds_read_b128 %5, %21 offset:128\n\t"
      "ds_read_b128 %6, %21 offset:1024\n\tds_read_b128 %7, %21 offset:1152\n\t"
      "ds_read_b128 %1, %20 offset:512\n\tds_read_b128 %8, %21 offset:256\n\tds_read_b128 %9, %21 offset:384\n\t"
      "ds_read_b128 %10, %21 offset:1280\n\tds_read_b128 %11, %21 offset:1408\n\t"
      "ds_read_b128 %2, %20 offset:1024\n\tds_read_b128 %12, %21 offset:512\n\tds_read_b128 %13, %21 offset:640\n\t"
      "ds_read_b128 %14, %21 offset:1536\n\tds_read_b128 %15, %21 offset:1664\n\t"
      "ds_read_b128 %3, %20 offset:1536\n\tds_read_b128 %16, %21 offset:768\n\tds_read_b128 %17, %21 offset:896\n\t"
      "ds_read_b128 %18, %21 offset:1792\n\tds_read_b128 %19, %21 offset:1920\n\ts_waitcnt lgkmcnt(0)"
      : "=&v"(p[0]), "=&v"(p[1]), "=&v"(p[2]), "=&v"(p[3]), "=&v"(w[0][0]), "=&v"(w[0][1]), "=&v"(w[0][2]), "=&v"(w[0][3]),
        "=&v"(w[1][0]), "=&v"(w[1][1]), "=&v"(w[1][2]), "=&v"(w[1][3]), "=&v"(w[2][0]), "=&v"(w[2][1]), "=&v"(w[2][2]),
        "=&v"(w[2][3]), "=&v"(w[3][0]), "=&v"(w[3][1]), "=&v"(w[3][2]), "=&v"(w[3][3])
      : "v"(pa), "v"(wa)
      : "memory");
}

template <int NOB>
__global__ void __launch_bounds__(256) hmm_viterbi_forward_kernel(const HmmArgs a) {
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

  // LDS: activation tile [K / 4][32] float4 | row maxima [4][32] | weight rings [waves][NBUF] units of 2 KiB
  const uint32_t act = static_cast<uint32_t>(reinterpret_cast<uintptr_t>(smem));
  const uint32_t red = act + NQ * 4096;
  float* const ring_p = smem + NQ * 1024 + kHmmWaves * 32 + wave * (NBUF * kHmmUnit);
  const uint32_t ring = red + kHmmWaves * 128 + wave * (NBUF * kHmmUnit * 4) + kh * 64 + (lane & 3) * 16;

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
  // unit u of a step = (owned block j, half block of inputs r): rows 32 ob .. of W, inputs 16 r ..
  auto issue = [&](const float* w, int u) {
    const int j = u / (2 * NQ), r = u - j * 2 * NQ;
    const int ob = wave + nwaves * j;
    const float* src = w + static_cast<int64_t>(32 * ob + (lane & 15)) * K + 16 * r + 4 * (lane >> 4);
    float* dst = ring_p + (u % NBUF) * kHmmUnit;
    __builtin_amdgcn_global_load_lds((ck::gptr_t)src, (ck::lptr_t)dst, 16, 0, 0);
    __builtin_amdgcn_global_load_lds((ck::gptr_t)(src + 16 * static_cast<int64_t>(K)), (ck::lptr_t)(dst + 256), 16, 0, 0);
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

    // ---- A: t = delta + e, kept; its row maximum; p = 2^96 exp(t - M) into the shared tile
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
    if (live) {
      float* dst = a.keep + (static_cast<int64_t>(b) * a.D + a.var[s]) * K + 4 * kh;
#pragma unroll
      for (int j = 0; j < NOB; ++j)
        if (j < nob) keep_store(dst + 32 * (wave + nwaves * j), e[j]);
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

    // ---- B: y = max_i W p on the wave's output blocks (vector ALU), log y stays in registers
    int u = 0;
    static_for<0, NOB>([&](auto jc) {
      constexpr int j = decltype(jc)::value;
      if (j >= nob) return;
      float acc[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[r] = 0.f;
      for (int r = 0; r < 2 * NQ; ++r, ++u) {
        if (u + NBUF - 1 < U) {
          issue(w, u + NBUF - 1);
          asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * (NBUF - 1)) : "memory");
        } else {
          asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        f32x4v p[4], wq[4][4];  // wq[c][g]: input quad c of the unit, output group g
        lds_read_unit(p, wq, act + r * 2048 + row * 16, ring + (u % NBUF) * (kHmmUnit * 4));
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
          for (int g = 0; g < 4; ++g) group_max(acc + 4 * g, wq[c][g], p[c]);
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
        d = fmaxf(fmaxf(d, w4.x * (*pg[g])[0]), w4.y * (*pg[g])[1]);
        d = fmaxf(fmaxf(d, w4.z * (*pg[g])[2]), w4.w * (*pg[g])[3]);
      }
    }
    d = ck::xhalf_max(d);
    if (live && kh == 0) a.out[b] = bad ? __builtin_nanf("") : scale + log_unscaled(d);
  }
}

// ---- the walk back ----------------------------------------------------------------------------------------------------------
// (value, index) of the better of two candidates: the larger value, the lower index between equal ones
__device__ __forceinline__ void take_better(float& v, int& i, float ov, int oi) {
  const bool t = ov > v || (ov == v && oi < i);
  v = t ? ov : v;
  i = t ? oi : i;
}
template <int CTRL>
__device__ __forceinline__ void argmax_dpp(float& v, int& i) {
  const float ov = __uint_as_float(__builtin_amdgcn_mov_dpp(__float_as_uint(v), CTRL, 0xF, 0xF, true));
  const int oi = __builtin_amdgcn_mov_dpp(i, CTRL, 0xF, 0xF, true);
  take_better(v, i, ov, oi);
}
// over the 64 lanes, every lane gets the result (the exchange pattern of ck::wave_reduce)
__device__ __forceinline__ void wave_argmax(float& v, int& i) {
  argmax_dpp<0xB1>(v, i);
  argmax_dpp<0x4E>(v, i);
  argmax_dpp<0x141>(v, i);
  argmax_dpp<0x140>(v, i);
  {
    const auto rv = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    const auto ri = __builtin_amdgcn_permlane16_swap(i, i, false, false);
    v = __uint_as_float(rv[0]), i = static_cast<int>(ri[0]);
    take_better(v, i, __uint_as_float(rv[1]), static_cast<int>(ri[1]));
  }
  {
    const auto rv = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    const auto ri = __builtin_amdgcn_permlane32_swap(i, i, false, false);
    v = __uint_as_float(rv[0]), i = static_cast<int>(ri[0]);
    take_better(v, i, __uint_as_float(rv[1]), static_cast<int>(ri[1]));
  }
}

constexpr int kBackRows = 4;  // rows (waves) of a workgroup of the walk back
constexpr int kNoState = 0x7fffffff;

__global__ void __launch_bounds__(64 * kBackRows) hmm_viterbi_backtrack_kernel(const float* const* w_steps, const int32_t* var, int T, int K,
                                                                               int num_states, int D, int B, const float* score,
                                                                               const float* keep, int64_t* states) {
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * kBackRows + (threadIdx.x >> 6);
  if (b >= B) return;
  int64_t* const out = states + static_cast<int64_t>(b) * D;
  if (!(score[b] > -INFINITY)) {  // no path of positive mass, or NaN
    if (lane == 0)
      for (int s = 0; s < T; ++s) out[var[s]] = -1;
    return;
  }
  const float* const base = keep + static_cast<int64_t>(b) * D * K;
  const float4 none = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
  float4 t[4], tn[4];  // the hand-off of this step, and of the one below it
  auto load_t = [&](int s, float4 (&v)[4]) {
    const float* src = base + static_cast<int64_t>(var[s]) * K + 4 * lane;
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = 4 * lane + 256 * e < K ? ck::gload4(src + 256 * e) : none;
  };
  load_t(T - 1, t);
  int z = 0;  // the row of W_s that the step above chose: unit 0 above the last step
  for (int s = T - 1; s >= 0; --s) {
    if (s > 0) load_t(s - 1, tn);
    const float* wr = w_steps[s] + static_cast<int64_t>(z) * K + 4 * lane;
    float bv = -INFINITY;
    int bi = kNoState;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int i0 = 4 * lane + 256 * e;
      if (i0 < K) {
        const float4 w4 = ck::gload4(wr + 256 * e);
        const float v[4] = {t[e].x + logf(w4.x), t[e].y + logf(w4.y), t[e].z + logf(w4.z), t[e].w + logf(w4.w)};
#pragma unroll
        for (int c = 0; c < 4; ++c)
          if (i0 + c < num_states) take_better(bv, bi, v[c], i0 + c);
      }
    }
    wave_argmax(bv, bi);
    z = bi < num_states ? bi : 0;  // (never past the weights, whatever the values were)
    if (lane == 0) out[var[s]] = bi < num_states ? bi : -1;
#pragma unroll
    for (int e = 0; e < 4; ++e) t[e] = tn[e];
  }
}

int viterbi_forward(const HmmArgs& a, void* stream) {
  const int NQ = a.K / 32, waves = NQ < kHmmWaves ? NQ : kHmmWaves;
  switch ((NQ + waves - 1) / waves) {
    case 1: return hmm_launch(hmm_viterbi_forward_kernel<1>, 8, kHmmWaves * 32, a, stream);
    case 2: return hmm_launch(hmm_viterbi_forward_kernel<2>, 8, kHmmWaves * 32, a, stream);
    case 3: return hmm_launch(hmm_viterbi_forward_kernel<3>, 8, kHmmWaves * 32, a, stream);
    case 4: return hmm_launch(hmm_viterbi_forward_kernel<4>, 8, kHmmWaves * 32, a, stream);
    case 5: return hmm_launch(hmm_viterbi_forward_kernel<5>, 3, kHmmWaves * 32, a, stream);
    case 6: return hmm_launch(hmm_viterbi_forward_kernel<6>, 3, kHmmWaves * 32, a, stream);
    case 7: return hmm_launch(hmm_viterbi_forward_kernel<7>, 3, kHmmWaves * 32, a, stream);
    default: return hmm_launch(hmm_viterbi_forward_kernel<8>, 3, kHmmWaves * 32, a, stream);
  }
}

}  // namespace

extern "C" int ck_hmm_viterbi_forward(const void* const* w_steps, const int32_t* step_fold, const int32_t* step_var, int T, int K,
                                      const float* rows, const int64_t* x, int D, int C, const int32_t* integrate, int B, float* score,
                                      float* keep, void* stream) {
  const char* name = "ck_hmm_viterbi_forward";
  CK_REQUIRE(w_steps && step_fold && step_var && rows && score && keep, "%s: null operand", name);
  CK_REQUIRE(T >= 1 && B >= 1 && D >= T, "%s: T = %d, B = %d, D = %d", name, T, B, D);
  CK_REQUIRE(K >= 32 && K <= 1024 && K % 32 == 0, "%s: K = %d is not a multiple of 32 in 32 .. 1024", name, K);
  CK_REQUIRE(x == nullptr || C >= 1, "%s: a table source needs C >= 1", name);
  CK_REQUIRE(x != nullptr || integrate == nullptr, "%s: a block source has its missing entries in the block", name);
  const HmmArgs a{reinterpret_cast<const float* const*>(w_steps), step_fold, step_var, rows, x, integrate, score, C, D, T, B, K, keep};
  return viterbi_forward(a, stream);
}

extern "C" int ck_hmm_viterbi_backtrack(const void* const* w_steps, const int32_t* step_var, int T, int K, int num_states, int D, int B,
                                        const float* score, const float* keep, int64_t* states, void* stream) {
  const char* name = "ck_hmm_viterbi_backtrack";
  CK_REQUIRE(w_steps && step_var && score && keep && states, "%s: null operand", name);
  CK_REQUIRE(T >= 1 && B >= 1 && D >= T, "%s: T = %d, B = %d, D = %d", name, T, B, D);
  CK_REQUIRE(K >= 32 && K <= 1024 && K % 32 == 0, "%s: K = %d is not a multiple of 32 in 32 .. 1024", name, K);
  CK_REQUIRE(num_states >= 1 && num_states <= K, "%s: %d states of %d units", name, num_states, K);
  const dim3 grid((B + kBackRows - 1) / kBackRows), block(64 * kBackRows);
  return ck::launch(hmm_viterbi_backtrack_kernel, grid, block, 0, stream, reinterpret_cast<const float* const*>(w_steps), step_var, T, K,
                    num_states, D, B, score, keep, states);
}
