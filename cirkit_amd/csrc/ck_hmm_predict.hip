// The chain-rule decomposition of a hidden Markov model in ONE launch ("Autoregressive conditionals of
// chains"): log p(x_{o_j} | x_{o_0 .. o_{j-1}}) for every position j of every row and, in the COND instantiation, the whole
// predictive distribution p(X_{o_j} = c | x_{o_0 .. o_{j-1}}).
//
// A chain plan GENERATES from step T - 1 (the prior is row 0 of W_{T-1}) down to step 0, so the generative order is
// o_j = var_{T-1-j} and the recursion that ck_hmm_backward runs is the predictive filter of that order:
//     beta_{T-1}[i] = log W_{T-1}[0, i],   beta_{s-1}[i] = log sum_o W_{s-1}[o, i] exp(e_s[o] + beta_s[o])
// beta_s, normalised, is p(z_s | x of the steps above s); with q_s = e_s + beta_s
//     log p(x_s | steps above) = logsumexp(q_s) - logsumexp(beta_s)                                     -> lp[b, T - 1 - s]
//     p(X_s = c | steps above) = sum_k E_s[c, k] exp(beta_s[k]) / sum_k exp(beta_s[k])                   -> cond[b, T - 1 - s, c]
// One walk down the chain gives every position: no forward pass, no (B, D, K) hand-off buffer, log p(x) never subtracted.
//
// Ownership is the backward pass's (ck_hmm.hip): a workgroup of min(K / 32, 4) waves owns 32 rows from step T - 1 down to 0, a
// wave its blocks of 32 units, beta stays in registers in MFMA output = input layout.  Per step s:
//   1  q = e + beta; the row maxima Mb of beta and Mq of q in ONE exchange between the waves; pb = 2^96 exp(beta - Mb) and
//      pq = 2^96 exp(q - Mq) (pq replaces q in its registers) and their row sums in a second exchange; the value stored is
//      (Mq + log Sq) - (Mb + log Sb).  Where the entry is missing e is zeros, q is beta bit for bit, both sides are formed by the
//      same instructions and the value is exactly 0.  The sums carry the factor 2^96 that log_unscaled takes off again, so the
//      terms kept reach as far down as the operands of the contraction do.
//   2  (COND) pb is the shared activation tile behind the second exchange's barrier.  It is contracted with the step's emission
//      matrix, (Cp, K) LINEAR probabilities with a category's row contiguous and the rows past C zero -- the row-major,
//      non-transposed weight shape of the FORWARD kernel: units of 32 categories x 16 states, two global_load_lds_dwordx4 a lane
//      into the wave's private ring, "at most 2 (NBUF - 1) requests outstanding" as there.  The blocks of 32 categories are dealt
//      to the waves (a runtime loop: one accumulator tile whatever C); a lane holds 4 consecutive categories per register group,
//      multiplies them by 1 / Sb and stores them 16 bytes at a time, as keep_store does.  The out stores count on vmcnt too but
//      only ever make a wait longer.
//   3  a barrier (every wave has read pb), pq into the same tile, a barrier, then beta_{s-1} = log_unscaled(W_{s-1}^T pq) with the
//      transposed units of ck_hmm_backward: eight global_load_lds_dword a lane, read back by ds_read2st64_b32.
// Without COND there is no step 2, pq goes into the tile before the second exchange and a step has the backward pass's two
// barriers.  The tile is used twice a step because two do not fit: at K = 1024 one takes 128 of the 160 KiB.  The ring is used
// twice a step as well, drained in between (the last NBUF - 1 units of a stream wait for everything).  NBUF = 8, 3 above K = 512.
//
// The emission contraction's own output is NOT reused as the next predictive state: y = E p gives the distribution over
// categories, the state after observing x_s is pq, which needs e_s[x_s] -- one row of the table of logarithms -- and its own
// maximum for the log-probability anyway; both exponentials of step 1 stay.
//
// Dead ends follow causality.  The observed value without mass: q is -inf everywhere, Mq is clamped, Sq = 0 and the value is -inf;
// pq = 0, so beta of every later position is -inf, Sb = 0, and both results are NaN (-inf - -inf; 0 x inf).  A category >= C: the
// row is NaN from its own position on, by a flag that is raised when that step is reached, not when its row was requested.
#include "ck_hmm.h"

namespace {

struct PredictArgs {
  const float* const* w;  // (T) the steps' evaluated weights, row-major (Ko, K)
  const int32_t* fold;    // (T) input fold of each step
  const int32_t* var;     // (T) its variable
  const float* rows;      // (F, C + 1, K) table of logarithms
  const float* emis;      // (F, Cp, K) linear table of hmm_emission_table_kernel (COND)
  const int64_t* x;       // (B, D) categories
  const int32_t* integ;   // (D) != 0: the variable is summed out; or nullptr
  float* lp;              // (B, T)
  float* cond;            // (B, T, Cp) (COND)
  int C, Cp, D, T, B, K;
};

__device__ __forceinline__ float xhalf_sum(float v) {
  const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}
// a lane's 8 values of a transposed weight unit (slots 0 .. 7, one dword each at stride 64 dwords) and the two operand quads of
// the activation tile that meet them (ck_hmm.hip: lds_read_wt)
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

template <int NOB, bool COND>
__global__ void __launch_bounds__(256) hmm_predict_kernel(const PredictArgs a) {
  constexpr int NBUF = NOB > 4 ? 3 : 8;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int K = a.K, NQ = K >> 5, T = a.T;
  const int nwaves = blockDim.x >> 6;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int kh = lane >> 5, row = lane & 31;
  const int b = blockIdx.x * 32 + row;
  const bool live = b < a.B;
  const int bl = live ? b : a.B - 1;  // (rows past B repeat the last one and store nothing)
  int nob = 0;                        // unit blocks of this wave
#pragma unroll
  for (int j = 0; j < NOB; ++j) nob += wave + nwaves * j < NQ ? 1 : 0;
  const int NCB = a.Cp >> 5;
  const int ncb = COND && wave < NCB ? (NCB - wave + nwaves - 1) / nwaves : 0;  // category blocks of this wave

  // LDS: activation tile [NQ][4][64] float4 | row maxima [2][4][32] | row sums [2][4][32] | weight rings [waves][NBUF][512] float
  const uint32_t act = static_cast<uint32_t>(reinterpret_cast<uintptr_t>(smem));
  const uint32_t red = act + NQ * 4096;
  const uint32_t rsum = red + 2 * kHmmWaves * 128;
  float* const ring_p = smem + NQ * 1024 + 4 * kHmmWaves * 32 + wave * (NBUF * kHmmUnit);
  const uint32_t ring = rsum + 2 * kHmmWaves * 128 + wave * (NBUF * kHmmUnit * 4);

  bool bad = false, badn = false;  // a category >= C at or above this step / at the step whose row was requested last
  auto load_x = [&](int s) -> int64_t { return s >= 0 ? a.x[static_cast<int64_t>(bl) * a.D + a.var[s]] : 0; };
  auto row_of = [&](int s, int64_t xv) -> const float* {  // nullptr: the entry is missing (or out of range: NaN from here on)
    if (xv < 0 || (a.integ != nullptr && a.integ[a.var[s]] != 0)) return nullptr;
    if (xv >= a.C) {
      badn = true;
      return nullptr;
    }
    return a.rows + (static_cast<int64_t>(a.fold[s]) * (a.C + 1) + xv) * K;
  };
  float e[NOB][16], be[NOB][16];
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
  // transition unit u of a step = (owned block j of COLUMNS, r): rows 16 r .. 16 r + 15 of W, columns 32 ib .. 32 ib + 31
  auto issue_t = [&](const float* w, int u) {
    const int j = u / (2 * NQ), r = u - j * 2 * NQ;
    const int ib = wave + nwaves * j;
    const float* src = w + static_cast<int64_t>(16 * r + 4 * kh) * K + 32 * ib + row;
    float* dst = ring_p + (u % NBUF) * kHmmUnit;
#pragma unroll
    for (int c = 0; c < 8; ++c)
      __builtin_amdgcn_global_load_lds((ck::gptr_t)(src + static_cast<int64_t>(8 * (c >> 2) + (c & 3)) * K), (ck::lptr_t)(dst + 64 * c), 4, 0,
                                       0);
  };
  // emission unit u of a step = (owned block jc of CATEGORIES, r): rows 32 cb .. of E, states 16 r .. 16 r + 15
  auto issue_e = [&](const float* em, int u) {
    const int jc = u / (2 * NQ), r = u - jc * 2 * NQ;
    const int cb = wave + nwaves * jc;
    const float* src = em + static_cast<int64_t>(32 * cb + row) * K + 16 * r + 4 * kh;
    float* dst = ring_p + (u % NBUF) * kHmmUnit;
    __builtin_amdgcn_global_load_lds((ck::gptr_t)src, (ck::lptr_t)dst, 16, 0, 0);
    __builtin_amdgcn_global_load_lds((ck::gptr_t)(src + 8), (ck::lptr_t)(dst + 256), 16, 0, 0);
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
  int64_t xn = load_x(T - 2);

  for (int s = T - 1; s >= 0; --s) {
    const bool first = s == 0;
    bad |= badn;
    const float* w = first ? nullptr : a.w[s - 1];
    const int U = first ? 0 : nob * NQ * 2;
    const float* em = COND ? a.emis + static_cast<int64_t>(a.fold[s]) * a.Cp * K : nullptr;
    const int UE = ncb * NQ * 2;
    if constexpr (COND) {
      for (int u = 0; u < NBUF - 1 && u < UE; ++u) issue_e(em, u);
    } else {
      for (int u = 0; u < NBUF - 1 && u < U; ++u) issue_t(w, u);
    }

    // ---- 1: q = e + beta, both row maxima in one exchange
    float mq = -INFINITY, mb = -INFINITY;
#pragma unroll
    for (int j = 0; j < NOB; ++j)
      if (j < nob) {
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          mb = fmaxf(mb, be[j][i]);
          e[j][i] += be[j][i];
          mq = fmaxf(mq, e[j][i]);
        }
      }
    mq = ck::xhalf_max(mq);
    mb = ck::xhalf_max(mb);
    asm volatile("ds_write_b32 %0, %1\n\tds_write_b32 %0, %2 offset:512" ::"v"(red + (wave * 32 + row) * 4), "v"(mq), "v"(mb) : "memory");
    sync_lds();
    for (int k = 0; k < nwaves; ++k) {
      float o0, o1;
      asm volatile("ds_read_b32 %0, %2\n\tds_read_b32 %1, %2 offset:512\n\ts_waitcnt lgkmcnt(0)"
                   : "=&v"(o0), "=&v"(o1)
                   : "v"(red + (k * 32 + row) * 4)
                   : "memory");
      mq = fmaxf(mq, o0);
      mb = fmaxf(mb, o1);
    }
    mq = ck::clamp_finite(mq);
    mb = ck::clamp_finite(mb);
    // pb = 2^96 exp(beta - Mb), pq = 2^96 exp(q - Mq) (in q's registers) and the wave's share of their row sums; the tile gets
    // pb (COND: the emission contraction reads it first) or pq
    const float nmq = exp_offset(mq, kHmmHead), nmb = exp_offset(mb, kHmmHead);
    float sq = 0.f, sb = 0.f;
#pragma unroll
    for (int j = 0; j < NOB; ++j)
      if (j < nob) {
        const uint32_t dst = act + (wave + nwaves * j) * 4096 + lane * 16;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          float pb[4];
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            pb[c] = __builtin_amdgcn_exp2f(fmaf(be[j][4 * g + c], kL2E, nmb));
            sb += pb[c];
            e[j][4 * g + c] = __builtin_amdgcn_exp2f(fmaf(e[j][4 * g + c], kL2E, nmq));
            sq += e[j][4 * g + c];
          }
          if constexpr (COND) {
            lds_w4(dst + g * 1024, pb[0], pb[1], pb[2], pb[3]);
          } else {
            if (!first) lds_w4(dst + g * 1024, e[j][4 * g], e[j][4 * g + 1], e[j][4 * g + 2], e[j][4 * g + 3]);
          }
        }
      }
    sq = xhalf_sum(sq);
    sb = xhalf_sum(sb);
    asm volatile("ds_write_b32 %0, %1\n\tds_write_b32 %0, %2 offset:512" ::"v"(rsum + (wave * 32 + row) * 4), "v"(sq), "v"(sb) : "memory");
    sync_lds();
    sq = 0.f, sb = 0.f;
    for (int k = 0; k < nwaves; ++k) {  // (every wave adds the shares in the same order)
      float o0, o1;
      asm volatile("ds_read_b32 %0, %2\n\tds_read_b32 %1, %2 offset:512\n\ts_waitcnt lgkmcnt(0)"
                   : "=&v"(o0), "=&v"(o1)
                   : "v"(rsum + (k * 32 + row) * 4)
                   : "memory");
      sq += o0;
      sb += o1;
    }
    if (live && wave == 0 && kh == 0) {
      float lq = mq + log_unscaled(sq), lb = mb + log_unscaled(sb);
      asm volatile("" : "+v"(lq), "+v"(lb));  // (both sides formed by the same instructions before anything is fused across them)
      a.lp[static_cast<int64_t>(b) * T + (T - 1 - s)] = bad ? __builtin_nanf("") : lq - lb;
    }

    // ---- 2: the predictive distribution over the categories, y = E_s pb / Sb, on the wave's blocks of categories
    if constexpr (COND) {
      const float inv = bad ? __builtin_nanf("") : 1.f / sb;  // (no mass above: 0 * inf = NaN)
      float* dst = a.cond + (static_cast<int64_t>(bl) * T + (T - 1 - s)) * a.Cp + 4 * kh;
      int u = 0;
      for (int jc = 0; jc < ncb; ++jc) {
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
        for (int r = 0; r < 2 * NQ; ++r, ++u) {
          if (u + NBUF - 1 < UE) {
            issue_e(em, u + NBUF - 1);
            asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * (NBUF - 1)) : "memory");
          } else {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
          }
          f32x4v w0, w1, p0, p1;
          const uint32_t wa = ring + lane * 16 + (u % NBUF) * (kHmmUnit * 4), pa = act + r * 2048 + lane * 16;
          lds_read4(w0, w1, p0, p1, wa, wa + 1024, pa, pa + 1024);
#pragma unroll
          for (int c = 0; c < 4; ++c) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(w0[c], p0[c], acc, 0, 0, 0);
#pragma unroll
          for (int c = 0; c < 4; ++c) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(w1[c], p1[c], acc, 0, 0, 0);
        }
        if (live) {
          float y[16];
#pragma unroll
          for (int r = 0; r < 16; ++r) y[r] = acc[r] * inv;
          keep_store(dst + 32 * (wave + nwaves * jc), y);
        }
      }
      if (first) break;
      // the ring is drained: the transition units start while the other waves finish with pb
      for (int v = 0; v < NBUF - 1 && v < U; ++v) issue_t(w, v);
      sync_lds();
#pragma unroll
      for (int j = 0; j < NOB; ++j)
        if (j < nob) {
          const uint32_t pd = act + (wave + nwaves * j) * 4096 + lane * 16;
#pragma unroll
          for (int g = 0; g < 4; ++g) lds_w4(pd + g * 1024, e[j][4 * g], e[j][4 * g + 1], e[j][4 * g + 2], e[j][4 * g + 3]);
        }
      sync_lds();
    }
    if (first) break;

    // the emission row of step s - 1 travels while this step contracts
    load_e(row_of(s - 1, xn));
    xn = load_x(s - 2);

    // ---- 3: beta_{s-1} = log(W_{s-1}^T pq) on the wave's blocks of columns, in registers
    int u = 0;
    static_for<0, NOB>([&](auto jc) {
      constexpr int j = decltype(jc)::value;
      if (j >= nob) return;
      f32x16 acc;
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[r] = 0.f;
      for (int r = 0; r < 2 * NQ; ++r, ++u) {
        if (u + NBUF - 1 < U) {
          issue_t(w, u + NBUF - 1);
          asm volatile("s_waitcnt vmcnt(%0)" ::"n"(8 * (NBUF - 1)) : "memory");
        } else {
          asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        f32x2v w01, w23, w45, w67;
        f32x4v p0, p1;
        lds_read_wt(w01, w23, w45, w67, p0, p1, ring + lane * 4 + (u % NBUF) * (kHmmUnit * 4), act + r * 2048 + lane * 16);
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
  }
}

// (F, C + 1, K) logarithms -> (F, Cp, K) linear probabilities, the rows past C zero; a thread four states of one (fold, category)
__global__ void __launch_bounds__(256) hmm_emission_table_kernel(const float* table, int K, int C, int Cp, int64_t quads, float* out) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (i >= quads) return;
  const int K4 = K >> 2;
  const int64_t fc = i / K4, f = fc / Cp;
  const int k4 = static_cast<int>(i - fc * K4), c = static_cast<int>(fc - f * Cp);
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  if (c < C) {
    const float4 t = ck::gload4(table + (f * (C + 1) + c) * K + 4 * k4);
    v = make_float4(expf(t.x), expf(t.y), expf(t.z), expf(t.w));
  }
  ck::gstore4(out + 4 * i, v);
}

template <int NOB>
int predict_launch(const PredictArgs& a, void* stream) {
  constexpr int NBUF = NOB > 4 ? 3 : 8;
  const int NQ = a.K / 32, waves = NQ < kHmmWaves ? NQ : kHmmWaves;
  const size_t lds = (static_cast<size_t>(NQ) * 1024 + 4 * kHmmWaves * 32 + static_cast<size_t>(waves) * NBUF * kHmmUnit) * sizeof(float);
  const dim3 grid((a.B + 31) / 32), block(64 * waves);
  auto kernel = a.cond != nullptr ? hmm_predict_kernel<NOB, true> : hmm_predict_kernel<NOB, false>;
  return ck::dispatch(
      [=](hipStream_t s) {
        if (lds > 48 * 1024) {
          hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                             static_cast<int>(lds));
          if (e != hipSuccess) return e;
        }
        hipLaunchKernelGGL(kernel, grid, block, lds, s, a);
        return hipGetLastError();
      },
      stream);
}

}  // namespace

extern "C" int ck_hmm_emission_table(const float* table, int F, int K, int C, float* emission, void* stream) {
  const char* name = "ck_hmm_emission_table";
  CK_REQUIRE(table && emission, "%s: null operand", name);
  CK_REQUIRE(F >= 1 && C >= 1, "%s: F = %d, C = %d", name, F, C);
  CK_REQUIRE(K >= 32 && K <= 1024 && K % 32 == 0, "%s: K = %d is not a multiple of 32 in 32 .. 1024", name, K);
  CK_REQUIRE(ck::aligned16(table) && ck::aligned16(emission), "%s: both tables are moved 16 bytes at a time", name);
  const int Cp = (C + 31) / 32 * 32;
  const int64_t quads = static_cast<int64_t>(F) * Cp * (K / 4), blocks = (quads + 255) / 256;
  CK_REQUIRE(blocks <= 0x7fffffff, "%s: F = %d, C = %d, K = %d: too many entries for one launch", name, F, C, K);
  return ck::launch(hmm_emission_table_kernel, dim3(static_cast<unsigned>(blocks)), dim3(256), 0, stream, table, K, C, Cp, quads, emission);
}

extern "C" int ck_hmm_predict(const void* const* w_steps, const int32_t* step_fold, const int32_t* step_var, int T, int K,
                              const float* rows, const int64_t* x, int D, int C, const int32_t* integrate, int B, float* log_probs,
                              const float* emission, float* cond, void* stream) {
  const char* name = "ck_hmm_predict";
  CK_REQUIRE(w_steps && step_fold && step_var && rows && x && log_probs, "%s: null operand", name);
  CK_REQUIRE(T >= 1 && B >= 1 && C >= 1 && D >= 1, "%s: T = %d, B = %d, C = %d, D = %d", name, T, B, C, D);
  CK_REQUIRE(K >= 32 && K <= 1024 && K % 32 == 0, "%s: K = %d is not a multiple of 32 in 32 .. 1024", name, K);
  CK_REQUIRE((emission == nullptr) == (cond == nullptr), "%s: the conditionals need the linear emission table, and only they", name);
  CK_REQUIRE(ck::aligned16(rows) && ck::aligned16(emission) && ck::aligned16(cond), "%s: tables and conditionals are moved 16 bytes at a time",
             name);
  const PredictArgs a{reinterpret_cast<const float* const*>(w_steps), step_fold, step_var, rows, emission, x, integrate, log_probs, cond,
                      C, (C + 31) / 32 * 32, D, T, B, K};
  const int NQ = K / 32, waves = NQ < kHmmWaves ? NQ : kHmmWaves;
  switch ((NQ + waves - 1) / waves) {
    case 1: return predict_launch<1>(a, stream);
    case 2: return predict_launch<2>(a, stream);
    case 3: return predict_launch<3>(a, stream);
    case 4: return predict_launch<4>(a, stream);
    case 5: return predict_launch<5>(a, stream);
    case 6: return predict_launch<6>(a, stream);
    case 7: return predict_launch<7>(a, stream);
    default: return predict_launch<8>(a, stream);
  }
}
