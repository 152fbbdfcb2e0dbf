// Soft (likelihood, Pearl's virtual) evidence for a hidden Markov model ("Soft evidence on chains").  The
// chain kernels stay what they are: they already take a (F, n, K) block of log emissions as their row source (x == NULL), and a
// soft emission is a contraction,
//     e_s[b, k] = log sum_c lambda[b, s, c] p_s(c | k) = m + log sum_c exp(log_lik[b, s, c] - m) E[f, c, k]
// with E the (F, Cp, K) linear table of ck_hmm_emission_table.  Two kernels on v_mfma_f32_32x32x2_f32 stand around them:
//
// hmm_soft_rows_kernel -- the block of emissions of n rows, a workgroup per (32-row tile, step).  No unit slice: the grid is
//   T x ceil(n / 32) workgroups of min(K / 32, 4) waves, 2048 at (T, K, C, B) = (64, 1024, 256, 1024), and a workgroup keeps
//   Cp x 128 bytes of LDS, so several share a CU.
//     soft step   the waves deal the 32 rows: a wave reads its row's C log-likelihoods twice (maximum m, clamped finite; then
//                 lam = 2^96 exp(l - m), ONCE per (row, step)) and leaves lam in LDS in the operand layout of the matrix pipe --
//                 float4 (g, lane = 32 kh + row) holds categories 8 g + 4 kh + 0 .. 3 of the row, what one ds_read_b128 hands to
//                 four MFMAs.  Behind a barrier every wave owns blocks of 32 units: the A operand of lane (unit o, kh) is
//                 E[f, 8 g + 4 kh + t, 32 q + o], a dword load whose 32 lanes of a half read one 128-byte segment of a table
//                 row; the table is used as it lies, categories along the contraction.  y comes out in the chain kernels' tile
//                 layout, e = m + log_unscaled(y) goes out 16 bytes at a time.
//     hard step   the row (fold, x) of the (F, C + 1, K) table of logarithms is copied; zeros where the entry is missing.
//   The 2^96 is the chain kernels' headroom (kHmmHead): the pipe and v_exp_f32 flush denormals, so with the largest lam at 1 a
//   category 88 nats below it would be lost; with it the terms kept reach 154 nats down, and a sum of C <= 2^10 terms <= 2^96
//   stays far from overflow.  All read entries -inf: m is clamped, every lam is 0, y = 0 and the row is -inf, never NaN.
//   One verdict word per (step, row): a NaN or +inf among the entries read, or a hard category >= C.  Every word is written by
//   the one workgroup that owns it -- no atomics, nothing to clear first.
// hmm_soft_flag_kernel -- a thread a row: NaN into out[b] where any step's verdict on the row is nonzero.  Runs between the
//   forward launch and whatever reads out (the max-product pass drops a NaN emission row: v_max3_f32).
// hmm_soft_leaf_kernel -- the posterior of every soft variable, p[b, j, c] = lam_c sum_k (gamma[b, k] / y[b, k]) E[f, c, k] =
//   d log Z / d log_lik[b, j, c], a workgroup per (32-row tile, soft variable).  The ratio is formed in the log2 domain,
//   lr_k = log2 gamma_k + (m - e_k) log2 e (it reaches e^80 and more where the evidence is unlikely under every state; gamma_k
//   = 0 or e_k = -inf: the term is 0, never 0 / 0), its row maximum M goes between the waves through LDS, and r_k = 2^96
//   2^(lr_k - M) is staged as the shared activation tile [K / 8][64] float4.  The waves own blocks of 32 categories: the A operand
//   of lane (category o, kh) is E[f, 32 cb + o, 8 g + 4 kh + 0 .. 3], ONE 16-byte load of the row as it lies -- the transposed
//   use of the table without a transposed copy.  The result is put together in the log2 domain as well,
//   p = 2^(log2 acc + (l_c - m) log2 e + M - 96): a weight that underflowed gives -inf and p = 0, never 0 x inf.
#include "ck_hmm.h"

namespace {

struct SoftArgs {
  const float* loglik;    // (n, S, Cl) log-likelihoods, entries at c >= C never read
  const int32_t* slot;    // rows: (T) soft slot of each step's variable or -1; leaf: (S) step of each soft slot or -1
  const int32_t* fold;    // (T) input fold of each step
  const int32_t* var;     // (T) its variable
  const float* rows;      // (F, C + 1, K) table of logarithms
  const float* emis;      // (F, Cp, K) linear table
  const int64_t* x;       // (n, ldx) hard categories, or nullptr: all missing
  const int32_t* integ;   // (D) != 0: the variable is summed out; or nullptr
  float* block;           // (F, n, K) log emissions
  float* m;               // (T, n) the maxima of the soft steps
  int32_t* flags;         // (T, n) verdicts
  const float* gamma;     // (n, D, K) state posteriors by variable (leaf)
  const float* logz;      // (n) (leaf)
  float* post;            // (n, S, Cp) (leaf)
  int C, Cp, Cl, S, ldx, D, T, n, K;
};

__global__ void __launch_bounds__(256) hmm_soft_rows_kernel(const SoftArgs a) {
  extern __shared__ __attribute__((aligned(16))) float smem[];  // lam [Cp / 8][64] float4 | m [32]
  const int K = a.K, NQ = K >> 5, n = a.n;
  const int nw = blockDim.x >> 6;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int t = blockIdx.y, tile = blockIdx.x;
  const int64_t f = a.fold[t];
  const int j = a.slot[t];
  float* const msh = smem + a.Cp * 32;

  if (j < 0) {  // a hard step: copy the table's row, zeros where the entry is missing
    const int v = a.var[t];
    const bool gone = a.x == nullptr || (a.integ != nullptr && a.integ[v] != 0);
    for (int r = wave; r < 32; r += nw) {
      const int b = tile * 32 + r;
      if (b >= n) break;
      const int64_t xv = gone ? -1 : a.x[static_cast<int64_t>(b) * a.ldx + v];
      const bool bad = xv >= a.C;
      const float* src = (xv >= 0 && !bad) ? a.rows + (f * (a.C + 1) + xv) * K : nullptr;
      float* dst = a.block + (f * n + b) * K;
      for (int k4 = lane; k4 < (K >> 2); k4 += 64)
        ck::gstore4(dst + 4 * k4, src != nullptr ? ck::gload4(src + 4 * k4) : make_float4(0.f, 0.f, 0.f, 0.f));
      if (lane == 0) a.flags[static_cast<int64_t>(t) * n + b] = bad ? 1 : 0;
    }
    return;
  }

  // ---- lam of the tile's 32 rows, once, in operand layout
  for (int r = wave; r < 32; r += nw) {
    const int b = tile * 32 + r;
    const int bl = b < n ? b : n - 1;  // (rows past n repeat the last one and store nothing)
    const float* ll = a.loglik + (static_cast<int64_t>(bl) * a.S + j) * a.Cl;
    float mx = -INFINITY;
    bool bad = false;
    for (int c = lane; c < a.C; c += 64) {
      const float l = *ck::as_global(ll + c);
      bad |= l != l || l == INFINITY;
      mx = fmaxf(mx, l);
    }
    mx = ck::clamp_finite(ck::wave_max(mx));
    const float off = exp_offset(mx, kHmmHead);
    for (int c = lane; c < a.Cp; c += 64) {
      const float lam = c < a.C ? __builtin_amdgcn_exp2f(fmaf(*ck::as_global(ll + c), kL2E, off)) : 0.f;
      smem[(((c >> 3) * 64 + ((c >> 2) & 1) * 32 + r) << 2) + (c & 3)] = lam;
    }
    const bool any = __any(bad);
    if (lane == 0) {
      msh[r] = mx;
      if (b < n) {
        a.m[static_cast<int64_t>(t) * n + b] = mx;
        a.flags[static_cast<int64_t>(t) * n + b] = any ? 1 : 0;
      }
    }
  }
  __syncthreads();

  // ---- y = lam E on the wave's blocks of 32 units, e = m + log y
  const int row = lane & 31, kh = lane >> 5;
  const int b = tile * 32 + row;
  const float mb = msh[row];
  const float4* lam4 = reinterpret_cast<const float4*>(smem);
  const float* E = a.emis + f * a.Cp * K;
  const int G = a.Cp >> 3;
  for (int q = wave; q < NQ; q += nw) {
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    const float* src = E + static_cast<int64_t>(4 * kh) * K + 32 * q + row;
    float w[4], wn[4];  // the next group's four segments travel while this one's MFMAs run (the last one is read twice)
#pragma unroll
    for (int c = 0; c < 4; ++c) w[c] = *ck::as_global(src + static_cast<int64_t>(c) * K);
    for (int g = 0; g < G; ++g) {
      const float* s8 = src + static_cast<int64_t>(8 * (g + 1 < G ? g + 1 : g)) * K;
#pragma unroll
      for (int c = 0; c < 4; ++c) wn[c] = *ck::as_global(s8 + static_cast<int64_t>(c) * K);
      const float4 p = lam4[g * 64 + lane];
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(w[0], p.x, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(w[1], p.y, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(w[2], p.z, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(w[3], p.w, acc, 0, 0, 0);
#pragma unroll
      for (int c = 0; c < 4; ++c) w[c] = wn[c];
    }
    if (b < n) {
      float e[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) e[r] = mb + log_unscaled(acc[r]);
      keep_store(a.block + (f * n + b) * K + 32 * q + 4 * kh, e);
    }
  }
}

__global__ void __launch_bounds__(256) hmm_soft_flag_kernel(const int32_t* flags, int T, int n, float* out) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= n) return;
  int any = 0;
  for (int t = 0; t < T; ++t) any |= flags[static_cast<int64_t>(t) * n + b];
  if (any != 0) out[b] = __builtin_nanf("");
}

// log2 of gamma / y per state of a lane's 16 values of one block of units; -inf where the term is 0
__device__ __forceinline__ void soft_ratio(const float* gsrc, const float* esrc, float mrow, float (&lr)[16]) {
  float e[16];
  keep_load(gsrc, lr);
  keep_load(esrc, e);
#pragma unroll
  for (int i = 0; i < 16; ++i)
    lr[i] = (lr[i] > 0.f && e[i] > -INFINITY) ? fmaf(mrow - e[i], kL2E, __builtin_amdgcn_logf(lr[i])) : -INFINITY;
}

__global__ void __launch_bounds__(256) hmm_soft_leaf_kernel(const SoftArgs a) {
  extern __shared__ __attribute__((aligned(16))) float smem[];  // r [K / 8][64] float4 | row maxima [4][32]
  const int K = a.K, NQ = K >> 5, n = a.n, NCB = a.Cp >> 5;
  const int nw = blockDim.x >> 6;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int row = lane & 31, kh = lane >> 5;
  const int j = blockIdx.y, b = blockIdx.x * 32 + row;
  const bool live = b < n;
  const int bl = live ? b : n - 1;
  float* const outp = a.post + (static_cast<int64_t>(bl) * a.S + j) * a.Cp + 4 * kh;
  const int t = a.slot[j];
  if (t < 0) {  // a soft variable that no step reads: the evidence does not depend on it
    const float zero[16] = {};
    for (int cb = wave; cb < NCB; cb += nw)
      if (live) keep_store(outp + 32 * cb, zero);
    return;
  }
  const int64_t f = a.fold[t];
  const float* gsrc = a.gamma + (static_cast<int64_t>(bl) * a.D + a.var[t]) * K + 4 * kh;
  const float* esrc = a.block + (f * n + bl) * K + 4 * kh;
  const float mrow = a.m[static_cast<int64_t>(t) * n + bl];
  float* const red = smem + NQ * 1024;

  // ---- the row maximum of log2(gamma / y), then r = 2^96 2^(lr - M) as the shared activation tile
  float mx = -INFINITY;
  for (int q = wave; q < NQ; q += nw) {
    float lr[16];
    soft_ratio(gsrc + 32 * q, esrc + 32 * q, mrow, lr);
#pragma unroll
    for (int i = 0; i < 16; ++i) mx = fmaxf(mx, lr[i]);
  }
  mx = ck::xhalf_max(mx);
  if (kh == 0) red[wave * 32 + row] = mx;
  __syncthreads();
  for (int k = 0; k < nw; ++k) mx = fmaxf(mx, red[k * 32 + row]);
  mx = ck::clamp_finite(mx);
  const float off = fabsf(mx) > 1e38f ? kHmmHead : kHmmHead - mx;
  float4* const act4 = reinterpret_cast<float4*>(smem);
  for (int q = wave; q < NQ; q += nw) {
    float lr[16];
    soft_ratio(gsrc + 32 * q, esrc + 32 * q, mrow, lr);
#pragma unroll
    for (int g = 0; g < 4; ++g)
      act4[(q * 4 + g) * 64 + lane] = make_float4(__builtin_amdgcn_exp2f(lr[4 * g] + off), __builtin_amdgcn_exp2f(lr[4 * g + 1] + off),
                                                  __builtin_amdgcn_exp2f(lr[4 * g + 2] + off), __builtin_amdgcn_exp2f(lr[4 * g + 3] + off));
  }
  __syncthreads();

  // ---- p = lam (E r) on the wave's blocks of 32 categories
  const float z = a.logz[bl];
  const bool dead = !(fabsf(z) < INFINITY);  // (a flag, or no mass)
  const float* ll = a.loglik + (static_cast<int64_t>(bl) * a.S + j) * a.Cl;
  const float* E = a.emis + f * a.Cp * K;
  const float back = (fabsf(mx) > 1e38f ? 0.f : mx) - kHmmHead;
  const int G = K >> 3;
  for (int cb = wave; cb < NCB; cb += nw) {
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    const float* src = E + static_cast<int64_t>(32 * cb + row) * K + 4 * kh;
    float4 wn = ck::gload4(src);  // the next group's 16 bytes travel while this one's MFMAs run (the last one is read twice)
    for (int g = 0; g < G; ++g) {
      const float4 w = wn;
      wn = ck::gload4(src + 8 * (g + 1 < G ? g + 1 : g));
      const float4 p = act4[g * 64 + lane];
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(w.x, p.x, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(w.y, p.y, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(w.z, p.z, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(w.w, p.w, acc, 0, 0, 0);
    }
    if (live) {
      float y[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int c = 32 * cb + 8 * (r >> 2) + 4 * kh + (r & 3);
        float p = 0.f;
        if (c < a.C) {
          const float lg = __builtin_amdgcn_logf(__builtin_amdgcn_frexp_mantf(acc[r])) +
                           (static_cast<float>(__builtin_amdgcn_frexp_expf(acc[r])) + back);
          p = __builtin_amdgcn_exp2f(fmaf(*ck::as_global(ll + c) - mrow, kL2E, lg));
        }
        y[r] = dead ? __builtin_nanf("") : p;
      }
      keep_store(outp + 32 * cb, y);
    }
  }
}

int soft_launch(void (*kernel)(const SoftArgs), dim3 grid, int waves, size_t lds, const SoftArgs& a, void* stream) {
  const dim3 block(64 * waves);
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

extern "C" int ck_hmm_soft_rows(const float* log_lik, int S, int Cl, const int32_t* step_slot, const int32_t* step_fold,
                                const int32_t* step_var, int T, int K, const float* rows, const float* emission, const int64_t* x,
                                int ldx, int C, const int32_t* integrate, int n, float* block, float* m, int32_t* flags, void* stream) {
  const char* name = "ck_hmm_soft_rows";
  CK_REQUIRE(log_lik && step_slot && step_fold && step_var && rows && emission && block && m && flags, "%s: null operand", name);
  CK_REQUIRE(T >= 1 && T <= 65535 && n >= 1 && S >= 1, "%s: T = %d, n = %d, S = %d", name, T, n, S);
  CK_REQUIRE(C >= 1 && C <= 1024 && Cl >= C, "%s: C = %d (1 .. 1024), log_lik has %d states", name, C, Cl);
  CK_REQUIRE(K >= 32 && K <= 1024 && K % 32 == 0, "%s: K = %d is not a multiple of 32 in 32 .. 1024", name, K);
  CK_REQUIRE(x == nullptr || ldx >= 1, "%s: ldx = %d", name, ldx);
  CK_REQUIRE(x != nullptr || integrate == nullptr, "%s: without x every hard variable is missing already", name);
  CK_REQUIRE(ck::aligned16(rows) && ck::aligned16(block), "%s: table and block are moved 16 bytes at a time", name);
  const int Cp = (C + 31) / 32 * 32, NQ = K / 32;
  const SoftArgs a{log_lik, step_slot, step_fold, step_var, rows, emission, x, integrate, block, m, flags, nullptr, nullptr, nullptr,
                   C, Cp, Cl, S, ldx, 0, T, n, K};
  const size_t lds = (static_cast<size_t>(Cp) * 32 + 32) * sizeof(float);
  return soft_launch(hmm_soft_rows_kernel, dim3((n + 31) / 32, T), NQ < kHmmWaves ? NQ : kHmmWaves, lds, a, stream);
}

extern "C" int ck_hmm_soft_flag(const int32_t* flags, int T, int n, float* out, void* stream) {
  const char* name = "ck_hmm_soft_flag";
  CK_REQUIRE(flags && out, "%s: null operand", name);
  CK_REQUIRE(T >= 1 && n >= 1, "%s: T = %d, n = %d", name, T, n);
  return ck::launch(hmm_soft_flag_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, flags, T, n, out);
}

extern "C" int ck_hmm_soft_leaf(const float* log_lik, int S, int Cl, const int32_t* soft_step, const int32_t* step_fold,
                                const int32_t* step_var, int T, int K, const float* emission, int C, const float* block, const float* m,
                                const float* gamma, int D, int n, const float* log_z, float* post, void* stream) {
  const char* name = "ck_hmm_soft_leaf";
  CK_REQUIRE(log_lik && soft_step && step_fold && step_var && emission && block && m && gamma && log_z && post, "%s: null operand", name);
  CK_REQUIRE(T >= 1 && n >= 1 && S >= 1 && S <= 65535 && D >= 1, "%s: T = %d, n = %d, S = %d, D = %d", name, T, n, S, D);
  CK_REQUIRE(C >= 1 && C <= 1024 && Cl >= C, "%s: C = %d (1 .. 1024), log_lik has %d states", name, C, Cl);
  CK_REQUIRE(K >= 32 && K <= 1024 && K % 32 == 0, "%s: K = %d is not a multiple of 32 in 32 .. 1024", name, K);
  CK_REQUIRE(ck::aligned16(emission) && ck::aligned16(block) && ck::aligned16(gamma) && ck::aligned16(post),
             "%s: table, block, posteriors and result are moved 16 bytes at a time", name);
  const int Cp = (C + 31) / 32 * 32, NQ = K / 32, NB = NQ > Cp / 32 ? NQ : Cp / 32;
  const SoftArgs a{log_lik, soft_step, step_fold, step_var, nullptr, emission, nullptr, nullptr, const_cast<float*>(block),
                   const_cast<float*>(m), nullptr, gamma, log_z, post, C, Cp, Cl, S, 0, D, T, n, K};
  const size_t lds = (static_cast<size_t>(NQ) * 1024 + kHmmWaves * 32) * sizeof(float);
  return soft_launch(hmm_soft_leaf_kernel, dim3((n + 31) / 32, S), NB < kHmmWaves ? NB : kHmmWaves, lds, a, stream);
}
