// EM training ("EM training"): the M-step of a whole circuit as ONE launch over a job table, behind
// `HipEMTrainer` (cirkit_amd/em.py).  A job names a raw parameter tensor of the store, the batch-summed statistics behind it
// (ck_stats.hip's accumulators, in the device plan's shapes) and how the parameter graph maps one to the other; the kernel
// inverts that graph in closed form and updates the raw tensor IN PLACE, row by row:
//
//   CK_EM_ROW_SOFTMAX  tensor -> softmax            n_i = N_i + pseudocount [support_i],  theta_hat = n / sum n,
//   CK_EM_ROW_LINEAR   tensor                        theta_old = the row as the graph normalises it (softmax of logits, the
//   CK_EM_MIXING       tensor [-> softmax] -> mixing  linear row over its sum),  theta = (1 - step) theta_old + step theta_hat;
//                                                    written as log theta (raw_log) or theta.  Mixing: row (f, k) of the (K, H)
//                                                    tensor gathers the entries h K + k of the (K, H K) statistics row.
//   CK_EM_GAUSSIAN     mean: tensor, stddev: tensor -> scaled_sigmoid(lo, hi); mean and VARIANCE blended by step
//   CK_EM_BINOMIAL     probs: tensor -> sigmoid;      p_hat = sum_c c N_c / (T sum_c N_c), blended by step
//
// A row whose denominator is 0 (no flow: a dead fold, a padded unit) returns before it writes anything.  Padded entries carry
// N = 0 and theta_old = 0, so they stay -inf (log) or 0 (linear) by the arithmetic itself.  The scaled-sigmoid and sigmoid
// pre-images take s clamped into [2^-24, 1 - 2^-24]: log s - log1p(-s) is finite for a collapsed variance and for p in {0, 1}.
//
// Work split (what tests/test_em_training.py aims at):
//   row length <= kWaveRow (256): one WAVE per row, four rows per 256-thread workgroup; lane l owns entries l, l + 64, ...
//   row length >  kWaveRow:       one WORKGROUP per row; thread t owns entries t, t + 256, ... (any length: the row is
//                                 re-read from L2, three passes, nothing is staged, so there is no single-pass limit)
//   CK_EM_GAUSSIAN:               one thread per unit.
// Sums: every lane adds its own entries in ascending order, the 64 lanes combine in ck::wave_sum's fixed butterfly, the four
// waves of a workgroup in wave order through LDS.  No float atomics: results are bit for bit the same from call to call.
#include <math.h>

#include "ck_internal.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / ck::kWave;
constexpr int kWaveRow = 256;
constexpr float kClampLo = 5.9604644775390625e-08f;  // 2^-24
constexpr float kClampHi = 1.f - 5.9604644775390625e-08f;

// sum / max over a row's group: the wave, or the workgroup's four waves in wave order (red: kWaves floats of LDS)
template <bool BLOCK, bool MAX>
__device__ __forceinline__ float group_reduce(float v, float* red) {
  v = ck::wave_reduce<MAX>(v);
  if constexpr (BLOCK) {
    __syncthreads();  // (the previous reduction's readers are done with red)
    if ((threadIdx.x & (ck::kWave - 1)) == 0) red[threadIdx.x / ck::kWave] = v;
    __syncthreads();
    v = red[0];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) v = MAX ? fmaxf(v, red[w]) : v + red[w];
  }
  return v;
}

__device__ __forceinline__ float logit_clamped(float s) {
  s = fminf(fmaxf(s, kClampLo), kClampHi);
  return logf(s) - log1pf(-s);
}
__device__ __forceinline__ float sigmoidf(float x) { return 1.f / (1.f + expf(-x)); }

// One row of a ROW_SOFTMAX / ROW_LINEAR / MIXING job; `t` the thread's index in the row's group of `nt` threads.
template <bool BLOCK>
__device__ __forceinline__ void em_row(const ck_em_job& j, int64_t row, int t, int nt, float step, float pseudo, float* red) {
  const int len = j.len;
  const bool mixing = j.kind == CK_EM_MIXING;
  // statistics / support entry i of the row: base + i * stride
  const int64_t base = mixing ? row * len * j.k + row % j.k : row * len;
  const int64_t stride = mixing ? j.k : 1;
  const float* __restrict__ N = j.stats + base;
  const float* S = j.support ? j.support + base : nullptr;  // (may BE the raw tensor: a bare weight is its own support)
  float* raw = j.raw + row * len;
  const bool lg = j.raw_log != 0;
  float nsum = 0.f, agg = lg ? -INFINITY : 0.f;  // agg: the row maximum of the logs, or the sum of the linear row
  for (int i = t; i < len; i += nt) {
    const float r = raw[i];
    const bool sup = S ? S[i * stride] > 0.f : (lg ? r > -INFINITY : r > 0.f);
    nsum += N[i * stride] + (sup ? pseudo : 0.f);
    agg = lg ? fmaxf(agg, r) : agg + fmaxf(r, 0.f);
  }
  nsum = group_reduce<BLOCK, false>(nsum, red);
  if (!(nsum > 0.f)) return;  // no mass: the row keeps its raw values (uniform over the group)
  if (lg) {
    const float mx = group_reduce<BLOCK, true>(agg, red);
    float e = 0.f;
    for (int i = t; i < len; i += nt) e += mx > -INFINITY ? expf(raw[i] - mx) : 0.f;
    const float esum = group_reduce<BLOCK, false>(e, red);
    for (int i = t; i < len; i += nt) {
      const float r = raw[i];
      const bool sup = S ? S[i * stride] > 0.f : r > -INFINITY;
      const float old = esum > 0.f ? expf(r - mx) / esum : 0.f;
      const float hat = (N[i * stride] + (sup ? pseudo : 0.f)) / nsum;
      raw[i] = logf((1.f - step) * old + step * hat);
    }
  } else {
    const float usum = group_reduce<BLOCK, false>(agg, red);
    for (int i = t; i < len; i += nt) {
      const float r = raw[i];
      const bool sup = S ? S[i * stride] > 0.f : r > 0.f;
      const float old = usum > 0.f ? fmaxf(r, 0.f) / usum : 0.f;
      const float hat = (N[i * stride] + (sup ? pseudo : 0.f)) / nsum;
      raw[i] = (1.f - step) * old + step * hat;
    }
  }
}

// One unit of a BINOMIAL job: the statistics row (T + 1 states) gives the success probability.
template <bool BLOCK>
__device__ __forceinline__ void em_binomial(const ck_em_job& j, int64_t row, int t, int nt, float step, float* red) {
  const float* __restrict__ N = j.stats + row * j.len;
  float tot = 0.f, num = 0.f;
  for (int c = t; c < j.len; c += nt) {
    tot += N[c];
    num += static_cast<float>(c) * N[c];
  }
  tot = group_reduce<BLOCK, false>(tot, red);
  num = group_reduce<BLOCK, false>(num, red);
  if (!(tot > 0.f) || t != 0) return;
  const float hat = num / (static_cast<float>(j.len - 1) * tot);
  j.raw[row] = logit_clamped((1.f - step) * sigmoidf(j.raw[row]) + step * hat);
}

// One unit of a GAUSSIAN job.  The moments are taken in fp64: s2 / s0 - mu_hat^2 cancels, and in fp32 its rounding alone would
// cost a narrow unit several digits of its variance (one thread per unit: the cost is nothing).
__device__ __forceinline__ void em_gaussian(const ck_em_job& j, int64_t u, float step) {
  const double s0 = j.stats[3 * u], s1 = j.stats[3 * u + 1], s2 = j.stats[3 * u + 2];
  if (!(s0 > 0.0)) return;
  const double a = step;
  const double mu_hat = s1 / s0;
  const double var_hat = fmax(s2 / s0 - mu_hat * mu_hat, 0.0);
  const double sd_old = j.lo + (j.hi - j.lo) * sigmoidf(j.raw2[u]);
  const double var = (1.0 - a) * sd_old * sd_old + a * var_hat;
  j.raw[u] = static_cast<float>((1.0 - a) * j.raw[u] + a * mu_hat);
  j.raw2[u] = logit_clamped(static_cast<float>((sqrt(var) - j.lo) / (j.hi - j.lo)));
}

__global__ void __launch_bounds__(kThreads) em_update_kernel(const ck_em_job* __restrict__ jobs, int njobs, float step, float pseudo) {
  __shared__ float red[kWaves];
  const int bid = blockIdx.x;
  int lo = 0, hi = njobs - 1;  // the last job whose block_begin <= bid
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (jobs[mid].block_begin <= bid) lo = mid; else hi = mid - 1;
  }
  const ck_em_job j = jobs[lo];
  const int64_t blk = bid - j.block_begin;
  const int tid = threadIdx.x;
  if (j.kind == CK_EM_GAUSSIAN) {
    const int64_t u = blk * kThreads + tid;
    if (u < j.rows) em_gaussian(j, u, step);
    return;
  }
  if (j.len <= kWaveRow) {
    const int64_t row = blk * kWaves + tid / ck::kWave;
    if (row >= j.rows) return;  // (whole waves leave; the wave form never meets a barrier)
    if (j.kind == CK_EM_BINOMIAL)
      em_binomial<false>(j, row, tid & (ck::kWave - 1), ck::kWave, step, red);
    else
      em_row<false>(j, row, tid & (ck::kWave - 1), ck::kWave, step, pseudo, red);
  } else if (j.kind == CK_EM_BINOMIAL) {
    em_binomial<true>(j, blk, tid, kThreads, step, red);
  } else {
    em_row<true>(j, blk, tid, kThreads, step, pseudo, red);
  }
}

int64_t job_blocks(int kind, int64_t rows, int len) {
  if (kind == CK_EM_GAUSSIAN) return (rows + kThreads - 1) / kThreads;
  return len <= kWaveRow ? (rows + kWaves - 1) / kWaves : rows;
}

}  // namespace

extern "C" {

int ck_em_job_blocks(int kind, int64_t rows, int len) {
  CK_REQUIRE(kind >= CK_EM_ROW_SOFTMAX && kind <= CK_EM_BINOMIAL && rows > 0 && len > 0 && job_blocks(kind, rows, len) <= 0x7fffffff,
             "ck_em_job_blocks: kind %d, %lld rows of %d", kind, static_cast<long long>(rows), len);
  return static_cast<int>(job_blocks(kind, rows, len));
}

int ck_em_update(const ck_em_job* jobs, const ck_em_job* device_jobs, int njobs, float step_size, float pseudocount, void* stream) {
  CK_REQUIRE(jobs != nullptr && device_jobs != nullptr && njobs > 0, "ck_em_update: no jobs");
  CK_REQUIRE(step_size > 0.f && step_size <= 1.f, "ck_em_update: step_size %g outside (0, 1]", static_cast<double>(step_size));
  CK_REQUIRE(pseudocount >= 0.f && pseudocount < INFINITY, "ck_em_update: pseudocount %g", static_cast<double>(pseudocount));
  int64_t blocks = 0;
  for (int i = 0; i < njobs; ++i) {
    const ck_em_job& j = jobs[i];
    CK_REQUIRE(j.kind >= CK_EM_ROW_SOFTMAX && j.kind <= CK_EM_BINOMIAL, "ck_em_update: job %d has unknown kind %d", i, j.kind);
    CK_REQUIRE(j.raw != nullptr && j.stats != nullptr, "ck_em_update: job %d: null pointer", i);
    CK_REQUIRE(j.rows > 0 && j.len > 0, "ck_em_update: job %d: %lld rows of %d", i, static_cast<long long>(j.rows), j.len);
    CK_REQUIRE(j.kind != CK_EM_ROW_SOFTMAX || j.raw_log != 0, "ck_em_update: job %d: a softmax row holds logits", i);
    CK_REQUIRE(j.kind != CK_EM_MIXING || (j.k > 0 && j.rows % j.k == 0),
               "ck_em_update: job %d: a mixing job of %lld rows needs its unit count (%d)", i, static_cast<long long>(j.rows), j.k);
    CK_REQUIRE(j.kind != CK_EM_GAUSSIAN || (j.len == 3 && j.raw2 != nullptr && j.hi > j.lo && j.lo >= 0.f),
               "ck_em_update: job %d: a Gaussian job needs 3 sums, the stddev tensor and 0 <= lo < hi", i);
    CK_REQUIRE(j.kind != CK_EM_BINOMIAL || j.len >= 2, "ck_em_update: job %d: a Binomial job needs total_count >= 1", i);
    CK_REQUIRE(j.block_begin == blocks, "ck_em_update: job %d begins at block %d, expected %lld (ck_em_job_blocks)", i,
               j.block_begin, static_cast<long long>(blocks));
    blocks += job_blocks(j.kind, j.rows, j.len);
    CK_REQUIRE(blocks <= 0x7fffffff, "ck_em_update: grid too large");
  }
  return ck::launch(em_update_kernel, dim3(static_cast<unsigned>(blocks)), dim3(kThreads), 0, stream, device_jobs, njobs,
                    step_size, pseudocount);
}

}  // extern "C"
