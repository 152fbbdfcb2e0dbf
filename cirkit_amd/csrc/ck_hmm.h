// What the chain kernels share (ck_hmm.hip: forward and backward on the matrix pipe; ck_hmm_viterbi.hip: max-product on the
// vector ALU): the argument block, the headroom of the linear-space activations, the hand-off buffer's lane mapping and the
// launch with the shared LDS layout  activation tile | reductions | per-wave weight rings.
#pragma once

#include "ck_internal.h"
#include "ck_tile.h"

namespace {

constexpr int kHmmWaves = 4;
constexpr int kHmmUnit = 512;  // floats of a weight unit (32 outputs x 16 inputs)
// p = 2^kHmmHead exp(t - M): the matrix pipe and v_exp_f32 flush denormals, so with the row maximum at 1 a state 88 nats below
// it is lost -- and it is the one that counts where the maximum meets a weight that small (peaked parameters: emissions 80
// nats apart).  The exponent range above 1 is free: softmax rows sum to 1, so y <= 2^96 and the states kept reach 154 nats down.
// (The backward pass contracts with W^T, whose rows -- the columns of W -- do not sum to 1: there y <= K 2^96 <= 2^106, still safe.)
constexpr float kHmmHead = 96.f;
// log(y 2^-kHmmHead) from the mantissa and the exponent of y: v_log_f32 of y itself rounds a result near 96 to 2^-17, 5e-6 nats a
// step where every state is as likely as the next (a row of missing entries), whatever is subtracted afterwards
__device__ __forceinline__ float log_unscaled(float y) {
  const float k = static_cast<float>(__builtin_amdgcn_frexp_expf(y)) - kHmmHead;
  return (__builtin_amdgcn_logf(__builtin_amdgcn_frexp_mantf(y)) + k) * kLN2;
}

struct HmmArgs {
  const float* const* w;  // (T) the steps' evaluated weights, row-major (Ko, K)
  const int32_t* fold;    // (T) input fold of each step
  const int32_t* var;     // (T) its variable
  const float* rows;      // emission rows, K floats each
  const int64_t* x;       // (B, D) categories: row (fold, x) of a (F, C + 1, K) table; nullptr: row (fold, b) of a (F, B, K) block
  const int32_t* integ;   // (D) != 0: the variable is summed out; or nullptr
  float* out;             // (B)
  int C, D, T, B, K;
  float* keep;            // (B, D, K) or nullptr: the hand-off of every step (KEEP forward), turned into posteriors in place (backward)
  float* pair_a;          // (B, D, K) or nullptr: the statistics backward leaves the pair sum's operand rows a'_s and r'_s here
  float* pair_r;          //   (ck_hmm_stats.hip), by variable like `keep`
};

__device__ __forceinline__ void lds_w4(uint32_t addr, float a, float b, float c, float d) {
  const f32x4v v = {a, b, c, d};
  asm volatile("ds_write_b128 %0, %1" ::"v"(addr), "v"(v) : "memory");
}
// a lane's 16 values of one block of units to and from a row of the (B, D, K) hand-off buffer: four 16-byte groups
__device__ __forceinline__ void keep_store(float* dst, const float (&v)[16]) {
#pragma unroll
  for (int g = 0; g < 4; ++g) ck::gstore4(dst + 8 * g, make_float4(v[4 * g], v[4 * g + 1], v[4 * g + 2], v[4 * g + 3]));
}
__device__ __forceinline__ void keep_load(const float* src, float (&v)[16]) {
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    const float4 t4 = ck::gload4(src + 8 * g);
    v[4 * g] = t4.x, v[4 * g + 1] = t4.y, v[4 * g + 2] = t4.z, v[4 * g + 3] = t4.w;
  }
}
__device__ __forceinline__ void sync_lds() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

template <class Kernel>
int hmm_launch(Kernel kernel, int nbuf, int red_floats, const HmmArgs& a, void* stream) {
  const int NQ = a.K / 32, waves = NQ < kHmmWaves ? NQ : kHmmWaves;
  const size_t lds = (static_cast<size_t>(NQ) * 1024 + red_floats + static_cast<size_t>(waves) * nbuf * kHmmUnit) * sizeof(float);
  const dim3 grid((a.B + 31) / 32), block(64 * waves);
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
