// The forward algorithm of a hidden Markov model, parallel in TIME, in two launches ("Time-parallel forward").
//
// ck_hmm.hip walks a chain with one workgroup per 32 rows: its time does not fall with B, one row costs what 4096 cost.  The chain
// is associative: steps [s_p, s_{p+1}) of row b are a K x K transfer matrix G_p (in the log domain: a matrix of log-sum-exps), and
// the matrices of disjoint runs of steps can be evaluated at the same time.  With the steps cut at s_p = floor(p T / P):
//
// Launch 1, hmm_scan_segments_kernel: every segment at once, two kinds of workgroup, both the forward's step (phase A: t = log y +
// e, row maximum across the waves, p = 2^96 exp(t - M) into the shared tile; phase B: y = W p on v_mfma_f32_32x32x2_f32 with the
// wave's private weight ring and its vmcnt discipline; the running scale per row) on the forward's unit blocks per wave:
//   * segment 0 -- 32 REAL rows a workgroup, v_{-1} = 0, steps [0, s_1): the forward as it is, ending in the hand-off
//     first[b, :] = log y + scale instead of a scalar;
//   * segment p >= 1 -- one workgroup per (row b, segment p, tile of 32 start states): its 32 rows are VIRTUAL, 32 copies of row b,
//     copy j started from the one-hot vector of state j (0 at unit j, -inf elsewhere), so that virtual row j ends as column
//     log G_p[:, j].  The emission row and x of a step are the same for the whole workgroup: x is read through a uniform index
//     (a scalar load), the row with the tile layout from one address per half-wave, nothing is gathered per lane.  A start state
//     whose emission is -inf is an all -inf row: the clamped maximum makes it a column of -inf, as for a row without mass.
//     A middle segment stores lg[b, p - 1, j, :] = log y + scale, K contiguous floats per start state straight from registers;
//     the last one ends each virtual row in the closing dot product with row 0 of W_{T-1} and stores one scalar last[b, j].
//   Start states >= num_states (padded units) are never stored and never read: the grid covers ceil(num_states / 32) tiles.
//   A category >= C sets the flag word of its (row, segment); every flag word is written by every call.
//
// Launch 2, hmm_scan_combine_kernel: one workgroup a row chains the P - 1 boundaries in order,
//     v <- first[b, :];   v'[o] = log sum_{j < num_states} exp(lg[b, p - 1, j, o] + v[j])  (p = 1 .. P - 2);
//     out[b] = log sum_j exp(last[b, j] + v[j])
// A matrix is specific to its row, so nothing is shared between rows and this runs on the vector ALU.  It stays in the log domain
// (maximum first, clamped finite, then the sum of exp2 with the 2^96 head: LSESumSemiring.apply_reduce, like the forward): a
// linear-space G rescaled per column would drop an entry 88 nats below its column maximum, which under peaked parameters can be
// the only route to a state.  v lives in LDS (two copies, alternating); 256 threads = (part of the start states) x (output o), so
// that a wave reads 64 consecutive floats of row j and a small K still uses the workgroup; the parts meet in LDS in a fixed order.
// The addresses of the next matrix do not depend on v: a thread requests its first kScanAhead rows of matrix p + 1 into registers
// before it reduces matrix p, so the chain is P reductions and not P round trips to memory behind each other.
#include "ck_hmm.h"

namespace {

struct HmmScanArgs {
  const float* const* w;  // as HmmArgs
  const int32_t* fold;
  const int32_t* var;
  const float* rows;     // (F, C + 1, K) table of logarithms
  const int64_t* x;      // (B, D)
  const int32_t* integ;  // (D) or nullptr
  int C, D, T, B, K;
  int P, num_states, tiles;  // tiles = ceil(num_states / 32)
  float* first;              // (B, K) segment 0's hand-off
  float* lg;                 // (B, P - 2, 32 tiles, K) log transfer matrices of the middle segments, [start state][end state]
  float* last;               // (B, K) the last segment's scalars, by start state
  int32_t* flags;            // (B, P) != 0: the segment met a category >= C
  float* out;                // (B)
};

template <int NOB>
__global__ void __launch_bounds__(256) hmm_scan_segments_kernel(const HmmScanArgs a) {
  constexpr int NBUF = 8;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int K = a.K, NQ = K >> 5, T = a.T, P = a.P;
  const int nwaves = blockDim.x >> 6;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int kh = lane >> 5, row = lane & 31;
  // which workgroup this is: the first ceil(B / 32) own real rows (segment 0), the others (row, segment >= 1, tile of start states)
  const int nreal = (a.B + 31) >> 5;
  const bool virt = static_cast<int>(blockIdx.x) >= nreal;
  int seg = 0, tile = 0, bu = 0;
  if (virt) {
    int id = blockIdx.x - nreal;
    tile = id % a.tiles, id /= a.tiles;
    seg = 1 + id % (P - 1), bu = id / (P - 1);
  }
  const int s0 = static_cast<int>(static_cast<int64_t>(seg) * T / P), s1 = static_cast<int>(static_cast<int64_t>(seg + 1) * T / P);
  const int b = virt ? bu : static_cast<int>(blockIdx.x) * 32 + row;
  const int jv = tile * 32 + row;  // (virtual rows: the start state)
  const bool live = virt ? jv < a.num_states : b < a.B;
  const int bl = b < a.B ? b : a.B - 1;  // (real rows past B repeat the last one and store nothing)
  int nob = 0;
#pragma unroll
  for (int j = 0; j < NOB; ++j) nob += wave + nwaves * j < NQ ? 1 : 0;

  // LDS as in the forward: activation tile [NQ][4][64] float4 | row maxima [4][32] | weight rings [waves][NBUF][2][64] float4
  const uint32_t act = static_cast<uint32_t>(reinterpret_cast<uintptr_t>(smem));
  const uint32_t red = act + NQ * 4096;
  float* const ring_p = smem + NQ * 1024 + kHmmWaves * 32 + wave * (NBUF * kHmmUnit);
  const uint32_t ring = red + kHmmWaves * 128 + wave * (NBUF * kHmmUnit * 4) + lane * 16;

  bool bad = false;
  auto load_x = [&](int s) -> int64_t {
    if (s >= s1) return 0;
    const int64_t v = a.var[s];
    return virt ? a.x[static_cast<int64_t>(bu) * a.D + v] : a.x[static_cast<int64_t>(bl) * a.D + v];
  };
  auto row_of = [&](int s, int64_t xv) -> const float* {  // nullptr: the entry is missing
    if (xv < 0 || (a.integ != nullptr && a.integ[a.var[s]] != 0)) return nullptr;
    if (xv >= a.C) {
      bad = true;
      return nullptr;
    }
    return a.rows + (static_cast<int64_t>(a.fold[s]) * (a.C + 1) + xv) * K;
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
  auto issue = [&](const float* w, int u) {
    const int j = u / (2 * NQ), r = u - j * 2 * NQ;
    const int ob = wave + nwaves * j;
    const float* src = w + static_cast<int64_t>(32 * ob + row) * K + 16 * r + 4 * kh;
    float* dst = ring_p + (u % NBUF) * kHmmUnit;
    __builtin_amdgcn_global_load_lds((ck::gptr_t)src, (ck::lptr_t)dst, 16, 0, 0);
    __builtin_amdgcn_global_load_lds((ck::gptr_t)(src + 8), (ck::lptr_t)(dst + 256), 16, 0, 0);
  };

  // v before the first step: zeros (segment 0), or the one-hot vector of the virtual row's start state
#pragma unroll
  for (int j = 0; j < NOB; ++j)
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int unit = 32 * (wave + nwaves * j) + 8 * (i >> 2) + 4 * kh + (i & 3);
      la[j][i] = virt && unit != jv ? -INFINITY : 0.f;
    }
  float scale = 0.f;
  load_e(row_of(s0, load_x(s0)));
  int64_t xn = load_x(s0 + 1);

  for (int s = s0; s < s1; ++s) {
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

    // the emission row of the segment's next step travels while this step contracts
    if (s + 1 < s1) {
      load_e(row_of(s + 1, xn));
      xn = load_x(s + 2);
    }

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

  // the verdict on the categories of this (row, segment): the tiles of a virtual row all reach the same one, tile 0 writes it
  if (virt) {
    if (tile == 0 && threadIdx.x == 0) a.flags[static_cast<int64_t>(bu) * P + seg] = bad ? 1 : 0;
  } else if (live && wave == 0 && kh == 0) {
    a.flags[static_cast<int64_t>(b) * P] = bad ? 1 : 0;
  }

  if (seg + 1 < P) {  // log y + scale of the segment's last step: K contiguous floats per (virtual) row
    if (live) {
      float* dst = (virt ? a.lg + ((static_cast<int64_t>(bu) * (P - 2) + (seg - 1)) * (32 * a.tiles) + jv) * K
                         : a.first + static_cast<int64_t>(b) * K) +
                   4 * kh;
#pragma unroll
      for (int j = 0; j < NOB; ++j)
        if (j < nob) {
#pragma unroll
          for (int i = 0; i < 16; ++i) la[j][i] += scale;
          keep_store(dst + 32 * (wave + nwaves * j), la[j]);
        }
    }
  } else if (wave == 0) {  // the last step of the chain: output unit 0 only
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
    if (live && kh == 0) a.last[static_cast<int64_t>(bu) * K + jv] = scale + log_unscaled(d);
  }
}

// ---- launch 2 -----------------------------------------------------------------------------------------------------------------
constexpr int kScanThreads = 256;
constexpr int kScanAhead = 16;  // rows of the next matrix a thread holds in registers (all of its share up to K = 64)

// the workgroup's maximum / sum of one value a thread, every thread gets it; the waves meet in `slot` (4 floats) in wave order
template <bool MAX>
__device__ __forceinline__ float scan_block_reduce(float v, float* slot) {
  v = ck::wave_reduce<MAX>(v);
  __syncthreads();  // (the slot's readers of an earlier reduction are done)
  if ((threadIdx.x & 63) == 0) slot[threadIdx.x >> 6] = v;
  __syncthreads();
  float r = slot[0];
#pragma unroll
  for (int k = 1; k < kScanThreads / 64; ++k) r = MAX ? fmaxf(r, slot[k]) : r + slot[k];
  return r;
}

template <int O2>  // outputs a thread owns: 1 (K <= 256, the start states split into 256 / K parts) or 2 (K <= 512)
__global__ void __launch_bounds__(kScanThreads) hmm_scan_combine_kernel(const HmmScanArgs a) {
  __shared__ float v[2][512];
  __shared__ float pm[kScanThreads], ps[kScanThreads], slot[4];
  const int K = a.K, P = a.P, ns = a.num_states, tid = threadIdx.x;
  const int64_t b = blockIdx.x;
  const int parts = O2 == 2 ? 1 : kScanThreads / K;
  const int part = O2 == 2 ? 0 : tid / K, o0 = tid - part * K;
  const bool act = part < parts;
  const int nm = act ? (ns - part + parts - 1) / parts : 0;  // start states j = part + parts i, i < nm, of this thread
  bool own[O2];
#pragma unroll
  for (int oo = 0; oo < O2; ++oo) own[oo] = act && o0 + kScanThreads * oo < K;

  const int64_t msize = static_cast<int64_t>(32 * a.tiles) * K;
  const float* const lg = a.lg + b * (P - 2) * msize;
  auto fetch = [&](const float* mat, float (&r)[O2][kScanAhead]) {
#pragma unroll
    for (int oo = 0; oo < O2; ++oo)
#pragma unroll
      for (int i = 0; i < kScanAhead; ++i)
        r[oo][i] = (own[oo] && i < nm) ? *ck::as_global(mat + static_cast<int64_t>(part + parts * i) * K + o0 + kScanThreads * oo) : -INFINITY;
  };
  float cur[O2][kScanAhead], nxt[O2][kScanAhead];
  if (P > 2) fetch(lg, cur);
  for (int o = tid; o < K; o += kScanThreads) v[0][o] = a.first[b * K + o];
  int32_t flagged = 0;
  for (int p = tid; p < P; p += kScanThreads) flagged |= a.flags[b * P + p];
  __syncthreads();

  int c = 0;
  for (int p = 1; p + 1 < P; ++p) {
    const float* mat = lg + (p - 1) * msize;
    if (p + 2 < P) fetch(mat + msize, nxt);
    const float* vc = v[c];
#pragma unroll
    for (int oo = 0; oo < O2; ++oo) {
      const float* col = mat + o0 + kScanThreads * oo;
      // the maximum first, clamped finite
      float m = -INFINITY;
#pragma unroll
      for (int i = 0; i < kScanAhead; ++i)
        if (i < nm) m = fmaxf(m, cur[oo][i] + vc[part + parts * i]);
      if (own[oo])
        for (int i = kScanAhead; i < nm; ++i) {
          const int j = part + parts * i;
          m = fmaxf(m, *ck::as_global(col + static_cast<int64_t>(j) * K) + vc[j]);
        }
      if (O2 == 1 && parts > 1) {
        pm[tid] = m;
        __syncthreads();
        if (act)
          for (int q = 0; q < parts; ++q) m = fmaxf(m, pm[q * K + o0]);
      }
      m = ck::clamp_finite(m);
      const float nml = exp_offset(m, kHmmHead);
      // then the sum of exp2
      float s = 0.f;
#pragma unroll
      for (int i = 0; i < kScanAhead; ++i)
        if (i < nm) s += __builtin_amdgcn_exp2f(fmaf(cur[oo][i] + vc[part + parts * i], kL2E, nml));
      if (own[oo])
        for (int i = kScanAhead; i < nm; ++i) {
          const int j = part + parts * i;
          s += __builtin_amdgcn_exp2f(fmaf(*ck::as_global(col + static_cast<int64_t>(j) * K) + vc[j], kL2E, nml));
        }
      if (O2 == 1 && parts > 1) {
        ps[tid] = s;
        __syncthreads();
        if (act) {
          s = 0.f;
          for (int q = 0; q < parts; ++q) s += ps[q * K + o0];  // (every part adds the shares in the same order)
        }
      }
      if (own[oo] && part == 0) v[c ^ 1][o0 + kScanThreads * oo] = log_unscaled(s) + m;
    }
    __syncthreads();
    c ^= 1;
#pragma unroll
    for (int oo = 0; oo < O2; ++oo)
#pragma unroll
      for (int i = 0; i < kScanAhead; ++i) cur[oo][i] = nxt[oo][i];
  }

  // the closing boundary: one output, the start states dealt over all threads
  float t[2];
  float m = -INFINITY;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int j = tid + kScanThreads * i;
    t[i] = j < ns ? a.last[b * K + j] + v[c][j] : -INFINITY;
    m = fmaxf(m, t[i]);
  }
  m = ck::clamp_finite(scan_block_reduce<true>(m, slot));
  const float nml = exp_offset(m, kHmmHead);
  float s = scan_block_reduce<false>(__builtin_amdgcn_exp2f(fmaf(t[0], kL2E, nml)) + __builtin_amdgcn_exp2f(fmaf(t[1], kL2E, nml)), slot);
  const float f = scan_block_reduce<true>(flagged != 0 ? 1.f : 0.f, slot);
  if (tid == 0) a.out[b] = f != 0.f ? __builtin_nanf("") : log_unscaled(s) + m;
}

template <int NOB>
int scan_launch_segments(const HmmScanArgs& a, void* stream) {
  constexpr int NBUF = 8;
  const int NQ = a.K / 32, waves = NQ < kHmmWaves ? NQ : kHmmWaves;
  const size_t lds = (static_cast<size_t>(NQ) * 1024 + kHmmWaves * 32 + static_cast<size_t>(waves) * NBUF * kHmmUnit) * sizeof(float);
  const int64_t groups = (a.B + 31) / 32 + static_cast<int64_t>(a.B) * (a.P - 1) * a.tiles;
  CK_REQUIRE(groups <= 0x7fffffff, "ck_hmm_scan_segments: %lld workgroups", static_cast<long long>(groups));
  const dim3 grid(static_cast<unsigned>(groups)), block(64 * waves);
  auto kernel = hmm_scan_segments_kernel<NOB>;
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

int scan_check(const char* name, const HmmScanArgs& a) {
  CK_REQUIRE(a.first && a.last && a.flags && (a.lg || a.P == 2), "%s: null scratch", name);
  CK_REQUIRE(a.T >= 2 && a.B >= 1, "%s: T = %d, B = %d", name, a.T, a.B);
  CK_REQUIRE(a.P >= 2 && a.P <= a.T, "%s: %d segments of %d steps", name, a.P, a.T);
  CK_REQUIRE(a.K >= 32 && a.K <= 512 && a.K % 32 == 0, "%s: K = %d is not a multiple of 32 in 32 .. 512", name, a.K);
  CK_REQUIRE(a.num_states >= 1 && a.num_states <= a.K, "%s: %d states of %d units", name, a.num_states, a.K);
  return 0;
}

HmmScanArgs scan_args(const void* const* w_steps, const int32_t* step_fold, const int32_t* step_var, int T, int K, int num_states,
                      const float* rows, const int64_t* x, int D, int C, const int32_t* integrate, int B, int P, float* first,
                      float* lg, float* last, int32_t* flags, float* out) {
  return HmmScanArgs{reinterpret_cast<const float* const*>(w_steps), step_fold, step_var, rows, x, integrate, C, D, T, B, K, P,
                     num_states, (num_states + 31) / 32, first, lg, last, flags, out};
}

}  // namespace

extern "C" int ck_hmm_scan_segments(const void* const* w_steps, const int32_t* step_fold, const int32_t* step_var, int T, int K,
                                    int num_states, const float* rows, const int64_t* x, int D, int C, const int32_t* integrate,
                                    int B, int P, float* first, float* lg, float* last, int32_t* flags, void* stream) {
  const HmmScanArgs a = scan_args(w_steps, step_fold, step_var, T, K, num_states, rows, x, D, C, integrate, B, P, first, lg, last,
                                  flags, nullptr);
  CK_REQUIRE(w_steps && step_fold && step_var && rows && x, "ck_hmm_scan_segments: null operand");
  CK_REQUIRE(C >= 1 && D >= 1, "ck_hmm_scan_segments: C = %d, D = %d", C, D);
  if (int st = scan_check("ck_hmm_scan_segments", a)) return st;
  const int NQ = K / 32, waves = NQ < kHmmWaves ? NQ : kHmmWaves;
  switch ((NQ + waves - 1) / waves) {
    case 1: return scan_launch_segments<1>(a, stream);
    case 2: return scan_launch_segments<2>(a, stream);
    case 3: return scan_launch_segments<3>(a, stream);
    default: return scan_launch_segments<4>(a, stream);
  }
}

extern "C" int ck_hmm_scan_combine(int T, int K, int num_states, int B, int P, const float* first, const float* lg, const float* last,
                                   const int32_t* flags, float* out, void* stream) {
  const HmmScanArgs a = scan_args(nullptr, nullptr, nullptr, T, K, num_states, nullptr, nullptr, 0, 0, nullptr, B, P,
                                  const_cast<float*>(first), const_cast<float*>(lg), const_cast<float*>(last),
                                  const_cast<int32_t*>(flags), out);
  CK_REQUIRE(out != nullptr, "ck_hmm_scan_combine: null operand");
  if (int st = scan_check("ck_hmm_scan_combine", a)) return st;
  const dim3 grid(B), block(kScanThreads);
  if (K <= kScanThreads) return ck::launch(hmm_scan_combine_kernel<1>, grid, block, 0, stream, a);
  return ck::launch(hmm_scan_combine_kernel<2>, grid, block, 0, stream, a);
}
