// The Baum-Welch E-step of a chain behind `HipHMM.expected_statistics` ("Expected statistics (Baum-Welch
// E-step)"): what follows the keeping forward and the statistics backward (ck_hmm.hip), which leave per (row, step) the posterior
// gamma_s and the operand rows a'_s, r'_s with  sum_{o,i} r'_{s+1}[o] W_s[o, i] a'_s[i] = 1  for a live row, zeros for a dead one.
//
// ck_hmm_pair_sum -- expected transition counts  N_s = W_s o (R_{s+1}^T A_s),  s = 0 .. T - 2: a K x K matrix per step, REDUCED OVER
// THE ROWS of the chunk.  The chain kernels keep rows on a workgroup and contract over units; this is the other GEMM shape.
//   * A workgroup of 4 waves owns (step, 128 x 128 output tile, row slice).  Wave (wo, wi) owns the 32 x 32 blocks
//     (wo + 2 jo, wi + 2 ji) of the tile -- interleaved, so K = 64 still has a block per wave -- 64 accumulator registers, and
//     walks the rows of its slice two at a time on v_mfma_f32_32x32x2_f32 (exact fp32): lane (m, kh) supplies
//     R[n + kh][32 qo + m] as operand A and A[n + kh][32 qi + m] as operand B.
//   * Operands are (rows, K) matrices with row stride D K.  16 rows x (128 + 128) floats are staged per step of the walk, every
//     thread four 16-byte loads (a row segment of 512 contiguous bytes per operand) held in registers while the previous stage
//     is contracted, then written to the other of two LDS buffers (2 x 16 KiB): one barrier a stage, each staged value read by two
//     waves.  A lane's LDS read is one dword, 32 consecutive lanes on 32 consecutive banks.
//   * Epilogue: edge += W_s o acc where a step has one row slice; otherwise the tile goes to scratch and `hmm_pair_reduce` adds
//     the slices in index order and multiplies by W_s.  No float atomics: bit-identical from call to call.
//   * The last step's single row, N_{T-1}[0, i] = sum_b gamma_{T-1}[b, i], is a column sum on the vector ALU by extra workgroups
//     of the same launch (64 columns; the 4 waves take every fourth row and are added in wave order).
// Row slices: a function of (T, K, B) alone -- until about 512 workgroups, at least 64 rows each.
//
// ck_hmm_leaf_sum -- emission counts: per (step, 64 states, 64 categories, row slice) a workgroup; each of its 4 waves walks every
// fourth row of the slice, one state a lane, and adds gamma[b, var_s, k] into a wave-private LDS histogram [bin][state] at bin
// x[b, var_s] (plain read-modify-write in row order; missing entries in one extra bin).  x is wave-uniform: a lane reads the
// entry of one of the wave's next 64 rows, the bins are broadcast by v_readlane, rows outside the workgroup's category slice are
// never loaded and eight rows are requested before the first is added.  Every category slice keeps its own missing bin (it
// re-reads the rows that miss the variable; nothing else is read twice).  The four histograms are added in wave order and written
// out transposed, (K, C), the missing bin spread over exp(table); with several row slices through scratch and `hmm_leaf_reduce`.
#include "ck_hmm.h"

namespace {

constexpr int kStatThreads = 256;
constexpr int64_t kStatTargetJobs = 512;  // row slices until a launch has about this many workgroups
constexpr int kStatMinSliceRows = 64;

// rows of a slice (a multiple of 16) and, through it, the number of slices: a function of the shapes alone
int slice_rows_of(int64_t jobs, int B) {
  const int64_t want = (kStatTargetJobs + jobs - 1) / jobs;
  int64_t rows = (B + want - 1) / want;
  rows = (rows + 15) / 16 * 16;
  return static_cast<int>(rows < kStatMinSliceRows ? kStatMinSliceRows : rows);
}

// ---- the pair sum ------------------------------------------------------------------------------------------------------------
constexpr int kPairTile = 128, kPairRows = 16;

struct PairArgs {
  const float* const* w;  // (T) the steps' weights, row-major (Ko, K)
  const int32_t* var;     // (T)
  const float* pa;        // (B, D, K) a'
  const float* pr;        // (B, D, K) r'
  const float* gamma;     // (B, D, K)
  float* edge;            // (T - 1) K^2 + K accumulators
  float* scratch;         // (S, (T - 1) K^2 + K) partial sums, S > 1
  int T, K, D, B, S, slice_rows, NT, pair_jobs;
};

__global__ void __launch_bounds__(kStatThreads) hmm_pair_kernel(const PairArgs a) {
  __shared__ __attribute__((aligned(16))) float sm[2][kPairRows][2 * kPairTile];
  const int K = a.K, NQ = K >> 5, tid = threadIdx.x;
  const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int m = lane & 31, kh = lane >> 5;
  const int64_t KK = static_cast<int64_t>(K) * K, total = static_cast<int64_t>(a.T - 1) * KK + K;
  int job = blockIdx.x;
  if (job >= a.pair_jobs) {
    // ---- the last step: column sums of gamma_{T-1}
    job -= a.pair_jobs;
    const int slice = job % a.S, col = 64 * (job / a.S) + lane;
    const int n0 = slice * a.slice_rows, n1 = min(a.B, n0 + a.slice_rows);
    const float* src = a.gamma + static_cast<int64_t>(a.var[a.T - 1]) * K + (col < K ? col : 0);
    const int64_t stride = static_cast<int64_t>(a.D) * K;
    float acc = 0.f;
    for (int n = n0 + wave; n < n1; n += 32) {
      float g[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) g[u] = n + 4 * u < n1 ? src[(n + 4 * u) * stride] : 0.f;
#pragma unroll
      for (int u = 0; u < 8; ++u) acc += g[u];
    }
    float* part = &sm[0][0][0];
    part[wave * 64 + lane] = acc;
    __syncthreads();
    if (wave == 0 && col < K) {
      const float t = ((part[lane] + part[64 + lane]) + part[128 + lane]) + part[192 + lane];
      const int64_t at = total - K + col;
      if (a.S == 1)
        a.edge[at] += t;
      else
        a.scratch[slice * total + at] = t;
    }
    return;
  }
  const int slice = job % a.S, tile = (job / a.S) % (a.NT * a.NT), s = job / (a.S * a.NT * a.NT);
  const int o0 = kPairTile * (tile / a.NT), i0 = kPairTile * (tile % a.NT);
  const int n0 = slice * a.slice_rows, n1 = min(a.B, n0 + a.slice_rows);
  const int wo = wave >> 1, wi = wave & 1;
  const bool ok_o[2] = {o0 / 32 + wo < NQ, o0 / 32 + wo + 2 < NQ}, ok_i[2] = {i0 / 32 + wi < NQ, i0 / 32 + wi + 2 < NQ};

  // a thread's four 16-byte pieces of a stage: piece u is row (tid + 256 u) / 64, operand ((tid >> 5) & 1), floats 4 (tid & 31) ..
  const int prow = tid >> 6, pcol = 4 * (tid & 31), pop = (tid >> 5) & 1;
  const int gcol = (pop ? i0 : o0) + pcol;
  const float* const src = (pop ? a.pa + static_cast<int64_t>(a.var[s]) * K : a.pr + static_cast<int64_t>(a.var[s + 1]) * K) + (gcol < K ? gcol : 0);
  const int64_t stride = static_cast<int64_t>(a.D) * K;
  float4 piece[4];
  auto fetch = [&](int nb) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int n = nb + prow + 4 * u;
      piece[u] = (n < n1 && gcol < K) ? ck::gload4(src + n * stride) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
  };
  auto put = [&](int buf) {
#pragma unroll
    for (int u = 0; u < 4; ++u) *reinterpret_cast<float4*>(&sm[buf][prow + 4 * u][kPairTile * pop + pcol]) = piece[u];
  };

  f32x16 acc[2][2];
#pragma unroll
  for (int jo = 0; jo < 2; ++jo)
#pragma unroll
    for (int ji = 0; ji < 2; ++ji)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[jo][ji][r] = 0.f;

  fetch(n0);
  put(0);
  __syncthreads();
  int buf = 0;
  for (int nb = n0; nb < n1; nb += kPairRows, buf ^= 1) {
    const bool more = nb + kPairRows < n1;
    if (more) fetch(nb + kPairRows);
#pragma unroll
    for (int kk = 0; kk < kPairRows / 2; ++kk) {
      const float* rowp = &sm[buf][2 * kk + kh][0];
      const float r0 = rowp[32 * wo + m], r1 = rowp[32 * (wo + 2) + m];
      const float a0 = rowp[kPairTile + 32 * wi + m], a1 = rowp[kPairTile + 32 * (wi + 2) + m];
      if (ok_o[0] && ok_i[0]) acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(r0, a0, acc[0][0], 0, 0, 0);
      if (ok_o[0] && ok_i[1]) acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(r0, a1, acc[0][1], 0, 0, 0);
      if (ok_o[1] && ok_i[0]) acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(r1, a0, acc[1][0], 0, 0, 0);
      if (ok_o[1] && ok_i[1]) acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(r1, a1, acc[1][1], 0, 0, 0);
    }
    if (more) put(buf ^ 1);
    __syncthreads();
  }

  // ---- epilogue: acc[jo][ji][r] is N[o][i], o = 32 qo + 8 (r >> 2) + 4 kh + (r & 3), i = 32 qi + m
  const float* w = a.w[s];
#pragma unroll
  for (int jo = 0; jo < 2; ++jo)
#pragma unroll
    for (int ji = 0; ji < 2; ++ji) {
      if (!(ok_o[jo] && ok_i[ji])) continue;
      const int ob = o0 + 32 * (wo + 2 * jo), i = i0 + 32 * (wi + 2 * ji) + m;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int64_t at = static_cast<int64_t>(ob + 8 * (r >> 2) + 4 * kh + (r & 3)) * K + i;
        if (a.S == 1) {
          const float wv = w[at];
          a.edge[s * KK + at] += wv > 0.f ? wv * acc[jo][ji][r] : 0.f;
        } else {
          a.scratch[slice * total + s * KK + at] = acc[jo][ji][r];
        }
      }
    }
}

__global__ void __launch_bounds__(kStatThreads) hmm_pair_reduce(const PairArgs a) {
  const int64_t KK = static_cast<int64_t>(a.K) * a.K, total = static_cast<int64_t>(a.T - 1) * KK + a.K;
  const int64_t at = static_cast<int64_t>(blockIdx.x) * kStatThreads + threadIdx.x;
  if (at >= total) return;
  float t = 0.f;
  for (int sl = 0; sl < a.S; ++sl) t += a.scratch[sl * total + at];
  if (at < total - a.K) {
    const float wv = a.w[at / KK][at % KK];
    t = wv > 0.f ? wv * t : 0.f;
  }
  a.edge[at] += t;
}

// ---- the emission counts -----------------------------------------------------------------------------------------------------
constexpr int kLeafCats = 64, kLeafStates = 64, kLeafPitch = 65;
constexpr int kLeafHist = (kLeafCats + 1) * kLeafPitch;  // floats of one histogram: [bin][state], bin kLeafCats the missing entries

struct LeafArgs {
  const float* gamma;     // (B, D, K)
  const int64_t* x;       // (B, D)
  const int32_t* integ;   // (D) or nullptr
  const int32_t* fold;    // (T)
  const int32_t* var;     // (T)
  const float* table;     // (F, C + 1, K) logarithms
  float* leaf;            // (F, K, C) accumulators
  float* scratch;         // (jobs, S, kLeafHist), S > 1
  int T, K, C, D, B, S, slice_rows, KB, NCS;
};

// += the summed histogram h of (step s, state block kb, category slice cs), transposed, the missing bin spread over p(c | k)
__device__ __forceinline__ void leaf_writeback(const LeafArgs& a, const float* h, int s, int kb, int cs) {
  const int64_t f = a.fold[s];
  const int c0 = cs * kLeafCats, nc = min(kLeafCats, a.C - c0), k0 = kb * kLeafStates, nk = min(kLeafStates, a.K - k0);
  for (int idx = threadIdx.x; idx < nk * nc; idx += kStatThreads) {
    const int k = idx / nc, c = idx - k * nc;
    float v = h[c * kLeafPitch + k];
    const float ms = h[kLeafCats * kLeafPitch + k];
    if (ms != 0.f) v = fmaf(ms, expf(a.table[(f * (a.C + 1) + c0 + c) * a.K + k0 + k]), v);
    a.leaf[(f * a.K + k0 + k) * a.C + c0 + c] += v;
  }
}

__global__ void __launch_bounds__(kStatThreads) hmm_leaf_kernel(const LeafArgs a) {
  extern __shared__ __attribute__((aligned(16))) float hist[];  // [4 waves][kLeafHist]
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  int job = blockIdx.x;
  const int slice = job % a.S;
  job /= a.S;
  const int cs = job % a.NCS, kb = (job / a.NCS) % a.KB, s = job / (a.NCS * a.KB);
  const int c0 = cs * kLeafCats, nc = min(kLeafCats, a.C - c0), k = kb * kLeafStates + lane;
  const int n0 = slice * a.slice_rows, n1 = min(a.B, n0 + a.slice_rows);
  const int var = a.var[s];
  const bool summed_out = a.integ != nullptr && a.integ[var] != 0, kvalid = k < a.K;
  for (int i = tid; i < 4 * kLeafHist; i += kStatThreads) hist[i] = 0.f;
  __syncthreads();
  float* const hw = hist + wave * kLeafHist + lane;
  const int64_t stride = static_cast<int64_t>(a.D) * a.K;
  const float* const src = a.gamma + static_cast<int64_t>(var) * a.K + (kvalid ? k : 0);
  // the wave's rows are n0 + wave + 4 j; lane l looks up the bin of row j = base + l, 64 rows at a time
  for (int base = n0 + wave; base < n1; base += 256) {
    const int mine = base + 4 * lane;
    int bin = -1;
    if (mine < n1) {
      const int64_t xv = a.x[static_cast<int64_t>(mine) * a.D + var];
      if (xv < 0 || summed_out)
        bin = kLeafCats;
      else if (xv >= c0 && xv < c0 + nc)
        bin = static_cast<int>(xv) - c0;
    }
    for (int j = 0; j < 64 && base + 4 * j < n1; j += 8) {
      int bj[8];
      float g[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        bj[u] = __builtin_amdgcn_readlane(bin, j + u);
        g[u] = (bj[u] >= 0 && kvalid) ? src[(base + 4 * (j + u)) * stride] : 0.f;
      }
#pragma unroll
      for (int u = 0; u < 8; ++u)
        if (bj[u] >= 0) hw[bj[u] * kLeafPitch] += g[u];
    }
  }
  __syncthreads();
  for (int i = tid; i < kLeafHist; i += kStatThreads)
    hist[i] = ((hist[i] + hist[kLeafHist + i]) + hist[2 * kLeafHist + i]) + hist[3 * kLeafHist + i];
  __syncthreads();
  if (a.S == 1) {
    leaf_writeback(a, hist, s, kb, cs);
  } else {
    float* dst = a.scratch + (static_cast<int64_t>(job) * a.S + slice) * kLeafHist;
    for (int i = tid; i < kLeafHist; i += kStatThreads) dst[i] = hist[i];
  }
}

__global__ void __launch_bounds__(kStatThreads) hmm_leaf_reduce(const LeafArgs a) {
  __shared__ float h[kLeafHist];
  const int job = blockIdx.x;
  const float* src = a.scratch + static_cast<int64_t>(job) * a.S * kLeafHist;
  for (int i = threadIdx.x; i < kLeafHist; i += kStatThreads) {
    float t = 0.f;
    for (int sl = 0; sl < a.S; ++sl) t += src[static_cast<int64_t>(sl) * kLeafHist + i];
    h[i] = t;
  }
  __syncthreads();
  leaf_writeback(a, h, job / (a.NCS * a.KB), (job / a.NCS) % a.KB, job % a.NCS);
}

struct PairShape {
  int NT, slice_rows, S;
  int64_t pair_jobs, last_jobs;
};
PairShape pair_shape(int T, int K, int B) {
  PairShape p;
  p.NT = (K + kPairTile - 1) / kPairTile;
  const int64_t per_slice = static_cast<int64_t>(T - 1) * p.NT * p.NT + (K + 63) / 64;
  p.slice_rows = slice_rows_of(per_slice, B);
  p.S = (B + p.slice_rows - 1) / p.slice_rows;
  p.pair_jobs = static_cast<int64_t>(T - 1) * p.NT * p.NT * p.S;
  p.last_jobs = static_cast<int64_t>((K + 63) / 64) * p.S;
  return p;
}
struct LeafShape {
  int KB, NCS, slice_rows, S;
  int64_t jobs;  // without the row slices
};
LeafShape leaf_shape(int T, int K, int C, int B) {
  LeafShape p;
  p.KB = (K + kLeafStates - 1) / kLeafStates;
  p.NCS = (C + kLeafCats - 1) / kLeafCats;
  p.jobs = static_cast<int64_t>(T) * p.KB * p.NCS;
  p.slice_rows = slice_rows_of(p.jobs, B);
  p.S = (B + p.slice_rows - 1) / p.slice_rows;
  return p;
}
bool shapes_ok(int T, int K, int B) { return T >= 1 && B >= 1 && K >= 32 && K <= 1024 && K % 32 == 0; }

}  // namespace

extern "C" int ck_hmm_stats_scratch(int T, int K, int C, int B) {
  if (!shapes_ok(T, K, B) || C < 1) return -1;
  const PairShape p = pair_shape(T, K, B);
  const LeafShape l = leaf_shape(T, K, C, B);
  const int64_t pf = p.S == 1 ? 0 : p.S * (static_cast<int64_t>(T - 1) * K * K + K), lf = l.S == 1 ? 0 : l.jobs * l.S * kLeafHist;
  const int64_t units = ((pf > lf ? pf : lf) + 1023) / 1024;
  return units <= 0x7fffffff ? static_cast<int>(units) : -1;
}

extern "C" int ck_hmm_pair_sum(const void* const* w_steps, const int32_t* step_var, int T, int K, int D, int B, const float* pair_a,
                               const float* pair_r, const float* gamma, float* edge, float* scratch, int64_t scratch_floats,
                               void* stream) {
  CK_REQUIRE(w_steps && step_var && pair_a && pair_r && gamma && edge, "ck_hmm_pair_sum: null operand");
  CK_REQUIRE(shapes_ok(T, K, B) && D >= T, "ck_hmm_pair_sum: T = %d, K = %d, D = %d, B = %d", T, K, D, B);
  const PairShape p = pair_shape(T, K, B);
  const int64_t total = static_cast<int64_t>(T - 1) * K * K + K;
  CK_REQUIRE(p.S == 1 || (scratch != nullptr && scratch_floats >= p.S * total),
             "ck_hmm_pair_sum: %d row slices need %lld floats of scratch, %lld given", p.S, static_cast<long long>(p.S * total),
             static_cast<long long>(scratch_floats));
  CK_REQUIRE(p.pair_jobs + p.last_jobs <= 0x7fffffff && total <= 0x7fffffffLL * kStatThreads, "ck_hmm_pair_sum: grid too large");
  const PairArgs a{reinterpret_cast<const float* const*>(w_steps), step_var, pair_a, pair_r, gamma, edge, scratch, T, K, D, B, p.S,
                   p.slice_rows, p.NT, static_cast<int>(p.pair_jobs)};
  const dim3 grid(static_cast<unsigned>(p.pair_jobs + p.last_jobs)), rgrid(static_cast<unsigned>((total + kStatThreads - 1) / kStatThreads));
  return ck::dispatch(
      [=](hipStream_t s) {
        hipLaunchKernelGGL(hmm_pair_kernel, grid, dim3(kStatThreads), 0, s, a);
        if (a.S > 1) hipLaunchKernelGGL(hmm_pair_reduce, rgrid, dim3(kStatThreads), 0, s, a);
        return hipGetLastError();
      },
      stream);
}

extern "C" int ck_hmm_leaf_sum(const int32_t* step_fold, const int32_t* step_var, int T, int K, const float* table, const int64_t* x,
                               int D, int C, const int32_t* integrate, int B, const float* gamma, float* leaf, float* scratch,
                               int64_t scratch_floats, void* stream) {
  CK_REQUIRE(step_fold && step_var && table && x && gamma && leaf, "ck_hmm_leaf_sum: null operand");
  CK_REQUIRE(shapes_ok(T, K, B) && D >= T && C >= 1, "ck_hmm_leaf_sum: T = %d, K = %d, C = %d, D = %d, B = %d", T, K, C, D, B);
  const LeafShape p = leaf_shape(T, K, C, B);
  CK_REQUIRE(p.S == 1 || (scratch != nullptr && scratch_floats >= p.jobs * p.S * kLeafHist),
             "ck_hmm_leaf_sum: %d row slices need %lld floats of scratch, %lld given", p.S,
             static_cast<long long>(p.jobs * p.S * kLeafHist), static_cast<long long>(scratch_floats));
  CK_REQUIRE(p.jobs * p.S <= 0x7fffffff, "ck_hmm_leaf_sum: grid too large");
  const LeafArgs a{gamma, x, integrate, step_fold, step_var, table, leaf, scratch, T, K, C, D, B, p.S, p.slice_rows, p.KB, p.NCS};
  const dim3 grid(static_cast<unsigned>(p.jobs * p.S)), rgrid(static_cast<unsigned>(p.jobs));
  constexpr int lds = 4 * kLeafHist * static_cast<int>(sizeof(float));
  return ck::dispatch(
      [=](hipStream_t s) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(hmm_leaf_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(hmm_leaf_kernel, grid, dim3(kStatThreads), lds, s, a);
        if (a.S > 1) hipLaunchKernelGGL(hmm_leaf_reduce, rgrid, dim3(kStatThreads), 0, s, a);
        return hipGetLastError();
      },
      stream);
}
