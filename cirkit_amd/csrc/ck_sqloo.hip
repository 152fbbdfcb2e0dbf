// Leave-one-out conditionals of squared circuits p(x) = |c(x)|^2 / Z ("Leave-one-out conditionals of
// squared circuits").  With every variable but v observed the derivative of the product circuit c (x) conj(c) is rank-1,
//     |c(x_-v, s)|^2 = |sum_k g_k a_k(s)|^2,   g_k = dc(x) / du_k  for the K units u_k of the input fold of v,
// so ONE pass over c itself, K values per row and fold, serves every variable of every row.  The pass carries D = log dc/du (never
// the flow g u / c, which is 0 exactly where the observed state is impossible) as a signed logarithm: `float` under lse-sum, c32
// under complex-lse-sum, whose argument is a multiple of pi because the parameters are real.  Per layer of c that has down folds
// (folds whose scope holds a query variable), from the output layer downwards (ck_squared_loo_down):
//     a layer with weights   P_i = log sum_k W[k][i] exp(D_k)   shifted by the largest finite Re D_k of the row, summed in
//                            linear space; argument pi where the sum is negative, -inf where it is exactly 0
//     a Hadamard layer       P = D
//     child slot h           D_child = P + sum over h' != h of value(h')      (c's arena, slot order; never total minus own)
// Only trees: every child is written exactly once, nothing is combined, no atomics, no initialisation of the arena.  The leaves
// (ck_squared_loo_leaf) evaluate A(s) = sum_k Re exp(D_k - m) a_k(s) and log m(s) = 2 (log |A(s)| + m) for every state.
#include "ck_sqpath.h"
#include "ck_tile.h"

namespace {

constexpr int kLdHead = CK_SQ_LOO_FOLD_WORDS;  // int64 words of a fold in front of its child (D, value) pairs
constexpr int kLdMaxH = 8;                     // children of a fold
constexpr int kLdLeaf = CK_SQ_LOO_LEAF_WORDS;
constexpr int kLdRows = 32;  // rows of a tile: one wave of the 32-unit form, one workgroup of the others
constexpr float kLdPi = 3.14159265358979323846f;

struct LdArgs {
  const float* vals;   // c's arena
  float* der;          // the derivative arena
  const int64_t* tab;  // [n][kLdHead + 2 H]
  const float* w;      // (folds, Ko, Ki) or null: a Hadamard layer
  int n, H, Ki, Ko, B;
};

// a signed logarithm (re, im) as the linear value of its real part after the shift by m: +-exp(re - m); the argument is a
// multiple of pi (real parameters), odd multiples are negative
template <bool CPLX>
__device__ __forceinline__ float ld_lin(float re, float im, float m) {
  const float e = expf(re - m);
  if constexpr (CPLX) return (static_cast<int>(rintf(im * 0.31830988618379067154f)) & 1) ? -e : e;
  return e;
}
// log of a linear value plus the shift: (log |y| + m, pi where y < 0); -inf where y is exactly 0
template <bool CPLX>
__device__ __forceinline__ void ld_log(float y, float m, float& re, float& im) {
  if constexpr (CPLX) {
    re = y == 0.f ? -INFINITY : logf(fabsf(y)) + m;
    im = y < 0.f ? kLdPi : 0.f;
  } else {
    re = y == 0.f ? -INFINITY : logf(y) + m;
    im = 0.f;
  }
}
template <bool CPLX>
__device__ __forceinline__ void ld_read(const float* p, int64_t e, float& re, float& im) {
  if constexpr (CPLX) {
    re = p[2 * e];
    im = p[2 * e + 1];
  } else {
    re = p[e];
    im = 0.f;
  }
}
template <bool CPLX>
__device__ __forceinline__ void ld_write(float* p, int64_t e, float re, float im) {
  if constexpr (CPLX) {
    p[2 * e] = re;
    p[2 * e + 1] = im;
  } else {
    p[e] = re;
  }
}
// the derivative of the output fold: log 1 at unit 0, -inf elsewhere
__device__ __forceinline__ float ld_top(int k) { return k == 0 ? 0.f : -INFINITY; }

// P of element i of row b into every child slot that is a down fold, plus the values of the other slots in slot order
template <bool CPLX>
__device__ __forceinline__ void ld_emit(const LdArgs& a, const int64_t* row, int64_t b, int i, float pre, float pim) {
  for (int h = 0; h < a.H; ++h) {
    const int64_t dout = row[kLdHead + 2 * h];
    if (dout < 0) continue;
    float re = pre, im = pim;
    for (int g = 0; g < a.H; ++g) {
      if (g == h) continue;
      float vr, vi;
      ld_read<CPLX>(a.vals, row[kLdHead + 2 * g + 1] + b * a.Ki + i, vr, vi);
      re += vr;
      im += vi;
    }
    ld_write<CPLX>(a.der, dout + b * a.Ki + i, re, im);
  }
}

// ---- a Hadamard layer: P = D, one thread per (fold, row, unit), no stage ---------------------------------------------------
template <bool CPLX>
__global__ void __launch_bounds__(256) ld_hadamard_kernel(LdArgs a) {
  const int64_t idx = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  const int64_t per = static_cast<int64_t>(a.B) * a.Ki;
  if (idx >= per * a.n) return;
  const int f = static_cast<int>(idx / per);
  const int64_t e = idx - f * per;
  const int64_t b = e / a.Ki;
  const int i = static_cast<int>(e - b * a.Ki);
  const int64_t* row = a.tab + static_cast<int64_t>(f) * (kLdHead + 2 * a.H);
  float re = ld_top(i), im = 0.f;
  if (row[1] >= 0) ld_read<CPLX>(a.der, row[1] + e, re, im);
  ld_emit<CPLX>(a, row, b, i, re, im);
}

// ---- any shape with weights: a workgroup takes one fold and kLdRows rows; W staged once, the sums on the VALU in the order
// k = 0 .. Ko - 1 whatever the row's place in the tile ---------------------------------------------------------------------
template <bool CPLX>
__global__ void __launch_bounds__(256) ld_down_kernel(LdArgs a) {
  extern __shared__ __attribute__((aligned(16))) char ld_smem[];
  const int t = threadIdx.x, Ki = a.Ki, Ko = a.Ko;
  float* w_s = reinterpret_cast<float*>(ld_smem);  // [Ko][Ki]
  float* e_s = w_s + Ko * Ki;                      // [kLdRows][Ko]
  float* m_s = e_s + kLdRows * Ko;                 // [kLdRows]
  const int nb = (a.B + kLdRows - 1) / kLdRows;
  const int f = blockIdx.x / nb;
  const int64_t* row = a.tab + static_cast<int64_t>(f) * (kLdHead + 2 * a.H);
  const int64_t b0 = static_cast<int64_t>(blockIdx.x - f * nb) * kLdRows, din = row[1];
  const int rows = a.B - b0 < kLdRows ? static_cast<int>(a.B - b0) : kLdRows;
  const float* wf = a.w + row[0] * Ko * Ki;
  for (int i = t; i < Ko * Ki; i += 256) w_s[i] = wf[i];
  if (t < rows) {
    float mx = -INFINITY;
    for (int k = 0; k < Ko; ++k) {
      float re = ld_top(k), im = 0.f;
      if (din >= 0) ld_read<CPLX>(a.der, din + (b0 + t) * Ko + k, re, im);
      mx = fmaxf(mx, re);
    }
    m_s[t] = ck::clamp_finite(mx);
  }
  __syncthreads();
  for (int e = t; e < rows * Ko; e += 256) {
    const int r = e / Ko, k = e - r * Ko;
    float re = ld_top(k), im = 0.f;
    if (din >= 0) ld_read<CPLX>(a.der, din + b0 * Ko + e, re, im);
    e_s[e] = ld_lin<CPLX>(re, im, m_s[r]);
  }
  __syncthreads();
  for (int e = t; e < rows * Ki; e += 256) {
    const int r = e / Ki, i = e - r * Ki;
    float acc = 0.f;
    for (int k = 0; k < Ko; ++k) acc = fmaf(w_s[k * Ki + i], e_s[r * Ko + k], acc);
    float re, im;
    ld_log<CPLX>(acc, m_s[r], re, im);
    ld_emit<CPLX>(a, row, b0 + r, i, re, im);
  }
}

// ---- 32 -> 32, and the 32 -> 1 root: a wave takes 32 rows in the register tile of ck_tile.h (lane (b, kh) holds units
// 8g + 4kh + t of row b in register 4g + t), the contraction E . W on v_mfma_f32_32x32x2_f32 with A[i][k] = W[k][i] read from the
// fold's staged matrix once per wave; the output layout of the MFMA is the input layout, so logarithm, sign, sibling sums and
// stores stay per lane.  Column b of the product depends on column b of E alone: a row's bits do not depend on its place --------
template <bool CPLX>
__device__ __forceinline__ void ld_tile_read(const float* base, int64_t elem, int kh, float (&re)[16], float (&im)[16]) {
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    if constexpr (CPLX) {
      const float* p = base + 2 * (elem + 8 * g + 4 * kh);
      const float4 q0 = ck::gload4(p), q1 = ck::gload4(p + 4);
      re[4 * g] = q0.x, im[4 * g] = q0.y, re[4 * g + 1] = q0.z, im[4 * g + 1] = q0.w;
      re[4 * g + 2] = q1.x, im[4 * g + 2] = q1.y, re[4 * g + 3] = q1.z, im[4 * g + 3] = q1.w;
    } else {
      const float4 q = ck::gload4(base + elem + 8 * g + 4 * kh);
      re[4 * g] = q.x, re[4 * g + 1] = q.y, re[4 * g + 2] = q.z, re[4 * g + 3] = q.w;
      im[4 * g] = im[4 * g + 1] = im[4 * g + 2] = im[4 * g + 3] = 0.f;
    }
  }
}
template <bool CPLX>
__device__ __forceinline__ void ld_tile_write(float* base, int64_t elem, int kh, const float (&re)[16], const float (&im)[16]) {
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    if constexpr (CPLX) {
      float* p = base + 2 * (elem + 8 * g + 4 * kh);
      ck::gstore4(p, make_float4(re[4 * g], im[4 * g], re[4 * g + 1], im[4 * g + 1]));
      ck::gstore4(p + 4, make_float4(re[4 * g + 2], im[4 * g + 2], re[4 * g + 3], im[4 * g + 3]));
    } else {
      ck::gstore4(base + elem + 8 * g + 4 * kh, make_float4(re[4 * g], re[4 * g + 1], re[4 * g + 2], re[4 * g + 3]));
    }
  }
}

template <bool CPLX>
__global__ void __launch_bounds__(256) ld_down32_kernel(LdArgs a) {
  __shared__ __attribute__((aligned(16))) float w_s[32 * 32];
  const int t = threadIdx.x, Ko = a.Ko;
  const int nb = (a.B + 4 * kLdRows - 1) / (4 * kLdRows);
  const int f = blockIdx.x / nb;
  const int64_t* row = a.tab + static_cast<int64_t>(f) * (kLdHead + 2 * a.H);
  const float* wf = a.w + row[0] * Ko * 32;
  for (int i = t; i < Ko * 32; i += 256) w_s[i] = wf[i];
  __syncthreads();
  const int lane = t & 63, bl = lane & 31, kh = lane >> 5;
  const int64_t w0 = static_cast<int64_t>(blockIdx.x - f * nb) * (4 * kLdRows) + (t >> 6) * kLdRows;
  if (w0 >= a.B) return;  // (no barrier below: a wave without rows leaves)
  const int64_t b = w0 + bl, din = row[1];
  const bool live = b < a.B;  // a partly filled tile: the other lanes read nothing, contribute E = 0 and store nothing
  float re[16], im[16], m;
  f32x16 acc;
  if (Ko == 32) {
#pragma unroll
    for (int j = 0; j < 16; ++j) re[j] = -INFINITY, im[j] = 0.f;
    if (live && din >= 0) ld_tile_read<CPLX>(a.der, din + b * 32, kh, re, im);
    if (live && din < 0 && kh == 0) re[0] = 0.f;
    m = row_max16(re);
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const float wj = w_s[(8 * (j >> 2) + 4 * kh + (j & 3)) * 32 + bl];  // A[i = bl][k]: W read transposed
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(wj, ld_lin<CPLX>(re[j], im[j], m), acc, 0, 0, 0);
    }
  } else {  // the root: one output unit, P_i = log (W[0][i] exp(D_0))
    float r0 = live ? 0.f : -INFINITY, i0 = 0.f;
    if (live && din >= 0) ld_read<CPLX>(a.der, din + b, r0, i0);
    m = ck::clamp_finite(r0);
    const float e0 = ld_lin<CPLX>(r0, i0, m);
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = w_s[8 * (r >> 2) + 4 * kh + (r & 3)] * e0;
  }
  if (!live) return;
  float pre[16], pim[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) ld_log<CPLX>(acc[r], m, pre[r], pim[r]);
  for (int h = 0; h < a.H; ++h) {
    const int64_t dout = row[kLdHead + 2 * h];
    if (dout < 0) continue;
#pragma unroll
    for (int r = 0; r < 16; ++r) re[r] = pre[r], im[r] = pim[r];
    for (int g = 0; g < a.H; ++g) {
      if (g == h) continue;
      float vr[16], vi[16];
      ld_tile_read<CPLX>(a.vals, row[kLdHead + 2 * g + 1] + b * 32, kh, vr, vi);
#pragma unroll
      for (int r = 0; r < 16; ++r) re[r] += vr[r], im[r] += vi[r];
    }
    ld_tile_write<CPLX>(a.der, dout + b * 32, kh, re, im);
  }
}

// ---- the leaves ------------------------------------------------------------------------------------------------------------
struct LdLeafArgs {
  const float* der;
  const int64_t* tab;  // [nq][kLdLeaf]
  const int64_t* x;    // (B, D) or null
  float* out;          // (B, nq, Cmax), or (B, nq) per entry
  int nq, Cmax, D, B, mode, R, maxC, maxK;
};

// one workgroup per (query variable, R rows): the variable's table staged once per chunk of 256 states (a table of logarithms
// shifted state by state), thread t takes state s0 + t of every row; then a wave per row: the logarithm of the sum over the
// states (lanes stride the states, whatever the row's place) and the row's output
template <bool CPLX>
__global__ void __launch_bounds__(256) ld_leaf_kernel(LdLeafArgs a) {
  extern __shared__ __attribute__((aligned(16))) char ld_smem[];
  const int t = threadIdx.x, R = a.R;
  const int nb = (a.B + R - 1) / R;
  const int q = blockIdx.x / nb;
  const int64_t* row = a.tab + static_cast<int64_t>(q) * kLdLeaf;
  const float* table = reinterpret_cast<const float*>(row[0]);
  const int C = static_cast<int>(row[1]), K = static_cast<int>(row[2]), tlog = static_cast<int>(row[3]);
  const int64_t din = row[4], var = row[5];
  const int64_t b0 = static_cast<int64_t>(blockIdx.x - q * nb) * R;
  const int rows = a.B - b0 < R ? static_cast<int>(a.B - b0) : R;
  float* av = reinterpret_cast<float*>(ld_smem);                              // [256][maxK + 1]
  float* e_s = av + (a.maxC < kSpStates ? a.maxC : kSpStates) * (a.maxK + 1);  // [R][maxK]
  float* m_s = e_s + R * a.maxK;                                              // [R]
  float* lm = m_s + R;                                                        // [R][maxC]
  if (t < rows) {
    float mx = -INFINITY;
    for (int k = 0; k < K; ++k) {
      float re = ld_top(k), im = 0.f;
      if (din >= 0) ld_read<CPLX>(a.der, din + (b0 + t) * K + k, re, im);
      mx = fmaxf(mx, re);
    }
    m_s[t] = ck::clamp_finite(mx);
  }
  __syncthreads();
  for (int e = t; e < rows * K; e += 256) {
    const int r = e / K, k = e - r * K;
    float re = ld_top(k), im = 0.f;
    if (din >= 0) ld_read<CPLX>(a.der, din + b0 * K + e, re, im);
    e_s[e] = ld_lin<CPLX>(re, im, m_s[r]);
  }
  for (int s0 = 0; s0 < C; s0 += kSpStates) {
    const int n = C - s0 < kSpStates ? C - s0 : kSpStates;
    __syncthreads();  // (e_s is written, av is free)
    for (int i = t; i < n * K; i += 256) {
      const int s = i / K, k = i - s * K;
      av[s * (K + 1) + k] = table[static_cast<int64_t>(s0) * K + i];
    }
    __syncthreads();
    if (t < n) {
      float* r = av + t * (K + 1);  // (this thread's state: nobody else touches it)
      float tm = 0.f;
      if (tlog) {
        tm = -INFINITY;
        for (int k = 0; k < K; ++k) tm = fmaxf(tm, r[k]);
        tm = ck::clamp_finite(tm);
        for (int k = 0; k < K; ++k) r[k] = expf(r[k] - tm);
      }
      for (int j = 0; j < rows; ++j) {
        float acc = 0.f;
        for (int k = 0; k < K; ++k) acc = fmaf(e_s[j * K + k], r[k], acc);
        lm[j * C + s0 + t] = acc == 0.f ? -INFINITY : 2.f * (logf(fabsf(acc)) + m_s[j] + tm);
      }
    }
  }
  __syncthreads();
  const int lane = t & 63;
  for (int j = t >> 6; j < rows; j += 4) {
    const float* l = lm + j * C;
    const int64_t b = b0 + j;
    float lse = 0.f;
    if (a.mode != 0) {
      float mx = -INFINITY;
      for (int s = lane; s < C; s += 64) mx = fmaxf(mx, l[s]);
      mx = ck::clamp_finite(ck::wave_max(mx));
      float sum = 0.f;
      for (int s = lane; s < C; s += 64) sum += expf(l[s] - mx);
      lse = logf(ck::wave_sum(sum)) + mx;
    }
    if (a.mode == 2) {
      if (lane == 0) {
        int64_t xs = a.x[b * a.D + var];
        xs = xs < 0 ? 0 : (xs >= C ? C - 1 : xs);  // (an absent entry: the host makes the row NaN)
        a.out[b * a.nq + q] = l[xs] - lse;
      }
    } else {
      float* o = a.out + (b * a.nq + q) * a.Cmax;
      for (int s = lane; s < a.Cmax; s += 64) o[s] = s < C ? l[s] - lse : -INFINITY;  // (columns past the variable's own states)
    }
  }
}

template <auto Kernel, class A>
int ld_dispatch(const A& a, int64_t blocks, size_t lds, void* stream) {
  const dim3 grid(static_cast<unsigned>(blocks)), block(256);
  return ck::dispatch(
      [=](hipStream_t s) {
        const hipError_t er = sp_raise_lds<Kernel>(lds, 0);
        if (er != hipSuccess) return er;
        hipLaunchKernelGGL(Kernel, grid, block, lds, s, a);
        return hipGetLastError();
      },
      stream);
}

constexpr size_t kLdMaxLds = 160 * 1024;

}  // namespace

extern "C" int ck_squared_loo_down(const float* values, int64_t value_elems, float* der, int64_t der_elems, const int64_t* folds_host,
                                   const int64_t* folds, int n, int H, const float* w, int num_weight_folds, int Ki, int Ko, int B,
                                   int complex_values, int form, void* stream) {
  const char* who = "ck_squared_loo_down";
  CK_REQUIRE(der && folds_host && folds, "%s: null pointer", who);
  CK_REQUIRE(n > 0 && B > 0 && der_elems > 0 && value_elems >= 0, "%s: bad sizes", who);
  CK_REQUIRE(H >= 1 && H <= kLdMaxH, "%s: %d children per fold, at most %d", who, H, kLdMaxH);
  CK_REQUIRE(Ki > 0 && Ki <= 1024 && Ko > 0 && Ko <= 1024, "%s: Ki=%d, Ko=%d", who, Ki, Ko);
  CK_REQUIRE(w ? num_weight_folds > 0 : Ki == Ko, "%s: %s", who, w ? "weight folds" : "a Hadamard layer has Ki = Ko");
  CK_REQUIRE(form == 0 || form == 1, "%s: form=%d", who, form);
  const int64_t in_words = static_cast<int64_t>(B) * Ko, out_words = static_cast<int64_t>(B) * Ki;
  const int64_t vec = complex_values ? 2 : 4;  // elements of 16 bytes: what the 32-unit form's vector accesses need of an offset
  bool all_top = true, any_down = false, aligned = ck::aligned16(values) && ck::aligned16(der);
  for (int f = 0; f < n; ++f) {  // the folds as the host knows them: every D inside its arena, every value that is read inside c's
    const int64_t* row = folds_host + static_cast<int64_t>(f) * (kLdHead + 2 * H);
    CK_REQUIRE(!w || (row[0] >= 0 && row[0] < num_weight_folds), "%s: fold %d: weight fold %lld of %d", who, f,
               static_cast<long long>(row[0]), num_weight_folds);
    CK_REQUIRE(row[1] == -1 || (row[1] >= 0 && row[1] + in_words <= der_elems), "%s: fold %d: D at %lld of %lld", who, f,
               static_cast<long long>(row[1]), static_cast<long long>(der_elems));
    all_top = all_top && row[1] == -1;
    aligned = aligned && (row[1] < 0 || row[1] % vec == 0);
    int nd = 0;
    for (int h = 0; h < H; ++h) nd += row[kLdHead + 2 * h] >= 0;
    for (int h = 0; h < H; ++h) {
      const int64_t d = row[kLdHead + 2 * h], o = row[kLdHead + 2 * h + 1];
      CK_REQUIRE(d == -1 || (d >= 0 && d + out_words <= der_elems), "%s: fold %d: child %d: D at %lld of %lld", who, f, h,
                 static_cast<long long>(d), static_cast<long long>(der_elems));
      const bool is_read = nd - (d >= 0 ? 1 : 0) > 0;  // (some OTHER slot is a down fold)
      CK_REQUIRE(!is_read || (values && o >= 0 && o + out_words <= value_elems), "%s: fold %d: child %d: value at %lld of %lld", who, f,
                 h, static_cast<long long>(o), static_cast<long long>(value_elems));
      aligned = aligned && (d < 0 || d % vec == 0) && (!is_read || o % vec == 0);
      any_down = any_down || d >= 0;
    }
  }
  CK_REQUIRE(any_down, "%s: no child is a down fold", who);
  const LdArgs a{values, der, folds, w, n, H, Ki, Ko, B};
  if (!w) {
    const int64_t blocks = (static_cast<int64_t>(n) * B * Ki + 255) / 256;
    CK_REQUIRE(blocks <= 0x7fffffffLL, "%s: %d folds x %d rows x %d units", who, n, B, Ki);
    return complex_values ? ld_dispatch<ld_hadamard_kernel<true>>(a, blocks, 0, stream) : ld_dispatch<ld_hadamard_kernel<false>>(a, blocks, 0, stream);
  }
  if (form == 0 && aligned && Ki == 32 && (Ko == 32 || (Ko == 1 && all_top))) {
    const int64_t blocks = static_cast<int64_t>(n) * ((B + 4 * kLdRows - 1) / (4 * kLdRows));
    CK_REQUIRE(blocks <= 0x7fffffffLL, "%s: %d folds x %d rows", who, n, B);
    return complex_values ? ld_dispatch<ld_down32_kernel<true>>(a, blocks, 0, stream) : ld_dispatch<ld_down32_kernel<false>>(a, blocks, 0, stream);
  }
  const size_t lds = (static_cast<size_t>(Ko) * Ki + static_cast<size_t>(kLdRows) * (Ko + 1)) * sizeof(float);
  if (lds > kLdMaxLds) return ck::fail(CK_ERR_UNSUPPORTED, "%s: a (%d, %d) weight matrix does not fit in LDS", who, Ko, Ki);
  const int64_t blocks = static_cast<int64_t>(n) * ((B + kLdRows - 1) / kLdRows);
  CK_REQUIRE(blocks <= 0x7fffffffLL, "%s: %d folds x %d rows", who, n, B);
  return complex_values ? ld_dispatch<ld_down_kernel<true>>(a, blocks, lds, stream) : ld_dispatch<ld_down_kernel<false>>(a, blocks, lds, stream);
}

extern "C" int ck_squared_loo_leaf(const float* der, int64_t der_elems, const int64_t* vars_host, const int64_t* vars, int nq, int C_max,
                                   const int64_t* x, int D, float* out, int mode, int B, int complex_values, void* stream) {
  const char* who = "ck_squared_loo_leaf";
  CK_REQUIRE(vars_host && vars && out, "%s: null pointer", who);
  CK_REQUIRE(nq > 0 && B > 0 && C_max > 0 && der_elems >= 0, "%s: bad sizes", who);
  CK_REQUIRE(mode >= 0 && mode <= 2 && (mode != 2 || (x && D > 0)), "%s: mode %d%s", who, mode, mode == 2 ? " needs the batch" : "");
  int maxC = 1, maxK = 1;
  for (int q = 0; q < nq; ++q) {
    const int64_t* row = vars_host + static_cast<int64_t>(q) * kLdLeaf;
    CK_REQUIRE(row[0] != 0 && row[1] > 0 && row[1] <= C_max && row[2] > 0 && row[2] <= 1024, "%s: variable %d: table, C=%lld, K=%lld", who, q,
               static_cast<long long>(row[1]), static_cast<long long>(row[2]));
    CK_REQUIRE(row[4] == -1 || (der && row[4] >= 0 && row[4] + static_cast<int64_t>(B) * row[2] <= der_elems), "%s: variable %d: D at %lld of %lld",
               who, q, static_cast<long long>(row[4]), static_cast<long long>(der_elems));
    CK_REQUIRE(mode != 2 || (row[5] >= 0 && row[5] < D), "%s: variable %d: column %lld of %d", who, q, static_cast<long long>(row[5]), D);
    maxC = std::max(maxC, static_cast<int>(row[1]));
    maxK = std::max(maxK, static_cast<int>(row[2]));
  }
  const auto lds_of = [&](int R) {
    return (sp_leaf_floats(maxC, maxK) - maxC + static_cast<size_t>(R) * (maxK + 1 + maxC)) * sizeof(float);
  };
  int R = kLdRows;  // rows of a workgroup: as many as fit beside the table (a row's result does not depend on it)
  while (R > 1 && lds_of(R) > kLdMaxLds / 2) R /= 2;
  if (lds_of(R) > kLdMaxLds) return ck::fail(CK_ERR_UNSUPPORTED, "%s: %d units, C=%d states do not fit in LDS", who, maxK, maxC);
  const int64_t blocks = static_cast<int64_t>(nq) * ((B + R - 1) / R);
  CK_REQUIRE(blocks <= 0x7fffffffLL, "%s: %d variables x %d rows", who, nq, B);
  const LdLeafArgs a{der, vars, x, out, nq, C_max, D, B, mode, R, maxC, maxK};
  return complex_values ? ld_dispatch<ld_leaf_kernel<true>>(a, blocks, lds_of(R), stream) : ld_dispatch<ld_leaf_kernel<false>>(a, blocks, lds_of(R), stream);
}
