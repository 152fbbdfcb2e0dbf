// Conditional sampling given evidence ("Conditional sampling"): each row n draws its unobserved
// variables from p(x_S | x_O) = c(x_O, x_S) / c(x_O).  The per-row log value of every unit under the row's evidence comes
// from the layer-wise marginal forward (one arena, (F, B, Ko) per layer); the walk weights each draw by those values, so the
// CDF rows depend on the sample and are built on the device, one wave per (fold, sample).
#include <math.h>

#include "ck_cond_policy.h"

using ck::CondDraw;  // (the walk policy: ck_cond_policy.h, shared with ck_soft_decode.hip)

int ck_sample_cond_walk(const ck_sample_layer* layers, const float* const* weights, int n_layers, int root_fold, int root_unit,
                        int total_folds, int S, const float* vals, const int64_t* val_off, int64_t row0, int64_t B, int64_t N,
                        int D, uint64_t seed, const void* ev, void* x, int x_float, void* stream) {
  const CondDraw p{static_cast<uint32_t>(seed), static_cast<uint32_t>(seed >> 32)};
  return ck::evidence_walk("ck_sample_cond_walk", layers, weights, n_layers, root_fold, root_unit, total_folds, S, vals,
                           val_off, row0, B, N, D, ev, x, x_float, p, stream);
}
