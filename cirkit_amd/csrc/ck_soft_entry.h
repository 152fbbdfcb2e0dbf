// The per-fold entry of a soft-variable set (cirkit_amd/soft_evidence.py, `SoftEvidenceState._build_set`), read by the
// posterior leaf (ck_soft.hip) and the decode leaf (ck_soft_decode.hip), DESIGN.md section 11 "Soft evidence".
#pragma once

#include <stdint.h>

namespace ck {

// Per soft variable s the entries qstart[s] .. qstart[s + 1] - 1, one per input fold over it, six int64 each.
struct SoftEntry {
  int64_t g, K, C;  // global fold, units, states
  const float* table;  // the fold's (C + 1, K) log table
  int64_t lin_off;     // element offset of its (K, C) block in linT
  int64_t mt_off;      // element offset of its K maxima in mt
};
static_assert(sizeof(SoftEntry) == 6 * sizeof(int64_t), "six int64 per entry");

}  // namespace ck
