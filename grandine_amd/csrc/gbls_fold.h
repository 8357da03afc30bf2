// Verified folds (include/grandine_bls_gpu_fold.h): per group of the each-call's sets, the sum of
// the decoded signatures whose set verified.  Host and device code shared by k_fold.hip, the C ABI
// and tests/native/fold_harness.cpp (which compiles the accumulation and the finish for the CPU):
// the argument rules, one lane's share of a group, and the finish that lane 0 of a group runs.
#pragma once
#include <cstddef>
#include <cstdint>

#include "bls_curve.h"

namespace gbls {

// The groups' CSR: both arrays present, fold_off[0] == 0, non-decreasing, every named set < n; the
// outputs that every group writes are required.  nfold == 0 names nothing and asks for nothing.  A
// group count whose offsets (nfold + 1 words) would not fit 32 bits is refused.
inline bool fold_args_ok(const uint32_t *fold_set, const uint32_t *fold_off, size_t nfold, size_t n,
                         const void *fold_out, const void *fold_count) {
  if (nfold == 0) return true;
  if ((uint64_t)nfold >= 0xffffffffull) return false;
  if (!fold_off || !fold_set || !fold_out || !fold_count) return false;
  if (fold_off[0] != 0) return false;
  for (size_t g = 0; g < nfold; g++)
    if (fold_off[g + 1] < fold_off[g]) return false;
  const uint32_t cnt = fold_off[nfold];
  for (uint32_t i = 0; i < cnt; i++)
    if (fold_set[i] >= n) return false;
  return true;
}

// Lane `lane` of `lanes` takes the group's entries lane, lane + lanes, ...: every occurrence whose
// set verified adds its signature once (mixed addition: a point met twice doubles, opposite points
// cancel, infinity is absorbed) and counts once.
HD void fold_lane_sum(g2j &acc, uint32_t &cnt, const g2a *sigs, const int32_t *verdicts, const uint32_t *set,
                      uint32_t b, uint32_t e, uint32_t lane, uint32_t lanes) {
  jac_set_inf(acc);
  cnt = 0;
  for (uint32_t i = b + lane; i < e; i += lanes) {
    const uint32_t s = set[i];
    if (verdicts[s] != 0) continue;  // GBLS_SUCCESS only
    jac_add_aff(acc, acc, sigs[s]);
    cnt++;
  }
}

// The group's finish: one affine conversion, the point, its count and (bytes != nullptr) its
// compression; an infinite sum is the all-zero point and 0xc0 followed by zeros.
HD void fold_finish(const g2j &acc, uint32_t cnt, g2a *out, uint8_t *bytes, uint32_t *count) {
  g2a r;
  jac_to_aff(r, acc);
  *out = r;
  *count = cnt;
  if (bytes) g2_compress(bytes, r);
}

}  // namespace gbls
