// Shared by the two translation units of the bucket MSM (k_msm.hip, k_msm_w4.hip): device code,
// included after gbls_common.h.
#pragma once
#include "gbls_common.h"

namespace gbls {

// the constant G1 half of an extra pair: table entry k (x, y Montgomery), c = 1
__device__ __forceinline__ void msm_weight(g1s &o, const uint32_t *table, uint32_t k) {
#pragma unroll
  for (int i = 0; i < 12; i++) {
    o.x.l[i] = table[24 * k + i];
    o.y.l[i] = table[24 * k + 12 + i];
  }
  fp_one(o.c);
}
// k_msm_w4.hip -- c = 5: the window sums S(s, w) = sum_b (b + 1) X(s, w, b) of nwin = nseg * W
// windows (16 buckets each) from the buckets' chunk partials, one workgroup per window; pair
// xb + t of window t = s * W + w: P = -[2^(5 w)] g1, and S Jacobian into Sj[t] or, Sj null,
// affine into H[xb + t]
void launch_msm_windows_w4(hipStream_t st, const g2j *chunk, const uint32_t *cstart, uint32_t nwin, uint32_t W,
                           bool r28, uint32_t xb, const uint32_t *seg_off, int empty_is_error, g1s *P, g2a *H,
                           int32_t *seg_err, g2j *Sj);

}  // namespace gbls
