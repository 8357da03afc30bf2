// gfx950 kernels: verified folds (gbls_fold.h).  Behind the each-call's verdicts, group g sums the
// decoded signatures of its named sets whose verdict is GBLS_SUCCESS; the group's lane 0 converts
// the sum to affine once and writes the point, its count and its compression in the same kernel.
#include "gbls_common.h"
#include "bls_w4.h"
#include "gbls_fold.h"
#include "gbls_rowfold.h"

namespace gbls {

// Many short groups: one DPP row (16 lanes) per group, as k_aggregate_rows.  Each lane sums every
// 16th passing member with mixed additions, the row folds its partial sums and counts in 4
// row_shl steps (lanes past the row end read zeros: infinity, count 0).
template <bool X>
__global__ void __launch_bounds__(WG) k_g2_fold_rows(const g2a *sigs, const int32_t *verdicts,
                                                     const uint32_t *set, const uint32_t *off, uint32_t nfold,
                                                     g2a *out, uint8_t *bytes, uint32_t *count) {
  if constexpr (X) w4::exclusive_simd();
  const uint32_t t = blockIdx.x * WG + threadIdx.x;
  const uint32_t g = t >> 4, r = t & 15;
  if (g >= nfold) return;  // whole rows
  g2j acc;
  uint32_t cnt, none = 0;
  fold_lane_sum(acc, cnt, sigs, verdicts, set, off[g], off[g + 1], r, 16);
  jac_row_fold<1>(acc, none);
  cnt += row_shl<1>(cnt);
  jac_row_fold<2>(acc, none);
  cnt += row_shl<2>(cnt);
  jac_row_fold<4>(acc, none);
  cnt += row_shl<4>(cnt);
  jac_row_fold<8>(acc, none);
  cnt += row_shl<8>(cnt);
  if (r != 0) return;
  fold_finish(acc, cnt, &out[g], bytes ? bytes + 96u * g : nullptr, &count[g]);
}

// A few long groups (a 2048-member committee, a 512-member sync committee): one 256-lane workgroup
// per group, an LDS tree over the lanes' partial sums.  A Jacobian G2 point is 72 words: at that
// lane stride (8 mod 64) every eighth lane's word k shares a bank.  The count rides in a 73rd word,
// and the odd stride spreads a wave's lanes over all banks.
struct g2j_lds {
  g2j v;
  uint32_t cnt;
};
static_assert(sizeof(g2j_lds) == 73 * 4, "odd LDS stride");

__global__ void __launch_bounds__(WGR) k_g2_fold_wg(const g2a *sigs, const int32_t *verdicts, const uint32_t *set,
                                                    const uint32_t *off, uint32_t nfold, g2a *out, uint8_t *bytes,
                                                    uint32_t *count) {
  __shared__ g2j_lds buf[WGR / 2];
  const uint32_t g = blockIdx.x;
  if (g >= nfold) return;  // (uniform per workgroup)
  g2j acc;
  uint32_t cnt;
  fold_lane_sum(acc, cnt, sigs, verdicts, set, off[g], off[g + 1], threadIdx.x, WGR);
  for (int w = WGR / 2; w > 0; w >>= 1) {
    __syncthreads();
    if (threadIdx.x >= (unsigned)w && threadIdx.x < (unsigned)2 * w) {
      buf[threadIdx.x - w].v = acc;
      buf[threadIdx.x - w].cnt = cnt;
    }
    __syncthreads();
    if (threadIdx.x < (unsigned)w) {
      g2j o = buf[threadIdx.x].v;
      jac_add(acc, acc, o);
      cnt += buf[threadIdx.x].cnt;
    }
  }
  if (threadIdx.x != 0) return;
  fold_finish(acc, cnt, &out[g], bytes ? bytes + 96u * g : nullptr, &count[g]);
}

// rows for many groups, the workgroup form for a few (the switch of launch_g2_aggregate_seg)
void launch_g2_fold(hipStream_t st, const g2a *sigs, const int32_t *verdicts, const uint32_t *set,
                    const uint32_t *off, uint32_t nfold, g2a *out, uint8_t *bytes, uint32_t *count) {
  if (nfold >= kRowAggregateMinSegs)
    (nblk(16 * (size_t)nfold) <= w4::kExclusiveMaxWaves ? k_g2_fold_rows<true> : k_g2_fold_rows<false>)<<<
        nblk(16 * (size_t)nfold), WG, 0, st>>>(sigs, verdicts, set, off, nfold, out, bytes, count);
  else if (nfold)
    k_g2_fold_wg<<<nfold, WGR, 0, st>>>(sigs, verdicts, set, off, nfold, out, bytes, count);
}

}  // namespace gbls
