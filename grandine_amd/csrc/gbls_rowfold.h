// 16-lane DPP row folds of Jacobian partial sums (k_aggregate_rows in k_keys.hip, the cooperative
// form of k_g1_committee_keys in k_committees.hip): VALU moves, no LDS, no barrier.
#pragma once
#include "gbls_common.h"

namespace gbls {

template <int K>
__device__ __forceinline__ uint32_t row_shl(uint32_t v) {
  return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x100 + K, 0xf, 0xf, true);
}
template <int K, class F>
__device__ __forceinline__ void jac_row_fold(jac<F> &acc, uint32_t &flag) {
  jac<F> o;
  uint32_t *d = reinterpret_cast<uint32_t *>(&o);
  const uint32_t *a = reinterpret_cast<const uint32_t *>(&acc);
#pragma unroll
  for (int i = 0; i < (int)(sizeof(jac<F>) / 4); i++) d[i] = row_shl<K>(a[i]);
  flag |= row_shl<K>(flag);
  jac_add(acc, acc, o);  // lanes past the row end read zeros: infinity
}

}  // namespace gbls
