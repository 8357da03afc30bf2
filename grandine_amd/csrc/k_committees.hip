// gfx950 kernel: per-set keys from cached committee sums (gbls_multi_verify_committees,
// gbls_g1_aggregate_committees).  An attestation's key is the sum of the committee members whose
// aggregation bit is set (helper_functions/src/accessors.rs:510-531, summed by
// Triple::verify_aggregate, helper_functions/src/verifier.rs:387-405); with the committee's whole
// sum C cached in a device table the key is C - S, S the sum of the few ABSENT members.
//
// Radix-32 arithmetic (bls_curve.h), the registry's own form: a list of a handful of keys costs
// less than the two conversions of every operand into the radix-2^28 form and back would, and the
// affine conversion (an inversion, the larger part of a short list's work) exists only in this
// layer.  Byte-identical to k_g1_aggregate_idx / k_aggregate_rows, which run the same formulas.
#include "gbls_common.h"
#include "gbls_committees.h"
#include "gbls_rowfold.h"

namespace gbls {

// ROW = false: one lane per set (short lists: the absentees of a well-attended committee).
// ROW = true: one 16-lane DPP row per set (long lists), each lane summing every 16th key, folded
// as in k_aggregate_rows; the row's lane 0 finishes the set.
template <bool ROW>
__global__ void __launch_bounds__(WG) k_g1_committee_keys(const g1a *reg, uint32_t nreg, const g1a *tab,
                                                          uint32_t ntab, const uint32_t *com,
                                                          const uint32_t *idx, const uint32_t *off,
                                                          uint32_t n, g1a *out, int32_t *st) {
  const uint32_t t = blockIdx.x * WG + threadIdx.x;
  const uint32_t s = ROW ? t >> 4 : t, r = ROW ? t & 15 : 0, step = ROW ? 16 : 1;
  if (s >= n) return;  // whole rows
  const uint32_t b = off[s], e = off[s + 1];
  g1j acc;
  jac_set_inf(acc);
  uint32_t bad = 0;
#pragma unroll 1
  for (uint32_t i = b + r; i < e; i += step) {
    const uint32_t v = idx[i];
    if (v >= nreg || aff_is_inf(reg[v]))  // out of range / invalid slot
      bad = 1;
    else
      jac_add_aff(acc, acc, reg[v]);
  }
  if constexpr (ROW) {
    jac_row_fold<1>(acc, bad);
    jac_row_fold<2>(acc, bad);
    jac_row_fold<4>(acc, bad);
    jac_row_fold<8>(acc, bad);
    if (r != 0) return;
  }
  uint32_t flags = (e == b ? CK_EMPTY : 0u) | (bad ? CK_BAD_INDEX : 0u);
  g1a C;
  fp_zero(C.x);
  fp_zero(C.y);
  const uint32_t c = com[s];
  if (c != kNoCommittee) {
    flags |= CK_COMMITTEE;
    if (c < ntab) C = tab[c];  // past the table: stays all-zero, an invalid slot
  }
  g1a key;
  st[s] = committee_key(key, C, acc, flags);
  out[s] = key;
}

void launch_g1_committee_keys(hipStream_t st, const g1a *reg, uint32_t nreg, const g1a *tab, uint32_t ntab,
                              const uint32_t *com, const uint32_t *idx, const uint32_t *off, uint32_t n,
                              uint32_t max_len, g1a *out, int32_t *status) {
  if (!n) return;
  if (max_len >= g_committee_row_min)
    k_g1_committee_keys<true><<<nblk(16 * (size_t)n), WG, 0, st>>>(reg, nreg, tab, ntab, com, idx, off, n,
                                                                 out, status);
  else
    k_g1_committee_keys<false><<<nblk(n), WG, 0, st>>>(reg, nreg, tab, ntab, com, idx, off, n, out, status);
}

}  // namespace gbls
