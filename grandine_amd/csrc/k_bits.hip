// gfx950 kernel: per-set keys from aggregation bits over resident committee members
// (gbls_multi_verify_bits, gbls_g1_aggregate_bits).  An attestation is (committee, aggregation
// bits, signature); with the committee's member list resident beside its cached sum the set is a
// slot and the bits as they arrived, and the choice between summing the participants and
// subtracting the absentees from the cached sum is made here, from the masked popcount.
//
// Radix-32 arithmetic and committee_key as the finish, as k_g1_committee_keys: the registry is
// stored in that form and the affine bytes equal those of every other key path.
#include "gbls_common.h"
#include "gbls_bits.h"
#include "gbls_rowfold.h"

namespace gbls {

// ROW = false: one lane per set.  ROW = true: one 16-lane DPP row per set, lane r taking members
// j = r (mod 16) (list entries for a plain set), folded as in k_aggregate_rows; the row's lane 0
// finishes the set.  Every lane of a row reads the set's descriptor and scans its whole bit row,
// so validity, popcount and direction are the same in all 16 lanes without an exchange.
template <bool ROW>
__global__ void __launch_bounds__(WG) k_g1_bits_keys(const g1a *reg, uint32_t nreg, const g1a *tab,
                                                     uint32_t ntab, const BitSet *sets, const uint32_t *rows,
                                                     uint32_t n, g1a *out, int32_t *st) {
  const uint32_t t = blockIdx.x * WG + threadIdx.x;
  const uint32_t s = ROW ? t >> 4 : t, r = ROW ? t & 15 : 0, lanes = ROW ? 16 : 1;
  if (s >= n) return;  // whole rows
  const BitSet d = sets[s];
  const bool committee = d.slot != kNoCommittee;
  const uint32_t *row = rows + d.row;
  uint32_t bad = 0, p = 0;
  bool subtract = false;
  if (committee) {
    if (!d.list || !bits_check(row, d.nbytes, d.cnt, &p)) bad = 1;
    subtract = committee_subtracts(d.cnt, p);
  }
  const uint32_t m = bad ? 0 : d.cnt;
  // a committee set walks its words (each lane its own bits of every word), a plain set its list
  const uint32_t end = committee ? (m + 31) / 32 : m, step = committee ? 1 : lanes;
  g1j acc;
  jac_set_inf(acc);
#pragma unroll 1
  for (uint32_t i = committee ? 0 : r; i < end; i += step) {
    uint32_t sel = committee ? bits_select(row[i], m, i, subtract, r, lanes) : 1u;
    const uint32_t base = committee ? 32 * i : i;
#pragma unroll 1
    while (sel) {
      const uint32_t v = d.list[base + bits_ctz(sel)];
      sel &= sel - 1;
      if (v >= nreg || aff_is_inf(reg[v]))  // out of range / invalid slot
        bad = 1;
      else
        jac_add_aff(acc, acc, reg[v]);
    }
  }
  if constexpr (ROW) {  // whole rows reach every fold, whatever their lanes added
    jac_row_fold<1>(acc, bad);
    jac_row_fold<2>(acc, bad);
    jac_row_fold<4>(acc, bad);
    jac_row_fold<8>(acc, bad);
    if (r != 0) return;
  }
  g1a C;
  fp_zero(C.x);
  fp_zero(C.y);
  if (committee && d.slot < ntab) C = tab[d.slot];  // past the table: stays all-zero, an invalid slot
  g1a key;
  st[s] = bits_key(key, C, acc, committee, subtract, d.cnt, p, bad);
  out[s] = key;
}

void launch_g1_bits_keys(hipStream_t st, const g1a *reg, uint32_t nreg, const g1a *tab, uint32_t ntab,
                         const void *sets, const uint32_t *rows, uint32_t n, uint32_t max_work, g1a *out,
                         int32_t *status) {
  if (!n) return;
  const BitSet *bs = static_cast<const BitSet *>(sets);
  if (max_work >= g_committee_row_min)
    k_g1_bits_keys<true><<<nblk(16 * (size_t)n), WG, 0, st>>>(reg, nreg, tab, ntab, bs, rows, n, out, status);
  else
    k_g1_bits_keys<false><<<nblk(n), WG, 0, st>>>(reg, nreg, tab, ntab, bs, rows, n, out, status);
}

}  // namespace gbls
