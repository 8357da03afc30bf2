// Cached committee key sums: the per-set step of k_g1_committee_keys (k_committees.hip), as
// __host__ __device__ text so that tests/native/committees_harness.cpp compiles the same lines for
// the CPU.
//
// A set names a cached committee sum C (an affine table slot) and a list of registry keys whose
// sum S the kernel has accumulated; its key is C - S.  Without a committee (GBLS_NO_COMMITTEE) the
// key is S, as k_g1_aggregate_idx forms it.  The engine does not check that the listed keys are
// members of the committee: the key is whatever the formula gives, so the arithmetic is complete
// (jac_add_aff recomputes S = -C as a doubling and S = C as the identity).
#pragma once
#include "bls_curve.h"

namespace gbls {

constexpr uint32_t kNoCommittee = 0xffffffffu;  // GBLS_NO_COMMITTEE
constexpr size_t kMaxCommittees = (size_t)1 << 20;

enum : uint32_t {
  CK_COMMITTEE = 1,  // the set names a committee slot (C: the slot, all-zero when out of range)
  CK_EMPTY = 2,      // its key list is empty
  CK_BAD_INDEX = 4,  // a listed index is past the registry or names an invalid / unloaded key
};

// The direction of a set whose participants are known (aggregation bits, gbls_bits.h): with p of a
// committee's m members participating, the key is formed as C minus the m - p absentees when those
// are the fewer, else as the participants' sum; a tie goes to the participants (the measured rule of
// the committees call, verifier.ABSENTEE_FORM_MAX_RATIO = 1).  p == m subtracts nothing: the key
// is C itself.
HD bool committee_subtracts(uint32_t m, uint32_t p) { return m - p < p; }

// key = C - S (CK_COMMITTEE) or S; returns the set's status and writes all-zero on a rejection.
//   BAD_ENCODING        a bad index, or a committee slot that is invalid (all-zero: never written,
//                       written with a nonzero status, an infinite sum) or past the table
//   AGGR_TYPE_MISMATCH  an empty list without a committee
// A committee with an empty list (full participation) is the cached sum itself, no inversion.
// An infinite key (every member absent) is a SUCCESS written all-zero, as in k_g1_aggregate_idx;
// the verification paths reject infinite keys.
HD int32_t committee_key(g1a &key, const g1a &C, const g1j &S, uint32_t flags) {
  int32_t status = ST_SUCCESS;
  if ((flags & CK_BAD_INDEX) || ((flags & CK_COMMITTEE) && aff_is_inf(C)))
    status = ST_BAD_ENCODING;
  else if (!(flags & CK_COMMITTEE) && (flags & CK_EMPTY))
    status = ST_AGGR_TYPE_MISMATCH;
  if (status != ST_SUCCESS) {
    fp_zero(key.x);
    fp_zero(key.y);
    return status;
  }
  if ((flags & CK_COMMITTEE) && (flags & CK_EMPTY)) {
    key = C;
    return ST_SUCCESS;
  }
  g1j t = S;
  if (flags & CK_COMMITTEE) {
    jac_neg(t, S);
    jac_add_aff(t, t, C);
  }
  jac_to_aff(key, t);
  return ST_SUCCESS;
}

}  // namespace gbls
