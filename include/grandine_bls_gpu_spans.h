/* grandine_bls_gpu_spans.h -- span sets: attestations over several committees (an extension of
 * grandine_bls_gpu_bits.h, whose conventions hold here: status codes, fail-closed pre-fill of the
 * outputs, gbls_last_error, segment-offset rules, thread safety).
 *
 * Since EIP-7549 an on-chain attestation is (committee_bits, aggregation_bits, signature):
 * committee_bits is a Bitvector[64] naming the committees of the slot that attested, and
 * aggregation_bits is ONE Bitlist, the concatenation of the named committees' bits in ascending
 * committee order.  With the slot's committees loaded into consecutive table slots by
 * gbls_committees_set_members, such a set is the base slot, the 8 bytes of committee_bits and the
 * bit string as it arrived.  The engine cuts each set into one piece per named committee, forms
 * every piece in its committee's cheaper direction (participants, or the cached sum minus the
 * absentees), and folds the pieces into the set's key.
 *
 *   gbls_g1_aggregate_spans   the key of each set
 *   gbls_multi_verify_spans   MultiVerifier::finish (helper_functions/src/verifier.rs:301-323)
 *                             over such keys, mixed with plain registry-indexed sets
 */
#ifndef GRANDINE_BLS_GPU_SPANS_H
#define GRANDINE_BLS_GPU_SPANS_H

#include "grandine_bls_gpu_bits.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Key resolution of the two calls below.  Set i is one of two kinds.
 *
 * A SPAN SET: com[i] is a base slot of the committee table and cbits[i] the SSZ bytes of
 * committee_bits: bit c is  cbits[i][c >> 3] >> (c & 7) & 1.  Each set bit c, in ascending order,
 * names slot com[i] + c, which must keep members (gbls_committees_set_members).  With m_c the
 * member count of the slot that bit c names and M the sum of the m_c, the bit string
 * bits[bits_off[i] .. bits_off[i+1]) is judged over M members exactly as a committee set's string
 * is judged over m in grandine_bls_gpu_bits.h: either SSZ encoding, every malformed form rejected.
 * This is the spec's len(aggregation_bits) == committee_offset.  Committee c's members take the
 * m_c bits that start at the sum of the earlier named committees' counts, and
 *   key_i = sum over the named committees of the sum of the members whose bit is set.
 * GBLS_BAD_ENCODING for the set, its key all-zero:
 *   cbits[i] all zero;
 *   a named slot past the table (com[i] + c is formed without 32-bit wrap-around), invalid, or
 *   keeping no members;
 *   a malformed string;
 *   A NAMED COMMITTEE WITHOUT A PARTICIPANT.  The spec asserts that every named committee has an
 *   attester.  This deliberately DIFFERS from gbls_multi_verify_bits, where a committee set with no
 *   bit set is an infinite key with GBLS_SUCCESS.
 * Contributions of committees that all have participants may still cancel to infinity: the key is
 * then all-zero with GBLS_SUCCESS, and a verification rejects it as every infinite key.
 * The set's pk_off range must be empty (GBLS_ERR_ARG otherwise).
 * The engine does not know the epoch's committee count: checking committee_index <
 * committees_per_slot stays with the caller (one mask compare on committee_bits).
 * A single-committee Bitvector set, such as the sync aggregate, is a span set with one bit.
 *
 * A PLAIN SET: com[i] == GBLS_NO_COMMITTEE.  Exactly as in gbls_multi_verify_bits.  cbits[i] must
 * be all zero and its bit range empty (GBLS_ERR_ARG otherwise).  pk_idx / pk_off may be NULL when
 * no set is plain.
 *
 * A call whose sets name more than 2^32 - 1 committees and plain lists in total is GBLS_ERR_ARG. */
int gbls_g1_aggregate_spans(const uint32_t *com, const uint8_t (*cbits)[8], const uint8_t *bits,
                            const uint32_t *bits_off, const uint32_t *pk_idx, const uint32_t *pk_off,
                            size_t n, gbls_p1_affine *out, int32_t *status);
/* gbls_multi_verify_bits over the keys above: compressed signatures decoded in the same
 * submission, sig_status filled and the first decoding error returned before the verdict,
 * GBLS_CALL_BLOCK honoured, n == 0 -> GBLS_VERIFY_FAIL, large one-segment batches sharded over the
 * engines (each shard uploads its slice).  A set whose key status is nonzero fails the batch, and
 * so does an infinite key.  GBLS_INIT_DEDUP and the message line cache apply unchanged.  This call
 * is NOT merged with concurrent callers by the coalescer, as the bits call is not: it always runs
 * as its own submission. */
int gbls_multi_verify_spans(const uint8_t (*msgs)[32], const uint8_t (*sigs)[96], const uint32_t *com,
                            const uint8_t (*cbits)[8], const uint8_t *bits, const uint32_t *bits_off,
                            const uint32_t *pk_idx, const uint32_t *pk_off, const uint64_t *rands,
                            size_t n, int32_t *sig_status, uint32_t call_flags);

#ifdef __cplusplus
}
#endif
#endif
