/* grandine_bls_gpu_bits.h -- aggregation-bit sets over resident committee members (an extension of
 * grandine_bls_gpu.h and grandine_bls_gpu_committees.h, whose conventions hold here: status codes,
 * fail-closed returns, gbls_last_error, segment-offset rules, thread safety).
 *
 * An attestation arrives as (committee, aggregation bits, signature), the sync aggregate as
 * (sync committee, Bitvector[512], signature).  With a committee's member list resident on the
 * device beside its cached sum, a set is the committee's 4-byte slot and the bits as they arrived:
 * no index list is built or uploaded, the engine checks that the bits fit the committee, and the
 * choice between summing the participants and subtracting the absentees from the cached sum is
 * made on the device, where the popcount is known.
 *
 *   gbls_committees_set_members  gbls_committees_set that also keeps each slot's member list
 *   gbls_g1_aggregate_bits       the key of each set: the sum of the members whose bit is set
 *   gbls_multi_verify_bits       MultiVerifier::finish (helper_functions/src/verifier.rs:301-323)
 *                                over such keys, mixed with plain registry-indexed sets
 */
#ifndef GRANDINE_BLS_GPU_BITS_H
#define GRANDINE_BLS_GPU_BITS_H

#include "grandine_bls_gpu.h"
#include "grandine_bls_gpu_committees.h"

#ifdef __cplusplus
extern "C" {
#endif

/* gbls_committees_set (same sums, statuses, growth, truncation on failure, ordering against
 * verifications in flight) that also keeps the member list of every slot it writes in device
 * memory, on every engine.  A slot whose status is not GBLS_SUCCESS keeps no members.
 * Members are dropped: of a slot, by a later gbls_committees_set on it (the sum stays); of every
 * slot, by gbls_committees_clear and by a gbls_registry_set with first < gbls_registry_size();
 * of the slots from `first` on, by a failure that truncates the table to `first`.
 * Memory: the indices of one call form one block per engine (4 bytes per member), held while any
 * slot written by that call still has its members from it, and freed behind the verifications
 * that may still read it.  Rewriting a whole range in one call, as an epoch rollover does,
 * releases the block of the call that wrote it before. */
int gbls_committees_set_members(size_t first, const uint32_t *idx, const uint32_t *off, size_t ncom,
                                int32_t *status);
size_t gbls_committees_members(size_t slot); /* member count kept for slot; 0: none kept (or no device) */

/* Key resolution of the two calls below.  Set i is one of two kinds.
 *
 * A COMMITTEE SET: com[i] names a slot that keeps m members.  Its bit string is
 * bits[bits_off[i] .. bits_off[i+1]) (byte offsets; bits_off follows the segment-offset rules over
 * n sets), in SSZ bit order: bit j is  bits[j >> 3] >> (j & 7) & 1.  Either SSZ encoding is
 * accepted, told apart without a flag:
 *   Bitvector[m]  exactly ceil(m/8) bytes, every bit at a position >= m zero (the sync aggregate)
 *   Bitlist       exactly m/8 + 1 bytes, the delimiter bit at position m set, every bit above it
 *                 zero (an attestation's aggregation_bits)
 * When m % 8 != 0 the two lengths coincide and bit m decides.  Anything else is GBLS_BAD_ENCODING
 * for that set: another length, a bit above the delimiter or (without one) at a position > m, the
 * long form without its delimiter.  So the engine enforces len(aggregation_bits) ==
 * len(committee) per set, and a key is by construction a subset sum of the committee:
 *   key_i = sum of registry[member_j] over the bits j < m that are set.
 * How the sum is formed (from the cached sum minus the members whose bit is clear when those are
 * the fewer, else from the participants) is not observable in the bytes.  No bit set: the key is
 * infinite, written all-zero with GBLS_SUCCESS, and a verification rejects it as every infinite
 * key.  GBLS_BAD_ENCODING, whatever the bits say: a slot past the table, an invalid slot, a slot
 * that keeps no members (loaded by gbls_committees_set, or dropped since).  A committee whose
 * WHOLE sum is infinite is an invalid slot (gbls_committees_set stores it all-zero), so its sets
 * are GBLS_BAD_ENCODING even when the selected members' sum is finite.
 * The set's pk_off range must be empty (GBLS_ERR_ARG otherwise).
 *
 * A PLAIN SET: com[i] == GBLS_NO_COMMITTEE.  Exactly as in gbls_multi_verify_committees: the sum
 * of registry[pk_idx[pk_off[i] .. pk_off[i+1])]; an empty list is GBLS_AGGR_TYPE_MISMATCH, a bad
 * index GBLS_BAD_ENCODING.  Its bit range must be empty (GBLS_ERR_ARG otherwise).  A block's
 * MultiVerifier::finish mixes attestations with the proposer, RANDAO and exit signatures: these
 * are its plain sets.  pk_idx / pk_off may be NULL when no set is plain. */
int gbls_g1_aggregate_bits(const uint32_t *com, const uint8_t *bits, const uint32_t *bits_off,
                           const uint32_t *pk_idx, const uint32_t *pk_off, size_t n,
                           gbls_p1_affine *out, int32_t *status);
/* gbls_multi_verify_committees over the keys above: compressed signatures decoded in the same
 * submission, sig_status filled and the first decoding error returned before the verdict,
 * GBLS_CALL_BLOCK honoured, n == 0 -> GBLS_VERIFY_FAIL, large batches sharded over the engines
 * (each shard uploads its slice of bits).  A set whose key status is nonzero fails the batch, and
 * so does an infinite key.  GBLS_INIT_DEDUP and the message line cache apply unchanged (sets are
 * grouped by message after their keys are resolved).  This call is NOT merged with concurrent
 * callers by the coalescer, as the committees call is not: it always runs as its own submission. */
int gbls_multi_verify_bits(const uint8_t (*msgs)[32], const uint8_t (*sigs)[96],
                           const uint32_t *com, const uint8_t *bits, const uint32_t *bits_off,
                           const uint32_t *pk_idx, const uint32_t *pk_off,
                           const uint64_t *rands, size_t n, int32_t *sig_status,
                           uint32_t call_flags);

#ifdef __cplusplus
}
#endif
#endif
