/* grandine_bls_gpu_committees.h -- cached committee key sums (an extension of grandine_bls_gpu.h,
 * whose conventions hold here: status codes, fail-closed returns, gbls_last_error, segment-offset
 * rules, thread safety).
 *
 * An attestation's key is the sum of the committee members whose aggregation bit is set; the sync
 * aggregate's key is the same over the 512 keys of current_sync_committee.  A committee is fixed
 * for an epoch (the sync committee for 256) and named by every aggregator, every block that
 * includes its attestations and every block's sync aggregate, and participation is high.  With
 * the committee's whole sum C cached on the device, a set's key is C minus the sum of its few
 * ABSENT members: a handful of additions instead of hundreds.
 *
 *   gbls_committees_set           the per-epoch committee computation (beacon_committee,
 *                                 helper_functions/src/accessors.rs:510-531) and
 *                                 current_sync_committee (transition_functions/src/altair/
 *                                 block_processing.rs:516-535): one cached sum per committee
 *   gbls_g1_aggregate_committees  Triple::verify_aggregate's key sum (helper_functions/src/
 *                                 verifier.rs:387-405) formed by subtraction
 *   gbls_multi_verify_committees  MultiVerifier::finish (verifier.rs:301-323) over such keys
 */
#ifndef GRANDINE_BLS_GPU_COMMITTEES_H
#define GRANDINE_BLS_GPU_COMMITTEES_H

#include "grandine_bls_gpu.h"

#ifdef __cplusplus
extern "C" {
#endif

/* a set that names no committee: its key is the plain sum of its index list */
#define GBLS_NO_COMMITTEE 0xffffffffu

/* Committee table: slot first+c holds  sum of registry[idx[off[c] .. off[c+1])], c < ncom.
 * Device-resident, replicated on every engine like the registry (each engine sums the slots from
 * its own registry replica).  off follows the segment-offset rules (else GBLS_ERR_ARG).
 * status[c]: GBLS_SUCCESS; GBLS_AGGR_TYPE_MISMATCH for an empty committee; GBLS_BAD_ENCODING for
 * an index past the registry or naming an invalid or unloaded key.  A slot stored all-zero is
 * INVALID: a slot whose status is not GBLS_SUCCESS, a slot between the old size and `first` that
 * was never written, and a slot whose sum is the point at infinity.
 * The table grows as needed, up to 2^20 slots (beyond: GBLS_ERR_ARG).  Rewriting a slot is
 * allowed (an epoch rollover reuses slots) and is ordered against verifications in flight exactly
 * as a registry write is: those already submitted read the old sum, later ones wait for the new
 * one on the device.  A sum is a snapshot of the registry at the time of the call: any
 * gbls_registry_set with first < gbls_registry_size() (it rewrites loaded keys) clears the whole
 * table (size 0); appends keep it.  On an engine failure the table is truncated to `first`, as
 * the registry is. */
int gbls_committees_set(size_t first, const uint32_t *idx, const uint32_t *off, size_t ncom,
                        int32_t *status);
size_t gbls_committees_size(void); /* slots; 0 without a device */
int gbls_committees_clear(void);

/* Key resolution of the two calls below; pk_off is required (segment-offset rules over n sets).
 * key_i = committee[com[i]] - sum registry[pk_idx[pk_off[i] .. pk_off[i+1])]   (com[i] != NO_COMMITTEE)
 *       = sum registry[pk_idx[pk_off[i] .. pk_off[i+1])]                       (com[i] == NO_COMMITTEE)
 * A committee set's list names the ABSENT members; an empty list is full participation and the
 * key is the cached sum.  com[i] >= gbls_committees_size() or an invalid slot is
 * GBLS_BAD_ENCODING for that set.  A NO_COMMITTEE set behaves exactly as in
 * gbls_multi_verify_compressed_ex with pk_idx + pk_off (an empty list: GBLS_AGGR_TYPE_MISMATCH).
 * An index past the registry or naming an invalid key is GBLS_BAD_ENCODING.  The engine does NOT
 * check that the listed keys are members of the committee: the key is whatever the formula gives,
 * computed exactly also when the list sums to the committee's sum (the key is infinity, written
 * all-zero with GBLS_SUCCESS) or to its negative (the key is twice the sum). */
int gbls_g1_aggregate_committees(const uint32_t *com, const uint32_t *pk_idx, const uint32_t *pk_off,
                                 size_t n, gbls_p1_affine *out, int32_t *status);
/* gbls_multi_verify_compressed_ex with the keys above: compressed signatures decoded in the same
 * submission, sig_status filled and the first decoding error returned before the verdict,
 * GBLS_CALL_BLOCK honoured, n == 0 -> GBLS_VERIFY_FAIL, large batches sharded over the engines.
 * A set whose key status is nonzero fails the batch, and so does an infinite key (every member
 * absent), as every infinite key does.  GBLS_INIT_DEDUP applies unchanged (sets are grouped by
 * message after their keys are resolved).  This call is NOT merged with concurrent callers by the
 * coalescer: it always runs as its own submission, as every call does under
 * GBLS_INIT_NO_COALESCE. */
int gbls_multi_verify_committees(const uint8_t (*msgs)[32], const uint8_t (*sigs)[96],
                                 const uint32_t *com, const uint32_t *pk_idx, const uint32_t *pk_off,
                                 const uint64_t *rands, size_t n, int32_t *sig_status,
                                 uint32_t call_flags);

#ifdef __cplusplus
}
#endif
#endif
