/* grandine_bls_gpu_each.h -- per-set and per-item verdicts over span sets (an extension of
 * grandine_bls_gpu_spans.h, whose set description and conventions hold here unchanged: the two kinds
 * of sets, every rejection, the GBLS_ERR_ARG cases, status codes, gbls_last_error, segment-offset
 * rules, thread safety).
 *
 * The batch call of grandine_bls_gpu_spans.h gives one verdict for one batch and runs as its own
 * submission.  The two calls here give the verdicts a node needs around it, over the same compact
 * sets (base slot, 8 bytes of committee_bits, the bit string as it arrived):
 *
 *   gbls_verify_each_spans    which sets of a failed batch verify on their own
 *                             (p2p/src/attestation_verifier.rs:228-240, 373-386: the per-item
 *                             fallback, without returning to explicit key points)
 *   gbls_verify_items_spans   several independent batches in one submission: the blocks of the
 *                             block verification pool, or gossip aggregates as 3-set items
 *                             (selection proof, aggregate-and-proof signature, attestation)
 *
 * Both ARE merged with concurrent callers of the same call by the coalescer: requests over span sets
 * join only requests over span sets, single checks only single checks, block-class calls only
 * block-class calls; every caller gets exactly its own verdicts and statuses.
 *
 * Outputs, both calls.  Before anything else verdicts is filled with GBLS_VERIFY_FAIL and both
 * status arrays with GBLS_BAD_ENCODING (fail closed).  Returns GBLS_SUCCESS when every output was
 * written, else GBLS_VERIFY_FAIL with gbls_last_error() set and the outputs back at that pre-fill.
 * n == 0 or nseg == 0 returns GBLS_SUCCESS and writes nothing further.  All three output arrays are
 * required (GBLS_ERR_ARG).
 *   sig_status[i]  the decompression status of signature i, as the batch call reports it.
 *   key_status[i]  the status the key call of grandine_bls_gpu_spans.h gives set i: 0 for a valid
 *                  key AND for a key that cancels to infinity; GBLS_BAD_ENCODING for every rejection
 *                  listed there (so a malformed attestation is told from an invalid signature) and
 *                  for a bad registry index; GBLS_AGGR_TYPE_MISMATCH for an empty plain list.
 * GBLS_INIT_DEDUP, the message line cache and GBLS_INIT_PER_CHECK apply as they do to
 * gbls_multi_verify_segments (the items call) and gbls_verify_batch_compressed (the each-call).
 */
#ifndef GRANDINE_BLS_GPU_EACH_H
#define GRANDINE_BLS_GPU_EACH_H

#include "grandine_bls_gpu_spans.h"

#ifdef __cplusplus
extern "C" {
#endif

/* n independent checks, Signature::verify / fast_aggregate_verify semantics per set (r_i = 1,
 * signature subgroup check, infinite key rejected), ONE submission.  verdicts[i] is GBLS_SUCCESS
 * iff the signature decodes, it is in the subgroup, key_status[i] is 0 with a key that is not
 * infinite, and the pairing check holds.  One bad set never changes a neighbour's outputs.
 * From 2048 checks on the grouped path of gbls_fast_aggregate_verify_batch runs (unless
 * GBLS_INIT_PER_CHECK): checks are first verified in groups under secret random 64-bit weights and
 * every member of a failed group is re-checked on its own, so a valid check always passes and an
 * invalid one passes only if its group's weighted product is 1 by accident, with probability about
 * 2^-64 (the random-linear-combination soundness of Signature::multi_verify). */
int gbls_verify_each_spans(const uint8_t (*msgs)[32], const uint8_t (*sigs)[96], const uint32_t *com,
                           const uint8_t (*cbits)[8], const uint8_t *bits, const uint32_t *bits_off,
                           const uint32_t *pk_idx, const uint32_t *pk_off, size_t n, int32_t *sig_status,
                           int32_t *key_status, int32_t *verdicts);

/* nseg independent random-linear-combination batches ("items"): sets [seg_off[s], seg_off[s+1])
 * form item s, one verdict per item.  verdicts[s] is what the batch call would return for item s
 * alone, reduced to GBLS_SUCCESS / GBLS_VERIFY_FAIL: a signature that does not decode shows in
 * sig_status and fails its item, a rejected or infinite key shows in key_status (the former) and
 * fails its item, and no item changes another's verdict.  As in gbls_multi_verify_segments, an
 * EMPTY item (seg_off[s] == seg_off[s+1]) is GBLS_VERIFY_FAIL, and a ZERO scalar fails its item
 * (the reference only draws NonZeroU64).  rands and seg_off are required.  GBLS_CALL_BLOCK in
 * call_flags is honoured. */
int gbls_verify_items_spans(const uint8_t (*msgs)[32], const uint8_t (*sigs)[96], const uint32_t *com,
                            const uint8_t (*cbits)[8], const uint8_t *bits, const uint32_t *bits_off,
                            const uint32_t *pk_idx, const uint32_t *pk_off, const uint64_t *rands, size_t n,
                            const uint32_t *seg_off, size_t nseg, int32_t *sig_status, int32_t *key_status,
                            int32_t *verdicts, uint32_t call_flags);

#ifdef __cplusplus
}
#endif
#endif
