/* grandine_bls_gpu_fold.h -- verified folds: the each-call of grandine_bls_gpu_each.h, which also
 * sums the signatures that passed (an extension of that header, whose conventions hold here
 * unchanged: the sets, every rejection, the GBLS_ERR_ARG cases, status codes, gbls_last_error,
 * offset rules, thread safety, the grouped regime from 2048 checks, GBLS_INIT_PER_CHECK and the
 * message line cache).
 *
 * A node that has verified single attestations or sync-committee messages goes on to aggregate the
 * ones that passed (operation_pools/src/attestation_agg_pool/tasks.rs:242-257 aggregate_attestation,
 * operation_pools/src/sync_committee_agg_pool/pool.rs:114,190, validator/src/validator.rs:2937).
 * The verifying submission has already decoded and subgroup-checked every signature, and the points
 * are still in device memory when the verdicts are written.  gbls_verify_each_fold therefore also
 * takes GROUPS of its own sets and returns, per group, the sum of the signatures whose set
 * verified, computed on the device behind the verdicts.  The signatures never leave the device, and
 * nothing is decoded a second time.
 *
 * Groups.  Group g names the sets fold_set[fold_off[g] .. fold_off[g+1]), CSR like every other
 * offset array here.  A set may be in several groups (an attestation pool adds one single to every
 * aggregate that lacks its bit), and a set may be named more than once in one group: each
 * occurrence adds once.  An empty group is legal.
 *
 * Outputs, beside the each-call's three arrays.
 *   fold_out[g]    the affine sum of the decoded signatures of the named sets whose verdicts[i] ==
 *                  GBLS_SUCCESS, in blst_p2_affine layout as gbls_g2_aggregate_segments writes it:
 *                  as a point, what aggregate_in_place over exactly those signatures gives, in any
 *                  order.  All-zero for infinity.
 *   fold_count[g]  the number of occurrences that entered the sum.  0 says that nothing passed.
 *   fold_bytes[g]  (fold_bytes may be NULL) that sum compressed; 0xc0 followed by zeros for
 *                  infinity, as SignatureBytes::empty.
 * A sum that cancels (a signature with its negation) has an all-zero fold_out, the infinity bytes
 * and its true count.
 *
 * Fail closed.  Before anything else, beside the each-call's pre-fill, fold_out and fold_count are
 * zeroed and fold_bytes is set to the infinity encoding; on any failure all outputs are back at that
 * pre-fill.  A set that fails for any reason (decoding, subgroup, key status, pairing) is never in
 * any sum and never changes another set's or another group's outputs.
 *
 * GBLS_ERR_ARG, beside the each-call's cases: nfold > 0 with fold_off, fold_set, fold_out or
 * fold_count NULL; fold_off[0] != 0 or fold_off decreasing; a fold_set entry >= n; a group count
 * that does not fit 32 bits.
 *
 * With nfold == 0 the call gives exactly the outputs of the each-call over span sets and launches
 * no further kernel.  Concurrent callers ARE merged by the coalescer, fold requests only with fold
 * requests; every caller gets exactly its own verdicts, statuses and sums.  A submission that
 * carries groups runs on one engine device.
 *
 * Only the each-call has a fold.  The items call follows Signature::multi_verify, which passes
 * sigs_groupcheck = false (bls/src/signature.rs:117-126): a signature with a cofactor-torsion
 * component can pass such a batch, and folding it would export it into an aggregate the node
 * publishes.  The each-call subgroup-checks every signature, so everything in a sum is in G2.
 */
#ifndef GRANDINE_BLS_GPU_FOLD_H
#define GRANDINE_BLS_GPU_FOLD_H

#include "grandine_bls_gpu_each.h"

#ifdef __cplusplus
extern "C" {
#endif

int gbls_verify_each_fold(const uint8_t (*msgs)[32], const uint8_t (*sigs)[96], const uint32_t *com,
                          const uint8_t (*cbits)[8], const uint8_t *bits, const uint32_t *bits_off,
                          const uint32_t *pk_idx, const uint32_t *pk_off, size_t n,
                          const uint32_t *fold_set, const uint32_t *fold_off, size_t nfold,
                          int32_t *sig_status, int32_t *key_status, int32_t *verdicts,
                          gbls_p2_affine *fold_out, uint8_t (*fold_bytes)[96] /* may be NULL */,
                          uint32_t *fold_count);

#ifdef __cplusplus
}
#endif
#endif
