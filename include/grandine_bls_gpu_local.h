/* grandine_bls_gpu_local.h -- local key sets: compressed public keys decoded inside the submission
 * (an extension of grandine_bls_gpu_each.h, whose conventions hold here unchanged: the fail-closed
 * pre-fill, the GBLS_ERR_ARG cases, merging with concurrent callers, GBLS_CALL_BLOCK,
 * GBLS_INIT_DEDUP, GBLS_INIT_PER_CHECK, the grouped regime from 2048 checks, the message line
 * cache).
 *
 * Span sets name committees of the table and plain sets name registry indices.  One kind of set
 * fits neither: a set whose key the caller holds only as 48 compressed bytes, with no registry
 * entry -- a deposit's pubkey (validate_deposits: an optimistic batch, then one check per deposit,
 * whose verdict is consensus-relevant), a BLS-to-execution change's from_bls_pubkey, a validator
 * above the mirrored, finalized registry length.  The calls here carry such keys in a LOCAL KEY
 * TABLE pkb[npkb], which lives for that call only, and know a third kind of set:
 *
 *   com[i] == GBLS_LOCAL_KEYS   the set's pk_off range holds POSITIONS into pkb, not registry
 *                               indices; its key is the sum of the named local keys.  Its cbits
 *                               are zero and its bit string is empty.
 *
 * Span sets and GBLS_NO_COMMITTEE sets are exactly as in grandine_bls_gpu_spans.h.  In every other
 * call 0xFFFFFFFE stays what it is there: a base slot past the table, rejected per set.
 *
 * Decoding.  Each local key is decoded once, however many sets name it, with PublicKey::try_from
 * semantics, exactly as gbls_g1_decompress(validate = 1) decodes it.  pkb_status (optional, may be
 * NULL; pre-filled with GBLS_BAD_ENCODING) receives that call's status of key j: GBLS_SUCCESS,
 * GBLS_BAD_ENCODING, GBLS_POINT_NOT_ON_CURVE, GBLS_POINT_NOT_IN_GROUP or GBLS_PK_IS_INFINITY.
 * A sharded batch decodes the whole table on every shard; it is meant to be small (a block's
 * deposits and address changes).
 *
 * A local set's key_status / status:
 *   GBLS_BAD_ENCODING        a named key is invalid, or a position is >= npkb (what a bad registry
 *                            index gives)
 *   GBLS_AGGR_TYPE_MISMATCH  an empty range
 *   0                        a valid sum, including one that cancels to infinity (verification
 *                            rejects an infinite key, as everywhere else)
 * A rejected set's key is all-zero; it never changes a neighbour's outputs.
 *
 * GBLS_ERR_ARG, beside the cases of grandine_bls_gpu_each.h: a local set with nonzero cbits or a
 * non-empty bit string; a local set when pk_off is NULL; pkb == NULL with npkb > 0; npkb that does
 * not fit 32 bits.
 *
 * With npkb == 0 and no local set the two verify calls give exactly the outputs of the each-call
 * and the items call of grandine_bls_gpu_each.h.  Requests of these calls merge with each other
 * (not with requests of the span calls) under the same class and priority rules; every caller
 * gets its own verdicts, statuses and pkb_status.
 */
#ifndef GRANDINE_BLS_GPU_LOCAL_H
#define GRANDINE_BLS_GPU_LOCAL_H

#include "grandine_bls_gpu_each.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GBLS_LOCAL_KEYS 0xFFFFFFFEu

/* The keys of n sets, as the key call of grandine_bls_gpu_spans.h gives them (out, status), local
 * sets included.  With n == 0 the table is decoded for pkb_status alone. */
int gbls_g1_aggregate_local(const uint32_t *com, const uint8_t (*cbits)[8], const uint8_t *bits,
                            const uint32_t *bits_off, const uint32_t *pk_idx, const uint32_t *pk_off,
                            const uint8_t (*pkb)[48], size_t npkb, size_t n, gbls_p1_affine *out, int32_t *status,
                            int32_t *pkb_status);

/* The each-call of grandine_bls_gpu_each.h over span, plain and local sets: n independent checks,
 * ONE submission (validate_deposits' per-deposit fallback: one verdict per deposit, pkb_status
 * says which pubkey was undecodable). */
int gbls_verify_each_local(const uint8_t (*msgs)[32], const uint8_t (*sigs)[96], const uint32_t *com,
                           const uint8_t (*cbits)[8], const uint8_t *bits, const uint32_t *bits_off,
                           const uint32_t *pk_idx, const uint32_t *pk_off, const uint8_t (*pkb)[48], size_t npkb,
                           size_t n, int32_t *sig_status, int32_t *key_status, int32_t *verdicts,
                           int32_t *pkb_status);

/* The items call of grandine_bls_gpu_each.h over span, plain and local sets: nseg independent
 * batches, one verdict per item (a block with its deposits and address changes as one item;
 * validate_deposits' optimistic batch as one item, which an undecodable pubkey fails). */
int gbls_verify_items_local(const uint8_t (*msgs)[32], const uint8_t (*sigs)[96], const uint32_t *com,
                            const uint8_t (*cbits)[8], const uint8_t *bits, const uint32_t *bits_off,
                            const uint32_t *pk_idx, const uint32_t *pk_off, const uint8_t (*pkb)[48], size_t npkb,
                            const uint64_t *rands, size_t n, const uint32_t *seg_off, size_t nseg,
                            int32_t *sig_status, int32_t *key_status, int32_t *verdicts, int32_t *pkb_status,
                            uint32_t call_flags);

#ifdef __cplusplus
}
#endif
#endif
