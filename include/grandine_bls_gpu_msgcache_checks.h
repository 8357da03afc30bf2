/* grandine_bls_gpu_msgcache_checks.h -- the message line cache for per-check calls, and prefetch
 * (an extension of grandine_bls_gpu_msgcache.h, whose conventions hold here: status codes,
 * fail-closed returns, gbls_last_error, thread safety, no device needed unless stated).
 *
 * The line cache (grandine_bls_gpu_msgcache.h) serves calls that take random scalars, and enters a
 * message only after a verification that carried it has passed.  This header closes both gaps.
 *
 * 1. Per-check calls.  gbls_verify, gbls_fast_aggregate_verify, gbls_aggregate_verify_batch,
 *    gbls_fast_aggregate_verify_batch, gbls_verify_batch_compressed and the per-set calls over span
 *    and local key sets (the verify_each calls of grandine_bls_gpu_each.h and
 *    grandine_bls_gpu_local.h) carry no random scalars: every check is its own segment with r_i = 1.
 *    They sign the slot's hottest roots -- sync-committee messages and contributions, singular
 *    attestations, the per-set fallback after a failed gossip batch.  gbls_msgcache_serve_checks(1)
 *    has them planned by message and served: a check whose message is an entry loads its pair's
 *    lines from the table; a message that missed is hashed and given lines ONCE per submission,
 *    however many checks carry it, and is entered when at least one check that carried it returned
 *    GBLS_SUCCESS.  Verdicts, sig_status, key_status and pkb_status are exactly what they are with
 *    serving off.  OFF by default; while off nothing changes and a per-check call moves no counter.
 *    NOT served, their checks counted `bypassed` as a sliced submission's sets are: the grouped
 *    regime (2048 checks and more in one submission without GBLS_INIT_PER_CHECK), checks whose
 *    messages are not 32 bytes long, gbls_fast_aggregate_verify_indexed, the _device entry points.
 *
 * 2. Prefetch.  The node knows a slot's roots before any signature arrives: the AttestationData
 *    roots of the head candidates, the sync-committee message and contribution roots, the signing
 *    roots of a block being imported.  gbls_msgcache_prefetch enters them: hash_to_G2 and the 68
 *    line events of every message that is not yet an entry, on every engine device, by the same
 *    kernels a verification's misses run -- no signature, no key, no verdict.
 *    THE CALLER VOUCHES FOR THESE ROOTS.  The cache otherwise enters a message only after a
 *    verification that carried it passed, so that a peer's junk, which cannot pass, never evicts
 *    an entry.  Prefetch bypasses that rule: prefetch only roots the node derived itself, never
 *    roots taken from a peer's message.  Prefetched entries are ordinary entries: least recently
 *    used first out, dropped by gbls_msgcache_clear and by a new gbls_msgcache_configure.
 */
#ifndef GRANDINE_BLS_GPU_MSGCACHE_CHECKS_H
#define GRANDINE_BLS_GPU_MSGCACHE_CHECKS_H

#include "grandine_bls_gpu_msgcache.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GBLS_PREFETCH_ENTERED 0   /* entered by this call */
#define GBLS_PREFETCH_PRESENT 1   /* was an entry already (its recency is refreshed) */
#define GBLS_PREFETCH_SKIPPED 2   /* not entered: cache off, no spare slot, no evictable entry */

/* Enters msgs[0 .. n) on every engine device and waits for it.  status (n, may be NULL) is
 * pre-filled SKIPPED.  A message repeated within the call is handled once and every occurrence
 * reports the same status.  At most a pool of spare slots' worth of missing messages is taken per
 * call (a quarter of the configured slots, at least 64, at most 4096); those beyond are SKIPPED.
 * With several engines a message is PRESENT only if it was an entry on every engine before the
 * call, ENTERED if it was missing on at least one and is an entry on every engine after it,
 * SKIPPED otherwise.
 * n == 0: GBLS_SUCCESS.  msgs == NULL with n > 0: GBLS_ERR_ARG.  Cache off: GBLS_SUCCESS, every
 * status SKIPPED, no device work and no device needed.  Otherwise it needs the engine and fails
 * closed like every call: on a failure nothing is entered and every status stays SKIPPED.
 * The main counters (gbls_msgcache_stats) count a prefetch like a served shard: lookups ==
 * hits + misses, an ENTERED message counts as published, evictions as usual, a missing message
 * that was not taken as bypassed.  Runs on a normal-class context, never a block-class one. */
int gbls_msgcache_prefetch(const uint8_t (*msgs)[32], size_t n, int32_t *status /* n, may be NULL */);

/* Serve per-check calls (1) or not (0, the default).  Process-wide and sticky like the policy bits;
 * needs no device; takes effect with the next submission. */
int gbls_msgcache_serve_checks(int on);          /* returns the previous setting; off by default */

/* Counters since the process started, over all devices:
 *   out[0] prefetched       messages a prefetch call reported ENTERED
 *   out[1] check_lookups    distinct messages looked up by served per-check submissions
 *   out[2] check_hits       ... that were entries
 *   out[3] check_published  ... entered after a check that carried them passed
 * The last three are included in lookups, hits and published of gbls_msgcache_stats. */
int gbls_msgcache_checks_stats(uint64_t out[4]); /* prefetched, check_lookups, check_hits, check_published */

#ifdef __cplusplus
}
#endif
#endif
