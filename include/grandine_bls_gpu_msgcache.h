/* grandine_bls_gpu_msgcache.h -- message line cache (an extension of grandine_bls_gpu.h, whose
 * conventions hold here: status codes, fail-closed returns, gbls_last_error, thread safety).
 *
 * Half of a batch verification depends on nothing but the messages: hash_to_G2 and the 68 Miller
 * line events of every H(m).  GBLS_INIT_DEDUP pays for them once per distinct message of one
 * submission; this cache pays for them once per message across submissions.  Gossip arrives in
 * batches of at most 64 sets that sign one of a handful of AttestationData roots of the slot, and
 * a block's sync aggregate, sync-committee messages and contributions repeat the same roots: a
 * call whose messages are all cached hashes nothing and generates no set-side lines.
 *
 * The cache is per engine device and device-resident: a table that maps a 32-byte message to its
 * line events.  It is OFF by default.  Verdicts, per-set rejections and signature statuses are
 * exactly what they are without it: lines are a function of the message alone, keys and
 * signatures enter the check as ever.
 *
 * Memory: 19 584 bytes per slot per engine device (4096 slots: 80 MB), plus a pool of spare slots
 * that calls in flight write their misses to (a quarter of the slots, at least 64, at most 4096).
 * The memory is allocated by the first served call on each device.
 *
 * Served: every host-pointer entry point that takes random scalars and 32-byte messages --
 * gbls_multi_verify, _segments, _indexed, _compressed, _compressed_ex, _bisect,
 * gbls_multi_verify_committees -- and whatever the coalescer merges out of them.
 * NOT served: the _device entry points (their messages are not on the host); single checks
 * (gbls_verify, the *_verify_batch calls: no random scalars); a submission so large that its line
 * buffer is generated in event slices, which bypasses the cache exactly as it bypasses
 * GBLS_INIT_DEDUP's grouping.
 *
 * Grouping: while the cache is on, a served submission is always planned by message, whatever the
 * GBLS_INIT_DEDUP policy bit says -- sets of one segment that carry one message share one Miller
 * pair.  The cache needs the plan's indirection between sets and pairs, and two sets of one
 * message must not fill two slots.
 *
 * Publication: a message that missed is entered only after its call has finished and only if the
 * verdict of a segment that carried it was GBLS_SUCCESS (for a batch sharded over several devices:
 * the batch's verdict).  An entry is never wrong whoever sent it; the rule is about eviction
 * pressure -- messages that cannot pass verification never displace entries.  Entries in use by a
 * call in flight are never evicted; the least recently used of the others is.
 */
#ifndef GRANDINE_BLS_GPU_MSGCACHE_H
#define GRANDINE_BLS_GPU_MSGCACHE_H

#include "grandine_bls_gpu.h"

#ifdef __cplusplus
extern "C" {
#endif

/* All four are thread-safe, need no device (like gbls_set_policy) and may be called while
 * verifications are in flight: a call already submitted finishes on the table it planned against,
 * and a replaced table's memory is freed only once no such call is left. */

/* Capacity in entries per engine device; 0 switches the cache off (the default).  More than 2^20:
 * GBLS_ERR_ARG, nothing changes.  A new capacity starts with an empty table; the same capacity
 * again changes nothing. */
int gbls_msgcache_configure(size_t slots);
size_t gbls_msgcache_slots(void); /* the configured capacity per device */
int gbls_msgcache_clear(void);    /* drops every entry, keeps the capacity (and the memory) */
/* Counters since the process started, over all devices:
 *   out[0] lookups    distinct messages looked up (per device shard of a served submission)
 *   out[1] hits       out[2] misses            lookups == hits + misses
 *   out[3] published  misses entered after a passing verdict
 *   out[4] evictions  entries displaced by a publication
 *   out[5] bypassed   messages computed but not cached: a miss with no spare slot or no evictable
 *                     entry, and every set of a sliced submission
 *   out[6] entries    entries now, all devices          out[7] reserved, 0 */
int gbls_msgcache_stats(uint64_t out[8]);

#ifdef __cplusplus
}
#endif
#endif
