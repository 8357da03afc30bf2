/* grandine_bls_gpu_telemetry.h -- engine telemetry: what the engine did with each call (an extension
 * of grandine_bls_gpu.h, whose conventions hold here unchanged; nothing here changes a verdict, a
 * status or an output of any other entry).
 *
 * A node keeps histograms around its verification calls (prometheus_metrics/src/metrics.rs:55-60,
 * 270-295: the attestation verifier's batch times).  With the engine behind them they measure "some
 * time in a library".  This header says how a call's time divides: held behind a block import, in a
 * collection window, queued for a leader, waiting for a context, for a staging slot, growing a
 * buffer, enqueueing, waiting for the device -- and how many callers and sets each submission
 * carried, and how much device and pinned memory the engine holds.
 *
 * Levels (process-wide, sticky, no device needed, may be set before the engine is initialised).
 *   0  (the default) nothing is recorded: an outermost entry does one relaxed atomic load of the
 *      level, every other hook reads a thread-local pointer and finds it null; no clock is read, no
 *      event is created, the counters and the trace do not move.
 *   1  counters and host-clock phases (steady clock, nanoseconds).
 *   2  adds device time per shard: two timing events on the shard's main stream.
 * Cost, from one capture on 64-set calls of 2.4 and 3.1 ms (DESIGN "Engine telemetry"): level 1 cannot
 * be told from level 0 (under 0.4 us per call, inside the run-to-run range): it is the level to be left on
 * in a node.  Level 2 costs 5 to 12 us per call (two event records per shard and one elapsed-time
 * query after the host wait) and is meant for captures (tools/engine_timeline.py).
 *
 * Classes: 0 normal, 1 block import (GBLS_CALL_BLOCK).  Kinds: what the coalescer distinguishes --
 * batches with scalars, single checks, span items, span checks, local items, local checks, the fold
 * -- then `direct` (host-pointer calls that never enter the coalescer: decoding, compression,
 * aggregation, the committees, bits and spans batch calls, prefetch, registry updates, hashing and
 * signing) and `device` (the device-pointer entry points: their enqueue time only; telemetry never
 * synchronises with the device on their behalf).
 *
 * A duration histogram has GBLS_TELEMETRY_BUCKETS log2 buckets: bucket 0 holds durations under
 * 1024 ns, bucket k holds 2^(k+9) <= d < 2^(k+10) ns, bucket 31 everything from 2^40 ns up; beside
 * them count, sum_ns and max_ns.
 *
 * Per (class, kind) cell:
 *   calls, sets          accepted calls and their sets.  A call refused for its arguments before any
 *                        work (GBLS_ERR_ARG) counts in `rejected` only; a call that ends with another
 *                        nonzero engine error code counts in `engine_errors` as well as in calls.
 *   caller phases        (one sample per call) hold: held back by a block import; window: a leader's
 *                        collection window; queue: the rest of the time from entering the coalescer to
 *                        the start of the call's submission; run: the submission, the same value for
 *                        every caller merged into it; total: entry to return.
 *                        total >= hold + window + queue + run.
 *   submissions, shards, callers, submitted_sets
 *                        a submission is one merged verification (a direct or device call is its own
 *                        submission of one caller); a shard is one context lease of it.
 *   callers_bin, sets_bin  per submission, power-of-two bins: bin 0 holds 0 and 1, bin b holds
 *                        2^(b-1) < x <= 2^b, the last bin everything above.
 *   shard phases         (one sample per shard) reglock: wait for the registry's shared lock (charged
 *                        to the submission's first shard); lease: wait for a context; staging: host
 *                        time in waits on a staging slot (staging_waits counts them); growth: host
 *                        time of buffer growths that wait on the host (growths counts all growths);
 *                        enqueue: lease obtained to last launch enqueued, waits included; sync: the
 *                        host's wait for completion; device (level 2): elapsed time between a timing
 *                        event at the shard's beginning and one behind its last work; lag (level 2):
 *                        (synced - first event recorded) - device, the part of the host-observed
 *                        interval in which the shard's stream was not between the two events (its
 *                        start delay on the GPU plus the completion notice); never negative.
 *                        run >= enqueue + sync, enqueue >= staging.
 *   fresh_contexts       shards that had to create their context.
 *
 * The trace is a ring of the GBLS_TELEMETRY_TRACE_CAPACITY (1024) most recent shard records; a new
 * record overwrites the oldest, and what was overwritten before it was read is counted.
 *
 * Recording is lock-free (relaxed atomic adds, a compare-exchange loop for max_ns, ring slots
 * claimed by ticket and stamped with a sequence number); a reader never makes a recording thread
 * wait, so a snapshot taken while calls run is consistent only counter by counter.
 *
 * Every struct starts with `size`: the caller passes sizeof of ITS struct, the library fills at most
 * that many bytes and stores the number it filled, so the structs may grow at their ends.
 */
#ifndef GRANDINE_BLS_GPU_TELEMETRY_H
#define GRANDINE_BLS_GPU_TELEMETRY_H

#include "grandine_bls_gpu.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GBLS_TELEMETRY_CLASSES 2
#define GBLS_TELEMETRY_KINDS 9
#define GBLS_TELEMETRY_PHASES 13 /* 5 caller phases, then 8 shard phases */
#define GBLS_TELEMETRY_CALLER_PHASES 5
#define GBLS_TELEMETRY_BUCKETS 32
#define GBLS_TELEMETRY_BINS 24
#define GBLS_TELEMETRY_TRACE_CAPACITY 1024
#define GBLS_TELEMETRY_MAX_ENGINES 16

typedef struct {
  uint64_t count, sum_ns, max_ns;
  uint64_t bucket[GBLS_TELEMETRY_BUCKETS];
} gbls_telemetry_hist;

typedef struct {
  uint64_t calls, sets, rejected, engine_errors;
  uint64_t submissions, shards, callers, submitted_sets;
  uint64_t fresh_contexts, staging_waits, growths, reserved;
  uint64_t callers_bin[GBLS_TELEMETRY_BINS];
  uint64_t sets_bin[GBLS_TELEMETRY_BINS];
  gbls_telemetry_hist phase[GBLS_TELEMETRY_PHASES];
} gbls_telemetry_cell;

typedef struct {
  uint32_t size;  /* in: sizeof the caller's struct; out: bytes filled */
  uint32_t level;
  uint64_t trace_written; /* shard records ever put into the ring */
  uint64_t trace_dropped; /* ... overwritten or skipped before a reader took them */
  gbls_telemetry_cell cell[GBLS_TELEMETRY_CLASSES][GBLS_TELEMETRY_KINDS];
} gbls_telemetry_snapshot;

typedef struct {
  uint64_t id;         /* the record's ticket: consecutive, in the order shards finished */
  uint64_t submission; /* shared by the shards of one submission */
  uint32_t cls, kind;
  uint32_t callers;  /* merged into the submission */
  uint32_t segments; /* of this shard */
  uint64_t sets;       /* of the submission */
  uint64_t shard_sets; /* of this shard */
  uint32_t engine;  /* index of the engine device */
  uint32_t fresh;   /* the shard created its context */
  uint64_t context; /* an id of the context, stable while the process lives */
  /* host timestamps, steady clock, ns: first arrival among the merged callers, start of the
   * submission, context obtained, (level 2) first timing event recorded, last launch enqueued, host
   * wait over.  first_arrival <= lead <= lease <= enqueued <= synced. */
  uint64_t first_arrival_ns, lead_ns, lease_ns, first_event_ns, enqueued_ns, synced_ns;
  uint64_t staging_wait_ns;
  uint32_t staging_waits, growths;
  uint64_t device_ns, lag_ns; /* zero at level 1 */
} gbls_telemetry_record;

typedef struct {
  uint32_t hip_device, reserved;
  uint64_t contexts_leased[GBLS_TELEMETRY_CLASSES], contexts_idle[GBLS_TELEMETRY_CLASSES];
  uint64_t workspace_bytes[GBLS_TELEMETRY_CLASSES]; /* every workspace buffer's capacity */
  uint64_t registry_bytes, committee_bytes, member_bytes;
  uint64_t linecache_bytes;
  uint64_t pinned_live_bytes;    /* staging ring slots */
  uint64_t pinned_retired_bytes; /* replaced staging buffers, kept until the process ends */
  uint64_t pinned_retired_buffers;
  uint64_t device_free_bytes, device_total_bytes; /* of the whole device, all processes */
} gbls_telemetry_engine_memory;

typedef struct {
  uint32_t size;    /* as above */
  uint32_t engines; /* entries filled; zero before the engine is initialised */
  gbls_telemetry_engine_memory engine[GBLS_TELEMETRY_MAX_ENGINES];
} gbls_telemetry_memory_info;

/* Sets the level (clamped to 0..2) and returns the previous one. */
int gbls_telemetry_enable(int level);

/* A snapshot of every counter and histogram.  Returns GBLS_SUCCESS, or GBLS_VERIFY_FAIL with
 * GBLS_ERR_ARG for a NULL pointer or a size below 8. */
int gbls_telemetry_read(gbls_telemetry_snapshot *out, size_t size);

/* Zeroes the counters and histograms and empties the trace. */
void gbls_telemetry_reset(void);

/* Drains the trace: writes up to max of the oldest unread records, in id order, and returns how
 * many.  *dropped (may be NULL) receives the number of records lost since the previous drain. */
size_t gbls_telemetry_trace(gbls_telemetry_record *records, size_t max, uint64_t *dropped);

/* Memory gauges, computed on demand, at any level; engines == 0 before the engine is initialised.
 * Not lock-free: it takes the registry's lock shared and may wait behind a registry update. */
int gbls_telemetry_memory(gbls_telemetry_memory_info *out, size_t size);

/* Names of the phases (0 .. GBLS_TELEMETRY_PHASES-1), kinds and classes; NULL past the end. */
const char *gbls_telemetry_phase_name(int i);
const char *gbls_telemetry_kind_name(int i);
const char *gbls_telemetry_class_name(int i);

#ifdef __cplusplus
}
#endif
#endif
