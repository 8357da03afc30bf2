// Engine telemetry: the recording structures behind include/grandine_bls_gpu_telemetry.h.
// Host-only C++ (no HIP): gbls_capi.hip records into the process-wide Store; tests/native/
// telemetry_main.cpp instantiates the same structures (a ring of capacity 8, the scheduler with
// stub contexts, a stub verifier and an injected clock) plain, under ASan + UBSan and under ThreadSanitizer.
//
// Recording is lock-free: counters and histograms are relaxed atomic adds, a maximum is a
// compare-exchange loop, a ring slot is claimed by ticket and stamped with a sequence number.  A
// reader (snapshot, trace drain) never makes a recorder wait; readers serialise among themselves.
#pragma once

#include <atomic>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <mutex>

#include "../../include/grandine_bls_gpu_telemetry.h"
#include "gbls_sched.h"

namespace gbls {
namespace tel {

constexpr int kClasses = GBLS_TELEMETRY_CLASSES;
constexpr int kBuckets = GBLS_TELEMETRY_BUCKETS;
constexpr int kBins = GBLS_TELEMETRY_BINS;

enum Kind { K_BATCH, K_CHECKS, K_SPAN_ITEMS, K_SPAN_CHECKS, K_LOCAL_ITEMS, K_LOCAL_CHECKS, K_FOLD, K_DIRECT, K_DEVICE, K_COUNT };
static_assert(K_COUNT == GBLS_TELEMETRY_KINDS, "kinds");
enum Phase {
  P_HOLD, P_WINDOW, P_QUEUE, P_RUN, P_TOTAL,  // per caller
  P_REGLOCK, P_LEASE, P_STAGING, P_GROWTH, P_ENQUEUE, P_SYNC, P_DEVICE, P_LAG,  // per shard
  P_COUNT
};
static_assert(P_COUNT == GBLS_TELEMETRY_PHASES && P_REGLOCK == GBLS_TELEMETRY_CALLER_PHASES, "phases");

inline const char *phase_name(int i) {
  static const char *const n[P_COUNT] = {"hold",    "window", "queue",   "run",  "total",  "reglock", "lease",
                                         "staging", "growth", "enqueue", "sync", "device", "lag"};
  return i >= 0 && i < P_COUNT ? n[i] : nullptr;
}
inline const char *kind_name(int i) {
  static const char *const n[K_COUNT] = {"batch",      "checks",       "span_items", "span_checks", "local_items",
                                         "local_checks", "fold",       "direct",     "device"};
  return i >= 0 && i < K_COUNT ? n[i] : nullptr;
}
inline const char *class_name(int i) {
  static const char *const n[kClasses] = {"normal", "block"};
  return i >= 0 && i < kClasses ? n[i] : nullptr;
}

// the kind of a coalescer request: what Request::kind() distinguishes, without the layout bits
// (points or indices, points or compressed signatures) that only keep unlike arrays apart
template <class Req>
inline int kind_of(const Req &r) {
  if (r.rands) return r.spans() ? (r.src.local ? K_LOCAL_ITEMS : K_SPAN_ITEMS) : K_BATCH;
  if (!r.spans()) return K_CHECKS;
  return r.src.fold ? K_FOLD : r.src.local ? K_LOCAL_CHECKS : K_SPAN_CHECKS;
}

// bucket 0: d < 1024 ns; bucket k: 2^(k+9) <= d < 2^(k+10); bucket 31: d >= 2^40
inline int bucket_of(uint64_t ns) {
  if (ns < 1024) return 0;
  const int k = 63 - __builtin_clzll(ns) - 9;
  return k > kBuckets - 1 ? kBuckets - 1 : k;
}
// bin 0: x <= 1; bin b: 2^(b-1) < x <= 2^b; the last bin everything above
inline int bin_of(uint64_t x) {
  if (x <= 1) return 0;
  const int b = 64 - __builtin_clzll(x - 1);
  return b > kBins - 1 ? kBins - 1 : b;
}

using Counter = std::atomic<uint64_t>;
inline void add(Counter &c, uint64_t v) { c.fetch_add(v, std::memory_order_relaxed); }
inline uint64_t get(const Counter &c) { return c.load(std::memory_order_relaxed); }

struct Hist {
  Counter count{0}, sum{0}, max{0};
  Counter bucket[kBuckets] = {};
  void record(uint64_t ns) {
    add(count, 1);
    add(sum, ns);
    add(bucket[bucket_of(ns)], 1);
    uint64_t m = max.load(std::memory_order_relaxed);
    while (ns > m && !max.compare_exchange_weak(m, ns, std::memory_order_relaxed)) {
    }
  }
  void read(gbls_telemetry_hist &o) const {
    o.count = get(count);
    o.sum_ns = get(sum);
    o.max_ns = get(max);
    for (int i = 0; i < kBuckets; i++) o.bucket[i] = get(bucket[i]);
  }
  void reset() {
    count.store(0, std::memory_order_relaxed);
    sum.store(0, std::memory_order_relaxed);
    max.store(0, std::memory_order_relaxed);
    for (Counter &b : bucket) b.store(0, std::memory_order_relaxed);
  }
};

struct Cell {
  Counter calls{0}, sets{0}, rejected{0}, engine_errors{0};
  Counter submissions{0}, shards{0}, callers{0}, submitted_sets{0};
  Counter fresh_contexts{0}, staging_waits{0}, growths{0};
  Counter callers_bin[kBins] = {}, sets_bin[kBins] = {};
  Hist phase[P_COUNT];
  void read(gbls_telemetry_cell &o) const {
    o.calls = get(calls), o.sets = get(sets), o.rejected = get(rejected), o.engine_errors = get(engine_errors);
    o.submissions = get(submissions), o.shards = get(shards), o.callers = get(callers);
    o.submitted_sets = get(submitted_sets);
    o.fresh_contexts = get(fresh_contexts), o.staging_waits = get(staging_waits), o.growths = get(growths);
    o.reserved = 0;
    for (int i = 0; i < kBins; i++) o.callers_bin[i] = get(callers_bin[i]), o.sets_bin[i] = get(sets_bin[i]);
    for (int i = 0; i < P_COUNT; i++) phase[i].read(o.phase[i]);
  }
  void reset() {
    for (Counter *c : {&calls, &sets, &rejected, &engine_errors, &submissions, &shards, &callers, &submitted_sets,
                       &fresh_contexts, &staging_waits, &growths})
      c->store(0, std::memory_order_relaxed);
    for (int i = 0; i < kBins; i++) callers_bin[i].store(0, std::memory_order_relaxed), sets_bin[i].store(0, std::memory_order_relaxed);
    for (Hist &h : phase) h.reset();
  }
};

// ---------------------------------------------------------------- the trace ring
// Rec: a POD made of 64-bit words whose first word receives the ticket.  A writer takes a ticket,
// claims slot ticket % N by moving its stamp from even to odd (a slot that another writer still
// holds -- it was lapped by a whole ring -- is left alone and the record is dropped, never waited
// for), stores the words, then stamps the slot 2 * ticket + 2.  A reader accepts a slot only when
// the stamp it read before and after the words is the one of the ticket it expects.
template <class Rec, size_t N>
struct Ring {
  static_assert(sizeof(Rec) % 8 == 0, "a record is made of 64-bit words");
  static constexpr size_t kWords = sizeof(Rec) / 8;
  struct Slot {
    std::atomic<uint64_t> stamp{0};
    std::atomic<uint64_t> w[kWords];
  };
  Slot slot[N];
  std::atomic<uint64_t> head{0};     // tickets issued
  std::atomic<uint64_t> dropped{0};  // cumulative, counted by drain: overwritten or unfinished when read
  std::mutex reader;                 // readers only
  uint64_t tail = 0;                 // next ticket to read (guarded by reader)

  uint64_t push(Rec r) {
    const uint64_t t = head.fetch_add(1, std::memory_order_relaxed);
    Slot &s = slot[t % N];
    uint64_t st = s.stamp.load(std::memory_order_relaxed);
    if ((st & 1) || st > 2 * t + 2 || !s.stamp.compare_exchange_strong(st, 2 * t + 1, std::memory_order_acq_rel, std::memory_order_relaxed))
      return t;  // (the reader that expects ticket t finds another stamp and counts it)
    uint64_t words[kWords];
    std::memcpy(words, &r, sizeof(Rec));
    words[0] = t;
    // (release stores and acquire loads of the words instead of fences: a reader that saw any word
    // of this record then sees the slot's stamp no older than the claim above)
    for (size_t i = 0; i < kWords; i++) s.w[i].store(words[i], std::memory_order_release);
    s.stamp.store(2 * t + 2, std::memory_order_release);
    return t;
  }
  // up to max of the oldest unread records in ticket order; *lost: records gone since the last drain
  size_t drain(Rec *out, size_t max, uint64_t *lost) {
    std::lock_guard<std::mutex> lk(reader);
    const uint64_t h = head.load(std::memory_order_acquire);
    uint64_t gone = 0;
    if (h - tail > N) {
      gone += h - tail - N;
      tail = h - N;
    }
    size_t n = 0;
    while (tail < h && n < max) {
      const uint64_t t = tail++;
      Slot &s = slot[t % N];
      const uint64_t want = 2 * t + 2;
      uint64_t words[kWords];
      if (s.stamp.load(std::memory_order_acquire) != want) {
        gone++;
        continue;
      }
      for (size_t i = 0; i < kWords; i++) words[i] = s.w[i].load(std::memory_order_acquire);
      if (s.stamp.load(std::memory_order_acquire) != want) {
        gone++;
        continue;
      }
      std::memcpy(&out[n++], words, sizeof(Rec));
    }
    dropped.fetch_add(gone, std::memory_order_relaxed);
    if (lost) *lost = gone;
    return n;
  }
  void discard() {
    std::lock_guard<std::mutex> lk(reader);
    tail = head.load(std::memory_order_acquire);
  }
};

// ---------------------------------------------------------------- what one call, submission, shard reports
// a caller's phases from what the scheduler wrote (gbls_sched.h CallPhases): everything between
// entering the coalescer and the start of the submission that is neither hold nor window is queue
struct CallTimes {
  uint64_t hold, window, queue, run, total;
};
inline CallTimes call_times(const sched::CallPhases &p, uint64_t entry_ns, uint64_t exit_ns) {
  CallTimes t{p.hold_ns, p.window_ns, 0, p.run_ns, exit_ns - entry_ns};
  // (a caller whose batch was led under a configuration without a clock -- the level was switched on
  // while that leader was inside -- has no lead stamp: nothing waited is recorded for it)
  const uint64_t waited = p.lead_ns >= p.submit_ns ? p.lead_ns - p.submit_ns : 0;
  t.queue = waited > t.hold + t.window ? waited - t.hold - t.window : 0;
  return t;
}

// The two host waits of a shard that no GPU test can provoke, behind hooks that take the clock so that
// the native program drives them with a stub pool and a stub wait.  clock == nullptr (level 0): no
// clock is read.
// ... the wait for a context lease (sched::CtxPool::acquire): *begin_ns before, *lease_ns after
template <class Pool, class Stream>
auto timed_acquire(Pool &pool, bool affine, Stream stream, int cls, bool *fresh, uint64_t (*clock)(), uint64_t *begin_ns,
                   uint64_t *lease_ns) -> decltype(pool.acquire(affine, stream, cls, fresh)) {
  if (clock) *begin_ns = clock();
  auto c = pool.acquire(affine, stream, cls, fresh);
  if (clock) *lease_ns = clock();
  return c;
}
// ... a host wait on a staging slot: its time and their count (w == nullptr: not recorded)
struct StagingWaits {
  uint64_t ns = 0;
  uint32_t count = 0;
};
template <class Wait>
auto timed_wait(uint64_t (*clock)(), StagingWaits *w, Wait &&wait) -> decltype(wait()) {
  if (!w) return wait();
  const uint64_t t0 = clock();
  auto r = wait();
  w->ns += clock() - t0;
  w->count++;
  return r;
}

template <size_t N = GBLS_TELEMETRY_TRACE_CAPACITY>
struct StoreT {
  std::atomic<int> level{0};
  std::atomic<uint64_t> next_submission{1};
  Cell cell[kClasses][K_COUNT];
  Ring<gbls_telemetry_record, N> ring;

  Cell &at(int cls, int kind) { return cell[cls ? 1 : 0][kind < 0 || kind >= K_COUNT ? K_DIRECT : kind]; }
  void record_rejected(int cls, int kind) { add(at(cls, kind).rejected, 1); }
  void record_call(int cls, int kind, uint64_t sets, const CallTimes &t, bool engine_error) {
    Cell &c = at(cls, kind);
    add(c.calls, 1);
    add(c.sets, sets);
    if (engine_error) add(c.engine_errors, 1);
    c.phase[P_HOLD].record(t.hold);
    c.phase[P_WINDOW].record(t.window);
    c.phase[P_QUEUE].record(t.queue);
    c.phase[P_RUN].record(t.run);
    c.phase[P_TOTAL].record(t.total);
  }
  void record_submission(int cls, int kind, uint64_t callers, uint64_t sets) {
    Cell &c = at(cls, kind);
    add(c.submissions, 1);
    add(c.callers, callers);
    add(c.submitted_sets, sets);
    add(c.callers_bin[bin_of(callers)], 1);
    add(c.sets_bin[bin_of(sets)], 1);
  }
  // one shard: its record goes into the ring, its phases into the cell.  reglock_ns, lease_wait_ns
  // and growth_ns are not in the record.  A shard the host waited for has one sample in every shard
  // phase (device and lag are zero samples unless it was timed, level 2); one it did not wait for
  // (the device kind) has no sync, device or lag sample
  void record_shard(const gbls_telemetry_record &r, uint64_t reglock_ns, uint64_t lease_wait_ns, uint64_t growth_ns,
                    uint64_t enqueue_ns, uint64_t sync_ns, bool waited) {
    Cell &c = at((int)r.cls, (int)r.kind);
    add(c.shards, 1);
    if (r.fresh) add(c.fresh_contexts, 1);
    add(c.staging_waits, r.staging_waits);
    add(c.growths, r.growths);
    c.phase[P_REGLOCK].record(reglock_ns);
    c.phase[P_LEASE].record(lease_wait_ns);
    c.phase[P_STAGING].record(r.staging_wait_ns);
    c.phase[P_GROWTH].record(growth_ns);
    c.phase[P_ENQUEUE].record(enqueue_ns);
    if (waited) {
      c.phase[P_SYNC].record(sync_ns);
      c.phase[P_DEVICE].record(r.device_ns);
      c.phase[P_LAG].record(r.lag_ns);
    }
    ring.push(r);
  }
  void read(gbls_telemetry_snapshot &o) {
    o.size = (uint32_t)sizeof(o);
    o.level = (uint32_t)level.load(std::memory_order_relaxed);
    o.trace_written = ring.head.load(std::memory_order_relaxed);
    o.trace_dropped = ring.dropped.load(std::memory_order_relaxed);
    for (int a = 0; a < kClasses; a++)
      for (int k = 0; k < K_COUNT; k++) cell[a][k].read(o.cell[a][k]);
  }
  void reset() {
    for (auto &row : cell)
      for (Cell &c : row) c.reset();
    ring.discard();
  }
};
using Store = StoreT<>;

}  // namespace tel
}  // namespace gbls
