// Stand-alone checks of the telemetry recording structures (grandine_amd/csrc/gbls_telemetry.h) and
// of the scheduler's telemetry stamps (gbls_sched.h), with stub contexts, a stub verifier and an
// injected clock.  Built and run plainly, with -fsanitize=address,undefined and with
// -fsanitize=thread by tests/test_telemetry_host.py.  Prints "telemetry: OK" when everything held.
//
// (As tests/native/sched_tsan.cpp: GCC 11's TSan runtime does not intercept pthread_cond_clockwait,
// so this test build makes libstdc++ wait through pthread_cond_timedwait; the engine build is unchanged.)
#include <bits/c++config.h>
#undef _GLIBCXX_USE_PTHREAD_COND_CLOCKWAIT

#include <atomic>
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <thread>
#include <vector>

#include "gbls_telemetry.h"

using namespace gbls;

#define CHECK(x)                                                  \
  do {                                                            \
    if (!(x)) {                                                   \
      std::printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #x);   \
      std::exit(1);                                               \
    }                                                             \
  } while (0)

// ---------------------------------------------------------------- histograms
static void buckets() {
  CHECK(tel::bucket_of(0) == 0 && tel::bucket_of(1023) == 0 && tel::bucket_of(1024) == 1);
  for (int k = 1; k <= 31; k++) {
    const uint64_t lo = 1ull << (k + 9);
    CHECK(tel::bucket_of(lo) == k);
    CHECK(tel::bucket_of(lo - 1) == k - 1);
    if (k < 31) CHECK(tel::bucket_of(2 * lo - 1) == k);
  }
  CHECK(tel::bucket_of(1ull << 40) == 31 && tel::bucket_of((1ull << 40) - 1) == 30);
  CHECK(tel::bucket_of(1ull << 41) == 31 && tel::bucket_of(UINT64_MAX) == 31);
  tel::Hist h;
  const uint64_t v[] = {0, 1023, 1024, 2047, 2048, 1ull << 40, 5000000};
  uint64_t sum = 0;
  for (uint64_t x : v) h.record(x), sum += x;
  gbls_telemetry_hist o;
  h.read(o);
  CHECK(o.count == 7 && o.sum_ns == sum && o.max_ns == (1ull << 40));
  CHECK(o.bucket[0] == 2 && o.bucket[1] == 2 && o.bucket[2] == 1 && o.bucket[31] == 1 && o.bucket[13] == 1);
  // bins: 1 in a bin of its own (with 0), then powers of two
  CHECK(tel::bin_of(0) == 0 && tel::bin_of(1) == 0 && tel::bin_of(2) == 1 && tel::bin_of(3) == 2 && tel::bin_of(4) == 2);
  CHECK(tel::bin_of(5) == 3 && tel::bin_of(64) == 6 && tel::bin_of(65) == 7 && tel::bin_of(UINT64_MAX) == tel::kBins - 1);
  h.reset();
  h.read(o);
  CHECK(o.count == 0 && o.sum_ns == 0 && o.max_ns == 0 && o.bucket[0] == 0);
  std::printf("buckets ok\n");
}

// ---------------------------------------------------------------- the ring at capacity 8
struct Rec {  // first word: the ticket; `sum` is a checksum of the other fields
  uint64_t id, a, b, c, sum;
};
static Rec make(uint64_t a) { return Rec{0, a, a * 3 + 1, ~a, a + (a * 3 + 1) + ~a}; }
static bool whole(const Rec &r) { return r.sum == r.a + r.b + r.c && r.b == r.a * 3 + 1 && r.c == ~r.a; }

static void ring_order() {
  tel::Ring<Rec, 8> ring;
  Rec out[16];
  uint64_t lost = 99;
  CHECK(ring.drain(out, 16, &lost) == 0 && lost == 0);
  for (uint64_t i = 0; i < 5; i++) ring.push(make(100 + i));
  CHECK(ring.drain(out, 16, &lost) == 5 && lost == 0);
  for (uint64_t i = 0; i < 5; i++) CHECK(out[i].id == i && out[i].a == 100 + i && whole(out[i]));
  // 13 more: the 8 most recent survive, 5 were overwritten
  for (uint64_t i = 0; i < 13; i++) ring.push(make(200 + i));
  CHECK(ring.drain(out, 3, &lost) == 3 && lost == 5);           // a short drain takes the oldest survivors
  for (uint64_t i = 0; i < 3; i++) CHECK(out[i].id == 10 + i && out[i].a == 205 + i);
  CHECK(ring.drain(out, 16, &lost) == 5 && lost == 0);
  for (uint64_t i = 0; i < 5; i++) CHECK(out[i].id == 13 + i && out[i].a == 208 + i && whole(out[i]));
  CHECK(ring.dropped.load() == 5 && ring.head.load() == 18);
  ring.push(make(1));
  ring.discard();
  CHECK(ring.drain(out, 16, &lost) == 0 && lost == 0);
  std::printf("ring ok\n");
}

static void ring_threads() {
  static tel::Ring<Rec, 8> ring;
  constexpr int kThreads = 8, kEach = 20000;
  std::atomic<int> live{kThreads};
  std::vector<std::thread> th;
  for (int t = 0; t < kThreads; t++)
    th.emplace_back([t, &live] {
      for (int i = 0; i < kEach; i++) ring.push(make((uint64_t)t << 32 | (uint64_t)i));
      live.fetch_sub(1);
    });
  uint64_t got = 0, lost_total = 0, last = 0;
  bool first = true;
  Rec out[8];
  for (;;) {
    const bool done = live.load() == 0;
    uint64_t lost = 0;
    const size_t n = ring.drain(out, 8, &lost);
    lost_total += lost;
    for (size_t i = 0; i < n; i++) {
      CHECK(whole(out[i]));                                     // never a torn record
      CHECK(first || out[i].id > last);                         // tickets only go up
      CHECK((out[i].a >> 32) < (uint64_t)kThreads && (uint32_t)out[i].a < (uint32_t)kEach);
      last = out[i].id, first = false;
    }
    got += n;
    if (done && n == 0) break;
  }
  for (auto &t : th) t.join();
  CHECK(got + lost_total == (uint64_t)kThreads * kEach);        // every ticket was read or counted as lost
  CHECK(ring.head.load() == (uint64_t)kThreads * kEach && ring.dropped.load() == lost_total);
  std::printf("ring threads ok read %" PRIu64 " lost %" PRIu64 "\n", got, lost_total);
}

// ---------------------------------------------------------------- counters under 8 recorders
static void counters_conserved() {
  static tel::StoreT<8> store;
  constexpr int kThreads = 8, kEach = 5000;
  std::vector<std::thread> th;
  for (int t = 0; t < kThreads; t++)
    th.emplace_back([t] {
      for (int i = 0; i < kEach; i++) {
        tel::CallTimes ct{1, 2, 3, 1000 + (uint64_t)i, 5000 + (uint64_t)t};
        store.record_call(t & 1, tel::K_BATCH, 3, ct, false);
        store.record_submission(t & 1, tel::K_BATCH, 2, 6);
        gbls_telemetry_record r{};
        r.cls = (uint32_t)(t & 1), r.kind = tel::K_BATCH, r.staging_waits = 1, r.growths = 2, r.fresh = i == 0;
        store.record_shard(r, 1, 2, 3, 4, 5, true);
      }
    });
  gbls_telemetry_snapshot snap;
  store.read(snap);  // a reader while they record: it must not disturb them (and TSan must stay quiet)
  for (auto &t : th) t.join();
  store.read(snap);
  uint64_t calls = 0;
  for (int a = 0; a < 2; a++) {
    const gbls_telemetry_cell &c = snap.cell[a][tel::K_BATCH];
    calls += c.calls;
    CHECK(c.calls == 4u * kEach && c.sets == 3 * c.calls && c.submissions == c.calls && c.callers == 2 * c.calls);
    CHECK(c.shards == c.calls && c.staging_waits == c.calls && c.growths == 2 * c.calls && c.fresh_contexts == 4);
    CHECK(c.callers_bin[1] == c.calls && c.sets_bin[3] == c.calls);
    for (int p = 0; p < tel::P_COUNT; p++) {
      uint64_t in_buckets = 0;
      for (uint64_t b : c.phase[p].bucket) in_buckets += b;
      CHECK(c.phase[p].count == c.calls && in_buckets == c.calls);
    }
    CHECK(c.phase[tel::P_HOLD].sum_ns == c.calls && c.phase[tel::P_RUN].max_ns == 1000 + kEach - 1);
    CHECK(c.phase[tel::P_TOTAL].max_ns == 5000u + 6 + (unsigned)a);
  }
  CHECK(calls == (uint64_t)kThreads * kEach && snap.trace_written == calls);
  store.reset();
  store.read(snap);
  CHECK(snap.cell[0][tel::K_BATCH].calls == 0 && snap.cell[1][tel::K_BATCH].phase[tel::P_RUN].count == 0);
  CHECK(tel::phase_name(tel::P_COUNT) == nullptr && tel::kind_name(tel::K_COUNT) == nullptr && tel::class_name(2) == nullptr);
  CHECK(tel::phase_name(-1) == nullptr && tel::phase_name(0) && tel::kind_name(tel::K_DEVICE) && tel::class_name(1));
  std::printf("counters ok\n");
}

// ---------------------------------------------------------------- the scheduler's stamps
struct P1 {
  int x;
};
struct P2 {
  int y;
};
using Req = sched::Request<P1, P2>;

static std::atomic<uint64_t> g_ticks{0};
static uint64_t fake_clock() { return 1000 * (g_ticks.fetch_add(1) + 1); }  // 1 us per reading

struct Caller {
  uint8_t msg[32] = {0};
  P2 sig{0};
  P1 key{0};
  uint64_t rand = 1;
  uint32_t seg[2] = {0, 1};
  int32_t verdict = -1;
  sched::CallPhases ph;
  Req req;
  explicit Caller(bool stamped) : req{msg, &sig, sched::KeySource<P1>(), &rand, 1, seg, 1, &verdict} {
    req.src.pts = &key;
    if (stamped) req.ph = &ph;
  }
};

template <class F>
static void spin_until(F &&f) {
  for (long i = 0; !f(); i++) {
    CHECK(i < 2000000000L);
    std::this_thread::yield();
  }
}

static void scheduler() {
  sched::Coalescer<Req> co;
  sched::Config cfg;
  cfg.clock = fake_clock;
  cfg.leaders = 2;
  cfg.merge_target = 2;              // a window ends when two sets are queued
  cfg.merge_window_us = 60 * 1000000;  // ... never by time in this program
  tel::StoreT<8> store;
  std::atomic<int> in_verify{0}, release{0};
  std::atomic<uint64_t> callers_seen{0}, submissions{0};
  std::vector<sched::BatchInfo> infos;
  std::mutex infos_mu;
  auto verify = [&](Req &m) {
    CHECK(m.bi != nullptr);
    {
      std::lock_guard<std::mutex> lk(infos_mu);
      infos.push_back(*m.bi);
    }
    callers_seen += m.bi->callers;
    submissions++;
    store.record_submission(0, tel::kind_of(m), m.bi->callers, m.bi->sets);
    in_verify++;
    if (m.n == 1 && m.msgs[0] == 0xAA) spin_until([&] { return release.load() != 0; });  // the blocker
    for (size_t s = 0; s < m.nseg; s++) m.verdicts[s] = 0;
    m.ok = true;
  };

  // 1. a lone caller: no hold, no window, the time before its submission is queue, then run
  {
    Caller a(true);
    const uint64_t t0 = fake_clock();
    CHECK(co.submit(a.req, cfg, verify));
    const uint64_t t1 = fake_clock();
    const tel::CallTimes ct = tel::call_times(a.ph, t0, t1);
    CHECK(a.ph.hold_ns == 0 && a.ph.window_ns == 0 && a.ph.submit_ns > t0 && a.ph.lead_ns > a.ph.submit_ns);
    CHECK(ct.queue == a.ph.lead_ns - a.ph.submit_ns && ct.run == a.ph.run_ns && ct.run > 0);
    CHECK(ct.total == t1 - t0 && ct.total >= ct.hold + ct.window + ct.queue + ct.run);
    CHECK(infos.size() == 1 && infos[0].callers == 1 && infos[0].sets == 1 && infos[0].first_arrival_ns == a.ph.submit_ns &&
          infos[0].lead_ns == a.ph.lead_ns);
  }
  // 2. a blocker in flight, a leader in its window, a follower that ends the window
  Caller blocker(true), lead(true), follow(true);
  blocker.msg[0] = 0xAA;
  const int seen = in_verify.load();
  std::thread tb([&] { co.submit(blocker.req, cfg, verify); });
  spin_until([&] { return in_verify.load() == seen + 1; });
  uint64_t before = g_ticks.load();
  std::thread tl([&] { co.submit(lead.req, cfg, verify); });
  spin_until([&] { return g_ticks.load() >= before + 2; });  // submit and window start were stamped: it waits
  std::thread tf([&] { co.submit(follow.req, cfg, verify); });
  tl.join();
  tf.join();
  release = 1;
  tb.join();
  CHECK(lead.verdict == 0 && follow.verdict == 0 && blocker.verdict == 0);
  CHECK(lead.ph.lead_ns == follow.ph.lead_ns && lead.ph.run_ns == follow.ph.run_ns && lead.ph.run_ns > 0);  // one batch
  CHECK(lead.ph.window_ns > 0 && follow.ph.window_ns == 0 && lead.ph.hold_ns == 0 && follow.ph.hold_ns == 0);
  {
    const tel::CallTimes cl = tel::call_times(lead.ph, lead.ph.submit_ns, lead.ph.lead_ns + lead.ph.run_ns);
    const tel::CallTimes cf = tel::call_times(follow.ph, follow.ph.submit_ns, follow.ph.lead_ns + follow.ph.run_ns);
    CHECK(follow.ph.submit_ns > lead.ph.submit_ns);
    // the follower's queue is the leader's window + queue, less the time the follower came later
    CHECK(cf.queue == cl.window + cl.queue - (follow.ph.submit_ns - lead.ph.submit_ns));
    CHECK(cl.run == cf.run && cl.total == cl.window + cl.queue + cl.run && cf.total == cf.queue + cf.run);
  }
  {
    std::lock_guard<std::mutex> lk(infos_mu);
    bool found = false;
    for (const sched::BatchInfo &b : infos)
      if (b.callers == 2) found = b.sets == 2 && b.first_arrival_ns == lead.ph.submit_ns && b.lead_ns == lead.ph.lead_ns;
    CHECK(found);
  }
  // 3. a held caller
  {
    std::atomic<int> hold{1};
    sched::Config hc = cfg;
    hc.hold = &hold;
    hc.hold_max_us = 60 * 1000000;
    Caller h(true);
    before = g_ticks.load();
    std::thread tholder([&] { co.submit(h.req, hc, verify); });
    spin_until([&] { return g_ticks.load() >= before + 2; });  // submit and hold start were stamped
    hold = 0;
    co.wake();
    tholder.join();
    const tel::CallTimes ct = tel::call_times(h.ph, h.ph.submit_ns, h.ph.lead_ns + h.ph.run_ns);
    CHECK(h.verdict == 0 && ct.hold > 0 && ct.window == 0 && ct.total == ct.hold + ct.queue + ct.run);
  }
  // 4. conservation: 8 threads x 50 requests; the callers of all submissions are the requests submitted
  {
    const uint64_t c0 = callers_seen.load();
    cfg.merge_window_us = 200;
    cfg.merge_target = 6;
    std::vector<std::thread> th;
    std::atomic<int> good{0};
    for (int t = 0; t < 8; t++)
      th.emplace_back([&] {
        for (int i = 0; i < 50; i++) {
          Caller c(true);
          if (co.submit(c.req, cfg, verify) && c.verdict == 0 && c.ph.run_ns > 0 && c.ph.lead_ns >= c.ph.submit_ns) good++;
        }
      });
    for (auto &t : th) t.join();
    CHECK(good.load() == 400 && callers_seen.load() - c0 == 400);
    gbls_telemetry_snapshot snap;
    store.read(snap);
    const gbls_telemetry_cell &c = snap.cell[0][tel::K_BATCH];
    CHECK(c.callers == callers_seen.load() && c.submissions == submissions.load() && c.submitted_sets == c.callers);
  }
  // 5. without the coalescer: one submission per caller, stamped the same way
  {
    sched::Config nc = cfg;
    nc.coalesce = false;
    Caller a(true);
    CHECK(co.submit(a.req, nc, verify));
    CHECK(a.ph.lead_ns == a.ph.submit_ns && a.ph.run_ns > 0 && a.ph.window_ns == 0);
  }
  // 6. hooks absent (level 0): requests without phases never read the clock, with or without the
  // coalescer, and the verifier sees no batch information
  {
    const uint64_t ticks = g_ticks.load();
    auto plain = [&](Req &m) {
      CHECK(m.bi == nullptr);
      for (size_t s = 0; s < m.nseg; s++) m.verdicts[s] = 0;
      m.ok = true;
    };
    std::vector<std::thread> th;
    for (int t = 0; t < 4; t++)
      th.emplace_back([&, t] {
        sched::Config c2 = cfg;
        c2.coalesce = t != 3;
        for (int i = 0; i < 50; i++) {
          Caller c(false);
          CHECK(co.submit(c.req, c2, plain) && c.verdict == 0);
        }
      });
    for (auto &t : th) t.join();
    sched::Config off = cfg;
    off.clock = nullptr;  // ... and a request with phases under a configuration without a clock
    Caller c(true);
    CHECK(co.submit(c.req, off, plain) && c.ph.submit_ns == 0 && c.ph.lead_ns == 0 && c.ph.run_ns == 0);
    CHECK(g_ticks.load() == ticks);
  }
  std::printf("scheduler ok\n");
}

// ---------------------------------------------------------------- stub contexts: the two host waits
// A lease that waits for a context and a wait on a staging slot, through the hooks the engine itself
// uses (tel::timed_acquire around sched::CtxPool::acquire, tel::timed_wait around the slot's event).
struct StubCtx {
  int cls = 0;
  bool used = false;
  int last_stream = 0;
  bool idle_on_gpu() { return true; }
};
static void waits() {
  sched::CtxPool<StubCtx> pool;
  tel::StoreT<8> store;
  std::vector<StubCtx *> held;
  bool fresh = false;
  uint64_t b = 0, l = 0;
  for (int i = 0; i < sched::kMaxCtx[1]; i++) {  // every block-class context leased: each lease costs one tick
    held.push_back(tel::timed_acquire(pool, false, 0, 1, &fresh, fake_clock, &b, &l));
    CHECK(fresh && held.back()->cls == 1 && l - b == 1000);
  }
  // the next lease of the class waits until one comes back; the clock moves five ticks meanwhile
  uint64_t wb = 0, wl = 0;
  const uint64_t before = g_ticks.load();
  StubCtx *late = nullptr;
  std::thread waiter([&] {
    bool f = true;
    late = tel::timed_acquire(pool, false, 0, 1, &f, fake_clock, &wb, &wl);
    CHECK(!f);
  });
  spin_until([&] { return g_ticks.load() == before + 1; });  // its begin stamp: it is inside acquire
  for (int i = 0; i < 5; i++) fake_clock();
  pool.release(held.back());
  waiter.join();
  CHECK(late == held.back() && wl - wb == 6000);
  // a normal-class lease is not held up by the exhausted block class
  StubCtx *n = tel::timed_acquire(pool, false, 0, 0, &fresh, fake_clock, &b, &l);
  CHECK(fresh && n->cls == 0 && l - b == 1000);
  // a wait on a staging slot that takes three ticks, twice; without a shard nothing is read
  tel::StagingWaits sw;
  auto slot_wait = [] { return (int)(fake_clock(), fake_clock(), fake_clock() != 0); };
  CHECK(tel::timed_wait(fake_clock, &sw, slot_wait) == 1 && sw.ns == 4000 && sw.count == 1);
  CHECK(tel::timed_wait(fake_clock, &sw, slot_wait) == 1 && sw.ns == 8000 && sw.count == 2);
  const uint64_t ticks = g_ticks.load();
  CHECK(tel::timed_wait(fake_clock, nullptr, [] { return 7; }) == 7 && g_ticks.load() == ticks);
  uint64_t nb = 5, nl = 5;
  pool.release(n);
  CHECK(tel::timed_acquire(pool, false, 0, 0, &fresh, nullptr, &nb, &nl) == n && nb == 5 && nl == 5 && g_ticks.load() == ticks);
  // ... and they arrive in the shard's histograms and counters
  gbls_telemetry_record r{};
  r.kind = tel::K_BATCH, r.staging_wait_ns = sw.ns, r.staging_waits = sw.count;
  store.record_shard(r, 0, wl - wb, 0, sw.ns + 1000, 0, true);
  gbls_telemetry_snapshot snap;
  store.read(snap);
  const gbls_telemetry_cell &c = snap.cell[0][tel::K_BATCH];
  CHECK(c.shards == 1 && c.staging_waits == 2 && c.phase[tel::P_LEASE].sum_ns == 6000 && c.phase[tel::P_LEASE].bucket[3] == 1);
  CHECK(c.phase[tel::P_STAGING].sum_ns == 8000 && c.phase[tel::P_STAGING].count == 1 &&
        c.phase[tel::P_ENQUEUE].sum_ns >= c.phase[tel::P_STAGING].sum_ns);
  int leased = 0;
  pool.for_each([&](StubCtx &) { leased++; });
  CHECK(leased == sched::kMaxCtx[1] + 1);
  std::printf("waits ok\n");
}

// ---------------------------------------------------------------- level switched on under a leader
// A caller that carries phases but was led by a configuration without a clock has no lead stamp:
// nothing waited is recorded for it, and nothing wraps.
static void unstamped() {
  sched::CallPhases p;
  p.submit_ns = 5000;  // lead_ns, run_ns stay 0
  const tel::CallTimes ct = tel::call_times(p, 4000, 9000);
  CHECK(ct.queue == 0 && ct.hold == 0 && ct.window == 0 && ct.run == 0 && ct.total == 5000);
  std::printf("unstamped ok\n");
}

int main() {
  buckets();
  ring_order();
  ring_threads();
  counters_conserved();
  scheduler();
  waits();
  unstamped();
  std::printf("telemetry: OK\n");
  return 0;
}
