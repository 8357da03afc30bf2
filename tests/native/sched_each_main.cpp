// The coalescer's merge of span-source requests (grandine_amd/csrc/gbls_sched.h), stand-alone:
// the requests behind gbls_verify_each_spans and gbls_verify_items_spans with a recording fake
// verifier in place of the GPU pipeline.  tests/test_each_sched.py builds and runs this program
// plainly and under AddressSanitizer + UndefinedBehaviorSanitizer.
//
//   1. kinds: span requests with and without index ranges are one kind; single checks, batches,
//      point- and index-source requests are kinds of their own.
//   2. run_merged over five span requests of different sizes (one without pk_off, one of plain
//      sets only, bit strings of odd byte lengths so that no string starts where a word does, an
//      empty item): the merged com, cbits, bits, bits_off, idx, off, seg_off and rands equal the
//      concatenation computed here, each caller receives exactly its slice of the verdicts and of
//      both status arrays, and a failed verification reaches every caller (ok and err).
//   3. Coalescer::submit from eight threads: span batches, one span single-check request, one
//      block-class span batch and one point-source batch, 40 rounds.  No submission mixes kinds
//      or classes, every caller receives its own outputs.
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <mutex>
#include <set>
#include <thread>

#include "gbls_sched.h"

namespace sched = gbls::sched;

struct P1 {
  uint8_t b[96];
};
struct P2 {
  uint8_t b[192];
};
using Req = sched::Request<P1, P2>;
constexpr uint32_t kNoCommittee = 0xffffffffu;

#define CHECK(cond, what)                                                  \
  do {                                                                     \
    if (!(cond)) {                                                         \
      std::fprintf(stderr, "sched_each: %s (line %d)\n", what, __LINE__);  \
      std::exit(1);                                                        \
    }                                                                      \
  } while (0)

// One caller's batch with storage.  Message i starts with the caller's id, so that the fake verifier
// can tell whose sets it was handed.
struct Caller {
  int id = 0;
  size_t n = 0;
  bool single = false, with_off = true, points = false;
  int prio = 0;
  std::vector<uint8_t> msgs, sigc, bits;
  std::vector<uint8_t> cbits;  // 8 n
  std::vector<uint32_t> com, boff, idx, off, seg;
  std::vector<uint64_t> rands;
  std::vector<P1> pts;
  std::vector<int32_t> verdicts, sst, kst;
  Req req() {
    Req r{msgs.data(), nullptr, sched::KeySource<P1>(), single ? nullptr : rands.data(), n, seg.data(),
          seg.size() - 1, verdicts.data()};
    if (points) {
      r.src.pts = pts.data();
    } else {
      r.src.com = com.data();
      r.src.cbits = reinterpret_cast<const uint8_t(*)[8]>(cbits.data());
      r.src.bits = bits.data();
      r.src.bits_off = boff.data();
      if (with_off) {
        r.src.idx = idx.data();
        r.src.off = off.data();
      }
      r.key_status = kst.data();
    }
    r.sigs_c = sigc.data();
    r.sig_status = sst.data();
    r.prio = prio;
    return r;
  }
};

// plain[i]: set i is a plain list of 1 + (i + id) % 3 indices; else a span set with a string of
// blen(i) bytes.  seg: the item offsets (ignored for single checks).
static Caller make_caller(int id, size_t n, const std::vector<bool> &plain, std::vector<uint32_t> seg, bool single,
                          bool with_off, int prio = 0, bool points = false) {
  Caller c;
  c.id = id;
  c.n = n;
  c.single = single;
  c.with_off = with_off;
  c.prio = prio;
  c.points = points;
  c.msgs.assign(32 * n, 0);
  c.sigc.assign(96 * n, 0);
  c.cbits.assign(8 * n, 0);
  c.com.resize(n);
  c.boff.assign(1, 0);
  c.off.assign(1, 0);
  c.rands.resize(n);
  c.pts.resize(points ? n : 0);
  for (size_t i = 0; i < n; i++) {
    c.msgs[32 * i] = (uint8_t)id;
    c.msgs[32 * i + 1] = (uint8_t)i;
    c.sigc[96 * i] = (uint8_t)(17 * id + 3 * i + 1);
    c.rands[i] = 1000u * (unsigned)id + i + 1;
    if (points) c.pts[i].b[0] = (uint8_t)(id + i);
    if (plain[i]) {
      c.com[i] = kNoCommittee;
      CHECK(with_off, "a plain set needs index ranges");
      for (size_t k = 0; k < 1 + (i + (size_t)id) % 3; k++) c.idx.push_back((uint32_t)(100 * id + 10 * i + k));
    } else {
      c.com[i] = (uint32_t)(7 * id + i);
      c.cbits[8 * i + (i % 8)] = (uint8_t)(1u << (id % 8));
      c.cbits[8 * i + 7] |= (uint8_t)(i + 1);
      const size_t blen = 1 + 2 * ((i + (size_t)id) % 3);  // 1, 3 or 5 bytes: odd offsets
      for (size_t k = 0; k < blen; k++) c.bits.push_back((uint8_t)(31 * id + 5 * i + k + 1));
    }
    c.boff.push_back((uint32_t)c.bits.size());
    c.off.push_back((uint32_t)c.idx.size());
  }
  if (single) {
    seg.resize(n + 1);
    for (size_t i = 0; i <= n; i++) seg[i] = (uint32_t)i;
  }
  CHECK(seg.front() == 0 && seg.back() == n, "item offsets");
  c.seg = seg;
  c.verdicts.assign(seg.size() - 1, -1);
  c.sst.assign(n, -1);
  c.kst.assign(n, -1);
  if (c.bits.empty()) c.bits.push_back(0);  // (data() of an empty vector may be null)
  if (c.idx.empty()) c.idx.push_back(0);
  return c;
}

// What the fake verifier answers, as functions of a request's OWN arrays: a wrong rebase of
// bits_off or off, or a slice handed to the wrong caller, changes them.
static int32_t want_sig_status(const Req &r, size_t i) { return 2 + r.sigs_c[96 * i] % 5; }
static int32_t want_key_status(const Req &r, size_t i) {
  if (!r.spans()) return -1;
  uint32_t h = r.src.com[i] * 31u;
  for (int k = 0; k < 8; k++) h = h * 131u + r.src.cbits[i][k];
  for (uint32_t k = r.src.bits_off[i]; k < r.src.bits_off[i + 1]; k++) h = h * 137u + r.src.bits[k];
  h = h * 139u + (r.src.bits_off[i + 1] - r.src.bits_off[i]);
  uint32_t nk = 0;  // (no index ranges: an empty range, as the merged request states it)
  if (r.src.off) {
    for (uint32_t k = r.src.off[i]; k < r.src.off[i + 1]; k++) h = h * 149u + r.src.idx[k];
    nk = r.src.off[i + 1] - r.src.off[i];
  }
  h = h * 151u + nk;
  return (int32_t)(h & 0x7fffffffu);
}
static int32_t want_verdict(const Req &r, size_t s) {
  uint32_t h = 7;
  for (uint32_t i = r.seg_off[s]; i < r.seg_off[s + 1]; i++)
    h = h * 163u + r.msgs[32 * i] * 256u + r.msgs[32 * i + 1] + (uint32_t)(r.rands ? r.rands[i] : 1);
  return (int32_t)(h & 0x7fffffffu);
}

struct Seen {
  std::vector<uint8_t> msgs, sigc, cbits, bits;
  std::vector<uint32_t> com, boff, idx, off, seg;
  std::vector<uint64_t> rands;
  size_t n = 0, nseg = 0;
  bool single = false, has_off = false;
  int prio = 0;
};

static void answer(Req &m, bool ok, int err) {
  for (size_t s = 0; s < m.nseg; s++) m.verdicts[s] = want_verdict(m, s);
  for (size_t i = 0; i < m.n; i++) {
    if (m.sig_status) m.sig_status[i] = want_sig_status(m, i);
    if (m.key_status) m.key_status[i] = want_key_status(m, i);
  }
  m.ok = ok;
  m.err = err;
}

static void check_outputs(Caller &c, const Req &r, bool ok, int err) {
  CHECK(r.ok == ok && r.err == err, "ok / err of a merged caller");
  for (size_t s = 0; s + 1 < c.seg.size(); s++) CHECK(c.verdicts[s] == want_verdict(r, s), "a caller's verdicts");
  for (size_t i = 0; i < c.n; i++) {
    CHECK(c.sst[i] == want_sig_status(r, i), "a caller's signature statuses");
    CHECK(c.kst[i] == want_key_status(r, i), "a caller's key statuses");
  }
}

static void test_kinds() {
  Caller a = make_caller(1, 3, {false, true, false}, {0, 1, 3}, false, true);
  Caller b = make_caller(2, 2, {false, false}, {0, 2}, false, false);
  Caller s = make_caller(3, 2, {false, true}, {}, true, true);
  Caller p = make_caller(4, 2, {false, false}, {0, 2}, false, true, 0, true);
  Req ra = a.req(), rb = b.req(), rs = s.req(), rp = p.req();
  CHECK(ra.spans() && rb.spans() && rs.spans() && !rp.spans(), "spans()");
  CHECK(ra.kind() == rb.kind(), "span batches with and without index ranges are one kind");
  CHECK(ra.kind() != rs.kind(), "single checks are a kind of their own");
  CHECK(ra.kind() != rp.kind() && rs.kind() != rp.kind(), "a point source is another kind");
  // no earlier kind collides: those are the values below 16
  CHECK(ra.kind() >= 16 && rs.kind() >= 16 && rp.kind() < 16, "the span bit");
  Req ri = rp;  // an index source with ranges
  ri.src.pts = nullptr;
  ri.src.idx = a.idx.data();
  ri.src.off = a.off.data();
  CHECK(ri.kind() < 16 && ri.kind() != rp.kind(), "an index source is another kind");
  CHECK(rb.nkeys() == 0 && ra.nkeys() == a.off[a.n] && rp.nkeys() == 2, "nkeys");
}

static void test_merge(bool single, bool fail) {
  // sizes 1, 4, 2, 5, 3; caller 2 has no index ranges, caller 3 only plain sets, caller 4 an empty item
  std::vector<Caller> cs;
  cs.push_back(make_caller(1, 1, {false}, {0, 1}, single, true));
  cs.push_back(make_caller(2, 4, {false, false, false, false}, {0, 3, 4}, single, false));
  cs.push_back(make_caller(3, 2, {true, true}, {0, 1, 2}, single, true));
  cs.push_back(make_caller(4, 5, {false, true, false, false, true}, {0, 2, 2, 5}, single, true));
  cs.push_back(make_caller(5, 3, {true, false, false}, {0, 3}, single, true));
  std::vector<Req> reqs;
  for (Caller &c : cs) reqs.push_back(c.req());
  std::vector<Req *> batch;
  for (Req &r : reqs) batch.push_back(&r);
  // the concatenation, computed here
  Seen want;
  want.seg.push_back(0);
  want.boff.push_back(0);
  want.off.push_back(0);
  for (Caller &c : cs) {
    const size_t nb = c.boff[c.n], nk = c.with_off ? c.off[c.n] : 0;
    for (size_t s = 1; s < c.seg.size(); s++) want.seg.push_back((uint32_t)(want.n + c.seg[s]));
    for (size_t i = 1; i <= c.n; i++) {
      want.boff.push_back((uint32_t)(want.bits.size() + c.boff[i]));
      want.off.push_back((uint32_t)(want.idx.size() + (c.with_off ? c.off[i] : 0)));
    }
    want.msgs.insert(want.msgs.end(), c.msgs.begin(), c.msgs.end());
    want.sigc.insert(want.sigc.end(), c.sigc.begin(), c.sigc.end());
    want.com.insert(want.com.end(), c.com.begin(), c.com.end());
    want.cbits.insert(want.cbits.end(), c.cbits.begin(), c.cbits.end());
    want.bits.insert(want.bits.end(), c.bits.begin(), c.bits.begin() + (std::ptrdiff_t)nb);
    want.idx.insert(want.idx.end(), c.idx.begin(), c.idx.begin() + (std::ptrdiff_t)nk);
    want.rands.insert(want.rands.end(), c.rands.begin(), c.rands.end());
    want.n += c.n;
  }
  CHECK(want.n == 15 && want.boff[5] % 4 != 0, "the shape");
  int calls = 0;
  Seen got;
  sched::run_merged(batch, [&](Req &m) {
    calls++;
    got.n = m.n;
    got.nseg = m.nseg;
    got.single = m.rands == nullptr;
    got.has_off = m.src.off != nullptr;
    CHECK(m.spans() && m.src.off && m.sigs_c && m.sig_status && m.key_status && !m.sigs && !m.src.pts, "the merged form");
    got.msgs.assign(m.msgs, m.msgs + 32 * m.n);
    got.sigc.assign(m.sigs_c, m.sigs_c + 96 * m.n);
    got.com.assign(m.src.com, m.src.com + m.n);
    got.cbits.assign(&m.src.cbits[0][0], &m.src.cbits[0][0] + 8 * m.n);
    got.boff.assign(m.src.bits_off, m.src.bits_off + m.n + 1);
    got.off.assign(m.src.off, m.src.off + m.n + 1);
    got.bits.assign(m.src.bits, m.src.bits + got.boff[m.n]);
    got.idx.assign(m.src.idx, m.src.idx + got.off[m.n]);
    got.seg.assign(m.seg_off, m.seg_off + m.nseg + 1);
    if (m.rands) got.rands.assign(m.rands, m.rands + m.n);
    for (size_t i = 0; i < m.n; i++)  // the pre-fill of the merged outputs: fail closed
      CHECK(m.sig_status[i] == 1 && m.key_status[i] == 1, "pre-fill");
    for (size_t s = 0; s < m.nseg; s++) CHECK(m.verdicts[s] == 5, "pre-fill");
    answer(m, !fail, fail ? 101 : 0);
  });
  CHECK(calls == 1, "one submission");
  CHECK(got.n == want.n && got.nseg == want.seg.size() - 1 && got.single == single, "n, nseg, class");
  CHECK(got.msgs == want.msgs && got.sigc == want.sigc, "msgs, sigs");
  CHECK(got.com == want.com && got.cbits == want.cbits, "com, cbits");
  CHECK(got.bits == want.bits && got.boff == want.boff, "bits, bits_off");
  CHECK(got.idx == want.idx && got.off == want.off, "idx, off");
  CHECK(got.seg == want.seg, "seg_off");
  CHECK(single ? got.rands.empty() : got.rands == want.rands, "rands");
  for (size_t k = 0; k < cs.size(); k++) check_outputs(cs[k], reqs[k], !fail, fail ? 101 : 0);
}

static void test_threads() {
  auto owner = std::make_unique<sched::Coalescer<Req>>();
  auto &co = *owner;
  sched::Config cfg;
  cfg.devices = 1;
  cfg.leaders = 1;
  cfg.merge_window_us = 50;
  std::mutex mu;
  std::atomic<int> merged{0};
  // which caller ids, classes and kinds each submission held
  auto verify = [&](Req &m) {
    std::set<int> ids;
    for (size_t i = 0; i < m.n; i++) ids.insert(m.msgs[32 * i]);
    {
      std::lock_guard<std::mutex> lk(mu);
      // ids 1..5: normal span batches; 6: the span single checks; 7: the block-class span batch; 8: points
      for (int id : ids) {
        const int cls = id <= 5 ? 0 : id;
        for (int other : ids) CHECK((other <= 5 ? 0 : other) == cls, "a submission mixed kinds or classes");
      }
      CHECK(m.prio == (ids.count(7) ? 1 : 0), "the class of a submission");
      CHECK((m.rands == nullptr) == (ids.count(6) != 0), "single checks in a batch submission");
    }
    if (ids.size() > 1) merged++;
    answer(m, true, 0);
  };
  std::vector<std::thread> threads;
  for (int id = 1; id <= 8; id++)
    threads.emplace_back([&, id] {
      for (int round = 0; round < 40; round++) {
        const size_t n = 1 + (size_t)((id + round) % 6);
        std::vector<bool> plain(n);
        for (size_t i = 0; i < n; i++) plain[i] = id != 2 && (i + (size_t)round) % 3 == 0;
        std::vector<uint32_t> seg{0, (uint32_t)(n / 2), (uint32_t)n};
        Caller c = make_caller(id, n, plain, seg, id == 6, id != 2, id == 7 ? 1 : 0, id == 8);
        Req r = c.req();
        CHECK(co.submit(r, cfg, verify) && r.done, "submit");
        check_outputs(c, r, true, 0);
      }
    });
  for (auto &t : threads) t.join();
  std::printf("sched_each: merged submissions %d\n", merged.load());
}

int main() {
  test_kinds();
  for (int single = 0; single < 2; single++)
    for (int fail = 0; fail < 2; fail++) test_merge(single != 0, fail != 0);
  test_threads();
  std::printf("sched_each: OK\n");
  return 0;
}
