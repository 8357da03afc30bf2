// The coalescer's merge of fold requests (grandine_amd/csrc/gbls_sched.h), stand-alone: the
// requests behind gbls_verify_each_fold with a recording fake verifier in place of the GPU
// pipeline.  tests/test_fold_sched.py builds and runs this program plainly and under
// AddressSanitizer + UndefinedBehaviorSanitizer, and checks the merged CSR it prints against a
// concatenation of its own.
//
//   1. kinds: a fold request (with or without groups) merges with neither a span single-check
//      request, a span batch nor a local request, and takes no earlier kind's value.
//   2. run_merged over five fold requests (one without groups, one with an empty group, one naming
//      a set twice, one without fold_bytes): the merged fold_set / fold_off equal the concatenation
//      computed here (each caller's entries moved up by its first set, its groups behind the earlier
//      callers'), each caller receives exactly its slices of the points, counts and bytes beside
//      its verdicts and statuses, and a failed verification reaches every caller with no fold
//      output written.
//   3. Coalescer::submit from eight threads, 40 rounds: fold callers (one of them without groups),
//      a span single-check caller and a local caller.  No submission mixes kinds; every caller
//      receives its own outputs.
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
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
      std::fprintf(stderr, "sched_fold: %s (line %d)\n", what, __LINE__);  \
      std::exit(1);                                                        \
    }                                                                      \
  } while (0)

// One caller's single checks over plain sets, with storage.  Message i starts with the caller's id.
struct Caller {
  int id = 0;
  size_t n = 0;
  bool fold = true, local = false, with_bytes = true;
  std::vector<uint8_t> msgs, sigc, bits, cbits, pkb;
  std::vector<uint32_t> com, boff, idx, off, seg, fset, foff;
  std::vector<int32_t> verdicts, sst, kst;
  std::vector<P2> fout;
  std::vector<uint8_t> fbytes;
  std::vector<uint32_t> fcnt;
  size_t nfold() const { return foff.empty() ? 0 : foff.size() - 1; }
  Req req() {
    Req r{msgs.data(), nullptr, sched::KeySource<P1>(), nullptr, n, seg.data(), n, verdicts.data()};
    r.src.com = com.data();
    r.src.cbits = reinterpret_cast<const uint8_t(*)[8]>(cbits.data());
    r.src.bits = bits.data();
    r.src.bits_off = boff.data();
    r.src.idx = idx.data();
    r.src.off = off.data();
    r.src.local = local;
    if (local) {
      r.src.pkb = reinterpret_cast<const uint8_t(*)[48]>(pkb.data());
      r.src.npkb = pkb.size() / 48;
    }
    r.src.fold = fold;
    if (nfold()) {
      r.src.fold_set = fset.data();
      r.src.fold_off = foff.data();
      r.src.nfold = nfold();
      r.src.fold_out = fout.data();
      r.src.fold_bytes = with_bytes ? reinterpret_cast<uint8_t(*)[96]>(fbytes.data()) : nullptr;
      r.src.fold_count = fcnt.data();
    }
    r.sigs_c = sigc.data();
    r.sig_status = sst.data();
    r.key_status = kst.data();
    return r;
  }
};

static Caller make_caller(int id, size_t n, const std::vector<std::vector<uint32_t>> &groups, bool fold = true,
                          bool local = false, bool with_bytes = true) {
  Caller c;
  c.id = id;
  c.n = n;
  c.fold = fold;
  c.local = local;
  c.with_bytes = with_bytes;
  c.msgs.assign(32 * n, 0);
  c.sigc.assign(96 * n, 0);
  c.cbits.assign(8 * n + 8, 0);
  c.com.assign(n, kNoCommittee);
  c.bits.assign(1, 0);
  c.boff.assign(n + 1, 0);
  c.pkb.assign(local ? 48 : 0, (uint8_t)id);
  for (size_t i = 0; i <= n; i++) {
    c.off.push_back((uint32_t)i);
    c.seg.push_back((uint32_t)i);
  }
  for (size_t i = 0; i < n; i++) {
    c.msgs[32 * i] = (uint8_t)id;
    c.msgs[32 * i + 1] = (uint8_t)i;
    c.sigc[96 * i] = (uint8_t)(17 * id + 3 * i + 1);
    c.idx.push_back((uint32_t)(100 * id + i));
  }
  if (c.idx.empty()) c.idx.push_back(0);
  if (!groups.empty()) c.foff.push_back(0);
  for (const auto &g : groups) {
    for (uint32_t s : g) {
      CHECK(s < n, "a group names the caller's own sets");
      c.fset.push_back(s);
    }
    c.foff.push_back((uint32_t)c.fset.size());
  }
  if (c.fset.empty()) c.fset.push_back(0);
  c.verdicts.assign(n, -1);
  c.sst.assign(n, -1);
  c.kst.assign(n, -1);
  // the callers' own pre-fill (the C entry writes it before the request is made)
  c.fout.assign(c.nfold(), P2{});
  c.fbytes.assign(96 * c.nfold(), 0);
  for (size_t g = 0; g < c.nfold(); g++) c.fbytes[96 * g] = 0xc0;
  c.fcnt.assign(c.nfold(), 0);
  return c;
}

// What the fake verifier answers, as functions of a request's OWN arrays.
static int32_t want_sig_status(const Req &r, size_t i) { return 2 + r.sigs_c[96 * i] % 5; }
static int32_t want_key_status(const Req &r, size_t i) { return (int32_t)(r.src.idx[r.src.off[i]] * 7u + 1); }
static int32_t want_verdict(const Req &r, size_t i) { return r.msgs[32 * i] * 256 + r.msgs[32 * i + 1]; }
// group g: a hash over the (caller id, set number) of its entries, in order -- a wrong rebase of
// fold_set, or a slice handed to the wrong caller, changes it
static uint32_t want_fold(const Req &r, size_t g) {
  uint32_t h = 11;
  for (uint32_t k = r.src.fold_off[g]; k < r.src.fold_off[g + 1]; k++) {
    const uint32_t s = r.src.fold_set[k];
    h = h * 167u + r.msgs[32 * s] * 256u + r.msgs[32 * s + 1] + 1;
  }
  return h;
}

static void answer(Req &m, bool ok, int err) {
  for (size_t i = 0; i < m.n; i++) {
    m.verdicts[i] = want_verdict(m, i);
    m.sig_status[i] = want_sig_status(m, i);
    m.key_status[i] = want_key_status(m, i);
  }
  // (a failing pipeline may have written part of its fold outputs: they must not reach a caller)
  for (size_t g = 0; g < m.src.nfold; g++) {
    const uint32_t h = want_fold(m, g);
    P2 *out = static_cast<P2 *>(m.src.fold_out);
    std::memcpy(out[g].b, &h, 4);
    out[g].b[191] = (uint8_t)(h >> 8);
    m.src.fold_count[g] = m.src.fold_off[g + 1] - m.src.fold_off[g];
    if (m.src.fold_bytes) {
      std::memcpy(m.src.fold_bytes[g], &h, 4);
      m.src.fold_bytes[g][95] = (uint8_t)h;
    }
  }
  m.ok = ok;
  m.err = err;
}

static void check_outputs(Caller &c, const Req &r, bool ok, int err) {
  CHECK(r.ok == ok && r.err == err, "ok / err of a merged caller");
  for (size_t i = 0; i < c.n; i++) {
    CHECK(c.verdicts[i] == want_verdict(r, i), "a caller's verdicts");
    CHECK(c.sst[i] == want_sig_status(r, i), "a caller's signature statuses");
    CHECK(c.kst[i] == want_key_status(r, i), "a caller's key statuses");
  }
  for (size_t g = 0; g < c.nfold(); g++) {
    uint32_t h = 0, hb = 0;
    std::memcpy(&h, c.fout[g].b, 4);
    std::memcpy(&hb, &c.fbytes[96 * g], 4);
    if (ok) {
      const uint32_t want = want_fold(r, g);
      CHECK(h == want && c.fout[g].b[191] == (uint8_t)(want >> 8), "a caller's fold points");
      CHECK(c.fcnt[g] == c.foff[g + 1] - c.foff[g], "a caller's fold counts");
      if (c.with_bytes) CHECK(hb == want && c.fbytes[96 * g + 95] == (uint8_t)want, "a caller's fold bytes");
    } else {  // a failure: nothing of the fold reaches a caller, its pre-fill stands
      CHECK(h == 0 && c.fout[g].b[191] == 0 && c.fcnt[g] == 0, "fold outputs after a failure");
      CHECK(c.fbytes[96 * g] == 0xc0 && c.fbytes[96 * g + 95] == 0, "fold bytes after a failure");
    }
    if (!c.with_bytes) CHECK(c.fbytes[96 * g] == 0xc0 && c.fbytes[96 * g + 1] == 0, "bytes nobody asked for");
  }
}

static void test_kinds() {
  Caller f = make_caller(1, 3, {{0, 1}, {2}});
  Caller f0 = make_caller(2, 2, {});            // the fold call without groups
  Caller s = make_caller(3, 2, {}, false);      // the each-call over span sets
  Caller l = make_caller(4, 2, {}, false, true);  // the each-call over local sets
  Req rf = f.req(), rf0 = f0.req(), rs = s.req(), rl = l.req();
  Req rb = rs;                                  // a span batch
  uint64_t rands[2] = {1, 2};
  rb.rands = rands;
  CHECK(rf.kind() == rf0.kind(), "fold requests with and without groups are one kind");
  CHECK(rf.kind() != rs.kind() && rf.kind() != rl.kind() && rf.kind() != rb.kind(), "a fold request is a kind of its own");
  CHECK((rf.kind() & 64) && !(rs.kind() & 64) && !(rl.kind() & 64) && !(rb.kind() & 64), "the fold bit");
  CHECK((rf.kind() & 16) && rf.kind() == (rs.kind() | 64), "one more bit beside the span bit");
  CHECK(rs.kind() < 64 && rl.kind() < 64 && rb.kind() < 64, "no earlier kind reaches the fold bit");
}

static std::vector<Caller> five() {
  std::vector<Caller> cs;
  cs.push_back(make_caller(1, 3, {{0, 1, 2}, {}, {2, 2, 0}}));            // an empty group, a set named twice
  cs.push_back(make_caller(2, 2, {}));                                     // nfold == 0 among the others
  cs.push_back(make_caller(3, 1, {{0}}));
  cs.push_back(make_caller(4, 5, {{4}, {0, 1, 2, 3, 4}, {3, 1}}, true, false, false));  // no bytes asked for
  cs.push_back(make_caller(5, 2, {{1, 0}, {1}}));
  return cs;
}

static void test_merge(bool fail) {
  std::vector<Caller> cs = five();
  std::vector<Req> reqs;
  for (Caller &c : cs) reqs.push_back(c.req());
  std::vector<Req *> batch;
  for (Req &r : reqs) batch.push_back(&r);
  // the concatenation, computed here
  std::vector<uint32_t> want_set, want_off{0};
  size_t at = 0;
  for (Caller &c : cs) {
    for (size_t g = 0; g < c.nfold(); g++) {
      for (uint32_t k = c.foff[g]; k < c.foff[g + 1]; k++) want_set.push_back((uint32_t)at + c.fset[k]);
      want_off.push_back((uint32_t)want_set.size());
    }
    at += c.n;
  }
  int calls = 0;
  std::vector<uint32_t> got_set, got_off;
  sched::run_merged(batch, [&](Req &m) {
    calls++;
    CHECK(m.n == 13 && m.nseg == 13 && !m.rands && m.src.fold && m.spans(), "the merged form");
    CHECK(m.src.nfold == want_off.size() - 1 && m.src.fold_out && m.src.fold_count && m.src.fold_bytes, "the merged groups");
    got_off.assign(m.src.fold_off, m.src.fold_off + m.src.nfold + 1);
    got_set.assign(m.src.fold_set, m.src.fold_set + got_off.back());
    for (size_t i = 0; i <= m.n; i++) CHECK(m.seg_off[i] == i, "identity segments");
    for (size_t g = 0; g < m.src.nfold; g++) CHECK(m.src.fold_count[g] == 0, "pre-fill of the merged counts");
    answer(m, !fail, fail ? 101 : 0);
  });
  CHECK(calls == 1, "one submission");
  CHECK(got_off == want_off && got_set == want_set, "the merged CSR");
  for (size_t k = 0; k < cs.size(); k++) check_outputs(cs[k], reqs[k], !fail, fail ? 101 : 0);
  if (!fail) {
    std::printf("csr_off");
    for (uint32_t v : got_off) std::printf(" %u", v);
    std::printf("\ncsr_set");
    for (uint32_t v : got_set) std::printf(" %u", v);
    std::printf("\n");
    for (Caller &c : cs) {
      std::printf("caller %zu", c.n);
      for (size_t g = 0; g < c.nfold(); g++) {
        std::printf(" |");
        for (uint32_t k = c.foff[g]; k < c.foff[g + 1]; k++) std::printf(" %u", c.fset[k]);
      }
      std::printf("\n");
    }
  }
}

// a merged request without any group at all: no fold arrays are handed on
static void test_merge_without_groups() {
  Caller a = make_caller(1, 2, {}), b = make_caller(2, 3, {});
  Req ra = a.req(), rb = b.req();
  std::vector<Req *> batch{&ra, &rb};
  sched::run_merged(batch, [&](Req &m) {
    CHECK(m.src.fold && m.src.nfold == 0 && !m.src.fold_set && !m.src.fold_off && !m.src.fold_out, "no groups");
    answer(m, true, 0);
  });
  check_outputs(a, ra, true, 0);
  check_outputs(b, rb, true, 0);
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
  auto verify = [&](Req &m) {
    std::set<int> ids;
    for (size_t i = 0; i < m.n; i++) ids.insert(m.msgs[32 * i]);
    {
      std::lock_guard<std::mutex> lk(mu);
      // ids 1..6: fold callers (6 without groups); 7: the span each-call; 8: the local each-call
      for (int id : ids) CHECK((id <= 6) == m.src.fold && (id == 8) == m.src.local, "a submission mixed kinds");
    }
    if (ids.size() > 1) merged++;
    answer(m, true, 0);
  };
  std::vector<std::thread> threads;
  for (int id = 1; id <= 8; id++)
    threads.emplace_back([&, id] {
      for (int round = 0; round < 40; round++) {
        const size_t n = 1 + (size_t)((id + round) % 6);
        std::vector<std::vector<uint32_t>> groups;
        if (id <= 5)
          for (size_t g = 0; g < 1 + (size_t)(round % 3); g++) {
            std::vector<uint32_t> grp;
            for (size_t k = 0; k < (g + (size_t)id + (size_t)round) % 4; k++) grp.push_back((uint32_t)((k * 5 + g + (size_t)round) % n));
            groups.push_back(grp);
          }
        Caller c = make_caller(id, n, groups, id <= 6, id == 8, id % 2 == 1);
        Req r = c.req();
        CHECK(co.submit(r, cfg, verify) && r.done, "submit");
        check_outputs(c, r, true, 0);
      }
    });
  for (auto &t : threads) t.join();
  std::printf("sched_fold: merged submissions %d\n", merged.load());
}

int main() {
  test_kinds();
  test_merge(false);
  test_merge(true);
  test_merge_without_groups();
  test_threads();
  std::printf("sched_fold: OK\n");
  return 0;
}
