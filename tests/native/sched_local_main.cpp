// The coalescer's merge of local-source requests (grandine_amd/csrc/gbls_sched.h), stand-alone: the
// requests behind gbls_verify_each_local and gbls_verify_items_local with a recording fake
// verifier in place of the GPU pipeline.  tests/test_local_sched.py builds and runs this program
// plainly and under AddressSanitizer + UndefinedBehaviorSanitizer.
//
//   1. kinds: a local source (span | local) is a kind of its own, with or without a table or
//      index ranges; batches, single checks and the block class stay apart as for span sources,
//      and no earlier kind collides.
//   2. run_merged over five local requests (tables of 3, 0, 5, 1 and 2 keys; the caller with no
//      key has no local set and no index ranges at all, another names a position past its own
//      table): the merged request equals the concatenation computed here, the key tables are
//      concatenated, positions are rebased in LOCAL sets only (registry indices stay, a position
//      past a caller's own table is sent past the merged table's end), and each caller receives
//      exactly its slice of the verdicts, of both status arrays and of the table's statuses.
//      A caller without pkb_status is left alone; a failed verification reaches every caller.
//   3. Coalescer::submit from eight threads: local batches with different tables, one local
//      single-check request, one block-class local batch and one span batch, 40 rounds.  No
//      submission mixes kinds or classes, every caller receives its own outputs.
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <mutex>
#include <set>
#include <string>
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
constexpr uint32_t kNoCommittee = 0xffffffffu, kLocal = sched::kLocalSet;

#define CHECK(cond, what)                                                  \
  do {                                                                     \
    if (!(cond)) {                                                         \
      std::fprintf(stderr, "sched_local: %s (line %d)\n", what, __LINE__); \
      std::exit(1);                                                        \
    }                                                                      \
  } while (0)

// One caller's batch with storage.  Set i is 'L' (local: 1 + (i + id) % 3 positions of its table),
// 'P' (plain: registry indices, chosen BELOW the table sizes so that a rebase of them would show)
// or 'S' (a span set with a bit string of odd length).
struct Caller {
  int id = 0;
  size_t n = 0, nk = 0;
  bool single = false, local = true, with_off = true, with_pst = true;
  int prio = 0;
  std::vector<uint8_t> msgs, sigc, bits, cbits, pkb;
  std::vector<uint32_t> com, boff, idx, off, seg;
  std::vector<uint64_t> rands;
  std::vector<int32_t> verdicts, sst, kst, pst;
  Req req() {
    Req r{msgs.data(), nullptr, sched::KeySource<P1>(), single ? nullptr : rands.data(), n, seg.data(),
          seg.size() - 1, verdicts.data()};
    r.src.com = com.data();
    r.src.cbits = reinterpret_cast<const uint8_t(*)[8]>(cbits.data());
    r.src.bits = bits.data();
    r.src.bits_off = boff.data();
    if (with_off) {
      r.src.idx = idx.data();
      r.src.off = off.data();
    }
    if (local) {
      r.src.local = true;
      r.src.pkb = nk ? reinterpret_cast<const uint8_t(*)[48]>(pkb.data()) : nullptr;
      r.src.npkb = nk;
      r.pkb_status = with_pst ? pst.data() : nullptr;
    }
    r.key_status = kst.data();
    r.sigs_c = sigc.data();
    r.sig_status = sst.data();
    r.prio = prio;
    return r;
  }
};

static Caller make_caller(int id, const char *kinds, size_t nk, std::vector<uint32_t> seg, bool single, int prio = 0,
                          bool local = true, int past = -1) {
  Caller c;
  c.id = id;
  c.n = std::strlen(kinds);
  c.nk = nk;
  c.single = single;
  c.prio = prio;
  c.local = local;
  const size_t n = c.n;
  c.msgs.assign(32 * n, 0);
  c.sigc.assign(96 * n, 0);
  c.cbits.assign(8 * n, 0);
  c.com.resize(n);
  c.boff.assign(1, 0);
  c.off.assign(1, 0);
  c.rands.resize(n);
  c.pkb.assign(48 * nk + 1, 0);
  for (size_t j = 0; j < nk; j++)
    for (size_t k = 0; k < 48; k++) c.pkb[48 * j + k] = (uint8_t)(97 * id + 13 * j + k);
  bool any_list = false;
  for (size_t i = 0; i < n; i++) {
    c.msgs[32 * i] = (uint8_t)id;
    c.msgs[32 * i + 1] = (uint8_t)i;
    c.sigc[96 * i] = (uint8_t)(17 * id + 3 * i + 1);
    c.rands[i] = 1000u * (unsigned)id + i + 1;
    if (kinds[i] == 'L') {
      CHECK(local && nk, "a local set needs a table");
      c.com[i] = kLocal;
      for (size_t k = 0; k < 1 + (i + (size_t)id) % 3; k++) c.idx.push_back((uint32_t)((i + 2 * k + (size_t)id) % nk));
      if ((int)i == past) c.idx.back() = (uint32_t)nk;  // past its own table
      any_list = true;
    } else if (kinds[i] == 'P') {
      c.com[i] = kNoCommittee;
      for (size_t k = 0; k < 1 + (i + (size_t)id) % 2; k++) c.idx.push_back((uint32_t)((i + k) % 3));  // 0..2
      any_list = true;
    } else {
      c.com[i] = (uint32_t)(7 * id + i);
      c.cbits[8 * i + (i % 8)] = (uint8_t)(1u << (id % 8));
      const size_t blen = 1 + 2 * ((i + (size_t)id) % 3);
      for (size_t k = 0; k < blen; k++) c.bits.push_back((uint8_t)(31 * id + 5 * i + k + 1));
    }
    c.boff.push_back((uint32_t)c.bits.size());
    c.off.push_back((uint32_t)c.idx.size());
  }
  c.with_off = any_list;  // a caller of span sets alone passes no index ranges
  if (single) {
    seg.resize(n + 1);
    for (size_t i = 0; i <= n; i++) seg[i] = (uint32_t)i;
  }
  CHECK(seg.front() == 0 && seg.back() == n, "item offsets");
  c.seg = seg;
  c.verdicts.assign(seg.size() - 1, -1);
  c.sst.assign(n, -1);
  c.kst.assign(n, -1);
  c.pst.assign(nk + 1, -1);  // (one guard slot past the table)
  if (c.bits.empty()) c.bits.push_back(0);
  if (c.idx.empty()) c.idx.push_back(0);
  return c;
}

// What the fake verifier answers, as functions of a request's OWN arrays.  A local set's key
// status hashes the BYTES of the table keys its positions name, so a wrong rebase, a rebased
// registry index or a table in the wrong order changes it.
static int32_t want_sig_status(const Req &r, size_t i) { return 2 + r.sigs_c[96 * i] % 5; }
static int32_t want_pkb_status(const Req &r, size_t j) {
  uint32_t h = 11;
  for (int k = 0; k < 48; k++) h = h * 167u + r.src.pkb[j][k];
  return (int32_t)(h & 0x7fffffffu);
}
static int32_t want_key_status(const Req &r, size_t i) {
  uint32_t h = r.src.com[i] * 31u;
  for (int k = 0; k < 8; k++) h = h * 131u + r.src.cbits[i][k];
  for (uint32_t k = r.src.bits_off[i]; k < r.src.bits_off[i + 1]; k++) h = h * 137u + r.src.bits[k];
  h = h * 139u + (r.src.bits_off[i + 1] - r.src.bits_off[i]);
  uint32_t nk = 0;
  if (r.src.off) {
    for (uint32_t k = r.src.off[i]; k < r.src.off[i + 1]; k++) {
      const uint32_t v = r.src.idx[k];
      if (r.src.com[i] != kLocal)
        h = h * 149u + v;
      else if (v < r.src.npkb)
        h = h * 157u + (uint32_t)want_pkb_status(r, v);
      else
        h = h * 173u + 99u;  // past the table, wherever past
    }
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

static void answer(Req &m, bool ok, int err) {
  for (size_t s = 0; s < m.nseg; s++) m.verdicts[s] = want_verdict(m, s);
  for (size_t i = 0; i < m.n; i++) {
    m.sig_status[i] = want_sig_status(m, i);
    m.key_status[i] = want_key_status(m, i);
  }
  if (m.pkb_status)
    for (size_t j = 0; j < m.src.npkb; j++) m.pkb_status[j] = want_pkb_status(m, j);
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
  for (size_t j = 0; j < c.nk; j++)
    CHECK(c.pst[j] == (c.local && c.with_pst ? want_pkb_status(r, j) : -1), "a caller's slice of the table's statuses");
  CHECK(c.pst[c.nk] == -1, "a write past a caller's pkb_status");
}

static void test_kinds() {
  Caller a = make_caller(1, "SLP", 3, {0, 1, 3}, false);
  Caller b = make_caller(2, "SS", 0, {0, 2}, false);             // no table, no ranges: still a local request
  Caller s = make_caller(3, "SL", 2, {}, true);
  Caller p = make_caller(4, "SP", 0, {0, 2}, false, 0, false);   // a span request
  Req ra = a.req(), rb = b.req(), rs = s.req(), rp = p.req();
  CHECK(ra.spans() && rb.spans() && rs.spans() && rp.spans(), "spans()");
  CHECK(ra.src.local && rb.src.local && !rp.src.local && !rb.src.off && !rb.src.pkb, "the sources");
  CHECK(ra.kind() == rb.kind(), "local batches with and without a table are one kind");
  CHECK(ra.kind() != rs.kind(), "single checks are a kind of their own");
  CHECK(ra.kind() != rp.kind() && rs.kind() != rp.kind(), "a span source is another kind");
  Req sp = rp;
  sp.rands = nullptr;
  CHECK(sp.kind() != rs.kind() && sp.kind() != ra.kind(), "span single checks are another kind");
  CHECK(ra.kind() >= 48 && rs.kind() >= 48 && rp.kind() >= 16 && rp.kind() < 32, "the span and local bits");
  CHECK(rb.nkeys() == 0 && ra.nkeys() == a.off[a.n], "nkeys");
}

static void test_merge(bool single, bool fail) {
  std::vector<Caller> cs;
  cs.push_back(make_caller(1, "L", 3, {0, 1}, single));
  cs.push_back(make_caller(2, "SSSS", 0, {0, 3, 4}, single));            // npkb == 0 among others, no ranges
  cs.push_back(make_caller(3, "LPLLP", 5, {0, 2, 2, 5}, single, 0, true, 2));  // set 2 names a position past its table
  cs.push_back(make_caller(4, "PL", 1, {0, 1, 2}, single));
  cs.push_back(make_caller(5, "SLP", 2, {0, 3}, single));
  cs[3].with_pst = false;  // pkb_status is optional
  std::vector<Req> reqs;
  for (Caller &c : cs) reqs.push_back(c.req());
  std::vector<Req *> batch;
  for (Req &r : reqs) batch.push_back(&r);
  // the concatenation, computed here
  std::vector<uint8_t> w_msgs, w_sigc, w_cbits, w_bits, w_pkb;
  std::vector<uint32_t> w_com, w_boff{0}, w_idx, w_off{0}, w_seg{0};
  std::vector<uint64_t> w_rands;
  size_t w_n = 0, total = 0;
  for (Caller &c : cs) total += c.nk;
  CHECK(total == 11, "the shape");
  size_t before = 0;
  for (Caller &c : cs) {
    const size_t nb = c.boff[c.n];
    for (size_t s = 1; s < c.seg.size(); s++) w_seg.push_back((uint32_t)(w_n + c.seg[s]));
    for (size_t i = 0; i < c.n; i++) {
      if (c.with_off)
        for (uint32_t k = c.off[i]; k < c.off[i + 1]; k++) {
          uint32_t v = c.idx[k];
          if (c.com[i] == kLocal) v = v < c.nk ? v + (uint32_t)before : (uint32_t)total;
          w_idx.push_back(v);
        }
      w_off.push_back((uint32_t)w_idx.size());
      w_boff.push_back((uint32_t)(w_bits.size() + c.boff[i + 1]));
    }
    w_msgs.insert(w_msgs.end(), c.msgs.begin(), c.msgs.end());
    w_sigc.insert(w_sigc.end(), c.sigc.begin(), c.sigc.end());
    w_com.insert(w_com.end(), c.com.begin(), c.com.end());
    w_cbits.insert(w_cbits.end(), c.cbits.begin(), c.cbits.end());
    w_bits.insert(w_bits.end(), c.bits.begin(), c.bits.begin() + (std::ptrdiff_t)nb);
    w_pkb.insert(w_pkb.end(), c.pkb.begin(), c.pkb.begin() + (std::ptrdiff_t)(48 * c.nk));
    w_rands.insert(w_rands.end(), c.rands.begin(), c.rands.end());
    w_n += c.n;
    before += c.nk;
  }
  // the rebase moved something, left the plain sets alone, and sent the stray position past the end
  CHECK(w_n == 15 && w_idx != [&] { std::vector<uint32_t> v; for (Caller &c : cs) if (c.with_off) v.insert(v.end(), c.idx.begin(), c.idx.begin() + c.off[c.n]); return v; }(), "the shape");
  CHECK(std::count(w_idx.begin(), w_idx.end(), (uint32_t)total) == 1, "one stray position");
  int calls = 0;
  sched::run_merged(batch, [&](Req &m) {
    calls++;
    CHECK(m.spans() && m.src.local && m.src.off && m.sigs_c && m.sig_status && m.key_status && m.pkb_status && !m.sigs &&
              !m.src.pts, "the merged form");
    CHECK(m.n == w_n && m.nseg == w_seg.size() - 1 && (m.rands == nullptr) == single && m.src.npkb == total, "n, nseg, class, npkb");
    CHECK(std::vector<uint8_t>(m.msgs, m.msgs + 32 * m.n) == w_msgs, "msgs");
    CHECK(std::vector<uint8_t>(m.sigs_c, m.sigs_c + 96 * m.n) == w_sigc, "sigs");
    CHECK(std::vector<uint32_t>(m.src.com, m.src.com + m.n) == w_com, "com");
    CHECK(std::vector<uint8_t>(&m.src.cbits[0][0], &m.src.cbits[0][0] + 8 * m.n) == w_cbits, "cbits");
    CHECK(std::vector<uint32_t>(m.src.bits_off, m.src.bits_off + m.n + 1) == w_boff, "bits_off");
    CHECK(std::vector<uint32_t>(m.src.off, m.src.off + m.n + 1) == w_off, "off");
    CHECK(std::vector<uint8_t>(m.src.bits, m.src.bits + w_boff[m.n]) == w_bits, "bits");
    CHECK(std::vector<uint32_t>(m.src.idx, m.src.idx + w_off[m.n]) == w_idx, "idx: positions rebased in local sets only");
    CHECK(std::vector<uint8_t>(&m.src.pkb[0][0], &m.src.pkb[0][0] + 48 * total) == w_pkb, "the concatenated tables");
    CHECK(std::vector<uint32_t>(m.seg_off, m.seg_off + m.nseg + 1) == w_seg, "seg_off");
    if (m.rands) CHECK(std::vector<uint64_t>(m.rands, m.rands + m.n) == w_rands, "rands");
    for (size_t i = 0; i < m.n; i++) CHECK(m.sig_status[i] == 1 && m.key_status[i] == 1, "pre-fill");
    for (size_t j = 0; j < total; j++) CHECK(m.pkb_status[j] == 1, "pre-fill of the table's statuses");
    for (size_t s = 0; s < m.nseg; s++) CHECK(m.verdicts[s] == 5, "pre-fill");
    answer(m, !fail, fail ? 101 : 0);
  });
  CHECK(calls == 1, "one submission");
  // every caller's outputs are what the verifier would have answered to its OWN request
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
  auto verify = [&](Req &m) {
    std::set<int> ids;
    for (size_t i = 0; i < m.n; i++) ids.insert(m.msgs[32 * i]);
    {
      std::lock_guard<std::mutex> lk(mu);
      // ids 1..5: normal local batches; 6: local single checks; 7: the block-class local batch; 8: a span batch
      for (int id : ids) {
        const int cls = id <= 5 ? 0 : id;
        for (int other : ids) CHECK((other <= 5 ? 0 : other) == cls, "a submission mixed kinds or classes");
      }
      CHECK(m.prio == (ids.count(7) ? 1 : 0), "the class of a submission");
      CHECK((m.rands == nullptr) == (ids.count(6) != 0), "single checks in a batch submission");
      CHECK(m.src.local == (ids.count(8) == 0) && (m.pkb_status != nullptr) == m.src.local, "a span request among local ones");
    }
    if (ids.size() > 1) merged++;
    answer(m, true, 0);
  };
  std::vector<std::thread> threads;
  for (int id = 1; id <= 8; id++)
    threads.emplace_back([&, id] {
      for (int round = 0; round < 40; round++) {
        const size_t n = 1 + (size_t)((id + round) % 6), nk = id == 2 || id == 8 ? 0 : 1 + (size_t)((id + round) % 4);
        std::string kinds(n, 'S');
        for (size_t i = 0; i < n; i++) kinds[i] = "SLP"[nk ? (i + (size_t)round) % 3 : 0];
        std::vector<uint32_t> seg{0, (uint32_t)(n / 2), (uint32_t)n};
        Caller c = make_caller(id, kinds.c_str(), nk, seg, id == 6, id == 7 ? 1 : 0, id != 8, round % 5 == 0 && nk ? (int)(round % n) : -1);
        Req r = c.req();
        CHECK(co.submit(r, cfg, verify) && r.done, "submit");
        check_outputs(c, r, true, 0);
      }
    });
  for (auto &t : threads) t.join();
  std::printf("sched_local: merged submissions %d\n", merged.load());
}

int main() {
  test_kinds();
  for (int single = 0; single < 2; single++)
    for (int fail = 0; fail < 2; fail++) test_merge(single != 0, fail != 0);
  test_threads();
  std::printf("sched_local: OK\n");
  return 0;
}
