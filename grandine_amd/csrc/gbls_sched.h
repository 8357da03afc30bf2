// Host-side scheduling of the engine: the per-device context pool and the cross-caller
// coalescer (f3).  Host-only C++ (no HIP): gbls_capi.hip instantiates it with its HIP
// contexts and its verification pipeline; tests/native/sched_tsan.cpp instantiates it with
// stub contexts and a stub verifier and runs it under ThreadSanitizer with 32 threads.
//
// Callers arrive concurrently from rayon workers, the de-low executor, the block
// verification pool and fork-choice workers (reference p2p/src/attestation_verifier.rs:68,
// 142-163; p2p/src/block_verification_pool.rs:39-49,103-128).
#pragma once

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <memory>
#include <mutex>
#include <vector>

namespace gbls {
namespace sched {

// ---------------------------------------------------------------- context pool
// Two classes of contexts: 0 = normal, 1 = block import (every stream at the highest
// priority).  Each class has its own cap, so a burst of normal calls (e.g. signature
// decompressions from every rayon worker) can never use up the slots block import needs, and
// the reverse.
constexpr int kClasses = 2;
constexpr int kMaxCtx[kClasses] = {64, 16};

// Ctx needs: int cls; bool used; <stream> last_stream; bool idle_on_gpu() (called under the
// pool mutex).
template <class Ctx>
struct CtxPool {
  std::mutex mu;
  std::condition_variable cv;
  std::vector<Ctx *> idle;
  std::vector<std::unique_ptr<Ctx>> all;
  int count[kClasses] = {0, 0};

  // A context of class `cls`: the idle one last used on `stream` (affine: stream order makes
  // its reuse free), else an idle one whose previous call has finished on the GPU, else a new
  // one (up to the class cap; *fresh = true, the caller initialises it), else the least
  // recently released idle one of the class (its reuse is ordered behind its previous call on
  // the GPU), else wait until one of the class comes back.
  template <class Stream>
  Ctx *acquire(bool affine, Stream stream, int cls, bool *fresh) {
    cls = cls ? 1 : 0;
    *fresh = false;
    std::unique_lock<std::mutex> lk(mu);
    for (;;) {
      Ctx *c = nullptr;
      for (size_t i = 0; affine && !c && i < idle.size(); i++)
        if (idle[i]->cls == cls && idle[i]->used && idle[i]->last_stream == stream) c = take(i);
      for (size_t i = 0; !c && i < idle.size(); i++)
        if (idle[i]->cls == cls && idle[i]->idle_on_gpu()) c = take(i);
      if (!c && count[cls] < kMaxCtx[cls]) {
        all.emplace_back(new Ctx());
        c = all.back().get();
        c->cls = cls;
        count[cls]++;
        *fresh = true;
      }
      for (size_t i = 0; !c && i < idle.size(); i++)
        if (idle[i]->cls == cls) c = take(i);
      if (c) return c;
      cv.wait(lk);  // every context of this class is leased: wait for one to come back
    }
  }
  // a new idle context of class cls, initialised by init(ctx) before any caller can lease it
  // (engine start: the first concurrent calls then find contexts instead of creating them)
  template <class Init>
  bool prewarm(int cls, Init &&init) {
    cls = cls ? 1 : 0;
    std::unique_ptr<Ctx> c(new Ctx());
    c->cls = cls;
    if (!init(*c)) return false;
    std::lock_guard<std::mutex> lk(mu);
    if (count[cls] >= kMaxCtx[cls]) return false;
    count[cls]++;
    idle.push_back(c.get());
    all.push_back(std::move(c));
    return true;
  }
  void release(Ctx *c) {
    {
      std::lock_guard<std::mutex> lk(mu);
      idle.push_back(c);
    }
    cv.notify_all();  // waiters of either class
  }
  size_t size() {
    std::lock_guard<std::mutex> lk(mu);
    return all.size();
  }
  // f(ctx) for every context, leased or idle (under the pool mutex: f must not block)
  template <class F>
  void for_each(F &&f) {
    std::lock_guard<std::mutex> lk(mu);
    for (auto &c : all) f(*c);
  }

 private:
  Ctx *take(size_t i) {
    Ctx *c = idle[i];
    idle.erase(idle.begin() + (std::ptrdiff_t)i);
    return c;
  }
};

// ---------------------------------------------------------------- coalescer
template <class G1>
struct KeySource {
  const G1 *pts = nullptr;        // points: one per set (off == nullptr) or summed per set
  const uint32_t *idx = nullptr;  // registry indices: one per set (off == nullptr) or summed
  const uint32_t *off = nullptr;  // per-set ranges [off[i], off[i+1]) of pts / idx
  // cached committee sums (with idx and off): set i's key is committee slot com[i] MINUS its
  // summed range, or the range's sum when com[i] names no committee.  Never merged by the
  // coalescer (Request::kind does not know it): such a call is its own submission.
  const uint32_t *com = nullptr;
  uint32_t max_len = 0;           // ... and the longest range (a device source: the launch form)
  // aggregation-bit sets (with com; gbls_bits.h): a committee set's key is the sum of the slot's
  // resident members whose bit is set, the other sets sum their idx range (off may be nullptr
  // when there is none).  Host source: the bit strings and their byte offsets.  Device source:
  // the BitSet descriptors and the repacked bit rows; max_len is then the longest set's work.
  const uint8_t *bits = nullptr;
  const uint32_t *bits_off = nullptr;
  const void *bit_sets = nullptr;
  const uint32_t *bit_rows = nullptr;
  // span sets (with com, bits and bits_off; gbls_spans.h): com[i] is a base slot and cbits[i] the 8
  // bytes of committee_bits, one bit string over the named committees.  Device source: the
  // SpanPiece and SpanSet descriptors (rows in bit_rows), their count and the most pieces of a set.
  const uint8_t (*cbits)[8] = nullptr;
  const void *span_pieces = nullptr;
  const void *span_sets = nullptr;
  uint32_t span_np = 0, span_max_pieces = 0;
  // local key sets (with the span fields; gbls_local.h): `local` marks a source of the local calls,
  // pkb[npkb] its call-local table of compressed keys; a set with com[i] == kLocalKeys sums the
  // table positions of its off range.  Device source: the compressed bytes (loc_in), the decoded
  // table loc[npkb] with its statuses (loc_st), and the local sets' pieces, the tail
  // [span_np - loc_np, span_np) of the piece array, with their longest list.
  bool local = false;
  const uint8_t (*pkb)[48] = nullptr;
  size_t npkb = 0;
  const uint8_t *loc_in = nullptr;
  const G1 *loc = nullptr;
  int32_t *loc_st = nullptr;
  uint32_t loc_np = 0, loc_max_len = 0;
  // verified folds (with the span fields, single checks only; gbls_fold.h): `fold` marks a source
  // of the fold call, whether or not it names a group.  Group g sums the signatures of the sets
  // fold_set[fold_off[g] .. fold_off[g+1]) that verified into fold_out[g] (an affine G2 point),
  // fold_count[g] and, when asked, fold_bytes[g].  A host source only: the submission that carries
  // groups runs on one engine.
  bool fold = false;
  const uint32_t *fold_set = nullptr;
  const uint32_t *fold_off = nullptr;
  size_t nfold = 0;
  void *fold_out = nullptr;
  uint8_t (*fold_bytes)[96] = nullptr;
  uint32_t *fold_count = nullptr;
};

// Merging callers of the fold call: caller c's groups follow the groups of the callers before it,
// and its fold_set entries move up by its first set in the merged call.  set/off: the merged CSR
// (off[0] == 0 written by the caller of this function), gat/eat: the groups and entries merged so
// far, at: the caller's first set.
inline void fold_concat(uint32_t *set, uint32_t *off, size_t gat, size_t eat, size_t at, const uint32_t *fold_set,
                        const uint32_t *fold_off, size_t nfold) {
  for (size_t g = 1; g <= nfold; g++) off[gat + g] = (uint32_t)(eat + fold_off[g]);
  const uint32_t cnt = nfold ? fold_off[nfold] : 0;
  for (uint32_t i = 0; i < cnt; i++) set[eat + i] = (uint32_t)(at + fold_set[i]);
}

// Merging callers of the local calls: the positions of a caller's LOCAL sets (com[i] ==
// kLocalSet, gbls_local.h kLocalKeys) move up by the number of local keys of the callers before
// it; registry indices stay as they are.  idx: the merged index array, off/com: the merged
// offsets and slots, [at, at + n) this caller's sets.  A position past the caller's OWN table
// must stay rejected after the move, so it is sent to the merged table's end (total), never
// into a later caller's keys.
constexpr uint32_t kLocalSet = 0xfffffffeu;
inline void local_rebase(uint32_t *idx, const uint32_t *off, const uint32_t *com, size_t at, size_t n, uint32_t before,
                         uint32_t own, uint32_t total) {
  for (size_t i = at; i < at + n; i++) {
    if (com[i] != kLocalSet) continue;
    for (uint32_t k = off[i]; k < off[i + 1]; k++) idx[k] = idx[k] < own ? idx[k] + before : total;
  }
}

// Telemetry (gbls_telemetry.h), written only for a request that carries `ph` under a Config that
// carries `clock`: when the caller entered submit, how long it was held and how long it sat in a
// collection window, when its submission started (the same for every member of a batch) and how
// long that ran.  What is left of lead_ns - submit_ns after hold and window is the time queued.
struct CallPhases {
  uint64_t submit_ns = 0, hold_ns = 0, window_ns = 0, lead_ns = 0, run_ns = 0;
};
// ... and what the verifier may read about the batch it is handed (Request::bi of the merged request)
struct BatchInfo {
  uint64_t first_arrival_ns = 0, lead_ns = 0;  // earliest submit_ns of the members; start of the submission
  uint32_t callers = 0;
  uint64_t sets = 0;
};

// One caller's batch (host pointers, borrowed for the call).  rands == nullptr: independent
// single checks (Signature::verify / fast_aggregate_verify semantics: r_i = 1, the
// signature's subgroup check, one segment per set), merged only with other single checks.
template <class G1, class G2>
struct Request {
  using g1_type = G1;
  using g2_type = G2;
  const uint8_t *msgs;
  const G2 *sigs;
  KeySource<G1> src;
  const uint64_t *rands;
  size_t n;
  const uint32_t *seg_off;
  size_t nseg;
  int32_t *verdicts;
  const uint8_t *sigs_c = nullptr;  // compressed signatures instead of sigs (96 B each)
  int32_t *sig_status = nullptr;    // their decompression statuses (with sigs_c)
  int32_t *key_status = nullptr;    // the sets' key statuses (a span source only)
  int32_t *pkb_status = nullptr;    // the local keys' statuses (a local source only, optional)
  int prio = 0;                     // 1: block import
  bool done = false, ok = false;
  int err = 0;                      // the verifier's side-channel error code
  CallPhases *ph = nullptr;         // telemetry: this caller's phases (null: none recorded)
  const BatchInfo *bi = nullptr;    // telemetry: the batch this request runs in (set by submit)
  bool spans() const { return src.cbits != nullptr; }
  // A span source (com, cbits, bits, bits_off; idx and off for its plain sets, off == nullptr
  // when it has none) is a kind of its own whether or not it carries index ranges; a local
  // source (span | local: a span source with a key table, empty or not) another, and a fold
  // source (span | fold: the fold call's requests, with or without groups) one more.
  int kind() const {
    const int sig = (sigs_c ? 4 : 0) | (rands ? 0 : 8);
    return spans() ? 16 | (src.local ? 32 : 0) | (src.fold ? 64 : 0) | sig
                   : (src.pts ? 1 : 0) | (src.off ? 2 : 0) | sig;
  }
  size_t nkeys() const { return src.off ? src.off[n] : spans() ? 0 : n; }
};

struct Config {
  bool coalesce = true;
  int devices = 1;
  int leaders = 2;                  // normal leaders per device (block import: 1 per device)
  size_t max_merged = 1 << 16;      // merged normal submissions stay below one C2 step
  size_t max_merged_block = 8192;   // block import: the latency cap
  size_t merge_target = 768;        // a new leader's collection window ends at this many sets
  int merge_window_us = 300;        // ... or after this long (only while another is in flight)
  // while *hold > 0 (a block import in progress), a normal request does not start a new
  // submission for up to hold_max_us: the block shares the GPU only with the normal
  // submissions already running (null: never hold)
  const std::atomic<int> *hold = nullptr;
  int hold_max_us = 4000;
  // telemetry: the clock (ns) that stamps the requests carrying Request::ph; null (the default)
  // or a request without ph: nothing is stamped and no clock is read
  uint64_t (*clock)() = nullptr;
};

// Runs the requests of `batch` (all of one kind) as ONE segmented verification: the merged
// request is handed to verify(Req &) (which sets ok and err), then every caller's verdicts and
// signature statuses (and, for span sources, key statuses) are copied back from its own range.
// Span sources: com and cbits are concatenated, the bit strings too with bits_off rebased, the
// plain sets' indices with off rebased (a request without off contributes empty ranges).
// Local sources: the key tables are concatenated too, the positions of each caller's LOCAL sets
// move up by the local keys before that caller (registry indices stay; gbls_local.h
// local_rebase), and every caller gets its own slice of the keys' statuses.  Tables that
// together do not fit 32 bits are not merged: each request then runs on its own.
// Fold sources: the groups' CSRs are concatenated (fold_concat: each caller's entries move up by
// its first set, its groups follow the earlier callers'), and every caller gets its own slices of
// the points, counts and bytes -- only when the merged verification succeeded, so that a failure
// leaves every caller's fold outputs as its pre-fill wrote them.  Groups or entries that together
// do not fit 32 bits are not merged either.
template <class Req, class Verify>
void run_merged(std::vector<Req *> &batch, Verify &&verify) {
  if (batch.size() == 1) {
    verify(*batch[0]);
    return;
  }
  const bool local = batch[0]->src.local;
  uint64_t nloc = 0;
  for (Req *r : batch) nloc += local ? r->src.npkb : 0;
  const bool fold = batch[0]->src.fold;
  uint64_t ngrp = 0, nent = 0;
  for (Req *r : batch) {
    ngrp += fold ? r->src.nfold : 0;
    nent += fold && r->src.nfold ? r->src.fold_off[r->src.nfold] : 0;
  }
  if (nloc > 0xffffffffull || ngrp >= 0xffffffffull || nent > 0xffffffffull) {
    for (Req *r : batch) {
      BatchInfo one;  // each request is then a submission of its own
      if (r->bi) {
        one = *r->bi;
        one.callers = 1;
        one.sets = r->n;
        r->bi = &one;
      }
      verify(*r);
      r->bi = nullptr;
    }
    return;
  }
  using G1 = typename Req::g1_type;
  using G2 = typename Req::g2_type;
  size_t n = 0, nseg = 0, nk = 0;
  for (Req *r : batch) {
    n += r->n;
    nseg += r->nseg;
    nk += r->nkeys();
  }
  const Req &r0 = *batch[0];
  const bool comp = r0.sigs_c != nullptr, single = r0.rands == nullptr, spans = r0.spans();
  std::vector<uint8_t> msgs(32 * n), sigc(comp ? 96 * n : 0);
  std::vector<G2> sigs(comp ? 0 : n);
  std::vector<int32_t> sst(comp ? n : 0, 1 /* BAD_ENCODING until decoded */);
  std::vector<uint64_t> rands(single ? 0 : n);
  std::vector<G1> pts;
  std::vector<uint32_t> idx, off, seg(nseg + 1);
  if (r0.src.pts)
    pts.resize(nk);
  else
    idx.resize(nk);
  if (r0.src.off || spans) off.resize(n + 1);
  std::vector<uint32_t> com, boff;
  std::vector<uint8_t> cbits, bits;
  std::vector<int32_t> kst(spans ? n : 0, 1 /* BAD_ENCODING until resolved */);
  if (spans) {
    size_t nb = 0;
    for (Req *r : batch) nb += r->src.bits_off[r->n];
    com.resize(n);
    cbits.resize(8 * n);
    bits.resize(nb);
    boff.resize(n + 1);
  }
  std::vector<uint8_t> pkb(local ? 48 * (size_t)nloc : 0);
  std::vector<int32_t> pst(local ? (size_t)nloc : 0, 1 /* BAD_ENCODING until decoded */);
  std::vector<int32_t> v(nseg, 5 /* VERIFY_FAIL */);
  std::vector<uint32_t> fset((size_t)nent), foff(ngrp ? (size_t)ngrp + 1 : 0, 0), fcnt((size_t)ngrp, 0);
  std::vector<G2> fpts((size_t)ngrp);
  std::vector<uint8_t> fbytes(96 * (size_t)ngrp);
  size_t at = 0, sat = 0, kat = 0, bat = 0, lat = 0, gat = 0, eat = 0;
  seg[0] = 0;
  for (Req *r : batch) {
    std::memcpy(&msgs[32 * at], r->msgs, 32 * r->n);
    if (comp)
      std::memcpy(&sigc[96 * at], r->sigs_c, 96 * r->n);
    else
      std::memcpy(&sigs[at], r->sigs, r->n * sizeof(G2));
    if (!single) std::memcpy(&rands[at], r->rands, r->n * 8);
    const size_t k = r->nkeys();
    if (r0.src.pts)
      std::memcpy(&pts[kat], r->src.pts, k * sizeof(G1));
    else if (k)
      std::memcpy(&idx[kat], r->src.idx, k * 4);
    if (r0.src.off || spans)
      for (size_t i = 0; i <= r->n; i++) off[at + i] = (uint32_t)(kat + (r->src.off ? r->src.off[i] : 0));
    if (spans) {
      const size_t nb = r->src.bits_off[r->n];
      if (r->n) {
        std::memcpy(&com[at], r->src.com, r->n * 4);
        std::memcpy(&cbits[8 * at], r->src.cbits, 8 * r->n);
      }
      if (nb) std::memcpy(&bits[bat], r->src.bits, nb);
      for (size_t i = 0; i <= r->n; i++) boff[at + i] = (uint32_t)(bat + r->src.bits_off[i]);
      bat += nb;
    }
    if (local) {
      if (r->src.npkb) std::memcpy(&pkb[48 * lat], r->src.pkb, 48 * r->src.npkb);
      if (r->src.off)
        local_rebase(idx.data(), off.data(), com.data(), at, r->n, (uint32_t)lat, (uint32_t)r->src.npkb, (uint32_t)nloc);
      lat += r->src.npkb;
    }
    if (fold && r->src.nfold) {
      fold_concat(fset.data(), foff.data(), gat, eat, at, r->src.fold_set, r->src.fold_off, r->src.nfold);
      gat += r->src.nfold;
      eat += r->src.fold_off[r->src.nfold];
    }
    for (size_t s = 1; s <= r->nseg; s++) seg[sat + s] = (uint32_t)(at + r->seg_off[s]);
    at += r->n;
    sat += r->nseg;
    kat += k;
  }
  Req m{msgs.data(), comp ? nullptr : sigs.data(), KeySource<G1>(), single ? nullptr : rands.data(),
        n, seg.data(), nseg, v.data()};
  if (r0.src.pts)
    m.src.pts = pts.data();
  else
    m.src.idx = idx.data();
  if (r0.src.off || spans) m.src.off = off.data();
  if (spans) {
    m.src.com = com.data();
    m.src.cbits = reinterpret_cast<const uint8_t(*)[8]>(cbits.data());
    m.src.bits = bits.data();
    m.src.bits_off = boff.data();
    m.key_status = kst.data();
  }
  if (local) {
    m.src.local = true;
    m.src.pkb = reinterpret_cast<const uint8_t(*)[48]>(pkb.data());
    m.src.npkb = (size_t)nloc;
    m.pkb_status = pst.data();
  }
  if (comp) {
    m.sigs_c = sigc.data();
    m.sig_status = sst.data();
  }
  m.src.fold = fold;
  if (ngrp) {
    m.src.fold_set = fset.data();
    m.src.fold_off = foff.data();
    m.src.nfold = (size_t)ngrp;
    m.src.fold_out = fpts.data();
    m.src.fold_bytes = reinterpret_cast<uint8_t(*)[96]>(fbytes.data());
    m.src.fold_count = fcnt.data();
  }
  m.prio = r0.prio;
  m.bi = r0.bi;
  verify(m);
  sat = 0;
  at = 0;
  lat = 0;
  gat = 0;
  for (Req *r : batch) {
    if (fold && r->src.nfold) {
      if (m.ok) {
        std::memcpy(r->src.fold_out, &fpts[gat], r->src.nfold * sizeof(G2));
        std::memcpy(r->src.fold_count, &fcnt[gat], r->src.nfold * 4);
        if (r->src.fold_bytes) std::memcpy(r->src.fold_bytes, &fbytes[96 * gat], 96 * r->src.nfold);
      }
      gat += r->src.nfold;
    }
    if (local && r->pkb_status && r->src.npkb) std::memcpy(r->pkb_status, &pst[lat], r->src.npkb * 4);
    if (local) lat += r->src.npkb;
    std::memcpy(r->verdicts, &v[sat], r->nseg * 4);
    if (comp) std::memcpy(r->sig_status, &sst[at], r->n * 4);
    if (spans && r->key_status) std::memcpy(r->key_status, &kst[at], r->n * 4);
    sat += r->nseg;
    at += r->n;
    r->ok = m.ok;
    r->err = m.err;
  }
}

// Concurrent batch verifications queue here; a caller that finds fewer than
// leaders x devices submissions in flight becomes a leader and verifies every queued request
// with the same key-source kind as ONE segmented submission (each keeping its own segments
// and verdicts), up to max_merged sets.  Block import (prio) has its own queue and leader
// slot per device, is merged only with other block requests (up to max_merged_block sets) and
// never waits in a collection window.
template <class Req>
class Coalescer {
 public:
  template <class Verify>
  bool submit(Req &r, const Config &cfg, Verify &&verify) {
    const bool tel = cfg.clock && r.ph;
    if (tel) r.ph->submit_ns = cfg.clock();
    if (!cfg.coalesce) {
      BatchInfo bi;
      if (tel) {
        bi.first_arrival_ns = bi.lead_ns = r.ph->lead_ns = r.ph->submit_ns;
        bi.callers = 1;
        bi.sets = r.n;
        r.bi = &bi;
      }
      verify(r);
      r.bi = nullptr;
      if (tel) r.ph->run_ns = cfg.clock() - r.ph->lead_ns;
      return r.ok;
    }
    const int max_leaders = (r.prio ? 1 : cfg.leaders) * std::max(1, cfg.devices);
    const size_t cap = r.prio ? cfg.max_merged_block : cfg.max_merged;
    std::vector<Req *> &q = r.prio ? pq_ : q_;
    int &leaders = r.prio ? pleaders_ : leaders_;
    std::unique_lock<std::mutex> lk(mu_);
    q.push_back(&r);
    cv_.notify_all();  // a leader collecting a batch (below) sees the new request at once
    bool waited = false, held = false;
    while (!r.done) {
      if (!r.prio && !held && cfg.hold && cfg.hold->load() > 0) {
        held = true;  // a block import is being verified: leave it the GPU for a while
        const uint64_t t0 = tel ? cfg.clock() : 0;
        const auto deadline =
            std::chrono::steady_clock::now() + std::chrono::microseconds(cfg.hold_max_us);
        cv_.wait_until(lk, deadline, [&] { return r.done || cfg.hold->load() == 0; });
        if (tel) {  // (done: it ended with the submission's start -- if that leader stamped it)
          const uint64_t t1 = r.done ? r.ph->lead_ns : cfg.clock();
          if (t1 >= t0) r.ph->hold_ns += t1 - t0;
        }
        continue;
      }
      if (leaders < max_leaders && !q.empty()) {
        // Another submission is already in flight: the GPU is busy, so a short collection
        // window costs little latency and lets the callers that return from that submission
        // join this one (without it the first of them leads a batch of one).  Never for block
        // import, never on an idle engine.
        auto queued = [&q]() {
          size_t t = 0;
          for (const Req *x : q) t += x->n;
          return t;
        };
        if (!r.prio && leaders > 0 && !waited && queued() < cfg.merge_target) {
          waited = true;
          const uint64_t t0 = tel ? cfg.clock() : 0;
          const auto deadline =
              std::chrono::steady_clock::now() + std::chrono::microseconds(cfg.merge_window_us);
          cv_.wait_until(lk, deadline, [&] { return r.done || queued() >= cfg.merge_target; });
          if (tel) {
            const uint64_t t1 = r.done ? r.ph->lead_ns : cfg.clock();
            if (t1 >= t0) r.ph->window_ns += t1 - t0;
          }
          continue;
        }
        leaders++;
        std::vector<Req *> batch;
        auto mine = std::find(q.begin(), q.end(), &r);
        const int kind = mine != q.end() ? r.kind() : q.front()->kind();
        size_t sets = 0;
        if (mine != q.end()) {
          batch.push_back(&r);
          sets = r.n;
          q.erase(mine);
        }
        for (auto it = q.begin(); it != q.end();) {
          if ((*it)->kind() == kind && (batch.empty() || sets + (*it)->n <= cap)) {
            sets += (*it)->n;
            batch.push_back(*it);
            it = q.erase(it);
          } else {
            ++it;
          }
        }
        // telemetry: the members that carry phases share the submission's start and duration
        BatchInfo bi;
        bool stamped = false;
        for (Req *b : batch) stamped = stamped || b->ph;
        stamped = stamped && cfg.clock;
        if (stamped) {
          bi.lead_ns = cfg.clock();
          bi.first_arrival_ns = bi.lead_ns;
          bi.callers = (uint32_t)batch.size();
          bi.sets = sets;
          for (Req *b : batch) {
            if (b->ph) {
              b->ph->lead_ns = bi.lead_ns;
              bi.first_arrival_ns = std::min(bi.first_arrival_ns, b->ph->submit_ns);
            }
            b->bi = &bi;
          }
        }
        lk.unlock();
        run_merged(batch, verify);  // writes verdicts, ok, err; `done` is published under mu_
        if (stamped) {
          const uint64_t ran = cfg.clock() - bi.lead_ns;
          for (Req *b : batch) {
            if (b->ph) b->ph->run_ns = ran;
            b->bi = nullptr;
          }
        }
        lk.lock();
        for (Req *b : batch) b->done = true;
        leaders--;
        cv_.notify_all();
      } else {
        cv_.wait(lk);
      }
    }
    return r.ok;
  }
  // wake waiting callers (e.g. when the hold of Config::hold is released)
  void wake() {
    std::lock_guard<std::mutex> lk(mu_);
    cv_.notify_all();
  }

 private:
  std::mutex mu_;
  std::condition_variable cv_;
  std::vector<Req *> q_, pq_;  // normal and block-import queues
  int leaders_ = 0, pleaders_ = 0;
};

}  // namespace sched
}  // namespace gbls
