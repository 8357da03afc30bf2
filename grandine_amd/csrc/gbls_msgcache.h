// Host index of the message line cache (include/grandine_bls_gpu_msgcache.h).  Host-only C++ (no
// HIP): gbls_capi.hip keeps one Index per engine device, all behind one mutex;
// tests/native/msgcache_index_main.cpp runs it under AddressSanitizer and UBSan against a model.
//
// The cache maps a 32-byte message to a SLOT of a device table that holds the message's 68 Miller
// line events (kSlotWords words).  The index owns `slots` entry slots plus a pool of spare slots:
//
//   FREE    on the free stack
//   TAKEN   handed to one call for a message it missed; no other call can see it.  After the
//           call's host synchronisation it is published (becomes an ENTRY) or returned
//   ENTRY   found by lookups; pinned by every call that hit it, from planning until after that
//           call's synchronisation.  Only unpinned entries are eviction victims (exact LRU)
//   ZOMBIE  an entry dropped by clear() while pinned: free once its last reader unpins
//
// A miss is published only when the caller says its verdict was GBLS_SUCCESS.  Lines are a function
// of the message alone, so an entry is right whoever sent it; the rule keeps a peer's junk
// messages, which cannot pass verification, from displacing entries.  A message that another call
// is filling is a plain miss (nobody waits); publishing a message that is present meanwhile is a
// no-op that returns the slot.
//
// Lookup: open addressing (linear probing, backward-shift deletion) keyed by all 32 bytes, with
// the process-keyed multilinear hash of gbls_dedup.h.  The key only moves table positions: slots
// come from a stack and victims from the LRU list, so a plan does not depend on the key.
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#include "gbls_dedup.h"

namespace gbls {
namespace msgcache {

constexpr uint32_t kNone = dedup::kNone;
constexpr size_t kSlotWords = 68 * 72;             // ML_EVENTS x 72 words: 19 584 bytes
constexpr size_t kMaxSlots = (size_t)1 << 20;      // gbls_msgcache_configure's bound
// spare slots beside `slots` entries: a quarter, at least 64 (a gossip batch of distinct
// messages), at most 4096
inline uint32_t spare_for(size_t slots) {
  const size_t q = slots / 4;
  return (uint32_t)(q < 64 ? 64 : q > 4096 ? 4096 : q);
}

enum Stat { LOOKUPS, HITS, MISSES, PUBLISHED, EVICTIONS, BYPASSED, kStats };
enum State : uint8_t { FREE, TAKEN, ENTRY, ZOMBIE };

// what one call holds between plan() and finish()
struct Txn {
  bool active = false;
  uint64_t epoch = 0;
  std::vector<uint32_t> hit;   // the slots it pinned
  std::vector<uint32_t> take;  // per miss, in plan order: its slot, or kNone (computed, not cached)
  void reset() {
    active = false;
    hit.clear();
    take.clear();
  }
};

struct Index {
  uint32_t slots = 0, total = 0, entries = 0;
  uint64_t epoch = 0;         // clear() starts a new one: takes of an older epoch are not published
  uint64_t *st = nullptr;     // kStats counters (the owner's, shared by every device's index)
  std::vector<uint8_t> key;   // total x 32
  std::vector<uint8_t> state;
  std::vector<uint32_t> pins, prev, next, free_;
  uint32_t head = kNone, tail = kNone;  // LRU list of the entries: head = most recently used
  std::vector<uint32_t> table;          // position -> slot (ENTRY slots only)
  uint32_t mask = 0;
  int shift = 32;
  dedup::HashKey hk;

  void reset(uint32_t nslots, uint32_t nspare, uint64_t *stats, const dedup::HashKey &k = dedup::process_key()) {
    slots = nslots;
    total = nslots + nspare;
    st = stats;
    hk = k;
    key.assign((size_t)total * 32, 0);
    pins.assign(total, 0);
    prev.assign(total, kNone);
    next.assign(total, kNone);
    size_t tsz = 16;
    while (tsz < 2 * (size_t)total) tsz <<= 1;
    mask = (uint32_t)(tsz - 1);
    shift = 32;
    for (size_t s = tsz; s > 1; s >>= 1) shift--;
    state.assign(total, FREE);
    drop_all();
  }
  // every entry dropped; slots that calls in flight still read or write stay theirs
  void clear() {
    epoch++;
    drop_all();
  }
  uint32_t find(const uint8_t *m) const {
    uint32_t at = pos(m), s;
    while ((s = table[at]) != kNone) {
      if (std::memcmp(&key[(size_t)s * 32], m, 32) == 0) return s;
      at = (at + 1) & mask;
    }
    return kNone;
  }
  // D DISTINCT messages: hit[i] = 1 and slot[i] = the pinned entry, or hit[i] = 0 and slot[i] = the
  // taken slot the call writes the lines to (kNone: none to spare, or max_take slots taken already)
  void plan(Txn &t, const uint8_t *msgs, size_t D, uint8_t *hit, uint32_t *slot, size_t max_take = SIZE_MAX) {
    t.reset();
    t.active = true;
    t.epoch = epoch;
    st[LOOKUPS] += D;
    for (size_t i = 0; i < D; i++) {
      const uint8_t *m = msgs + 32 * i;
      uint32_t s = find(m);
      if (s != kNone) {
        st[HITS]++;
        pins[s]++;
        touch(s);
        t.hit.push_back(s);
        hit[i] = 1;
      } else {
        st[MISSES]++;
        hit[i] = 0;
        if (!free_.empty() && max_take) {
          max_take--;
          s = free_.back();
          free_.pop_back();
          state[s] = TAKEN;
          std::memcpy(&key[(size_t)s * 32], m, 32);
        } else {
          st[BYPASSED]++;
        }
        t.take.push_back(s);
      }
      slot[i] = s;
    }
  }
  // after the call's host synchronisation.  ok (nullable: none): per miss of t.take, whether its
  // verdict was GBLS_SUCCESS.  entered (nullable, per miss of t.take): whether the message was an
  // entry right after its turn (published, or present meanwhile), whatever a later one evicts
  void finish(Txn &t, const uint8_t *ok, uint8_t *entered = nullptr) {
    if (!t.active) return;
    for (uint32_t s : t.hit) unpin(s);
    for (size_t j = 0; j < t.take.size(); j++) {
      const uint32_t s = t.take[j];
      if (entered) entered[j] = 0;
      if (s == kNone) continue;
      if (ok && ok[j] && t.epoch == epoch) {
        publish(s);
        if (entered) entered[j] = find(&key[(size_t)s * 32]) != kNone;  // (a returned slot keeps its key)
      } else {
        release(s);
      }
    }
    t.reset();
  }

 private:
  uint32_t pos(const uint8_t *m) const { return shift >= 32 ? 0 : dedup::hash(hk, 0, m) >> shift; }
  void release(uint32_t s) {
    state[s] = FREE;
    free_.push_back(s);
  }
  void unpin(uint32_t s) {
    if (--pins[s] == 0 && state[s] == ZOMBIE) release(s);
  }
  void drop_all() {
    table.assign((size_t)mask + 1, kNone);
    head = tail = kNone;
    entries = 0;
    free_.clear();
    for (uint32_t s = total; s-- > 0;) {  // the stack hands out slot 0 first
      if (state[s] == ENTRY || state[s] == ZOMBIE) state[s] = pins[s] ? ZOMBIE : FREE;
      if (state[s] == FREE) free_.push_back(s);
      prev[s] = next[s] = kNone;
    }
  }
  void unlink(uint32_t s) {
    (prev[s] != kNone ? next[prev[s]] : head) = next[s];
    (next[s] != kNone ? prev[next[s]] : tail) = prev[s];
    prev[s] = next[s] = kNone;
  }
  void push_front(uint32_t s) {
    prev[s] = kNone;
    next[s] = head;
    if (head != kNone) prev[head] = s;
    head = s;
    if (tail == kNone) tail = s;
  }
  void touch(uint32_t s) {
    if (head == s) return;
    unlink(s);
    push_front(s);
  }
  void table_insert(uint32_t s) {
    uint32_t at = pos(&key[(size_t)s * 32]);
    while (table[at] != kNone) at = (at + 1) & mask;
    table[at] = s;
  }
  void table_erase(uint32_t s) {
    uint32_t at = pos(&key[(size_t)s * 32]);
    while (table[at] != s) at = (at + 1) & mask;
    // backward shift: close the gap with every later member of the run that may move up
    uint32_t hole = at;
    for (uint32_t j = (at + 1) & mask; table[j] != kNone; j = (j + 1) & mask) {
      const uint32_t home = pos(&key[(size_t)table[j] * 32]);
      // table[j] may move to `hole` unless its home lies cyclically in (hole, j]
      const bool stays = hole <= j ? (home > hole && home <= j) : (home > hole || home <= j);
      if (!stays) {
        table[hole] = table[j];
        hole = j;
      }
    }
    table[hole] = kNone;
  }
  void publish(uint32_t s) {
    if (slots == 0 || find(&key[(size_t)s * 32]) != kNone) return release(s);  // present meanwhile
    if (entries == slots) {  // the least recently used unpinned entry makes room
      uint32_t v = tail;
      while (v != kNone && pins[v]) v = prev[v];
      if (v == kNone) {
        st[BYPASSED]++;
        return release(s);
      }
      table_erase(v);
      unlink(v);
      release(v);
      entries--;
      st[EVICTIONS]++;
    }
    state[s] = ENTRY;
    table_insert(s);
    push_front(s);
    entries++;
    st[PUBLISHED]++;
  }
};

// ---- a shard's plan: its message groups (gbls_dedup.h), which of them hit and at which slot, and
// the pair numbering the pipeline runs on: the M groups that missed are pairs [0, M) -- hashing
// and line generation run unchanged on that prefix, over the M messages of miss_msgs -- and the
// groups that hit are pairs [M, U).  Kept in the context, so a steady caller allocates nothing.
struct ShardPlan {
  dedup::Plan groups;              // the shard's sets by (segment, message): U groups
  dedup::Plan uniq;                // the U group messages as ONE segment: D distinct messages
  uint32_t U = 0, M = 0, D = 0;
  std::vector<uint8_t> gmsgs;      // U x 32: the groups' messages (uniq's input)
  std::vector<uint8_t> umsgs;      // D x 32: the distinct messages, the index's input
  std::vector<uint32_t> uof;       // group -> distinct message
  std::vector<uint8_t> uhit;       // D
  std::vector<uint32_t> uslot;     // D
  std::vector<uint32_t> umiss;     // distinct message -> its position in txn.take (misses)
  std::vector<uint32_t> pair_of;   // group -> pair
  std::vector<uint32_t> inv;       // pair -> group
  std::vector<uint8_t> miss_msgs;  // M x 32, in pair order
  std::vector<uint32_t> csr;       // [off (U + 1)][sets (n)] of the groups in PAIR order (k_g1s_msgsum)
  std::vector<uint32_t> hit_slot;  // U - M: the slot of pair M + k
  // per-check plans (gbls_msgcache_checks.h): the last ncopy of those pairs carry a message that
  // missed; they load from the slot its first pair fills, after that store.  0 in a shard plan
  uint32_t ncopy = 0;
  std::vector<uint32_t> store_pair, store_slot;  // the miss pairs that have a slot to fill
  std::vector<uint8_t> seg_ok;     // per segment: its verdict was GBLS_SUCCESS (the caller's, for plan_verdicts)
  std::vector<uint8_t> ok;         // per txn.take entry (finish)
  Txn txn;
};

// the shard's groups and distinct messages (no index involved: the caller may still decide that the
// submission bypasses the cache)
inline void plan_groups(ShardPlan &p, const uint8_t *msgs, size_t n, const uint32_t *seg_off, size_t nseg,
                        const dedup::HashKey &key = dedup::process_key()) {
  dedup::build(p.groups, msgs, n, seg_off, nseg, key);
  const dedup::Plan &g = p.groups;
  const uint32_t U = g.ngroups;
  p.U = U;
  p.gmsgs.resize((size_t)32 * U);
  for (uint32_t q = 0; q < U; q++) std::memcpy(&p.gmsgs[32 * (size_t)q], msgs + 32 * (size_t)g.first[q], 32);
  p.uof.resize(U);
  if (nseg > 1) {  // a message of two segments is two groups and one cache entry
    const uint32_t one[2] = {0, U};
    dedup::build(p.uniq, p.gmsgs.data(), U, one, 1, key);
    p.D = p.uniq.ngroups;
    for (uint32_t q = 0; q < U; q++) p.uof[q] = p.uniq.of[q];
    p.umsgs.resize((size_t)32 * p.D);
    for (uint32_t u = 0; u < p.D; u++)
      std::memcpy(&p.umsgs[32 * (size_t)u], &p.gmsgs[32 * (size_t)p.uniq.first[u]], 32);
  } else {
    p.D = U;
    for (uint32_t q = 0; q < U; q++) p.uof[q] = q;
    p.umsgs = p.gmsgs;
  }
}

// after plan_groups: the lookups and the pair numbering.  ix == nullptr plans without a cache
// (every group misses, nothing to store): the tests' form
inline void plan_cache(ShardPlan &p, Index *ix) {
  const dedup::Plan &g = p.groups;
  const uint32_t U = p.U;
  const size_t n = g.n, nseg = g.nseg;
  p.ncopy = 0;
  p.uhit.assign(p.D, 0);
  p.uslot.assign(p.D, kNone);
  if (ix)
    ix->plan(p.txn, p.umsgs.data(), p.D, p.uhit.data(), p.uslot.data());
  else
    p.txn.reset();
  p.umiss.assign(p.D, kNone);
  uint32_t nm = 0;
  for (uint32_t u = 0; u < p.D; u++)
    if (!p.uhit[u]) p.umiss[u] = nm++;
  // pairs: misses first, each class in group order
  p.pair_of.resize(U);
  uint32_t M = 0;
  for (uint32_t q = 0; q < U; q++)
    if (!p.uhit[p.uof[q]]) p.pair_of[q] = M++;
  p.M = M;
  p.miss_msgs.resize((size_t)32 * M);
  p.hit_slot.resize(U - M);
  p.store_pair.clear();
  p.store_slot.clear();
  uint32_t h = M;
  for (uint32_t q = 0; q < U; q++) {
    const uint32_t u = p.uof[q];
    if (p.uhit[u]) {
      p.hit_slot[h - M] = p.uslot[u];
      p.pair_of[q] = h++;
    } else {
      std::memcpy(&p.miss_msgs[32 * (size_t)p.pair_of[q]], &p.gmsgs[32 * (size_t)q], 32);
      // the first group of a distinct message fills its slot
      if (p.uslot[u] != kNone && (nseg == 1 || p.uniq.first[u] == q)) {
        p.store_pair.push_back(p.pair_of[q]);
        p.store_slot.push_back(p.uslot[u]);
      }
    }
  }
  p.csr.resize((size_t)U + 1 + n);
  std::vector<uint32_t> &inv = p.inv;
  inv.resize(U);
  for (uint32_t q = 0; q < U; q++) inv[p.pair_of[q]] = q;
  uint32_t at = 0;
  for (uint32_t pr = 0; pr < U; pr++) {
    const uint32_t q = inv[pr];
    p.csr[pr] = at;
    for (uint32_t j = g.grp_off[q]; j < g.grp_off[q + 1]; j++) p.csr[(size_t)U + 1 + at++] = g.grp_set[j];
  }
  p.csr[U] = at;
}
inline void plan_shard(ShardPlan &p, Index *ix, const uint8_t *msgs, size_t n, const uint32_t *seg_off,
                       size_t nseg, const dedup::HashKey &key = dedup::process_key()) {
  plan_groups(p, msgs, n, seg_off, nseg, key);
  plan_cache(p, ix);
}

// which misses to publish: a distinct message is published when a segment that carries it passed
// (seg_ok[s] != 0), or, with seg_ok == nullptr, when all_ok
inline void plan_verdicts(ShardPlan &p, const uint8_t *seg_ok, bool all_ok) {
  p.ok.assign(p.txn.take.size(), 0);
  const dedup::Plan &g = p.groups;
  for (uint32_t s = 0; s < g.nseg; s++) {
    if (!(seg_ok ? seg_ok[s] != 0 : all_ok)) continue;
    for (uint32_t q = g.grp_seg_off[s]; q < g.grp_seg_off[s + 1]; q++) {
      const uint32_t j = p.umiss[p.uof[q]];
      if (j != kNone && j < p.ok.size()) p.ok[j] = 1;
    }
  }
}

}  // namespace msgcache
}  // namespace gbls
