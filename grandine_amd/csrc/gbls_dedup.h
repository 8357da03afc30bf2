// Host-side grouping of a batch's sets by message (GBLS_INIT_DEDUP).  Host-only C++ (no HIP):
// gbls_capi.hip builds a plan per device shard of a host-pointer batch;
// tests/native/dedup_plan_main.cpp runs it under AddressSanitizer and UBSan.
//
// Sets of ONE segment that carry the same 32-byte message form a group: the group needs one
// hash_to_G2, one set of Miller lines and one Miller pair, e(sum_i r_i pk_i, H(m)).  Segments are
// independent batches with independent verdicts, so a message that occurs in two segments makes
// two groups.  Equality is the full 32 bytes; the hash only picks the table slot.
//
// Messages (signing roots) are chosen by peers, so the table's hash is keyed per process from
// getrandom: the multilinear family h = k_0 + sum k_i w_i mod 2^64 over the message's eight
// 32-bit words and the segment, of which the upper half is strongly universal -- two different
// (segment, message) pairs collide in a slot with probability 2^-32 scaled by the table size,
// whatever the sender picks without the key.  Expected O(n); the table has >= 2 n slots.
#pragma once

#include <cerrno>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#include <sys/random.h>

namespace gbls {
namespace dedup {

constexpr uint32_t kNone = 0xffffffffu;

struct Plan {
  uint32_t n = 0, nseg = 0;
  uint32_t ngroups = 0;               // U; U == n: no duplicates, the caller takes the plain path
  uint32_t max_group = 0;             // the largest group's size
  std::vector<uint8_t> msgs;          // the U unique messages, 32 bytes each, in group order
  std::vector<uint32_t> grp_off;      // U + 1: group g's members are grp_set[grp_off[g] .. grp_off[g + 1])
  std::vector<uint32_t> grp_set;      // n set indices, ascending within a group
  std::vector<uint32_t> grp_seg_off;  // nseg + 1: segment s's groups are [grp_seg_off[s], grp_seg_off[s + 1])
  bool has_duplicates() const { return ngroups < n; }
  // build's working memory, kept so that a plan object reused across calls allocates nothing
  std::vector<uint32_t> table, first, count, of;  // slot -> group; group -> first member, size; set -> group
};

struct HashKey {
  uint64_t k[10];
};
// the process's key (first use; getrandom never fails for 80 bytes once the pool is up, and a
// failure only leaves a fixed key: grouping stays correct, only its worst case is no longer
// out of a sender's reach)
inline const HashKey &process_key() {
  static const HashKey key = [] {
    HashKey h;
    for (int i = 0; i < 10; i++) h.k[i] = 0x9e3779b97f4a7c15ull * (uint64_t)(2 * i + 1);
    uint8_t *p = reinterpret_cast<uint8_t *>(h.k);
    size_t got = 0;
    while (got < sizeof(h.k)) {
      ssize_t r = getrandom(p + got, sizeof(h.k) - got, 0);
      if (r < 0) {
        if (errno == EINTR) continue;
        break;
      }
      got += (size_t)r;
    }
    return h;
  }();
  return key;
}

inline uint32_t hash(const HashKey &key, uint32_t seg, const uint8_t *m) {
  uint32_t w[8];
  std::memcpy(w, m, 32);
  uint64_t h = key.k[0] + key.k[1] * seg;
  for (int i = 0; i < 8; i++) h += key.k[2 + i] * w[i];
  return (uint32_t)(h >> 32);
}

// Groups ordered by segment, then by first member: the sets are walked in order (segments are
// ranges of sets), and a group is created when its first member is met.  Deterministic for a
// given input (the key only moves table slots).  seg_off: nseg + 1 nondecreasing offsets,
// seg_off[0] = 0, seg_off[nseg] = n.
inline void build(Plan &p, const uint8_t *msgs, size_t n, const uint32_t *seg_off, size_t nseg,
                  const HashKey &key = process_key()) {
  p.n = (uint32_t)n;
  p.nseg = (uint32_t)nseg;
  p.ngroups = 0;
  p.max_group = 0;
  p.msgs.clear();
  p.grp_off.clear();
  p.grp_set.assign(n, 0);
  p.grp_seg_off.assign(nseg + 1, 0);
  size_t slots = 16;
  while (slots < 2 * n) slots <<= 1;
  int shift = 32;
  for (size_t s = slots; s > 1; s >>= 1) shift--;
  std::vector<uint32_t> &table = p.table, &first = p.first, &count = p.count, &of = p.of;
  table.assign(slots, kNone);
  first.clear();
  count.clear();
  first.reserve(n);
  count.reserve(n);
  of.resize(n);
  for (size_t s = 0; s < nseg; s++) {
    p.grp_seg_off[s] = (uint32_t)first.size();
    for (uint32_t i = seg_off[s]; i < seg_off[s + 1]; i++) {
      const uint8_t *m = msgs + 32 * (size_t)i;
      size_t at = hash(key, (uint32_t)s, m) >> shift;
      uint32_t g;
      // groups of earlier segments stay in the table; their first members lie below seg_off[s]
      while ((g = table[at]) != kNone &&
             (first[g] < seg_off[s] || std::memcmp(msgs + 32 * (size_t)first[g], m, 32) != 0))
        at = (at + 1) & (slots - 1);
      if (g == kNone) {
        g = (uint32_t)first.size();
        table[at] = g;
        first.push_back(i);
        count.push_back(0);
      }
      of[i] = g;
      count[g]++;
    }
  }
  const size_t U = first.size();
  p.grp_seg_off[nseg] = (uint32_t)U;
  p.ngroups = (uint32_t)U;
  p.grp_off.assign(U + 1, 0);
  for (size_t g = 0; g < U; g++) {
    p.grp_off[g + 1] = p.grp_off[g] + count[g];
    if (count[g] > p.max_group) p.max_group = count[g];
  }
  for (size_t g = 0; g < U; g++) count[g] = p.grp_off[g];  // now each group's fill position
  for (uint32_t i = 0; i < n; i++) p.grp_set[count[of[i]]++] = i;
  if (U == n) return;  // no duplicates: the caller uploads nothing of this plan
  p.msgs.resize(32 * U);
  for (size_t g = 0; g < U; g++) std::memcpy(&p.msgs[32 * g], msgs + 32 * (size_t)first[g], 32);
}

}  // namespace dedup
}  // namespace gbls
