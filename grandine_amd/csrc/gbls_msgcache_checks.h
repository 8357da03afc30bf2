// Host side of include/grandine_bls_gpu_msgcache_checks.h, above the index of gbls_msgcache.h.
// Host-only C++ (no HIP): gbls_capi.hip drives it; tests/native/msgcache_prefetch_main.cpp runs it
// plain and under AddressSanitizer and UBSan against a model.
//
//   prefetch    the call's distinct messages (Prefetch), each engine device's lookups and takes
//               (DevicePrefetch: prefetch_lookup before the device work, prefetch_finish after its
//               synchronisation) and the merge of the devices' statuses (merge_status)
//   per check   the plan of a submission of independent checks (plan_checks): one segment and one
//               pair per check, a missed message hashed once however many checks carry it
#pragma once

#include "gbls_msgcache.h"

namespace gbls {
namespace msgcache {

// gbls_msgcache_prefetch's statuses (GBLS_PREFETCH_*)
enum PrefetchStatus : int32_t { PF_ENTERED = 0, PF_PRESENT = 1, PF_SKIPPED = 2 };

// ---- the call: n messages, D distinct ones in order of first occurrence
struct Prefetch {
  dedup::Plan uniq;
  uint32_t D = 0;
  std::vector<uint8_t> umsgs;  // D x 32
};
inline void prefetch_groups(Prefetch &p, const uint8_t *msgs, size_t n, const dedup::HashKey &key = dedup::process_key()) {
  const uint32_t one[2] = {0, (uint32_t)n};
  dedup::build(p.uniq, msgs, n, one, 1, key);
  p.D = p.uniq.ngroups;
  p.umsgs.resize((size_t)32 * p.D);
  for (uint32_t u = 0; u < p.D; u++) std::memcpy(&p.umsgs[32 * (size_t)u], msgs + 32 * (size_t)p.uniq.first[u], 32);
}
// status (n, the caller's) from the distinct messages' statuses: every occurrence reports the same
inline void prefetch_scatter(const Prefetch &p, const int32_t *ustatus, int32_t *status) {
  for (uint32_t i = 0; i < p.uniq.n; i++) status[i] = ustatus[p.uniq.of[i]];
}

// ---- one engine device's part of the call
struct DevicePrefetch {
  Txn txn;
  std::vector<uint8_t> hit;         // D
  std::vector<uint32_t> slot;       // D: the entry, the taken slot, or kNone (skipped)
  std::vector<uint32_t> fill;       // the distinct messages this device computes, in order
  std::vector<uint8_t> fill_msgs;   // fill.size() x 32
  std::vector<uint32_t> fill_slot;  // ... and where their lines go
  std::vector<uint8_t> ok, entered; // per txn.take entry (finish)
};
// Under the index's lock.  Present messages are hits (pinned, their recency refreshed); at most
// `limit` missing ones take a spare slot, in order; the others are counted as a served shard
// counts a miss without a spare slot (a miss that is bypassed) and stay out.
inline void prefetch_lookup(DevicePrefetch &dp, Index &ix, const Prefetch &p, size_t limit) {
  dp.hit.assign(p.D, 0);
  dp.slot.assign(p.D, kNone);
  ix.plan(dp.txn, p.umsgs.data(), p.D, dp.hit.data(), dp.slot.data(), limit);
  dp.fill.clear();
  dp.fill_slot.clear();
  for (uint32_t u = 0; u < p.D; u++)
    if (!dp.hit[u] && dp.slot[u] != kNone) {
      dp.fill.push_back(u);
      dp.fill_slot.push_back(dp.slot[u]);
    }
  dp.fill_msgs.resize((size_t)32 * dp.fill.size());
  for (size_t j = 0; j < dp.fill.size(); j++)
    std::memcpy(&dp.fill_msgs[32 * j], &p.umsgs[32 * (size_t)dp.fill[j]], 32);
}
// Under the index's lock, after the device's synchronisation.  done: the lines are in the taken
// slots (every message ok); otherwise the slots are returned and nothing is published.
// ustatus (D): this device's statuses -- a taken message is ENTERED only if it
// became an entry at its turn (a clear() meanwhile, or a table whose entries are all pinned, leaves
// it out); a later message of the same call may evict it again (a call larger than the capacity).
inline void prefetch_finish(DevicePrefetch &dp, Index &ix, const Prefetch &p, bool done, int32_t *ustatus) {
  dp.ok.assign(dp.txn.take.size(), done ? 1 : 0);
  dp.entered.assign(dp.txn.take.size(), 0);
  ix.finish(dp.txn, dp.ok.data(), dp.entered.data());  // (resets the transaction, not our vectors)
  size_t j = 0;  // the misses, in plan order
  for (uint32_t u = 0; u < p.D; u++) {
    if (dp.hit[u])
      ustatus[u] = PF_PRESENT;
    else
      ustatus[u] = dp.entered[j++] ? PF_ENTERED : PF_SKIPPED;
  }
}
// several engines: PRESENT only if present on every engine, ENTERED if missing on at least one and
// an entry on every engine now, SKIPPED otherwise.  acc: the merge so far (first: none yet)
inline void merge_status(int32_t *acc, const int32_t *dev, size_t D, bool first) {
  for (size_t u = 0; u < D; u++) {
    if (first)
      acc[u] = dev[u];
    else if (acc[u] == PF_SKIPPED || dev[u] == PF_SKIPPED)
      acc[u] = PF_SKIPPED;
    else if (acc[u] == PF_ENTERED || dev[u] == PF_ENTERED)
      acc[u] = PF_ENTERED;
  }
}

// ---- a submission of n independent checks (one segment per check, r_i = 1)
inline void plan_check_groups(ShardPlan &p, const uint8_t *msgs, size_t n, std::vector<uint32_t> &ident,
                              const dedup::HashKey &key = dedup::process_key()) {
  ident.resize(n + 1);
  for (size_t i = 0; i <= n; i++) ident[i] = (uint32_t)i;
  plan_groups(p, msgs, n, ident.data(), n, key);  // U == n: group q is check q
}
// After plan_check_groups: the lookups and the pair numbering of the checks.
//   [0, M)              the pairs whose lines are generated: the first check of every missed
//                       message, and every check of a missed message that got no slot
//   [M, U - ncopy)      the checks whose message hit: lines from the entry
//   [U - ncopy, U)      the other checks of a missed message that has a slot: lines from that slot,
//                       once its first pair's lines are stored there
// ix == nullptr plans without a cache (every check generates, nothing to store): the tests' form
inline void plan_checks(ShardPlan &p, Index *ix) {
  const dedup::Plan &g = p.groups;
  const uint32_t U = p.U;
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
  // the first group of distinct message u (U == 1: plan_groups leaves uniq alone)
  auto first_of = [&](uint32_t u) { return g.nseg > 1 ? p.uniq.first[u] : u; };
  auto cls = [&](uint32_t q) {  // 0 generates, 1 hit, 2 copy
    const uint32_t u = p.uof[q];
    if (p.uhit[u]) return 1;
    return p.uslot[u] != kNone && first_of(u) != q ? 2 : 0;
  };
  p.pair_of.resize(U);
  uint32_t cnt[3] = {0, 0, 0};
  for (uint32_t q = 0; q < U; q++) cnt[cls(q)]++;
  const uint32_t M = cnt[0];
  p.M = M;
  p.ncopy = cnt[2];
  p.miss_msgs.resize((size_t)32 * M);
  p.hit_slot.resize(U - M);
  p.store_pair.clear();
  p.store_slot.clear();
  uint32_t at[3] = {0, M, M + cnt[1]};
  for (uint32_t q = 0; q < U; q++) {
    const uint32_t u = p.uof[q], k = (uint32_t)cls(q), pr = at[k]++;
    p.pair_of[q] = pr;
    if (k) {
      p.hit_slot[pr - M] = p.uslot[u];
    } else {
      std::memcpy(&p.miss_msgs[32 * (size_t)pr], &p.gmsgs[32 * (size_t)q], 32);
      if (p.uslot[u] != kNone) {
        p.store_pair.push_back(pr);
        p.store_slot.push_back(p.uslot[u]);
      }
    }
  }
  // one set per group: the CSR in pair order is the inverse of pair_of
  p.csr.resize((size_t)2 * U + 1);
  p.inv.resize(U);
  for (uint32_t q = 0; q < U; q++) p.inv[p.pair_of[q]] = q;
  for (uint32_t pr = 0; pr < U; pr++) {
    p.csr[pr] = pr;
    p.csr[(size_t)U + 1 + pr] = g.grp_set[g.grp_off[p.inv[pr]]];
  }
  p.csr[U] = U;
}

}  // namespace msgcache
}  // namespace gbls
