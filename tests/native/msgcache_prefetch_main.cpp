// Stand-alone driver of the host side of prefetch and of the per-check plan
// (grandine_amd/csrc/gbls_msgcache_checks.h) over two engines' indices, built by
// tests/test_msgcache_prefetch_index.py plain and with AddressSanitizer and UBSan and run as a
// program: msgcache_prefetch_main SCRIPT runs the operations of SCRIPT, one output line each.
// SCRIPT lines (message ids are small integers, expanded to 32 bytes by msg_of):
//   cfg SLOTS SPARE                       both engines
//   prefetch LIMIT ENGINES DONE id ..     one call over engines [0, ENGINES): lookups, then every
//                                         engine's finish (DONE 0: the device work failed), merged
//   checks E T id_0 .. id_{n-1}           call T plans n checks on engine E (its hits are pinned)
//   fin E T ok_0 .. ok_{n-1}              call T ends: per check, whether it passed
//   clear E
// Every operation runs on two sides, one with the process key (getrandom) and one with a fixed
// key: the output must not depend on the key, and the program fails if the two differ.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <map>
#include <sstream>
#include <string>
#include <vector>

#include "../../grandine_amd/csrc/gbls_msgcache_checks.h"

using namespace gbls::msgcache;

static void msg_of(uint32_t id, uint8_t *out) {
  uint32_t w[8];
  for (int i = 0; i < 8; i++) w[i] = (id + 1) * 0x9e3779b1u + (uint32_t)i * 0x85ebca6bu * id;
  std::memcpy(out, w, 32);
}
static uint32_t id_of(const uint8_t *m, uint32_t max_id) {
  uint8_t t[32];
  for (uint32_t id = 0; id <= max_id; id++) {
    msg_of(id, t);
    if (!std::memcmp(t, m, 32)) return id;
  }
  return kNone;
}

struct Engine {
  Index ix;
  uint64_t st[kStats] = {0};
  std::map<int, ShardPlan> calls;
};
struct Side {
  Engine e[2];
};

static void list(std::ostringstream &o, const char *name, const std::vector<uint32_t> &v) {
  o << " " << name;
  for (uint32_t x : v) o << " " << (x == kNone ? -1 : (long)x);
  o << " ;";
}

// entries, the counters, the entries' messages from the most recently used, slots not free
static std::string state(const Engine &e, uint32_t max_id) {
  std::ostringstream o;
  o << "entries " << e.ix.entries << " stats";
  for (int i = 0; i < kStats; i++) o << " " << e.st[i];
  o << " lru";
  for (uint32_t k = e.ix.head; k != kNone; k = e.ix.next[k]) o << " " << id_of(&e.ix.key[(size_t)k * 32], max_id);
  uint32_t busy = 0, pins = 0;
  for (uint32_t k = 0; k < e.ix.total; k++) {
    busy += e.ix.state[k] != FREE;
    pins += e.ix.pins[k];
  }
  o << " busy " << busy << " pins " << pins;
  return o.str();
}

static std::vector<uint8_t> read_msgs(std::istringstream &in, uint32_t &max_id, uint32_t *n_out) {
  std::vector<uint8_t> msgs(1);
  uint32_t id, n = 0;
  while (in >> id) {
    if (id > max_id) max_id = id;
    msgs.resize((size_t)32 * (n + 1) + 1);
    msg_of(id, &msgs[(size_t)32 * n++]);
  }
  *n_out = n;
  return msgs;
}

static std::string run(Side &s, const std::string &line, const gbls::dedup::HashKey &key, uint32_t &max_id) {
  std::istringstream in(line);
  std::string op;
  in >> op;
  std::ostringstream o;
  o << op;
  if (op == "cfg") {
    uint32_t slots, spare;
    in >> slots >> spare;
    for (Engine &e : s.e) {
      e.ix.reset(slots, spare, e.st, key);
      e.calls.clear();
    }
  } else if (op == "clear") {
    int e;
    in >> e;
    s.e[e].ix.clear();
  } else if (op == "prefetch") {
    uint32_t limit, engines, done, n;
    in >> limit >> engines >> done;
    const std::vector<uint8_t> msgs = read_msgs(in, max_id, &n);
    Prefetch pf;
    prefetch_groups(pf, msgs.data(), n, key);
    std::vector<DevicePrefetch> dp(engines);
    for (uint32_t k = 0; k < engines; k++) prefetch_lookup(dp[k], s.e[k].ix, pf, limit);
    std::vector<int32_t> ust(pf.D, PF_SKIPPED), dev(pf.D), status(n, -1);
    std::vector<uint32_t> fills;
    for (uint32_t k = 0; k < engines; k++) {
      fills.push_back((uint32_t)dp[k].fill.size());
      for (size_t j = 0; j < dp[k].fill.size(); j++)  // the messages to compute are the taken ones, in order
        if (std::memcmp(&dp[k].fill_msgs[32 * j], &pf.umsgs[32 * (size_t)dp[k].fill[j]], 32) ||
            dp[k].fill_slot[j] != dp[k].slot[dp[k].fill[j]] || s.e[k].ix.state[dp[k].fill_slot[j]] != TAKEN)
          return "bad fill";
      prefetch_finish(dp[k], s.e[k].ix, pf, done != 0, dev.data());
      merge_status(ust.data(), dev.data(), pf.D, k == 0);
    }
    if (!done) ust.assign(pf.D, PF_SKIPPED);
    prefetch_scatter(pf, ust.data(), status.data());
    o << " D " << pf.D;
    list(o, "status", std::vector<uint32_t>(status.begin(), status.end()));
    list(o, "fills", fills);
  } else if (op == "checks") {
    int e, t;
    uint32_t n;
    in >> e >> t;
    const std::vector<uint8_t> msgs = read_msgs(in, max_id, &n);
    ShardPlan &p = s.e[e].calls[t];
    std::vector<uint32_t> ident;
    plan_check_groups(p, msgs.data(), n, ident, key);
    plan_checks(p, &s.e[e].ix);
    o << " " << e << " " << t << " U " << p.U << " M " << p.M << " C " << p.ncopy << " D " << p.D;
    std::vector<uint32_t> ids, hit;
    for (uint32_t u = 0; u < p.D; u++) {
      ids.push_back(id_of(&p.umsgs[(size_t)32 * u], max_id));
      hit.push_back(p.uhit[u]);
    }
    list(o, "ids", ids);
    list(o, "hit", hit);
    list(o, "slot", p.uslot);
    list(o, "pair_of", p.pair_of);
    list(o, "hit_slot", p.hit_slot);
    list(o, "store_pair", p.store_pair);
    list(o, "store_slot", p.store_slot);
    list(o, "csr", p.csr);
    ids.clear();
    for (uint32_t k = 0; k < p.M; k++) ids.push_back(id_of(&p.miss_msgs[(size_t)32 * k], max_id));
    list(o, "miss_ids", ids);
  } else if (op == "fin") {
    int e, t;
    in >> e >> t;
    ShardPlan &p = s.e[e].calls.at(t);
    std::vector<uint8_t> ok(p.groups.nseg + 1);
    for (uint32_t k = 0; k < p.groups.nseg; k++) {
      int v;
      in >> v;
      ok[k] = (uint8_t)v;
    }
    plan_verdicts(p, ok.data(), false);
    s.e[e].ix.finish(p.txn, p.ok.data());
    s.e[e].calls.erase(t);
    o << " " << e << " " << t;
  } else {
    return "?";
  }
  o << " | " << state(s.e[0], max_id) << " | " << state(s.e[1], max_id);
  return o.str();
}

int main(int argc, char **argv) {
  if (argc < 2) return 2;
  std::ifstream f(argv[1]);
  if (!f) return 2;
  gbls::dedup::HashKey fixed;
  for (int i = 0; i < 10; i++) fixed.k[i] = 0x0123456789abcdefull * (uint64_t)(i + 3) | 1;
  Side a, b;
  uint32_t max_a = 0, max_b = 0;
  std::string line;
  while (std::getline(f, line)) {
    if (line.empty()) continue;
    const std::string ra = run(a, line, gbls::dedup::process_key(), max_a), rb = run(b, line, fixed, max_b);
    if (ra != rb) {
      std::fprintf(stderr, "the plan depends on the hash key:\n%s\n%s\n", ra.c_str(), rb.c_str());
      return 1;
    }
    std::printf("%s\n", ra.c_str());
  }
  return 0;
}
