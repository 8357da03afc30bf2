// Stand-alone driver of the message line cache's host index and shard plan
// (grandine_amd/csrc/gbls_msgcache.h), built by tests/test_msgcache_index.py with AddressSanitizer
// and UBSan and run as a program.
//   msgcache_index_main SCRIPT            runs the operations of SCRIPT, one output line each
//   msgcache_index_main --time N D REPS   host cost of planning N sets on D distinct messages
//                                         against a warm index (best of REPS), in microseconds
// SCRIPT lines (message ids are small integers, expanded to 32 bytes by msg_of):
//   cfg SLOTS SPARE
//   plan T NSEG off_0 .. off_NSEG id_0 .. id_{n-1}    call T plans (its hits are pinned)
//   fin T ok_0 .. ok_{NSEG-1}                         call T ends: per segment, whether it passed
//   clear
// Every operation runs on two indices, one with the process key (getrandom) and one with a fixed
// key: the output must not depend on the key, and the program fails if the two differ.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <map>
#include <sstream>
#include <string>
#include <vector>

#include "../../grandine_amd/csrc/gbls_msgcache.h"

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

struct Side {
  Index ix;
  uint64_t st[kStats] = {0};
  std::map<int, ShardPlan> calls;
};

static void list(std::ostringstream &o, const char *name, const std::vector<uint32_t> &v) {
  o << " " << name;
  for (uint32_t x : v) o << " " << (x == kNone ? -1 : (long)x);
  o << " ;";
}

static std::string state(const Side &s, uint32_t max_id) {
  std::ostringstream o;
  o << "entries " << s.ix.entries << " stats";
  for (int i = 0; i < kStats; i++) o << " " << s.st[i];
  o << " slots";
  for (uint32_t k = 0; k < s.ix.total; k++) {
    const uint8_t *m = &s.ix.key[(size_t)k * 32];
    o << " " << (int)s.ix.state[k] << ":" << s.ix.pins[k] << ":";
    if (s.ix.state[k] == FREE) o << "-";
    else o << id_of(m, max_id);
  }
  o << " lru";
  for (uint32_t k = s.ix.head; k != kNone; k = s.ix.next[k]) o << " " << k;
  return o.str();
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
    s.ix.reset(slots, spare, s.st, key);
    s.calls.clear();
  } else if (op == "clear") {
    s.ix.clear();
  } else if (op == "plan") {
    int t;
    uint32_t nseg;
    in >> t >> nseg;
    std::vector<uint32_t> off(nseg + 1);
    for (uint32_t &x : off) in >> x;
    const uint32_t n = off[nseg];
    std::vector<uint8_t> msgs((size_t)32 * n + 1);
    for (uint32_t i = 0; i < n; i++) {
      uint32_t id;
      in >> id;
      if (id > max_id) max_id = id;
      msg_of(id, &msgs[(size_t)32 * i]);
    }
    ShardPlan &p = s.calls[t];
    plan_shard(p, &s.ix, msgs.data(), n, off.data(), nseg, key);
    o << " " << t << " U " << p.U << " M " << p.M << " D " << p.D;
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
    int t;
    in >> t;
    ShardPlan &p = s.calls.at(t);
    std::vector<uint8_t> ok(p.groups.nseg + 1);
    for (uint32_t k = 0; k < p.groups.nseg; k++) {
      int v;
      in >> v;
      ok[k] = (uint8_t)v;
    }
    plan_verdicts(p, ok.data(), false);
    s.ix.finish(p.txn, p.ok.data());
    s.calls.erase(t);
    o << " " << t;
  } else {
    return "?";
  }
  o << " | " << state(s, max_id);
  return o.str();
}

static int time_plan(uint32_t n, uint32_t distinct, int reps) {
  Side s;
  s.ix.reset(distinct < 16 ? 16 : distinct, spare_for(distinct), s.st);
  std::vector<uint8_t> msgs((size_t)32 * n);
  for (uint32_t i = 0; i < n; i++) msg_of((i * 2654435761u) % distinct, &msgs[(size_t)32 * i]);
  const uint32_t off[2] = {0, n};
  ShardPlan p;
  std::vector<uint8_t> ok(1, 1);
  for (int warm = 0; warm < 2; warm++) {  // the first call publishes, the second is all hits
    plan_shard(p, &s.ix, msgs.data(), n, off, 1);
    plan_verdicts(p, ok.data(), false);
    s.ix.finish(p.txn, p.ok.data());
  }
  double best = 1e30;
  for (int r = 0; r < reps; r++) {
    const auto t0 = std::chrono::steady_clock::now();
    plan_shard(p, &s.ix, msgs.data(), n, off, 1);
    plan_verdicts(p, ok.data(), false);
    s.ix.finish(p.txn, p.ok.data());
    const double us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
    if (us < best) best = us;
  }
  std::printf("plan_us %.1f hits %llu\n", best, (unsigned long long)s.st[HITS]);
  return 0;
}

int main(int argc, char **argv) {
  if (argc >= 5 && !std::strcmp(argv[1], "--time"))
    return time_plan((uint32_t)std::atoi(argv[2]), (uint32_t)std::atoi(argv[3]), std::atoi(argv[4]));
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
      std::fprintf(stderr, "the index depends on the hash key:\n%s\n%s\n", ra.c_str(), rb.c_str());
      return 1;
    }
    std::printf("%s\n", ra.c_str());
  }
  return 0;
}
