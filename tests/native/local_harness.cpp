// Test-only host build of the local key sets' host rules (grandine_amd/csrc/gbls_local.h): the
// layout of a launch's pieces (the local sets' pieces in the tail of the piece array, in set
// order, whatever the interleaving and whichever slice of the sets a shard takes), a local set's
// piece, and the argument rules; and, behind the plain-piece loop of k_g1_span_pieces (lane or
// row order) and the finish of k_g1_span_keys (gbls_spans.h span_key), what a local set's piece
// gives over a small table: sums, a repeated position, a key with its negation, an empty range,
// a position past the table, an invalid (all-zero) key.  A stand-alone program (its own main);
// tests/test_local_host.py builds and runs it plainly and under ASan/UBSan, and checks the
// layouts it prints against its own computation.  Not part of the product.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../grandine_amd/csrc/gbls_local.h"

using namespace gbls;

static int fails = 0;
#define CHECK(x)                                         \
  do {                                                   \
    if (!(x)) {                                          \
      std::printf("FAILED line %d: %s\n", __LINE__, #x); \
      fails++;                                           \
    }                                                    \
  } while (0)

static void mul_small(g1a &r, const g1a &base, uint64_t k) {
  g1j t;
  mul_u64(t, base, k);
  jac_to_aff(r, t);
}

// a plain piece over table[ntab] with `lanes` lanes (lane r takes entries r mod lanes), folded in
// ascending order, then the set's finish: the status, the key in *key
static int32_t piece_key(const std::vector<g1a> &table, const std::vector<uint32_t> &list, uint32_t lanes, g1a *key) {
  // the list in a heap buffer of exactly its size: a read outside it is a report
  uint32_t *buf = static_cast<uint32_t *>(std::malloc(list.size() * 4 + (list.empty() ? 4 : 0)));
  if (!list.empty()) std::memcpy(buf, list.data(), list.size() * 4);
  SpanPiece p;
  const uint32_t off[2] = {0, (uint32_t)list.size()};
  local_list_piece(p, 0, buf, off, 0, 0);
  CHECK(p.slot == kNoCommittee && p.cnt == list.size() && p.bit == 0 && p.set == 0 && p.list == buf);
  const uint32_t nreg = (uint32_t)table.size();
  uint32_t bad = 0;
  g1j total;
  jac_set_inf(total);
  for (uint32_t r = 0; r < lanes; r++) {
    g1j acc;
    jac_set_inf(acc);
    for (uint32_t i = r; i < p.cnt; i += lanes) {
      const uint32_t v = p.list[i];
      if (v >= nreg || aff_is_inf(table[v]))
        bad = 1;
      else
        jac_add_aff(acc, acc, table[v]);
    }
    jac_add(total, total, acc);
  }
  std::free(buf);
  const uint32_t flags = SP_PLAIN | (bad ? SP_BAD_INDEX : 0u) | (p.cnt == 0 ? SP_EMPTY : 0u);
  return span_key(*key, total, 1, flags, true);
}

static bool same(const g1a &a, const g1a &b) { return std::memcmp(&a, &b, sizeof(g1a)) == 0; }

static void test_pieces() {
  g1a G, zero;
  fp_set(G.x, k::G1X_M);
  fp_set(G.y, k::G1Y_M);
  std::memset(&zero, 0, sizeof zero);
  // table[j] = (j + 2) G for j < 6, table[6] = -(3 G) = -table[1], table[7] invalid (all-zero)
  std::vector<g1a> table(8);
  for (uint32_t j = 0; j < 6; j++) mul_small(table[j], G, j + 2);
  table[6] = table[1];
  fp_neg(table[6].y, table[6].y);
  table[7] = zero;
  std::vector<uint32_t> longl;
  uint64_t longsum = 0;
  for (uint32_t i = 0; i < 300; i++) {
    longl.push_back((7 * i + 1) % 6);
    longsum += (7 * i + 1) % 6 + 2;
  }
  for (uint32_t lanes : {1u, 16u}) {
    g1a key, want;
    CHECK(piece_key(table, {}, lanes, &key) == ST_AGGR_TYPE_MISMATCH && same(key, zero));  // an empty range
    CHECK(piece_key(table, {4}, lanes, &key) == ST_SUCCESS && same(key, table[4]));
    mul_small(want, G, 2 + 3 + 7);
    CHECK(piece_key(table, {0, 1, 5}, lanes, &key) == ST_SUCCESS && same(key, want));
    mul_small(want, G, 8);
    CHECK(piece_key(table, {2, 2}, lanes, &key) == ST_SUCCESS && same(key, want));            // a repeated position doubles
    CHECK(piece_key(table, {1, 6}, lanes, &key) == ST_SUCCESS && same(key, zero));            // a key with its negation
    CHECK(piece_key(table, {0, 8}, lanes, &key) == ST_BAD_ENCODING && same(key, zero));       // a position >= npkb
    CHECK(piece_key(table, {0xffffffffu}, lanes, &key) == ST_BAD_ENCODING && same(key, zero));
    CHECK(piece_key(table, {0, 7, 1}, lanes, &key) == ST_BAD_ENCODING && same(key, zero));    // an invalid key inside a list
    CHECK(piece_key({}, {0}, lanes, &key) == ST_BAD_ENCODING && same(key, zero));             // an empty table
    mul_small(want, G, longsum);
    CHECK(piece_key(table, longl, lanes, &key) == ST_SUCCESS && same(key, want));
  }
}

// 'L' local, 'P' plain, a digit d: a span set naming d + 1 committees (0 stands for 64)
struct Sets {
  std::vector<uint32_t> com, off, boff;
  std::vector<uint8_t> cbits, bits;
  std::vector<uint32_t> idx;
  size_t n = 0;
  const uint8_t (*masks() const)[8] { return reinterpret_cast<const uint8_t(*)[8]>(cbits.data()); }
};
static Sets make_sets(const char *kinds) {
  Sets s;
  s.n = std::strlen(kinds);
  s.cbits.assign(8 * s.n + 8, 0);
  s.off.push_back(0);
  s.boff.push_back(0);
  for (size_t i = 0; i < s.n; i++) {
    if (kinds[i] == 'L' || kinds[i] == 'P') {
      s.com.push_back(kinds[i] == 'L' ? kLocalKeys : kNoCommittee);
      for (size_t k = 0; k < i % 3; k++) s.idx.push_back((uint32_t)(10 * i + k));  // (every third range empty)
    } else {
      const uint32_t k = kinds[i] == '0' ? 64 : (uint32_t)(kinds[i] - '0') + 1;
      s.com.push_back((uint32_t)(3 * i));
      for (uint32_t c = 0; c < k; c++) s.cbits[8 * i + (c >> 3)] |= (uint8_t)(1u << (c & 7));
      s.bits.push_back((uint8_t)(i + 1));
    }
    s.off.push_back((uint32_t)s.idx.size());
    s.boff.push_back((uint32_t)s.bits.size());
  }
  if (s.idx.empty()) s.idx.push_back(0);
  if (s.bits.empty()) s.bits.push_back(0);
  return s;
}

static void show_layout(const char *kinds, size_t b, size_t e) {
  const Sets s = make_sets(kinds);
  std::vector<uint32_t> first(e - b + 1, 0xdeadbeefu);
  LocalLayout lay;
  CHECK(local_layout(s.com.data(), s.masks(), b, e, first.data(), &lay));
  CHECK(first[e - b] == 0xdeadbeefu);  // nothing written past the slice
  // every piece index is taken exactly once, local sets in the tail, each kind in set order
  std::vector<int> taken(lay.np_span + lay.np_local, 0);
  uint32_t last_s = 0, last_l = lay.np_span;
  for (size_t i = b; i < e; i++) {
    const uint32_t k = local_set_pieces(s.com.data(), s.masks(), i), f = first[i - b];
    const bool loc = local_is(s.com.data(), i);
    CHECK(loc ? (f >= lay.np_span && f == last_l) : (f + k <= lay.np_span && f == last_s));
    (loc ? last_l : last_s) = f + k;
    for (uint32_t q = f; q < f + k; q++) {
      CHECK(q < taken.size());
      if (q < taken.size()) taken[q]++;
    }
    // the set's piece over the shard's slice of the index lists
    if (s.com[i] == kLocalKeys || s.com[i] == kNoCommittee) {
      SpanPiece p;
      const uint32_t *slice = s.idx.data() + s.off[b];
      local_list_piece(p, (uint32_t)(i - b), slice, s.off.data(), b, i);
      CHECK(p.list == s.idx.data() + s.off[i] && p.cnt == s.off[i + 1] - s.off[i] && p.set == i - b);
      CHECK(p.slot == kNoCommittee && p.bit == 0);
      local_list_piece(p, 0, nullptr, nullptr, b, i);  // no ranges at all: an empty list
      CHECK(p.list == nullptr && p.cnt == 0);
    }
  }
  for (int t : taken) CHECK(t == 1);
  std::printf("layout %s %zu %zu %u %u", kinds, b, e, lay.np_span, lay.np_local);
  for (size_t i = b; i < e; i++) std::printf(" %u", first[i - b]);
  std::printf("\n");
}

static void test_args() {
  const Sets s = make_sets("L2PL0P");
  uint8_t pkb[2 * 48] = {0};
  auto ok = [&](const Sets &t, const uint32_t *off, const void *keys, size_t nk) {
    return local_args_ok(t.com.data(), t.masks(), t.bits.data(), t.boff.data(), t.idx.data(), off, keys, nk, t.n);
  };
  CHECK(ok(s, s.off.data(), pkb, 2));
  CHECK(ok(s, s.off.data(), nullptr, 0));        // an empty table: every position is past it, per set
  CHECK(!ok(s, nullptr, pkb, 2));                // a local set when pk_off is NULL
  CHECK(!ok(s, s.off.data(), nullptr, 2));       // pkb == NULL with npkb > 0
  if (sizeof(size_t) > 4) CHECK(!ok(s, s.off.data(), pkb, (size_t)1 << 32));  // npkb past 32 bits
  CHECK(ok(s, s.off.data(), pkb, 0xffffffffu));
  Sets t = s;
  t.cbits[8 * 3] = 1;                            // a local set with committee bits
  CHECK(!ok(t, t.off.data(), pkb, 2));
  t = s;
  for (size_t i = 4; i <= t.n; i++) t.boff[i]++;  // a local set (3) with a bit string
  t.bits.push_back(1);
  CHECK(!ok(t, t.off.data(), pkb, 2));
  t = s;
  for (size_t i = 2; i <= t.n; i++) t.off[i]++;   // a span set (1) with a key range
  t.idx.push_back(0);
  CHECK(!ok(t, t.off.data(), pkb, 2));
  t = s;
  t.off[2] = 5, t.off[3] = 4;                     // decreasing offsets
  CHECK(!ok(t, t.off.data(), pkb, 2));
  const Sets spans = make_sets("213");
  CHECK(ok(spans, nullptr, nullptr, 0) && ok(spans, nullptr, pkb, 2));  // no local set: pk_off may be NULL
  CHECK(!local_args_ok(nullptr, s.masks(), s.bits.data(), s.boff.data(), s.idx.data(), s.off.data(), pkb, 2, s.n));
  CHECK(!local_args_ok(s.com.data(), nullptr, s.bits.data(), s.boff.data(), s.idx.data(), s.off.data(), pkb, 2, s.n));
  CHECK(!local_args_ok(s.com.data(), s.masks(), s.bits.data(), nullptr, s.idx.data(), s.off.data(), pkb, 2, s.n));
}

int main() {
  test_pieces();
  test_args();
  const char *mixed = "L2PL0PLLP7L";
  show_layout(mixed, 0, 11);
  show_layout(mixed, 0, 0);    // an empty slice
  show_layout(mixed, 3, 8);    // shard slices
  show_layout(mixed, 8, 11);
  show_layout(mixed, 4, 5);    // one span set of 64 pieces
  show_layout("LLLL", 0, 4);   // local sets only
  show_layout("P3P", 0, 3);    // none
  if (fails) return 1;
  std::printf("local_harness: OK\n");
  return 0;
}
