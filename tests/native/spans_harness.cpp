// Test-only host build of the span-set key steps: the functions of grandine_amd/csrc/gbls_spans.h
// (committee_bits to pieces, the window of a bit row at an arbitrary bit offset, the per-committee
// direction and contribution, the set's finish), the text k_g1_span_pieces and k_g1_span_keys
// compile for gfx950, behind the accumulation loops of the kernels' forms (one lane per piece or 16,
// lane r taking members j = r mod 16; one lane per set or 16, lane r folding pieces r mod 16; the
// row folds as the DPP fold does, lanes past the row end reading all-zero words).  Built as a
// shared object for tests/test_spans_host.py, and with -DSPANS_MAIN as a stand-alone program that
// checks committee sizes, window residues, encodings and malformed strings against the curve
// formulas themselves under ASan/UBSan.  Not part of the product.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../grandine_amd/csrc/gbls_spans.h"

using namespace gbls;

namespace {

// the fold of 16 lanes' values into lane 0, as jac_row_fold<1, 2, 4, 8> does
void row_fold(g1j (&acc)[16], uint32_t (&flag)[16]) {
  for (uint32_t k = 1; k < 16; k <<= 1)
    for (uint32_t r = 0; r < 16; r++) {  // ascending: lane r + k still holds its pre-step value
      g1j o;
      uint32_t of = 0;
      if (r + k < 16) {
        o = acc[r + k];
        of = flag[r + k];
      } else {
        std::memset(&o, 0, sizeof(o));
      }
      flag[r] |= of;
      jac_add(acc[r], acc[r], o);
    }
}

}  // namespace

extern "C" {

// word w of the window at bit `bit` of the string as it arrives (read only through bits_repack)
uint32_t h_span_window(const uint8_t *bits, uint32_t nbytes, uint32_t bit, uint32_t w) {
  std::vector<uint32_t> row(bits_row_words(nbytes) + 1, 0xdeadbeefu);  // the guard word is never read
  bits_repack(row.data(), bits, nbytes);
  return span_window(row.data(), bits_row_words(nbytes), bit, w);
}

// committee_bits to pieces over a table of ntab slots with counts[s] members (0: keeps none).
// out[4 k ..]: piece k's slot, count, bit offset, 1 when it has a list.  Returns the pieces.
uint32_t h_span_pieces(uint32_t com, const uint8_t *cbits, uint32_t ntab, const uint32_t *counts, uint32_t *out,
                       uint32_t *M) {
  static const uint32_t dummy = 0;
  SpanPiece pc[64];
  const uint32_t k = span_pieces(
      7, com, cbits,
      [&](uint32_t slot, const uint32_t **list, uint32_t *cnt) {
        if (slot >= ntab || !counts[slot]) return false;
        *list = &dummy;
        *cnt = counts[slot];
        return true;
      },
      pc, M);
  for (uint32_t i = 0; i < k; i++) {
    out[4 * i] = pc[i].slot;
    out[4 * i + 1] = pc[i].cnt;
    out[4 * i + 2] = pc[i].bit;
    out[4 * i + 3] = pc[i].list != nullptr && pc[i].set == 7;
  }
  return k;
}

// Key of one span set.  The table: ntab slots, slot s with cached sum C96[96 s ..] (all-zero =
// invalid) and members mem_off[s] .. mem_off[s + 1] of keys96 (96 bytes each; an all-zero key
// counts as a bad member, as in the kernel); keeps[s] = 0: the slot keeps no members.
// bits / nbytes: the string as it arrives, at any alignment.  piece_lanes / fold_lanes = 1 or 16.
// Returns the status; out96 receives the key; info[0] = pieces, info[1] = M, then per piece
// [participants, 1 when it subtracted, keys added, flags].
int h_span_key(uint32_t com, const uint8_t *cbits, uint32_t ntab, const uint8_t *C96, const uint32_t *mem_off,
               const uint8_t *keeps, const uint8_t *keys96, const uint8_t *bits, uint32_t nbytes,
               uint32_t piece_lanes, uint32_t fold_lanes, uint8_t *out96, uint32_t *info) {
  std::vector<uint32_t> ids(mem_off[ntab] + 1);
  for (uint32_t i = 0; i < mem_off[ntab]; i++) ids[i] = i;
  std::vector<uint32_t> row(bits_row_words(nbytes) + 1, 0xdeadbeefu);
  bits_repack(row.data(), bits, nbytes);
  const uint32_t nw = bits_row_words(nbytes);
  SpanPiece pc[64];
  SpanSet set = {0, 0, 0, nbytes, 0};
  set.npieces = span_pieces(
      0, com, cbits,
      [&](uint32_t slot, const uint32_t **list, uint32_t *cnt) {
        if (slot >= ntab || !keeps[slot]) return false;
        *list = ids.data() + mem_off[slot];
        *cnt = mem_off[slot + 1] - mem_off[slot];
        return true;
      },
      pc, &set.M);
  std::vector<g1j> contrib(set.npieces + 1);
  std::vector<uint32_t> pflags(set.npieces + 1);
  info[0] = set.npieces;
  info[1] = set.M;
  for (uint32_t q = 0; q < set.npieces; q++) {  // k_g1_span_pieces
    const SpanPiece &d = pc[q];
    const uint32_t m = d.list ? d.cnt : 0;
    const uint32_t p = span_count(row.data(), nw, d.bit, m);
    const bool subtract = committee_subtracts(m, p);
    g1j acc[16];
    uint32_t bad[16] = {0}, adds = 0;
    for (uint32_t r = 0; r < 16; r++) {
      if (r < piece_lanes)
        jac_set_inf(acc[r]);
      else
        std::memset(&acc[r], 0, sizeof(g1j));  // what a row_shl reads past the row end
    }
    for (uint32_t r = 0; r < piece_lanes; r++)
      for (uint32_t i = 0; i < (m + 31) / 32; i++) {
        uint32_t sel = bits_select(span_window(row.data(), nw, d.bit, i), m, i, subtract, r, piece_lanes);
        while (sel) {
          const uint32_t j = 32 * i + bits_ctz(sel);
          sel &= sel - 1;
          if (j >= m) return -1;  // the kernel would read past the member list
          g1a k;
          std::memcpy(&k, keys96 + 96 * (size_t)d.list[j], 96);
          adds++;
          if (aff_is_inf(k))
            bad[r] = 1;
          else
            jac_add_aff(acc[r], acc[r], k);
        }
      }
    if (piece_lanes > 1) row_fold(acc, bad);
    g1a C;
    std::memset(&C, 0, sizeof(C));
    if (d.slot < ntab) std::memcpy(&C, C96 + 96 * (size_t)d.slot, 96);
    pflags[q] = span_contribution(contrib[q], C, acc[0], d.list != nullptr, subtract, p, bad[0]);
    info[2 + 4 * q] = p;
    info[3 + 4 * q] = subtract ? 1 : 0;
    info[4 + 4 * q] = adds;
    info[5 + 4 * q] = pflags[q];
  }
  g1j acc[16];  // k_g1_span_keys
  uint32_t flags[16] = {0};
  for (uint32_t r = 0; r < 16; r++) {
    if (r < fold_lanes)
      jac_set_inf(acc[r]);
    else
      std::memset(&acc[r], 0, sizeof(g1j));
  }
  for (uint32_t r = 0; r < fold_lanes; r++)
    for (uint32_t i = r; i < set.npieces; i += fold_lanes) {
      flags[r] |= pflags[i];
      jac_add(acc[r], acc[r], contrib[i]);
    }
  if (fold_lanes > 1) row_fold(acc, flags);
  uint32_t p = 0;
  const bool ok = bits_check(row.data(), set.nbytes, set.M, &p);
  g1a key;
  const int32_t st = span_key(key, acc[0], set.npieces, flags[0], ok);
  std::memcpy(out96, &key, 96);
  return st;
}

// a plain set's finish: flags as the piece kernel forms them for a list of m keys
int h_span_plain(const uint8_t *keys96, uint32_t m, uint8_t *out96) {
  g1j acc;
  jac_set_inf(acc);
  uint32_t bad = 0;
  for (uint32_t i = 0; i < m; i++) {
    g1a k;
    std::memcpy(&k, keys96 + 96 * (size_t)i, 96);
    if (aff_is_inf(k))
      bad = 1;
    else
      jac_add_aff(acc, acc, k);
  }
  g1a key;
  const int32_t st = span_key(key, acc, 1, SP_PLAIN | (bad ? SP_BAD_INDEX : 0u) | (m == 0 ? SP_EMPTY : 0u), true);
  std::memcpy(out96, &key, 96);
  return st;
}

}  // extern "C"

#ifdef SPANS_MAIN
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

struct Table {
  std::vector<g1a> C, keys;
  std::vector<uint32_t> off;
  std::vector<uint8_t> keeps;
};

// the string in a heap buffer of exactly shift + nbytes bytes: a read outside it is a report
static int run(const Table &t, uint32_t com, const uint8_t *cbits, const std::vector<uint8_t> &s, uint32_t shift,
               uint32_t pl, uint32_t fl, uint8_t *out, uint32_t *info) {
  uint8_t *buf = static_cast<uint8_t *>(std::malloc(shift + s.size() + (s.empty() && !shift ? 1 : 0)));
  if (!s.empty()) std::memcpy(buf + shift, s.data(), s.size());
  const int st = h_span_key(com, cbits, (uint32_t)t.C.size(), (const uint8_t *)t.C.data(), t.off.data(),
                            t.keeps.data(), (const uint8_t *)t.keys.data(), buf + shift, (uint32_t)s.size(), pl, fl,
                            out, info);
  std::free(buf);
  return st;
}

int main() {
  g1a G, zero;
  fp_set(G.x, k::G1X_M);
  fp_set(G.y, k::G1Y_M);
  std::memset(&zero, 0, sizeof(zero));
  const uint32_t sizes[] = {1, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65};
  const uint32_t ns = sizeof(sizes) / sizeof(sizes[0]);
  // slot s: sizes[s % ns] members, member j of slot s has scalar 3 + 2 (global position)
  Table t;
  t.off.push_back(0);
  std::vector<uint64_t> sc;
  for (uint32_t s = 0; s < 2 * ns; s++) {
    uint64_t all = 0;
    for (uint32_t j = 0; j < sizes[s % ns]; j++) {
      const uint64_t k = 3 + 2 * (uint64_t)t.keys.size();
      g1a P;
      mul_small(P, G, k);
      t.keys.push_back(P);
      sc.push_back(k);
      all += k;
    }
    g1a C;
    mul_small(C, G, all);
    t.C.push_back(C);
    t.off.push_back((uint32_t)t.keys.size());
    t.keeps.push_back(1);
  }
  uint8_t out[96];
  std::vector<uint32_t> info(2 + 4 * 64);
  uint32_t seen = 0;  // the bit residues at which a window started
  // one mask: the named committees' patterns, both encodings, shifted strings, every form pair
  // (quick: one pair), and the malformed strings over M
  auto check_mask = [&](uint32_t com, const std::vector<uint32_t> &named, uint32_t pattern, bool quick) {
    uint8_t cbits[8] = {0};
    for (uint32_t c : named) cbits[c >> 3] |= (uint8_t)(1u << (c & 7));
    std::vector<uint8_t> bit;
    uint64_t want_k = 0;
    uint32_t at = 0;
    std::vector<uint32_t> pcs, dir;
    for (uint32_t i = 0; i < named.size(); i++) {
      const uint32_t s = com + named[i], m = sizes[s % ns];
      seen |= 1u << (at & 31);
      // per committee: everyone, one absent, one present, every other (rotating with the pattern)
      const uint32_t kind = (pattern + i) % 4;
      uint32_t p = 0;
      for (uint32_t j = 0; j < m; j++) {
        const bool b = kind == 0 ? true : kind == 1 ? (j != m / 2 || m == 1) : kind == 2 ? j == m / 3 : (j % 2 == 0);
        bit.push_back(b);
        if (b) {
          want_k += sc[t.off[s] + j];
          p++;
        }
      }
      pcs.push_back(p);
      dir.push_back(m - p < p);
      at += m;
    }
    g1a want;
    mul_small(want, G, want_k);
    const uint32_t M = (uint32_t)bit.size();
    for (int list = 0; list < 2; list++) {
      std::vector<uint8_t> s(list ? M / 8 + 1 : (M + 7) / 8, 0);
      for (uint32_t j = 0; j < M; j++)
        if (bit[j]) s[j >> 3] |= (uint8_t)(1u << (j & 7));
      if (list) s[M >> 3] |= (uint8_t)(1u << (M & 7));
      for (uint32_t shift : {0u, 3u})
        for (uint32_t pl : {1u, 16u})
          for (uint32_t fl : {1u, 16u}) {
            if (quick && (shift != (uint32_t)(list ? 3 : 0) || pl == fl)) continue;
            const int st = run(t, com, cbits, s, shift, pl, fl, out, info.data());
            CHECK(st == ST_SUCCESS && std::memcmp(out, &want, 96) == 0);
            CHECK(info[0] == named.size() && info[1] == M);
            for (uint32_t i = 0; i < named.size(); i++)
              CHECK(info[2 + 4 * i] == pcs[i] && info[3 + 4 * i] == dir[i] && info[5 + 4 * i] == 0);
          }
      // malformed over M: one byte long, one short, a stray top bit
      std::vector<uint8_t> u = s;
      u.push_back(0);
      CHECK(run(t, com, cbits, u, 1, 16, 16, out, info.data()) == ST_BAD_ENCODING && std::memcmp(out, &zero, 96) == 0);
      u = s;
      u.pop_back();
      if (!(list && M % 8 == 0)) CHECK(run(t, com, cbits, u, 2, 1, 1, out, info.data()) == ST_BAD_ENCODING);
      u = s;
      const uint32_t top = 8 * (uint32_t)s.size() - 1;
      if (top > M) {
        u[top >> 3] |= 0x80;
        CHECK(run(t, com, cbits, u, 0, 16, 1, out, info.data()) == ST_BAD_ENCODING);
      }
    }
  };
  for (uint32_t com = 0; com < ns; com++)
    for (uint32_t span : {1u, 2u, 3u, 13u}) {
      // the named committees: `span` of them, every other index from 1 on (bit 0 for one)
      std::vector<uint32_t> named;
      for (uint32_t i = 0; i < span; i++) named.push_back(span == 1 ? 0 : (i < 7 ? 2 * i + 1 : i + 7));
      if (com + named.back() >= 2 * ns) continue;
      for (uint32_t pattern = 0; pattern < 4; pattern++) check_mask(com, named, pattern, false);
    }
  // masks from base 0 whose last window starts at each of the 32 bit residues of a row word
  const std::vector<uint32_t> residue[32] = {
      {8, 9},          {0, 1},          {0, 9, 10},   {0, 6, 19, 20},    {0, 3, 6, 16, 17}, {1, 4, 17, 18}, {1, 7, 8},
      {1, 2},          {2, 3},          {3, 4},       {0, 3, 4},         {0, 3, 9, 10},     {0, 3, 6, 19, 20},
      {1, 7, 14, 15},  {1, 14, 15},     {4, 5},       {5, 6},            {6, 7},            {0, 6, 7},
      {0, 3, 16, 17},  {0, 3, 9, 16, 17}, {1, 4, 7, 8}, {1, 4, 5},       {1, 5, 6},         {1, 6, 7},
      {2, 6, 7},       {3, 6, 7},       {0, 3, 6, 7}, {0, 3, 6, 9, 10},  {1, 4, 14, 15},    {4, 17, 18},
      {7, 8}};
  for (uint32_t r = 0; r < 32; r++) check_mask(0, residue[r], r, true);
  CHECK(seen == 0xffffffffu);
  // an empty mask; a committee without a participant among others; a slot past the table; a base
  // that would wrap 32 bits; a slot without members; an invalid cached sum
  uint8_t none[8] = {0}, two[8] = {3, 0, 0, 0, 0, 0, 0, 0}, far[8] = {0, 0, 0, 0, 0, 0, 0, 0x80};
  std::vector<uint8_t> s((1 + 7 + 7) / 8, 0);
  CHECK(run(t, 0, none, {}, 0, 1, 1, out, info.data()) == ST_BAD_ENCODING);
  s[0] = 0x02;  // committee 0 (1 member) empty, committee 1 (7 members) has its first
  CHECK(run(t, 0, two, s, 0, 1, 16, out, info.data()) == ST_BAD_ENCODING && (info[5] & SP_EMPTY));
  s[0] = 0x03;
  CHECK(run(t, 0, two, s, 0, 16, 1, out, info.data()) == ST_SUCCESS);
  CHECK(run(t, 2 * ns - 1, two, s, 0, 1, 1, out, info.data()) == ST_BAD_ENCODING);
  CHECK(run(t, 0xffffffc1u, far, s, 0, 1, 1, out, info.data()) == ST_BAD_ENCODING);  // + 63 = 2^32: not slot 0
  Table v = t;
  v.keeps[1] = 0;
  CHECK(run(v, 0, two, s, 0, 1, 1, out, info.data()) == ST_BAD_ENCODING);
  v = t;
  v.C[0] = zero;
  CHECK(run(v, 0, two, s, 0, 16, 16, out, info.data()) == ST_BAD_ENCODING && (info[5] & SP_BAD_SLOT));
  // plain sets
  CHECK(h_span_plain((const uint8_t *)t.keys.data(), 0, out) == ST_AGGR_TYPE_MISMATCH);
  g1a three;
  mul_small(three, G, 3 + 5);
  CHECK(h_span_plain((const uint8_t *)t.keys.data(), 2, out) == ST_SUCCESS && std::memcmp(out, &three, 96) == 0);
  if (fails) return 1;
  std::printf("spans_harness: OK\n");
  return 0;
}
#endif
