// Test-only host build of the aggregation-bit key step: the per-set functions of
// grandine_amd/csrc/gbls_bits.h (bit-string repacking and validation, the direction rule, the
// per-lane member selection, the finish), the text k_g1_bits_keys compiles for gfx950, behind the
// accumulation loops of the kernel's two forms (one lane per set; 16 lanes per set, lane r taking
// members j = r mod 16, folded as the DPP row fold does, lanes past the row end reading all-zero
// words).  Built as a shared object for tests/test_bits_host.py, and with -DBITS_MAIN as a
// stand-alone program that checks sizes, patterns, encodings and unaligned strings against the
// curve formulas themselves under ASan/UBSan.  Not part of the product.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../grandine_amd/csrc/gbls_bits.h"

using namespace gbls;

extern "C" {

// Key of one committee set.  C96: the cached sum (all-zero = invalid slot).  keys96: the m members'
// keys, 96 bytes each (an all-zero key counts as a bad member, as in the kernel); has_members = 0:
// the slot keeps none.  bits / nbytes: the bit string as it arrives, at any alignment, read only
// through bits_repack.  lanes = 1 or 16.  Returns the status; out96 receives the key;
// info[0] = members whose bit is set, info[1] = 1 when the set subtracted, info[2] = keys added.
int h_bits_key(const uint8_t *C96, const uint8_t *keys96, uint32_t m, uint32_t has_members, const uint8_t *bits,
               uint32_t nbytes, uint32_t lanes, uint8_t *out96, uint32_t *info) {
  g1a C;
  std::memcpy(&C, C96, 96);
  std::vector<uint32_t> row(bits_row_words(nbytes) + 1, 0xdeadbeefu);  // repack owns every word it reads
  bits_repack(row.data(), bits, nbytes);
  uint32_t p = 0, bad0 = 0;
  bool subtract = false;
  if (!has_members || !bits_check(row.data(), nbytes, m, &p)) bad0 = 1;
  subtract = committee_subtracts(m, p);
  const uint32_t mm = bad0 ? 0 : m;
  g1j acc[16];
  uint32_t bad[16] = {0}, adds = 0;
  for (uint32_t r = 0; r < 16; r++) {
    if (r < lanes) {
      jac_set_inf(acc[r]);
      bad[r] = bad0;
    } else {
      std::memset(&acc[r], 0, sizeof(g1j));  // what a row_shl reads past the row end
    }
  }
  for (uint32_t r = 0; r < lanes; r++)
    for (uint32_t i = 0; i < (mm + 31) / 32; i++) {
      uint32_t sel = bits_select(row[i], mm, i, subtract, r, lanes);
      while (sel) {
        const uint32_t j = 32 * i + bits_ctz(sel);
        sel &= sel - 1;
        if (j >= m) return -1;  // the kernel would read past the member list
        g1a q;
        std::memcpy(&q, keys96 + 96 * (size_t)j, 96);
        adds++;
        if (aff_is_inf(q))
          bad[r] = 1;
        else
          jac_add_aff(acc[r], acc[r], q);
      }
    }
  if (lanes > 1)
    for (uint32_t k = 1; k < 16; k <<= 1)
      for (uint32_t r = 0; r < 16; r++) {  // ascending: lane r + k still holds its pre-step value
        g1j o;
        uint32_t ob = 0;
        if (r + k < 16) {
          o = acc[r + k];
          ob = bad[r + k];
        } else {
          std::memset(&o, 0, sizeof(o));
        }
        bad[r] |= ob;
        jac_add(acc[r], acc[r], o);
      }
  g1a key;
  const int32_t st = bits_key(key, C, acc[0], true, subtract, m, p, bad[0]);
  std::memcpy(out96, &key, 96);
  if (info) {
    info[0] = p;
    info[1] = subtract ? 1 : 0;
    info[2] = adds;
  }
  return st;
}

// the launch-form work the host computes from the raw string
uint32_t h_bits_work(const uint8_t *bits, uint32_t nbytes, uint32_t m) {
  std::vector<uint32_t> row(bits_row_words(nbytes) + 1, 0);
  bits_repack(row.data(), bits, nbytes);
  return bits_work(row.data(), nbytes, m);
}

}  // extern "C"

#ifdef BITS_MAIN
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

// the string in a heap buffer of exactly off + nbytes bytes: a read outside it is a report
static int run(const g1a &C, const std::vector<g1a> &P, const std::vector<uint8_t> &s, uint32_t off, uint32_t lanes,
               uint8_t *out, uint32_t *info) {
  uint8_t *buf = static_cast<uint8_t *>(std::malloc(off + s.size() + (s.empty() && !off ? 1 : 0)));
  if (!s.empty()) std::memcpy(buf + off, s.data(), s.size());
  const int st = h_bits_key((const uint8_t *)&C, (const uint8_t *)P.data(), (uint32_t)P.size(), 1, buf + off,
                            (uint32_t)s.size(), lanes, out, info);
  std::free(buf);
  return st;
}

int main() {
  g1a G, zero;
  fp_set(G.x, k::G1X_M);
  fp_set(G.y, k::G1Y_M);
  std::memset(&zero, 0, sizeof(zero));
  uint8_t out[96];
  uint32_t info[3];
  for (uint32_t m : {1u, 7u, 8u, 9u, 15u, 16u, 17u, 31u, 32u, 33u, 63u, 64u, 65u, 257u}) {
    std::vector<g1a> P(m);
    uint64_t all = 0;
    for (uint32_t i = 0; i < m; i++) {
      mul_small(P[i], G, 3 + 2 * i);  // (3 + 2 i) G
      all += 3 + 2 * i;
    }
    g1a C;
    mul_small(C, G, all);
    for (uint32_t pattern = 0; pattern < 6; pattern++) {
      std::vector<uint8_t> set(m, 0);
      for (uint32_t j = 0; j < m; j++)
        set[j] = pattern == 0 ? 1 : pattern == 1 ? 0 : pattern == 2 ? j == m / 2 : pattern == 3 ? j != m / 3
                 : pattern == 4 ? j % 2 == 0 : j < m / 2;
      uint64_t want_k = 0;
      uint32_t p = 0;
      for (uint32_t j = 0; j < m; j++)
        if (set[j]) {
          want_k += 3 + 2 * j;
          p++;
        }
      g1a want = zero;
      if (p) mul_small(want, G, want_k);
      for (int list = 0; list < 2; list++) {
        std::vector<uint8_t> s(list ? m / 8 + 1 : (m + 7) / 8, 0);
        for (uint32_t j = 0; j < m; j++)
          if (set[j]) s[j >> 3] |= (uint8_t)(1u << (j & 7));
        if (list) s[m >> 3] |= (uint8_t)(1u << (m & 7));
        for (uint32_t off = 0; off < 4; off++)
          for (uint32_t lanes : {1u, 16u}) {
            const int st = run(C, P, s, off, lanes, out, info);
            CHECK(st == ST_SUCCESS && std::memcmp(out, &want, 96) == 0);
            CHECK(info[0] == p && info[1] == (m - p < p ? 1u : 0u) && info[2] == (m - p < p ? m - p : p));
          }
        // malformed: one byte long (for a Bitvector[8 k]: the long form without its delimiter), one
        // short (a Bitlist of 8 k members then IS the Bitvector: skipped), the last bit of the last
        // byte where it is neither a member nor the delimiter
        std::vector<uint8_t> t = s;
        t.push_back(0);
        CHECK(run(C, P, t, 1, 16, out, info) == ST_BAD_ENCODING);
        t = s;
        t.pop_back();
        if (!(list && m % 8 == 0)) CHECK(run(C, P, t, 3, 1, out, info) == ST_BAD_ENCODING);
        t = s;
        const uint32_t top = 8 * (uint32_t)s.size() - 1;
        if (top > m) {
          t[top >> 3] |= 0x80;
          CHECK(run(C, P, t, 2, 16, out, info) == ST_BAD_ENCODING && std::memcmp(out, &zero, 96) == 0);
        }
      }
    }
    // an invalid cached sum, in both directions; a slot without members; a bad member
    std::vector<uint8_t> full((m + 7) / 8, 0), none((m + 7) / 8, 0);
    for (uint32_t j = 0; j < m; j++) full[j >> 3] |= (uint8_t)(1u << (j & 7));
    CHECK(run(zero, P, full, 0, 1, out, info) == ST_BAD_ENCODING);
    CHECK(run(zero, P, none, 0, 16, out, info) == ST_BAD_ENCODING);
    CHECK(h_bits_key((const uint8_t *)&C, (const uint8_t *)P.data(), m, 0, full.data(), (uint32_t)full.size(), 1, out,
                     info) == ST_BAD_ENCODING);
    std::vector<g1a> Q = P;
    Q[m - 1] = zero;
    CHECK(run(C, Q, none, 0, 16, out, info) == ST_SUCCESS);  // not among the keys added
    if (m > 2) {  // the bad member is among those added: one clear bit, the last
      std::vector<uint8_t> t = full;
      t[(m - 1) >> 3] &= (uint8_t)~(1u << ((m - 1) & 7));
      CHECK(run(C, Q, t, 1, 16, out, info) == ST_BAD_ENCODING && std::memcmp(out, &zero, 96) == 0);
    }
  }
  if (fails) return 1;
  std::printf("bits_harness: OK\n");
  return 0;
}
#endif
