// Test-only host build of the cached-committee key step: the per-set function of
// grandine_amd/csrc/gbls_committees.h, the text k_g1_committee_keys compiles for gfx950, behind
// the accumulation loops of the kernel's two forms (one lane per set; 16 lanes per set folded as
// the DPP row fold does, lanes past the row end reading all-zero words).  Built as a shared
// object for tests/test_committees_host.py, and with -DCOMMITTEES_MAIN as a stand-alone program
// that checks the degenerate cases against the curve formulas themselves under ASan/UBSan.  Not
// part of the product.
#include <cstdio>
#include <cstring>

#include "../../grandine_amd/csrc/gbls_committees.h"

using namespace gbls;

extern "C" {

// key of one set: C (96 bytes, all-zero = invalid slot) with CK_COMMITTEE in flags, the nkeys
// listed keys (96 bytes each; an all-zero key counts as a bad index, as in the kernel), lanes = 1
// or 16.  Returns the status; out96 receives the key.
int h_committee_key(const uint8_t *C96, const uint8_t *keys96, uint32_t nkeys, uint32_t flags, uint32_t lanes,
                    uint8_t *out96) {
  g1a C;
  std::memcpy(&C, C96, 96);
  g1j acc[16];
  uint32_t bad[16] = {0};
  for (uint32_t r = 0; r < 16; r++) {
    if (r < lanes) {
      jac_set_inf(acc[r]);
    } else {
      std::memset(&acc[r], 0, sizeof(g1j));  // what a row_shl reads past the row end
    }
  }
  for (uint32_t r = 0; r < lanes; r++)
    for (uint32_t i = r; i < nkeys; i += lanes) {
      g1a p;
      std::memcpy(&p, keys96 + 96 * (size_t)i, 96);
      if (aff_is_inf(p))
        bad[r] = 1;
      else
        jac_add_aff(acc[r], acc[r], p);
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
  uint32_t f = (flags & CK_COMMITTEE) | (nkeys == 0 ? CK_EMPTY : 0u) | (bad[0] ? CK_BAD_INDEX : 0u) |
               (flags & CK_BAD_INDEX);
  g1a key;
  int32_t st = committee_key(key, C, acc[0], f);
  std::memcpy(out96, &key, 96);
  return st;
}

}  // extern "C"

#ifdef COMMITTEES_MAIN
static int fails = 0;
#define CHECK(x)                                      \
  do {                                                \
    if (!(x)) {                                       \
      std::printf("FAILED line %d: %s\n", __LINE__, #x); \
      fails++;                                        \
    }                                                 \
  } while (0)

static void mul_small(g1a &r, const g1a &base, uint32_t k) {
  g1j t;
  mul_u64(t, base, (uint64_t)k);
  jac_to_aff(r, t);
}

int main() {
  g1a G, zero;
  fp_set(G.x, k::G1X_M);
  fp_set(G.y, k::G1Y_M);
  std::memset(&zero, 0, sizeof(zero));
  g1a P[20];
  for (uint32_t i = 0; i < 20; i++) mul_small(P[i], G, 3 + 2 * i);  // (3 + 2 i) G
  uint8_t out[96];
  for (uint32_t lanes : {1u, 16u}) {
    // committee = P[0..20): C = (sum of 3 + 2 i) G = 440 G; absentees P[0..m): key = C - their sum
    g1a C;
    mul_small(C, G, 440);
    for (uint32_t m : {0u, 1u, 2u, 17u, 20u}) {
      uint32_t s = 0;
      for (uint32_t i = 0; i < m; i++) s += 3 + 2 * i;
      int st = h_committee_key((const uint8_t *)&C, (const uint8_t *)P, m, CK_COMMITTEE, lanes, out);
      g1a want;
      mul_small(want, G, 440 - s);  // m = 20: every member absent, the key is infinity (all-zero)
      CHECK(st == ST_SUCCESS && std::memcmp(out, &want, 96) == 0);
      // the same list without a committee: the plain sum
      st = h_committee_key((const uint8_t *)&zero, (const uint8_t *)P, m, 0, lanes, out);
      mul_small(want, G, s);
      CHECK(st == (m ? ST_SUCCESS : ST_AGGR_TYPE_MISMATCH) && std::memcmp(out, m ? (const void *)&want : &zero, 96) == 0);
    }
    // S = C: identity; S = -C: doubling
    g1a nC = C, C2;
    fp_neg(nC.y, C.y);
    mul_small(C2, G, 880);
    CHECK(h_committee_key((const uint8_t *)&C, (const uint8_t *)&C, 1, CK_COMMITTEE, lanes, out) == ST_SUCCESS &&
          std::memcmp(out, &zero, 96) == 0);
    CHECK(h_committee_key((const uint8_t *)&C, (const uint8_t *)&nC, 1, CK_COMMITTEE, lanes, out) == ST_SUCCESS &&
          std::memcmp(out, &C2, 96) == 0);
    // S infinite from a nonempty list of cancelling keys: the key is C
    g1a pair[2] = {P[4], P[4]};
    fp_neg(pair[1].y, P[4].y);
    CHECK(h_committee_key((const uint8_t *)&C, (const uint8_t *)pair, 2, CK_COMMITTEE, lanes, out) == ST_SUCCESS &&
          std::memcmp(out, &C, 96) == 0);
    // an invalid slot, a bad index
    CHECK(h_committee_key((const uint8_t *)&zero, (const uint8_t *)P, 1, CK_COMMITTEE, lanes, out) == ST_BAD_ENCODING &&
          std::memcmp(out, &zero, 96) == 0);
    g1a withbad[3] = {P[0], zero, P[1]};
    CHECK(h_committee_key((const uint8_t *)&C, (const uint8_t *)withbad, 3, CK_COMMITTEE, lanes, out) == ST_BAD_ENCODING &&
          std::memcmp(out, &zero, 96) == 0);
  }
  if (fails) return 1;
  std::printf("committees_harness: OK\n");
  return 0;
}
#endif
