/* C99 consumer of include/grandine_bls_gpu_local.h: includes the header in a -std=c99 -Wall -Wextra
 * -Werror -pedantic translation unit, calls its three entry points once with small arguments and
 * links against grandine_amd/lib/libgrandine_bls.so.  Without a GPU (the CPU suite) every call must
 * fail closed: GBLS_VERIFY_FAIL with GBLS_ERR_NO_DEVICE, verdicts at GBLS_VERIFY_FAIL, the keys
 * all-zero and every status array, the table's included, at GBLS_BAD_ENCODING.  Prints
 * "name rc error" per call and the outputs; tests/test_local_abi.py checks them. */
#include <stdio.h>
#include <string.h>

#include "grandine_bls_gpu_local.h"

#define CALL(name, expr)                                \
  do {                                                  \
    int rc_ = (int)(expr);                              \
    printf("%s %d %d\n", name, rc_, gbls_last_error()); \
  } while (0)

static void show(const char *what, const int32_t *v, size_t n) {
  size_t i;
  printf("%s", what);
  for (i = 0; i < n; i++) printf(" %d", (int)v[i]);
  printf("\n");
}

int main(void) {
  /* three sets: a one-committee span with a one-byte string, a plain set of one registry index, a
   * local set of two table positions; a table of two keys that do not decode (all-zero bytes) */
  static uint8_t m32[3][32], s96[3][96], bits[1] = {3}, cbits[3][8] = {{1, 0, 0, 0, 0, 0, 0, 0}, {0}, {0}};
  static uint8_t pkb[2][48];
  static uint64_t rands[3] = {1, 2, 3};
  static uint32_t boff[4] = {0, 1, 1, 1}, poff[4] = {0, 0, 1, 3}, idx[3] = {0, 0, 1};
  static uint32_t com[3] = {0, GBLS_NO_COMMITTEE, GBLS_LOCAL_KEYS};
  static uint32_t seg[3] = {0, 1, 3};
  static int32_t sst[3], kst[3], v[3], pst[2];
  static gbls_p1_affine keys[3];
  size_t i, nonzero = 0;

  CALL("gbls_init", gbls_init(0, 0));
  memset(kst, 0, sizeof kst), memset(pst, 0, sizeof pst), memset(keys, 0xff, sizeof keys);
  CALL("gbls_g1_aggregate_local",
       gbls_g1_aggregate_local(com, (const uint8_t(*)[8])cbits, bits, boff, idx, poff, (const uint8_t(*)[48])pkb, 2, 3,
                               keys, kst, pst));
  show("keys_status", kst, 3);
  show("keys_pkb_status", pst, 2);
  for (i = 0; i < sizeof keys; i++) nonzero += ((const unsigned char *)keys)[i] != 0;
  printf("keys_nonzero_bytes %d\n", (int)nonzero);
  memset(sst, 0, sizeof sst), memset(kst, 0, sizeof kst), memset(v, 0, sizeof v), memset(pst, 0, sizeof pst);
  CALL("gbls_verify_each_local",
       gbls_verify_each_local((const uint8_t(*)[32])m32, (const uint8_t(*)[96])s96, com, (const uint8_t(*)[8])cbits,
                              bits, boff, idx, poff, (const uint8_t(*)[48])pkb, 2, 3, sst, kst, v, pst));
  show("each_sig_status", sst, 3);
  show("each_key_status", kst, 3);
  show("each_verdicts", v, 3);
  show("each_pkb_status", pst, 2);
  memset(sst, 0, sizeof sst), memset(kst, 0, sizeof kst), memset(v, 0, sizeof v), memset(pst, 0, sizeof pst);
  CALL("gbls_verify_items_local",
       gbls_verify_items_local((const uint8_t(*)[32])m32, (const uint8_t(*)[96])s96, com, (const uint8_t(*)[8])cbits,
                               bits, boff, idx, poff, (const uint8_t(*)[48])pkb, 2, rands, 3, seg, 2, sst, kst, v, pst,
                               GBLS_CALL_BLOCK));
  show("items_sig_status", sst, 3);
  show("items_key_status", kst, 3);
  show("items_verdicts", v, 2);
  show("items_pkb_status", pst, 2);
  return 0;
}
