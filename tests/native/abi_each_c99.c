/* C99 consumer of include/grandine_bls_gpu_each.h: includes the header in a -std=c99 -Wall -Wextra
 * -Werror -pedantic translation unit, calls its two entry points once with small arguments and
 * links against grandine_amd/lib/libgrandine_bls.so.  Without a GPU (the CPU suite) every call must
 * fail closed: GBLS_VERIFY_FAIL with GBLS_ERR_NO_DEVICE, verdicts at GBLS_VERIFY_FAIL and both
 * status arrays at GBLS_BAD_ENCODING.  Prints "name rc error" per call and the outputs;
 * tests/test_each_abi.py checks them. */
#include <stdio.h>
#include <string.h>

#include "grandine_bls_gpu_each.h"

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
  /* two sets: a one-committee span with a one-byte string, a plain set of one registry index */
  static uint8_t m32[2][32], s96[2][96], bits[1] = {3}, cbits[2][8] = {{1, 0, 0, 0, 0, 0, 0, 0}, {0}};
  static uint64_t rands[2] = {1, 2};
  static uint32_t boff[3] = {0, 1, 1}, poff[3] = {0, 0, 1}, idx[1] = {0}, com[2] = {0, GBLS_NO_COMMITTEE};
  static uint32_t seg[3] = {0, 1, 2};
  static int32_t sst[2], kst[2], v[2];

  CALL("gbls_init", gbls_init(0, 0));
  memset(sst, 0, sizeof sst), memset(kst, 0, sizeof kst), memset(v, 0, sizeof v);
  CALL("gbls_verify_each_spans",
       gbls_verify_each_spans((const uint8_t(*)[32])m32, (const uint8_t(*)[96])s96, com, (const uint8_t(*)[8])cbits,
                              bits, boff, idx, poff, 2, sst, kst, v));
  show("each_sig_status", sst, 2);
  show("each_key_status", kst, 2);
  show("each_verdicts", v, 2);
  memset(sst, 0, sizeof sst), memset(kst, 0, sizeof kst), memset(v, 0, sizeof v);
  CALL("gbls_verify_items_spans",
       gbls_verify_items_spans((const uint8_t(*)[32])m32, (const uint8_t(*)[96])s96, com, (const uint8_t(*)[8])cbits,
                               bits, boff, idx, poff, rands, 2, seg, 2, sst, kst, v, GBLS_CALL_BLOCK));
  show("items_sig_status", sst, 2);
  show("items_key_status", kst, 2);
  show("items_verdicts", v, 2);
  return 0;
}
