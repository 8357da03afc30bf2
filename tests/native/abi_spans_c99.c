/* C99 consumer of include/grandine_bls_gpu_spans.h: includes the header in a -std=c99 -Wall -Wextra
 * -Werror -pedantic translation unit, calls its two entry points once with one-element arguments
 * and links against grandine_amd/lib/libgrandine_bls.so.  Without a GPU (the CPU suite) every call
 * must fail closed: GBLS_VERIFY_FAIL with GBLS_ERR_NO_DEVICE, failure-filled statuses, a zeroed
 * key.  Prints "name rc error" per call; tests/test_spans_abi.py checks the output. */
#include <stdio.h>
#include <string.h>

#include "grandine_bls_gpu_spans.h"

#define CALL(name, expr)                                \
  do {                                                  \
    int rc_ = (int)(expr);                              \
    printf("%s %d %d\n", name, rc_, gbls_last_error()); \
  } while (0)

int main(void) {
  static uint8_t m32[1][32], s96[1][96], bits[1] = {3}, cbits[1][8] = {{1, 0, 0, 0, 0, 0, 0, 0}};
  static gbls_p1_affine p1[1];
  static uint64_t rands[1] = {1};
  static uint32_t off2[2] = {0, 1}, none2[2] = {0, 0}, com[1] = {0};
  static int32_t st[1];
  size_t k;
  int zero = 1;

  CALL("gbls_init", gbls_init(0, 0));
  st[0] = 0;
  memset(p1, 0xff, sizeof p1);
  CALL("gbls_g1_aggregate_spans",
       gbls_g1_aggregate_spans(com, (const uint8_t(*)[8])cbits, bits, off2, NULL, none2, 1, p1, st));
  for (k = 0; k < 6; k++) zero = zero && p1[0].x[k] == 0 && p1[0].y[k] == 0;
  printf("key_status %d\n", (int)st[0]);
  printf("key_zero %d\n", zero);
  st[0] = 0;
  CALL("gbls_multi_verify_spans",
       gbls_multi_verify_spans((const uint8_t(*)[32])m32, (const uint8_t(*)[96])s96, com,
                               (const uint8_t(*)[8])cbits, bits, off2, NULL, NULL, rands, 1, st, GBLS_CALL_BLOCK));
  printf("sig_status %d\n", (int)st[0]);
  return 0;
}
