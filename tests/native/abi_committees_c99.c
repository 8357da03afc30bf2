/* C99 consumer of include/grandine_bls_gpu_committees.h: includes the header in a -std=c99 -Wall
 * -Wextra -Werror -pedantic translation unit, calls its five entry points once with one-element
 * arguments and links against grandine_amd/lib/libgrandine_bls.so.  Without a GPU (the CPU suite)
 * every call must fail closed: GBLS_VERIFY_FAIL with GBLS_ERR_NO_DEVICE, failure-filled outputs,
 * and a table size of 0.  Prints "name rc error" per call; tests/test_committees_abi.py checks the
 * output. */
#include <stdio.h>
#include <string.h>

#include "grandine_bls_gpu_committees.h"

#define CALL(name, expr)                                \
  do {                                                  \
    int rc_ = (int)(expr);                              \
    printf("%s %d %d\n", name, rc_, gbls_last_error()); \
  } while (0)

int main(void) {
  static uint8_t m32[1][32], s96[1][96];
  static gbls_p1_affine p1[1];
  static uint64_t rands[1] = {1};
  static uint32_t off2[2] = {0, 1}, idx[1] = {0}, com[1] = {GBLS_NO_COMMITTEE};
  static int32_t st[1];
  size_t k;
  int zero = 1;

  CALL("gbls_init", gbls_init(0, 0));
  st[0] = 0;
  CALL("gbls_committees_set", gbls_committees_set(0, idx, off2, 1, st));
  printf("set_status %d\n", (int)st[0]);
  printf("gbls_committees_size %lu\n", (unsigned long)gbls_committees_size());
  CALL("gbls_committees_clear", gbls_committees_clear());
  st[0] = 0;
  memset(p1, 0xff, sizeof p1);
  CALL("gbls_g1_aggregate_committees", gbls_g1_aggregate_committees(com, idx, off2, 1, p1, st));
  for (k = 0; k < 6; k++) zero = zero && p1[0].x[k] == 0 && p1[0].y[k] == 0;
  printf("key_status %d\n", (int)st[0]);
  printf("key_zero %d\n", zero);
  st[0] = 0;
  com[0] = 0;
  CALL("gbls_multi_verify_committees",
       gbls_multi_verify_committees((const uint8_t(*)[32])m32, (const uint8_t(*)[96])s96, com, idx, off2,
                                    rands, 1, st, GBLS_CALL_BLOCK));
  printf("sig_status %d\n", (int)st[0]);
  return 0;
}
