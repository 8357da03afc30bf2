/* C99 consumer of include/grandine_bls_gpu_msgcache.h: includes the header in a -std=c99 -Wall
 * -Wextra -Werror -pedantic translation unit, calls its four entry points and links against
 * grandine_amd/lib/libgrandine_bls.so.  None of the four needs a device: without a GPU (the CPU
 * suite) configure, clear and stats succeed with zero counters, while a verification call still
 * fails closed with GBLS_ERR_NO_DEVICE.  Prints "name rc error" per call;
 * tests/test_msgcache_abi.py checks the output. */
#include <stdio.h>

#include "grandine_bls_gpu_msgcache.h"

#define CALL(name, expr)                                \
  do {                                                  \
    int rc_ = (int)(expr);                              \
    printf("%s %d %d\n", name, rc_, gbls_last_error()); \
  } while (0)

int main(void) {
  static uint8_t m32[1][32];
  static gbls_p1_affine p1[1];
  static gbls_p2_affine p2[1];
  static uint64_t rands[1] = {1};
  uint64_t st[8];
  int k;

  CALL("gbls_init", gbls_init(0, 0));
  printf("slots_default %lu\n", (unsigned long)gbls_msgcache_slots());
  CALL("too_many", gbls_msgcache_configure(((size_t)1 << 20) + 1));
  CALL("gbls_msgcache_configure", gbls_msgcache_configure(4096));
  printf("gbls_msgcache_slots %lu\n", (unsigned long)gbls_msgcache_slots());
  CALL("gbls_msgcache_clear", gbls_msgcache_clear());
  CALL("gbls_multi_verify", gbls_multi_verify((const uint8_t(*)[32])m32, p2, p1, rands, 1));
  for (k = 0; k < 8; k++) st[k] = 99;
  CALL("gbls_msgcache_stats", gbls_msgcache_stats(st));
  printf("stats");
  for (k = 0; k < 8; k++) printf(" %lu", (unsigned long)st[k]);
  printf("\n");
  CALL("off_again", gbls_msgcache_configure(0));
  printf("slots_off %lu\n", (unsigned long)gbls_msgcache_slots());
  return 0;
}
