/* C99 consumer of include/grandine_bls_gpu_msgcache_checks.h: includes the header in a -std=c99
 * -Wall -Wextra -Werror -pedantic translation unit, calls its three entry points and links against
 * grandine_amd/lib/libgrandine_bls.so.  Without a GPU (the CPU suite) serve_checks and checks_stats
 * succeed, prefetch with the cache off answers SKIPPED, and prefetch with the cache on fails closed
 * with GBLS_ERR_NO_DEVICE.  Prints "name rc error" per call; tests/test_msgcache_checks_abi.py
 * checks the output. */
#include <stdio.h>

#include "grandine_bls_gpu_msgcache_checks.h"

#define CALL(name, expr)                                \
  do {                                                  \
    int rc_ = (int)(expr);                              \
    printf("%s %d %d\n", name, rc_, gbls_last_error()); \
  } while (0)

int main(void) {
  static uint8_t m32[3][32];
  int32_t status[3];
  uint64_t st[4];
  int k;

  m32[1][0] = 1;
  m32[2][0] = 1; /* a repeated root */
  CALL("gbls_init", gbls_init(0, 0));
  CALL("serve_default", gbls_msgcache_serve_checks(1));
  CALL("gbls_msgcache_serve_checks", gbls_msgcache_serve_checks(0));
  CALL("serve_off", gbls_msgcache_serve_checks(0));
  for (k = 0; k < 3; k++) status[k] = 77;
  CALL("prefetch_off", gbls_msgcache_prefetch((const uint8_t(*)[32])m32, 3, status));
  printf("status_off %d %d %d\n", (int)status[0], (int)status[1], (int)status[2]);
  CALL("prefetch_none", gbls_msgcache_prefetch(NULL, 0, NULL));
  CALL("prefetch_null", gbls_msgcache_prefetch(NULL, 3, status));
  CALL("configure", gbls_msgcache_configure(64));
  for (k = 0; k < 3; k++) status[k] = 77;
  CALL("gbls_msgcache_prefetch", gbls_msgcache_prefetch((const uint8_t(*)[32])m32, 3, status));
  printf("status_on %d %d %d\n", (int)status[0], (int)status[1], (int)status[2]);
  for (k = 0; k < 4; k++) st[k] = 99;
  CALL("gbls_msgcache_checks_stats", gbls_msgcache_checks_stats(st));
  printf("stats");
  for (k = 0; k < 4; k++) printf(" %lu", (unsigned long)st[k]);
  printf("\n");
  CALL("stats_null", gbls_msgcache_checks_stats(NULL));
  CALL("off_again", gbls_msgcache_configure(0));
  printf("constants %d %d %d\n", GBLS_PREFETCH_ENTERED, GBLS_PREFETCH_PRESENT, GBLS_PREFETCH_SKIPPED);
  return 0;
}
