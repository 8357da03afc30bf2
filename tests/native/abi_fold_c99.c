/* C99 consumer of include/grandine_bls_gpu_fold.h: includes the header in a -std=c99 -Wall -Wextra
 * -Werror -pedantic translation unit, calls its entry point with three sets in three groups (one
 * of them empty, one naming a set twice) and links against grandine_amd/lib/libgrandine_bls.so.
 * Without a GPU (the CPU suite) the call must fail closed: GBLS_VERIFY_FAIL with
 * GBLS_ERR_NO_DEVICE, verdicts at GBLS_VERIFY_FAIL, both status arrays at GBLS_BAD_ENCODING, the
 * points all-zero, the counts zero and the bytes at the infinity encoding.  Prints "name rc error"
 * per call and the outputs; tests/test_fold_abi.py checks them. */
#include <stdio.h>
#include <string.h>

#include "grandine_bls_gpu_fold.h"

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
  /* a one-committee span with a one-byte string, and two plain sets of one registry index each */
  static uint8_t m32[3][32], s96[3][96], bits[1] = {3}, cbits[3][8] = {{1, 0, 0, 0, 0, 0, 0, 0}, {0}, {0}};
  static uint32_t boff[4] = {0, 1, 1, 1}, poff[4] = {0, 0, 1, 2}, idx[2] = {0, 1};
  static uint32_t com[3] = {0, GBLS_NO_COMMITTEE, GBLS_NO_COMMITTEE};
  static uint32_t fset[5] = {0, 1, 2, 1, 1}, foff[4] = {0, 3, 3, 5};
  static int32_t sst[3], kst[3], v[3];
  static gbls_p2_affine out[3];
  static uint8_t fb[3][96];
  static uint32_t cnt[3];
  size_t i, g, nonzero = 0, inf = 0;

  CALL("gbls_init", gbls_init(0, 0));
  memset(sst, 0, sizeof sst), memset(kst, 0, sizeof kst), memset(v, 0, sizeof v);
  memset(out, 0xff, sizeof out), memset(fb, 0xff, sizeof fb), memset(cnt, 0xff, sizeof cnt);
  CALL("gbls_verify_each_fold",
       gbls_verify_each_fold((const uint8_t(*)[32])m32, (const uint8_t(*)[96])s96, com, (const uint8_t(*)[8])cbits, bits,
                             boff, idx, poff, 3, fset, foff, 3, sst, kst, v, out, fb, cnt));
  show("fold_sig_status", sst, 3);
  show("fold_key_status", kst, 3);
  show("fold_verdicts", v, 3);
  for (i = 0; i < sizeof out; i++) nonzero += ((const unsigned char *)out)[i] != 0;
  printf("fold_out_nonzero_bytes %d\n", (int)nonzero);
  printf("fold_count %u %u %u\n", (unsigned)cnt[0], (unsigned)cnt[1], (unsigned)cnt[2]);
  for (g = 0; g < 3; g++) {
    int ok = fb[g][0] == 0xc0;
    for (i = 1; i < 96; i++) ok = ok && fb[g][i] == 0;
    inf += (size_t)ok;
  }
  printf("fold_bytes_infinity %d\n", (int)inf);
  /* no bytes asked for, and no groups at all */
  memset(out, 0xff, sizeof out), memset(cnt, 0xff, sizeof cnt);
  CALL("no_bytes", gbls_verify_each_fold((const uint8_t(*)[32])m32, (const uint8_t(*)[96])s96, com,
                                         (const uint8_t(*)[8])cbits, bits, boff, idx, poff, 3, fset, foff, 3, sst, kst, v,
                                         out, NULL, cnt));
  nonzero = 0;
  for (i = 0; i < sizeof out; i++) nonzero += ((const unsigned char *)out)[i] != 0;
  printf("no_bytes_out_nonzero_bytes %d\n", (int)nonzero);
  printf("no_bytes_count %u %u %u\n", (unsigned)cnt[0], (unsigned)cnt[1], (unsigned)cnt[2]);
  memset(v, 0, sizeof v);
  CALL("no_groups", gbls_verify_each_fold((const uint8_t(*)[32])m32, (const uint8_t(*)[96])s96, com,
                                          (const uint8_t(*)[8])cbits, bits, boff, idx, poff, 3, NULL, NULL, 0, sst, kst, v,
                                          NULL, NULL, NULL));
  show("no_groups_verdicts", v, 3);
  return 0;
}
