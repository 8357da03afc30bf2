/* C99 consumer of include/grandine_bls_gpu_telemetry.h: includes the header in a -std=c99 -Wall
 * -Wextra -Werror -pedantic translation unit, calls every entry and links against
 * grandine_amd/lib/libgrandine_bls.so.  No engine is opened: the level is set and read back, the
 * counters are all zero, the trace is empty, the memory gauges list no engine and hold zeros, and
 * the name functions end in NULL.  Prints one line per fact; tests/test_telemetry_abi.py checks
 * them. */
#include <stdio.h>
#include <string.h>

#include "grandine_bls_gpu_telemetry.h"

static size_t nonzero(const void *p, size_t from, size_t n) {
  size_t i, k = 0;
  for (i = from; i < n; i++) k += ((const unsigned char *)p)[i] != 0;
  return k;
}

static int count(const char *(*name)(int)) {
  int i = 0;
  while (name(i) != NULL) i++;
  return name(i + 1) == NULL && name(-1) == NULL ? i : -1;
}

int main(void) {
  static gbls_telemetry_snapshot snap;
  static gbls_telemetry_memory_info mem;
  static gbls_telemetry_record recs[4];
  struct {
    uint32_t size, level;
    uint64_t trace_written;
  } head; /* an older, shorter struct: the read fills only what fits */
  uint64_t dropped = 77;
  int a, b, c, d, rc;
  size_t n;

  a = gbls_telemetry_enable(1);
  b = gbls_telemetry_enable(2);
  c = gbls_telemetry_enable(7); /* clamped to 2 */
  d = gbls_telemetry_enable(0);
  printf("gbls_telemetry_enable %d %d %d %d %d\n", a, b, c, d, gbls_telemetry_enable(0));

  memset(&snap, 0xff, sizeof snap);
  rc = gbls_telemetry_read(&snap, sizeof snap);
  printf("gbls_telemetry_read %d %u %u %d\n", rc, (unsigned)snap.size, (unsigned)snap.level,
         (int)nonzero(&snap, 8, sizeof snap));
  memset(&head, 0xff, sizeof head);
  rc = gbls_telemetry_read((gbls_telemetry_snapshot *)(void *)&head, sizeof head);
  printf("short_read %d %u %u\n", rc, (unsigned)head.size, (unsigned)sizeof head);
  printf("bad_read %d %d\n", gbls_telemetry_read(NULL, sizeof snap), gbls_telemetry_read(&snap, 4));

  gbls_telemetry_reset();
  memset(recs, 0, sizeof recs);
  n = gbls_telemetry_trace(recs, 4, &dropped);
  printf("gbls_telemetry_trace %d %d %d\n", (int)n, (int)dropped, (int)gbls_telemetry_trace(recs, 4, NULL));

  memset(&mem, 0xff, sizeof mem);
  rc = gbls_telemetry_memory(&mem, sizeof mem);
  printf("gbls_telemetry_memory %d %u %u %d\n", rc, (unsigned)mem.size, (unsigned)mem.engines,
         (int)nonzero(&mem, 8, sizeof mem));

  printf("gbls_telemetry_phase_name %d %s %s\n", count(gbls_telemetry_phase_name), gbls_telemetry_phase_name(0),
         gbls_telemetry_phase_name(GBLS_TELEMETRY_PHASES - 1));
  printf("gbls_telemetry_kind_name %d %s %s\n", count(gbls_telemetry_kind_name), gbls_telemetry_kind_name(0),
         gbls_telemetry_kind_name(GBLS_TELEMETRY_KINDS - 1));
  printf("gbls_telemetry_class_name %d %s %s\n", count(gbls_telemetry_class_name), gbls_telemetry_class_name(0),
         gbls_telemetry_class_name(GBLS_TELEMETRY_CLASSES - 1));
  printf("sizes %u %u %u %u %u %u\n", (unsigned)sizeof(gbls_telemetry_hist), (unsigned)sizeof(gbls_telemetry_cell),
         (unsigned)sizeof(gbls_telemetry_snapshot), (unsigned)sizeof(gbls_telemetry_record),
         (unsigned)sizeof(gbls_telemetry_engine_memory), (unsigned)sizeof(gbls_telemetry_memory_info));
  printf("capacity %d\n", GBLS_TELEMETRY_TRACE_CAPACITY);
  return 0;
}
