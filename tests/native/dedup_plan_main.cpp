// Stand-alone driver of the message-grouping plan (grandine_amd/csrc/gbls_dedup.h), built by
// tests/test_dedup_plan.py with AddressSanitizer and UBSan and run as a program.
//   dedup_plan_main FILE [--time REPS]
// FILE: u32 n, u32 nseg, u32 seg_off[nseg + 1], then n messages of 32 bytes (little endian).
// Prints the plan as text.  The plan is built twice, with the process key (getrandom) and with a
// fixed key: the output must not depend on the key, and the program fails if the two differ.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../grandine_amd/csrc/gbls_dedup.h"

using gbls::dedup::Plan;

static void print_list(const char *name, const std::vector<uint32_t> &v) {
  std::printf("%s", name);
  for (uint32_t x : v) std::printf(" %u", x);
  std::printf("\n");
}

int main(int argc, char **argv) {
  if (argc < 2) return 2;
  FILE *f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  uint32_t hdr[2];
  if (std::fread(hdr, 4, 2, f) != 2) return 2;
  const uint32_t n = hdr[0], nseg = hdr[1];
  std::vector<uint32_t> seg(nseg + 1);
  if (std::fread(seg.data(), 4, nseg + 1, f) != nseg + 1) return 2;
  std::vector<uint8_t> msgs(32 * (size_t)n);
  if (n && std::fread(msgs.data(), 32, n, f) != n) return 2;
  std::fclose(f);
  if (seg[0] != 0 || seg[nseg] != n) return 2;

  Plan a, b;
  gbls::dedup::build(a, msgs.data(), n, seg.data(), nseg);
  gbls::dedup::HashKey fixed;
  for (int i = 0; i < 10; i++) fixed.k[i] = 0x0123456789abcdefull * (uint64_t)(i + 3) | 1;
  gbls::dedup::build(b, msgs.data(), n, seg.data(), nseg, fixed);
  if (a.ngroups != b.ngroups || a.max_group != b.max_group || a.msgs != b.msgs || a.grp_off != b.grp_off ||
      a.grp_set != b.grp_set || a.grp_seg_off != b.grp_seg_off) {  // (scratch members aside)
    std::fprintf(stderr, "plan depends on the hash key\n");
    return 1;
  }
  std::printf("n %u nseg %u groups %u max_group %u duplicates %d\n", a.n, a.nseg, a.ngroups, a.max_group,
              a.has_duplicates() ? 1 : 0);
  print_list("grp_seg_off", a.grp_seg_off);
  print_list("grp_off", a.grp_off);
  print_list("grp_set", a.grp_set);
  std::printf("msgs ");
  for (uint8_t x : a.msgs) std::printf("%02x", x);
  std::printf("\n");
  if (argc >= 4 && !std::strcmp(argv[2], "--time")) {  // host cost of one build (best of REPS)
    const int reps = std::atoi(argv[3]);
    double best = 1e30;
    for (int r = 0; r < reps; r++) {
      const auto t0 = std::chrono::steady_clock::now();
      gbls::dedup::build(b, msgs.data(), n, seg.data(), nseg);
      const double us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
      if (us < best) best = us;
    }
    std::printf("build_us %.1f\n", best);
  }
  return 0;
}
