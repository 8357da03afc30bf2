// Test-only host build of the verified folds' shared code (grandine_amd/csrc/gbls_fold.h): the
// argument rules, and the accumulation and finish that k_fold.hip compiles for the device, here
// compiled for the CPU and run in the two orders the kernels use:
//   rows  16 lanes per group, lane r taking every 16th entry, folded by the four row_shl steps
//         (lane r += lane r + K for K = 1, 2, 4, 8; lanes past the row end read infinity)
//   wg    256 lanes per group, lane t taking every 256th entry, the LDS tree (t += t + w for
//         w = 128 .. 1)
// Input (argv[1]): "n", then n lines "<384 hex digits of an affine G2 point, Montgomery limbs>
// <verdict>", then "g", then g lines "<k> <set> ... <set>".  Output: per order and group
// "<order> <g> <count> <point hex> <compressed hex>"; tests/test_fold_host.py compares them with
// the Python oracle.  A stand-alone program (its own main), run plainly and under ASan/UBSan.
// Not part of the product.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../grandine_amd/csrc/gbls_fold.h"

using namespace gbls;

static int fails = 0;
#define CHECK(x)                                         \
  do {                                                   \
    if (!(x)) {                                          \
      std::printf("FAILED line %d: %s\n", __LINE__, #x); \
      fails++;                                           \
    }                                                    \
  } while (0)

static void hex(const void *p, size_t n) {
  const unsigned char *b = static_cast<const unsigned char *>(p);
  for (size_t i = 0; i < n; i++) std::printf("%02x", b[i]);
}

// the inputs in heap buffers of exactly their size: a read outside them is a report
struct Input {
  g2a *sigs = nullptr;
  int32_t *verdicts = nullptr;
  uint32_t *set = nullptr, *off = nullptr;
  uint32_t n = 0, ng = 0;
  ~Input() {
    std::free(sigs), std::free(verdicts), std::free(set), std::free(off);
  }
};

static bool read_input(const char *path, Input &in) {
  std::FILE *f = std::fopen(path, "r");
  if (!f) return false;
  bool ok = std::fscanf(f, "%u", &in.n) == 1;
  in.sigs = static_cast<g2a *>(std::malloc(in.n * sizeof(g2a) + !in.n));
  in.verdicts = static_cast<int32_t *>(std::malloc(in.n * 4 + !in.n));
  std::vector<char> line(2 * sizeof(g2a) + 1);
  for (uint32_t i = 0; ok && i < in.n; i++) {
    ok = std::fscanf(f, "%384s %d", line.data(), &in.verdicts[i]) == 2 && std::strlen(line.data()) == 2 * sizeof(g2a);
    unsigned char *b = reinterpret_cast<unsigned char *>(&in.sigs[i]);
    for (size_t k = 0; ok && k < sizeof(g2a); k++) {
      unsigned v = 0;
      ok = std::sscanf(&line[2 * k], "%2x", &v) == 1;
      b[k] = (unsigned char)v;
    }
  }
  ok = ok && std::fscanf(f, "%u", &in.ng) == 1;
  std::vector<uint32_t> set, off{0};
  for (uint32_t g = 0; ok && g < in.ng; g++) {
    uint32_t k = 0;
    ok = std::fscanf(f, "%u", &k) == 1;
    for (uint32_t j = 0; ok && j < k; j++) {
      uint32_t s = 0;
      ok = std::fscanf(f, "%u", &s) == 1;
      set.push_back(s);
    }
    off.push_back((uint32_t)set.size());
  }
  std::fclose(f);
  in.set = static_cast<uint32_t *>(std::malloc(set.size() * 4 + set.empty()));
  in.off = static_cast<uint32_t *>(std::malloc(off.size() * 4));
  if (!set.empty()) std::memcpy(in.set, set.data(), set.size() * 4);
  std::memcpy(in.off, off.data(), off.size() * 4);
  return ok;
}

static void run(const Input &in, const char *order, uint32_t lanes) {
  for (uint32_t g = 0; g < in.ng; g++) {
    std::vector<g2j> acc(lanes);
    std::vector<uint32_t> cnt(lanes);
    for (uint32_t r = 0; r < lanes; r++)
      fold_lane_sum(acc[r], cnt[r], in.sigs, in.verdicts, in.set, in.off[g], in.off[g + 1], r, lanes);
    if (lanes == 16) {  // the row fold: every lane adds the lane K above it, ascending K
      for (uint32_t K = 1; K < 16; K <<= 1) {
        std::vector<g2j> a2 = acc;
        std::vector<uint32_t> c2 = cnt;
        for (uint32_t r = 0; r < 16; r++) {
          g2j o;
          std::memset(&o, 0, sizeof o);  // past the row end: zeros, infinity
          if (r + K < 16) o = acc[r + K];
          jac_add(a2[r], a2[r], o);
          c2[r] += r + K < 16 ? cnt[r + K] : 0;
        }
        acc = a2, cnt = c2;
      }
    } else {  // the LDS tree
      for (uint32_t w = lanes / 2; w > 0; w >>= 1)
        for (uint32_t t = 0; t < w; t++) {
          g2j o = acc[t + w];
          jac_add(acc[t], acc[t], o);
          cnt[t] += cnt[t + w];
        }
    }
    g2a out;
    uint8_t bytes[96], none[96];
    uint32_t count = 0xffffffffu;
    std::memset(&out, 0xff, sizeof out), std::memset(bytes, 0xff, sizeof bytes), std::memset(none, 0xa5, sizeof none);
    fold_finish(acc[0], cnt[0], &out, bytes, &count);
    g2a out2;
    uint32_t count2 = 0;
    fold_finish(acc[0], cnt[0], &out2, nullptr, &count2);  // no bytes asked for: the same point and count
    CHECK(std::memcmp(&out, &out2, sizeof out) == 0 && count == count2);
    std::printf("%s %u %u ", order, g, count);
    hex(&out, sizeof out);
    std::printf(" ");
    hex(bytes, 96);
    std::printf("\n");
  }
}

static void test_args() {
  const uint32_t set[5] = {0, 1, 2, 1, 1}, off[4] = {0, 3, 3, 5};
  int out = 0, cnt = 0;
  CHECK(fold_args_ok(set, off, 3, 3, &out, &cnt));
  CHECK(fold_args_ok(nullptr, nullptr, 0, 3, nullptr, nullptr));  // no groups: nothing is required
  CHECK(fold_args_ok(nullptr, nullptr, 0, 0, nullptr, nullptr));
  CHECK(!fold_args_ok(set, nullptr, 3, 3, &out, &cnt));
  CHECK(!fold_args_ok(nullptr, off, 3, 3, &out, &cnt));
  CHECK(!fold_args_ok(set, off, 3, 3, nullptr, &cnt));
  CHECK(!fold_args_ok(set, off, 3, 3, &out, nullptr));
  CHECK(!fold_args_ok(set, off, 3, 2, &out, &cnt));               // an entry == n
  CHECK(!fold_args_ok(set, off, 3, 0, &out, &cnt));               // no sets at all, but entries
  const uint32_t one[4] = {1, 3, 3, 5}, down[4] = {0, 3, 2, 5}, empty[3] = {0, 0, 0};
  CHECK(!fold_args_ok(set, one, 3, 3, &out, &cnt));               // fold_off[0] != 0
  CHECK(!fold_args_ok(set, down, 3, 3, &out, &cnt));              // decreasing
  CHECK(fold_args_ok(set, empty, 2, 3, &out, &cnt));              // only empty groups
  CHECK(fold_args_ok(set, empty, 2, 0, &out, &cnt));              // ... of a call without sets
  CHECK(!fold_args_ok(nullptr, empty, 2, 3, &out, &cnt));         // fold_set NULL, even when no group names a set
  if (sizeof(size_t) > 4) {                                        // a group count past 32 bits (nothing is read)
    CHECK(!fold_args_ok(set, off, (size_t)1 << 32, 3, &out, &cnt));
    CHECK(!fold_args_ok(set, off, (size_t)0xffffffffu, 3, &out, &cnt));
  }
  const uint32_t big[1] = {0xffffffffu}, boff[2] = {0, 1};
  CHECK(!fold_args_ok(big, boff, 1, 0xffffffffu, &out, &cnt));
}

int main(int argc, char **argv) {
  test_args();
  if (argc > 1) {
    Input in;
    if (!read_input(argv[1], in)) {
      std::printf("FAILED: input\n");
      return 1;
    }
    CHECK(fold_args_ok(in.set, in.off, in.ng, in.n, in.sigs, in.verdicts));
    run(in, "rows", 16);
    run(in, "wg", 256);
  }
  if (fails) return 1;
  std::printf("fold_harness: OK\n");
  return 0;
}
