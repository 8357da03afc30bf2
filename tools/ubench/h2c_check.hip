// The map stage of hash_to_G2 and the Fp2 square root of point decoding on RAW field elements, on
// MI355X: `h2c_check IN OUT` reads a case file written by tools/ubench/h2c_vectors.py (an op code
// and the operands as engine-form limb images, 12 words per fp; nothing is converted) and runs
// every case twice: ONE CASE PER LANE with the lane policy (LanePow / LanePowCurve: fp_pow_pm3d4,
// work-groups of 64, as k_h2c_map and k_g2_decompress run it) and ONE CASE PER 16-LANE ROW with
// the row policy (RowPow of bls_dfp.h, the struct k_h2c_map_row and k_g2_decompress_row pass).
// It calls the functions the kernels call -- fp2_sqrt_pow (bls_curve.h), fp2_sqrt_norm_inv and
// map_to_g2 (bls_hash.h) -- and writes every result word.  It checks nothing itself beyond the
// HIP status: tests/test_gpu_h2c_map.py recomputes every result with Python integers.
// `h2c_check --host IN OUT` runs the lane policy through the headers' host branches on the CPU
// (tests/test_h2c_vectors.py): the same file layout, the row half of OUT left at its fill.
// Build: make -C tools/ubench
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../grandine_amd/csrc/gbls_common.h"
#include "../../grandine_amd/csrc/bls_dfp.h"

using namespace gbls;

// op codes (h2c_vectors.py OPS)
enum : uint32_t {
  SQRT_POW = 0,       // a                -> flag, r               (1 + 24 words)
  SQRT_NORM_INV = 1,  // a, gamma, nd     -> r, ndinv              (24 + 12 words)
  MAP_TO_G2 = 2,      // u                -> the Jacobian point    (72 words)
  OP_COUNT = 3
};
constexpr int FP = 12;
constexpr int IN_WORDS = 4 + 4 * FP;  // op, 3 spare words, a.c0 a.c1 gamma nd
constexpr int OUT_WORDS = 72;
constexpr int LANES = 64;
constexpr uint32_t FILL = 0xeeeeeeeeu;

template <class T>
HD void ldw(T &r, const uint32_t *s) {
  uint32_t *w = reinterpret_cast<uint32_t *>(&r);
#pragma unroll
  for (int i = 0; i < (int)(sizeof(T) / 4); i++) w[i] = s[i];
}
template <class T>
HD void stw(uint32_t *d, const T &a) {
  const uint32_t *w = reinterpret_cast<const uint32_t *>(&a);
#pragma unroll
  for (int i = 0; i < (int)(sizeof(T) / 4); i++) d[i] = w[i];
}
static_assert(sizeof(fp) == 4 * FP && sizeof(fp2) == 8 * FP && sizeof(g2j) == 4 * OUT_WORDS, "raw word layout");

// one case with the exponentiation policy the caller's kernel form uses
template <class Pow>
HD void run_case(const uint32_t *rec, uint32_t *o, const Pow &pow) {
  const uint32_t *a = rec + 4;
  switch (rec[0]) {
    case SQRT_POW: {
      fp2 x, r;
      ldw(x, a);
      fp2_zero(r);  // a non-square leaves r undefined in the header; the words are then not compared
      const bool ok = fp2_sqrt_pow(r, x, pow);
      o[0] = ok ? 1u : 0u;
      stw(o + 1, r);
      break;
    }
    case SQRT_NORM_INV: {
      fp2 x, r;
      fp gamma, nd, ndinv;
      ldw(x, a);
      ldw(gamma, a + 2 * FP);
      ldw(nd, a + 3 * FP);
      fp2_sqrt_norm_inv(r, ndinv, x, gamma, nd, pow);
      stw(o, r);
      stw(o + 2 * FP, ndinv);
      break;
    }
    case MAP_TO_G2: {
      fp2 u;
      ldw(u, a);
      g2j q;
      map_to_g2(q, u, pow);
      stw(o, q);
      break;
    }
    default: break;
  }
}

__global__ void __launch_bounds__(LANES) k_h2c_lane(const uint32_t *in, uint32_t n, uint32_t *out) {
  const uint32_t i = blockIdx.x * LANES + threadIdx.x;
  if (i >= n) return;
  // the decoder's policy for its square root, the map's for the rest: the same fp_pow_pm3d4
  if (in[(size_t)IN_WORDS * i] == SQRT_POW)
    run_case(in + (size_t)IN_WORDS * i, out + (size_t)OUT_WORDS * i, LanePowCurve());
  else
    run_case(in + (size_t)IN_WORDS * i, out + (size_t)OUT_WORDS * i, LanePow());
}
__global__ void __launch_bounds__(LANES) k_h2c_row(const uint32_t *in, uint32_t n, uint32_t *out) {
  const uint32_t i = (blockIdx.x * LANES + threadIdx.x) >> 4;
  if (i >= n) return;  // whole rows
  uint32_t o[OUT_WORDS];
#pragma unroll
  for (int k = 0; k < OUT_WORDS; k++) o[k] = FILL;
  run_case(in + (size_t)IN_WORDS * i, o, RowPow());
  if ((threadIdx.x & 15) == 0) {
#pragma unroll
    for (int k = 0; k < OUT_WORDS; k++) out[(size_t)OUT_WORDS * i + k] = o[k];
  }
}

#define HIP_OK(call)                                               \
  do {                                                             \
    const hipError_t err_ = (call);                                \
    if (err_ != hipSuccess) {                                      \
      fprintf(stderr, "%s: %s\n", #call, hipGetErrorString(err_)); \
      return 2;                                                    \
    }                                                              \
  } while (0)

int main(int argc, char **argv) {
  const bool host = argc == 4 && !strcmp(argv[1], "--host");
  if (argc != 3 && !host) {
    fprintf(stderr, "usage: h2c_check [--host] IN OUT\n");
    return 1;
  }
  FILE *f = fopen(argv[argc - 2], "rb");
  if (!f) return 1;
  uint32_t n = 0;
  if (fread(&n, 4, 1, f) != 1 || n == 0 || n > (1u << 16)) return 1;
  std::vector<uint32_t> in((size_t)n * IN_WORDS);
  if (fread(in.data(), 4, in.size(), f) != in.size()) return 1;
  fclose(f);
  for (uint32_t i = 0; i < n; i++)
    if (in[(size_t)i * IN_WORDS] >= OP_COUNT) {
      fprintf(stderr, "case %u: unknown op %u\n", i, in[(size_t)i * IN_WORDS]);
      return 1;
    }
  // OUT: the lane policy's n x OUT_WORDS result words, then the row policy's
  const size_t half = (size_t)n * OUT_WORDS;
  std::vector<uint32_t> o(2 * half, FILL);
  if (host) {
    for (uint32_t i = 0; i < n; i++) {
      const uint32_t *rec = &in[(size_t)i * IN_WORDS];
      if (rec[0] == SQRT_POW)
        run_case(rec, &o[(size_t)i * OUT_WORDS], LanePowCurve());
      else
        run_case(rec, &o[(size_t)i * OUT_WORDS], LanePow());
    }
  } else {
    uint32_t *din, *dout;
    HIP_OK(hipMalloc(&din, in.size() * 4));
    HIP_OK(hipMalloc(&dout, 2 * half * 4));
    HIP_OK(hipMemcpy(din, in.data(), in.size() * 4, hipMemcpyHostToDevice));
    HIP_OK(hipMemset(dout, 0xee, 2 * half * 4));
    k_h2c_lane<<<(n + LANES - 1) / LANES, LANES>>>(din, n, dout);
    HIP_OK(hipGetLastError());
    k_h2c_row<<<(16 * n + LANES - 1) / LANES, LANES>>>(din, n, dout + half);
    HIP_OK(hipGetLastError());
    HIP_OK(hipDeviceSynchronize());
    HIP_OK(hipMemcpy(o.data(), dout, 2 * half * 4, hipMemcpyDeviceToHost));
  }
  f = fopen(argv[argc - 1], "wb");
  if (!f) return 1;
  if (fwrite(o.data(), 4, o.size(), f) != o.size()) return 1;
  if (fclose(f) != 0) return 1;
  printf("h2c_check: %u cases%s, %zu result words\n", n, host ? " (host, lane policy)" : " x 2 policies", o.size());
  return 0;
}
