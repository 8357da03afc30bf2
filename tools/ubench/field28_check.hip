// bls_field28.h function by function on MI355X: `field28_check IN OUT` reads a case file written
// by tools/ubench/field28_vectors.py (an op code, an aux word and the operands as RAW limb images:
// 14 words per r28::fe, 12 per engine-form fp; nothing is converted), runs ONE CASE PER LANE in
// work-groups of 64 (fp_pow_pm3d4's LDS table is laid out for 64 lanes) and writes every result
// word.  It calls the public r28:: functions, so on the GPU the device branch runs: the generated
// v_mad_u64_u32 products of bls_fpmul28_gen.h, and fe2_mul3k's Karatsuba form, which has no host
// counterpart.  The _st forms park their words in LDS at st + threadIdx.x with stride 64, as
// k_ml_group28 does.  It checks nothing itself beyond the HIP status: tests/test_gpu_field28.py
// recomputes every result with Python integers.
// `field28_check --host IN OUT` runs the same cases through the header's host branches (the
// plain-C mul_n) on the CPU, for tests/test_field28_vectors.py: the same file layout, and the
// same words wherever the result is a single product; fe2_mul3k then returns the schoolbook
// representative (equal mod p only).
// Build: make -C tools/ubench
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../grandine_amd/csrc/gbls_common.h"
#include "../../grandine_amd/csrc/bls_field.h"

using namespace gbls;

// op codes (field28_vectors.py OP_LIST)
enum : uint32_t {
  MUL = 0,        // r = a b, r fresh
  MUL_RA = 1,     // a = a b
  MUL_RB = 2,     // b = a b
  MUL_AA = 3,     // r = a a (a == b by reference)
  SQR = 4,        // r = a^2, r fresh
  SQR_RA = 5,     // a = a^2 (fp_pow_pm3d4)
  MUL2 = 6,       // r = a b + c d, r fresh
  MUL2_RC = 7,    // c = a b + c d (fe2_mul with r aliasing a)
  MUL4 = 8,
  MUL6 = 9,
  MUL3K = 10,     // fe2_mul3k, the u sums formed with fe2_sum
  FE2_MUL = 11,
  FE2_MUL_RA = 12,
  FE2_SQR = 13,
  FE2_MUL_FE = 14,
  SP_FROM_ENGINE = 15,
  SP_MUL_SP_LAZY = 16,
  SP_MUL_SP = 17,
  M034 = 18,      // the five forms of f * line: aux of a chain is form - M034
  M034_ST = 19,
  M034_LAZY = 20,
  M034_LAZY_ST = 21,
  M034_KARA_ST = 22,
  TO_ENGINE_SCALED = 23,
  FROM_FP = 24,
  TO_FP = 25,
  POW_PM3D4 = 26,
  CHAIN = 27,     // sp_mul_sp_lazy, then CHAIN_STEPS dense x sparse steps; every accumulator
  OP_COUNT = 28
};
constexpr int IN_WORDS = 4 + 252;
constexpr int FE = 14, FE2 = 28, SP = 84, FE12 = 168, FP = 12;
constexpr int CHAIN_STEPS = 30;
constexpr int STASH_WORDS = 154;  // fe12_mul_034_st: 84 + 70 words per lane
constexpr int LANES = 64;

static size_t out_words(uint32_t op) {
  switch (op) {
    case MUL: case MUL_RA: case MUL_RB: case MUL_AA: case SQR: case SQR_RA: case MUL2: case MUL2_RC:
    case MUL4: case MUL6: case FROM_FP: return FE;
    case MUL3K: case FE2_MUL: case FE2_MUL_RA: case FE2_SQR: case FE2_MUL_FE: return FE2;
    case SP_FROM_ENGINE: return SP;
    case SP_MUL_SP_LAZY: case SP_MUL_SP: case M034: case M034_ST: case M034_LAZY: case M034_LAZY_ST:
    case M034_KARA_ST: return FE12;
    case TO_ENGINE_SCALED: return 12 * FP;
    case TO_FP: case POW_PM3D4: return FP;
    case CHAIN: return (size_t)(CHAIN_STEPS + 1) * FE12;
    default: return 0;
  }
}

// raw words <-> the header's structs (plain arrays of limbs, as the header itself reads them)
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
static_assert(sizeof(r28::fe) == 4 * FE && sizeof(r28::fe2) == 4 * FE2 && sizeof(r28::sp) == 4 * SP &&
                  sizeof(r28::fe12) == 4 * FE12 && sizeof(fp) == 4 * FP && sizeof(fp12) == 4 * 12 * FP,
              "raw word layout");

HD void dense_step(uint32_t form, r28::fe12 &acc, const r28::sp &s, uint32_t *st, uint32_t stride) {
  switch (form) {
    case 0: {
      r28::fe12 r;
      r28::fe12_mul_034(r, acc, s);
      acc = r;
      break;
    }
    case 1: {
      r28::fe12 r;
      r28::fe12_mul_034_st(r, acc, s, st, stride);
      acc = r;
      break;
    }
    case 2: r28::fe12_mul_034_lazy(acc, s); break;
    case 3: r28::fe12_mul_034_lazy_st(acc, s, st, stride); break;
    default: r28::fe12_mul_034_kara_st(acc, s, st, stride); break;
  }
}

// one case: rec = the record, o = its out_words(op) result words, st / stride = its stash
HD void run_case(const uint32_t *rec, uint32_t *o, uint32_t *st, uint32_t stride) {
  const uint32_t op = rec[0];
  const uint32_t *a = rec + 4;
  switch (op) {
    case MUL: case MUL_RA: case MUL_RB: case MUL_AA: {
      r28::fe x, y, r;
      ldw(x, a);
      ldw(y, a + FE);
      if (op == MUL) {
        r28::mul(r, x, y);
      } else if (op == MUL_RA) {
        r28::mul(x, x, y);
        r = x;
      } else if (op == MUL_RB) {
        r28::mul(y, x, y);
        r = y;
      } else {
        r28::mul(r, x, x);
      }
      stw(o, r);
      break;
    }
    case SQR: case SQR_RA: {
      r28::fe x, r;
      ldw(x, a);
      if (op == SQR) {
        r28::sqr(r, x);
      } else {
        r28::sqr(x, x);
        r = x;
      }
      stw(o, r);
      break;
    }
    case MUL2: case MUL2_RC: {
      r28::fe x, y, z, t, r;
      ldw(x, a);
      ldw(y, a + FE);
      ldw(z, a + 2 * FE);
      ldw(t, a + 3 * FE);
      if (op == MUL2) {
        r28::mul2(r, x, y, z, t);
      } else {
        r28::mul2(z, x, y, z, t);
        r = z;
      }
      stw(o, r);
      break;
    }
    case MUL4: {
      r28::fe v[8], r;
#pragma unroll
      for (int i = 0; i < 8; i++) ldw(v[i], a + FE * i);
      r28::mul4(r, v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7]);
      stw(o, r);
      break;
    }
    case MUL6: {
      r28::fe v[12], r;
#pragma unroll
      for (int i = 0; i < 12; i++) ldw(v[i], a + FE * i);
      r28::mul6(r, v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7], v[8], v[9], v[10], v[11]);
      stw(o, r);
      break;
    }
    case MUL3K: {  // x0 u0 x1 u1 x2 u2 (fe2 each); the sums as fe12_mul_034_kara_st forms them
      r28::fe2 x0, u0, x1, u1, x2, u2, r;
      ldw(x0, a);
      ldw(u0, a + FE2);
      ldw(x1, a + 2 * FE2);
      ldw(u1, a + 3 * FE2);
      ldw(x2, a + 4 * FE2);
      ldw(u2, a + 5 * FE2);
      r28::fe s0, s1, s2;
      r28::fe2_sum(s0, u0);
      r28::fe2_sum(s1, u1);
      r28::fe2_sum(s2, u2);
      r28::fe2_mul3k(r, x0, u0, s0, x1, u1, s1, x2, u2, s2);
      stw(o, r);
      break;
    }
    case FE2_MUL: case FE2_MUL_RA: {
      r28::fe2 x, y, r;
      ldw(x, a);
      ldw(y, a + FE2);
      if (op == FE2_MUL) {
        r28::fe2_mul(r, x, y);
      } else {
        r28::fe2_mul(x, x, y);
        r = x;
      }
      stw(o, r);
      break;
    }
    case FE2_SQR: {
      r28::fe2 x, r;
      ldw(x, a);
      r28::fe2_sqr(r, x);
      stw(o, r);
      break;
    }
    case FE2_MUL_FE: {
      r28::fe2 x, r;
      r28::fe y;
      ldw(x, a);
      ldw(y, a + FE2);
      r28::fe2_mul_fe(r, x, y);
      stw(o, r);
      break;
    }
    case SP_FROM_ENGINE: {  // L0 L2 L3 (fp2), Px Py Pc (fp)
      fp2 L0, L2, L3;
      fp Px, Py, Pc;
      ldw(L0, a);
      ldw(L2, a + 2 * FP);
      ldw(L3, a + 4 * FP);
      ldw(Px, a + 6 * FP);
      ldw(Py, a + 7 * FP);
      ldw(Pc, a + 8 * FP);
      r28::sp s;
      r28::sp_from_engine(s, L0, L2, L3, Px, Py, Pc);
      stw(o, s);
      break;
    }
    case SP_MUL_SP_LAZY: case SP_MUL_SP: {
      r28::sp x, y;
      ldw(x, a);
      ldw(y, a + SP);
      r28::fe12 r;
      if (op == SP_MUL_SP_LAZY)
        r28::sp_mul_sp_lazy(r, x, y);
      else
        r28::sp_mul_sp(r, x, y);
      stw(o, r);
      break;
    }
    case M034: case M034_ST: case M034_LAZY: case M034_LAZY_ST: case M034_KARA_ST: case CHAIN: {
      // a chain is the inner loop of k_ml_group28 in miniature on the lines s0 s1 s2: acc = s0 s1,
      // then step j multiplies by s[(j + 2) % 3]; a single product is one step on a given f
      r28::fe12 acc;
      uint32_t form, steps;
      const uint32_t *lines;
      uint32_t *d = o;
      if (op == CHAIN) {
        r28::sp x, y;
        ldw(x, a);
        ldw(y, a + SP);
        r28::sp_mul_sp_lazy(acc, x, y);
        stw(d, acc);
        d += FE12;
        form = rec[1];
        steps = CHAIN_STEPS;
        lines = a;
      } else {
        ldw(acc, a);
        form = op - M034;
        steps = 1;
        lines = a;  // step 0 reads line (0 + 2) % 3: the 84 words after the 168 of f
      }
      for (uint32_t j = 0; j < steps; j++) {
        r28::sp s;
        ldw(s, lines + SP * ((j + 2) % 3));
        dense_step(form, acc, s, st, stride);
        stw(d, acc);
        d += FE12;
      }
      break;
    }
    case TO_ENGINE_SCALED: {
      r28::fe12 x;
      ldw(x, a);
      fp12 r;
      r28::fe12_to_engine_scaled(r, x);
      stw(o, r);
      break;
    }
    case FROM_FP: {
      fp x;
      ldw(x, a);
      r28::fe r;
      r28::from_fp(r, x);
      stw(o, r);
      break;
    }
    case TO_FP: {
      r28::fe x;
      ldw(x, a);
      fp r;
      r28::to_fp(r, x);
      stw(o, r);
      break;
    }
    case POW_PM3D4: {
      fp x, r;
      ldw(x, a);
      fp_pow_pm3d4(r, x);
      stw(o, r);
      break;
    }
    default: break;
  }
}

__global__ void __launch_bounds__(LANES) k_field28(const uint32_t *in, const uint64_t *off, uint32_t n, uint32_t *out) {
  __shared__ uint32_t park[STASH_WORDS * LANES];
  const uint32_t i = blockIdx.x * LANES + threadIdx.x;
  if (i >= n) return;  // no barrier anywhere below
  run_case(in + (size_t)IN_WORDS * i, out + off[i], park + threadIdx.x, LANES);
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
    fprintf(stderr, "usage: field28_check [--host] IN OUT\n");
    return 1;
  }
  FILE *f = fopen(argv[argc - 2], "rb");
  if (!f) return 1;
  uint32_t n = 0;
  if (fread(&n, 4, 1, f) != 1 || n == 0 || n > (1u << 16)) return 1;
  std::vector<uint32_t> in((size_t)n * IN_WORDS);
  if (fread(in.data(), 4, in.size(), f) != in.size()) return 1;
  fclose(f);
  std::vector<uint64_t> off(n);
  size_t total = 0;
  for (uint32_t i = 0; i < n; i++) {
    const uint32_t *rec = &in[(size_t)i * IN_WORDS];
    if (rec[0] >= OP_COUNT || (rec[0] == CHAIN ? rec[1] > M034_KARA_ST - M034 : rec[1] != 0)) {
      fprintf(stderr, "case %u: unknown op %u / aux %u\n", i, rec[0], rec[1]);
      return 1;
    }
    off[i] = total;
    total += out_words(rec[0]);
  }
  std::vector<uint32_t> o(total, 0xeeeeeeeeu);
  if (host) {
    std::vector<uint32_t> stash(STASH_WORDS);
    for (uint32_t i = 0; i < n; i++) run_case(&in[(size_t)i * IN_WORDS], &o[off[i]], stash.data(), 1);
  } else {
    uint32_t *din, *dout;
    uint64_t *doff;
    HIP_OK(hipMalloc(&din, in.size() * 4));
    HIP_OK(hipMalloc(&doff, off.size() * 8));
    HIP_OK(hipMalloc(&dout, total * 4));
    HIP_OK(hipMemcpy(din, in.data(), in.size() * 4, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(doff, off.data(), off.size() * 8, hipMemcpyHostToDevice));
    HIP_OK(hipMemset(dout, 0xee, total * 4));
    k_field28<<<(n + LANES - 1) / LANES, LANES>>>(din, doff, n, dout);
    HIP_OK(hipGetLastError());
    HIP_OK(hipDeviceSynchronize());
    HIP_OK(hipMemcpy(o.data(), dout, total * 4, hipMemcpyDeviceToHost));
  }
  f = fopen(argv[argc - 1], "wb");
  if (!f) return 1;
  if (fwrite(o.data(), 4, total, f) != total) return 1;
  if (fclose(f) != 0) return 1;
  printf("field28_check: %u cases%s, %zu result words\n", n, host ? " (host)" : "", total);
  return 0;
}
