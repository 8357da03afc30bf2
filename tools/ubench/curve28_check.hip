// bls_curve28.h function by function on MI355X: `curve28_check IN OUT` reads a case file written
// by tools/ubench/curve28_vectors.py (an op code, a 64-bit scalar and the operands as RAW limb
// images: 14 words per r28::fe, 12 per engine-form fp; nothing is converted), runs ONE CASE PER
// LANE in work-groups of 64 and writes every result word.  It calls the header's own functions in
// the forms the kernels call them (fresh and aliased outputs where the header allows aliasing), so
// on the GPU the device branch runs: the generated v_mad_u64_u32 products of bls_fpmul28_gen.h
// under the point routines' register pressure.  The ops are spread over a few kernels, each of
// which runs its own ops' lanes and retires the others at once:
//   k_point       the point formulas, maps, conversions, single line steps and g1h28
//   k_line_chain  the 68 line events from an affine Q, Q's coordinates in LDS as k_lines_lane28
//   k_xabs_lds    g2_xabs_aff28 with k_h2c_chain28's attributes (two waves per SIMD), the affine
//                 base parked in LDS at the odd stride of 57 words
//   k_xabs_reg    the same chain with the base in registers (second half of the op's result)
//   k_in_group    g2_in_group28 with the base in LDS, as k_g2_check28
//   k_clear       clear_mid28, clear_post28, clear_cofactor28_staged, clear_cofactor28
//   k_g1mul       g1_mul_u64_w3_28 followed by g1s_from_jac28
// It checks nothing itself beyond the HIP status: tests/test_gpu_curve28.py recomputes every
// result with Python integers.  `curve28_check --host IN OUT` runs the same cases through the
// headers' host branches on the CPU (tests/test_curve28_vectors.py): the same file layout and,
// the host and device products returning the same integers, the same words.
// Build: make -C tools/ubench
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../grandine_amd/csrc/gbls_common.h"
#include "../../grandine_amd/csrc/bls_curve28.h"

using namespace gbls;

// op codes (curve28_vectors.py OP_LIST)
enum : uint32_t {
  G2_DBL = 0,     // jac_dbl28, r fresh
  G2_DBL_RP,      // r = p
  G2_ADD,         // jac_add28, r fresh
  G2_ADD_RA,      // r = a
  G2_MADD_T,      // jac_add_aff28<true>, r fresh
  G2_MADD_T_RA,   // r = a
  G2_MADD_F,      // jac_add_aff28<false>, r fresh
  G2_MADD_F_RA,   // r = a
  G2_NEG,
  G2_EQ,
  G1_DBL,
  G1_DBL_RP,
  G1_ADD,
  G1_ADD_RA,
  G1_NEG,
  G1_EQ,
  PSI,
  PSI2,
  OF_AFF,         // g2j_of_aff28
  TO_AFF,         // jac_to_aff28
  FE2_INV,
  INV,
  HALF,
  FE2_HALF,
  MUL_3B,
  STORE12,
  LOAD12,
  G2J_RT,         // g2j_store12 then g2j_load12: the engine-layout words, then the point again
  G2A_RT,
  G2J_IN,
  G2J_OUT,
  LINE_DBL,       // L0 L2 L3, then T
  LINE_ADD,
  G1H_LOAD,
  G1H_ADD,        // r fresh
  G1H_ADD_RA,
  G1H_ADD_RB,
  G1H_STORE,
  LINE_CHAIN,     // 68 x (L0 L2 L3), then T
  XABS,           // g2_xabs_aff28: base in LDS, then base in registers
  IN_GROUP,
  CLEAR_MID,      // t2a, then T
  CLEAR_POST,
  CLEAR_STAGED,
  CLEAR_FULL,
  G1MUL,
  OP_COUNT
};
constexpr int FE = 14, FE2 = 28, FP = 12;
constexpr int G2J = 3 * FE2, G2A = 2 * FE2, G1J = 3 * FE, G1S = 3 * FP;
constexpr int IN_WORDS = 4 + 2 * G2J;
constexpr int LANES = 64;
constexpr int EVENTS = 68;

static size_t out_words(uint32_t op) {
  switch (op) {
    case G2_DBL: case G2_DBL_RP: case G2_ADD: case G2_ADD_RA: case G2_MADD_T: case G2_MADD_T_RA:
    case G2_MADD_F: case G2_MADD_F_RA: case G2_NEG: case PSI: case PSI2: case OF_AFF: case G2J_IN:
    case CLEAR_POST: case CLEAR_STAGED: case CLEAR_FULL: return G2J;
    case G2_EQ: case G1_EQ: case IN_GROUP: return 1;
    case G1_DBL: case G1_DBL_RP: case G1_ADD: case G1_ADD_RA: case G1_NEG: case G1H_LOAD: case G1H_ADD:
    case G1H_ADD_RA: case G1H_ADD_RB: return G1J;
    case TO_AFF: return G2A;
    case FE2_INV: case FE2_HALF: case MUL_3B: return FE2;
    case INV: case HALF: case LOAD12: return FE;
    case STORE12: return FP;
    case G2J_RT: return 6 * FP + G2J;
    case G2A_RT: return 4 * FP + G2A;
    case G2J_OUT: return 6 * FP;
    case LINE_DBL: case LINE_ADD: return 2 * G2J;
    case G1H_STORE: case G1MUL: return G1S;
    case LINE_CHAIN: return (size_t)(EVENTS + 1) * G2J;
    case XABS: return 2 * G2J;
    case CLEAR_MID: return G2A + G2J;
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
static_assert(sizeof(r28::fe) == 4 * FE && sizeof(r28::fe2) == 4 * FE2 && sizeof(r28::g2j28) == 4 * G2J &&
                  sizeof(r28::g2a28) == 4 * G2A && sizeof(r28::g1j28) == 4 * G1J && sizeof(r28::g2h28) == 4 * G2J &&
                  sizeof(r28::g1h28) == 4 * G1J && sizeof(g1s) == 4 * G1S && sizeof(g2j) == 24 * FP &&
                  sizeof(g2a) == 16 * FP && sizeof(g1a) == 8 * FP,
              "raw word layout");

// Jacobian ops over either coordinate field
template <class F, int FORM>
HD void run_jac(const uint32_t *a, uint32_t *o) {
  jac<F> p, q, r;
  ldw(p, a);
  ldw(q, a + sizeof(jac<F>) / 4);
  switch (FORM) {
    case 0:
      r28::jac_dbl28(r, p);
      break;
    case 1:
      r28::jac_dbl28(p, p);
      r = p;
      break;
    case 2:
      r28::jac_add28(r, p, q);
      break;
    case 3:
      r28::jac_add28(p, p, q);
      r = p;
      break;
    case 4:
      jac_neg(r, p);
      break;
    default:
      o[0] = jac_eq(p, q) ? 1u : 0u;
      return;
  }
  stw(o, r);
}

// One op of k_point.  The op is a template parameter so that the host mode can compile every op
// as a function of its own (the headers force every call inline: one function holding all ops
// takes the host compiler many minutes); the kernel dispatches on the record's op word.
template <uint32_t op>
HD void run_point(const uint32_t *rec, uint32_t *o) {
  const uint32_t *a = rec + 4;
  switch (op) {
    case G2_DBL: case G2_DBL_RP: case G2_ADD: case G2_ADD_RA: run_jac<r28::fe2, (int)op - (int)G2_DBL>(a, o); break;
    case G2_NEG: run_jac<r28::fe2, 4>(a, o); break;
    case G2_EQ: run_jac<r28::fe2, 5>(a, o); break;
    case G1_DBL: case G1_DBL_RP: case G1_ADD: case G1_ADD_RA: run_jac<r28::fe, (int)op - (int)G1_DBL>(a, o); break;
    case G1_NEG: run_jac<r28::fe, 4>(a, o); break;
    case G1_EQ: run_jac<r28::fe, 5>(a, o); break;
    case G2_MADD_T: case G2_MADD_T_RA: case G2_MADD_F: case G2_MADD_F_RA: {
      r28::g2j28 p, r;
      r28::g2a28 q;
      ldw(p, a);
      ldw(q, a + G2J);
      if (op == G2_MADD_T) {
        r28::jac_add_aff28<true>(r, p, q);
      } else if (op == G2_MADD_T_RA) {
        r28::jac_add_aff28<true>(p, p, q);
        r = p;
      } else if (op == G2_MADD_F) {
        r28::jac_add_aff28<false>(r, p, q);
      } else {
        r28::jac_add_aff28<false>(p, p, q);
        r = p;
      }
      stw(o, r);
      break;
    }
    case PSI: case PSI2: {
      r28::g2j28 p, r;
      ldw(p, a);
      if (op == PSI)
        r28::g2_psi28(r, p);
      else
        r28::g2_psi2_28(r, p);
      stw(o, r);
      break;
    }
    case OF_AFF: {
      r28::g2a28 q;
      r28::g2j28 r;
      ldw(q, a);
      r28::g2j_of_aff28(r, q);
      stw(o, r);
      break;
    }
    case TO_AFF: {
      r28::g2j28 p;
      r28::g2a28 r;
      ldw(p, a);
      r28::jac_to_aff28(r, p);
      stw(o, r);
      break;
    }
    case FE2_INV: case FE2_HALF: case MUL_3B: {
      r28::fe2 x, r;
      ldw(x, a);
      if (op == FE2_INV)
        r28::fe2_inv(r, x);
      else if (op == FE2_HALF)
        r28::fe2_half(r, x);
      else
        r28::fe2_mul_3b(r, x);
      stw(o, r);
      break;
    }
    case INV: case HALF: {
      r28::fe x, r;
      ldw(x, a);
      if (op == INV)
        r28::inv(r, x);
      else
        r28::half(r, x);
      stw(o, r);
      break;
    }
    case STORE12: {
      r28::fe x;
      fp r;
      ldw(x, a);
      r28::store12(r, x);
      stw(o, r);
      break;
    }
    case LOAD12: {
      fp x;
      r28::fe r;
      ldw(x, a);
      r28::load12(r, x);
      stw(o, r);
      break;
    }
    case G2J_RT: {
      r28::g2j28 p, r;
      g2j s;
      ldw(p, a);
      r28::g2j_store12(s, p);
      r28::g2j_load12(r, s);
      stw(o, s);
      stw(o + 6 * FP, r);
      break;
    }
    case G2A_RT: {
      r28::g2a28 p, r;
      g2a s;
      ldw(p, a);
      r28::g2a_store12(s, p);
      r28::g2a_load12(r, s);
      stw(o, s);
      stw(o + 4 * FP, r);
      break;
    }
    case G2J_IN: {
      g2j p;
      r28::g2j28 r;
      ldw(p, a);
      r28::g2j_in(r, p);
      stw(o, r);
      break;
    }
    case G2J_OUT: {
      r28::g2j28 p;
      g2j r;
      ldw(p, a);
      r28::g2j_out(r, p);
      stw(o, r);
      break;
    }
    case LINE_DBL: case LINE_ADD: {  // T, then the affine Q
      r28::g2h28 T;
      r28::fe2 qx, qy;
      ldw(T, a);
      ldw(qx, a + G2J);
      ldw(qy, a + G2J + FE2);
      auto put = [&](int c, const r28::fe2 &v) { stw(o + (c >> 1) * FE2, v); };
      if (op == LINE_DBL)
        r28::line_dbl28(T, put);
      else
        r28::line_add28(T, qx, qy, put);
      stw(o + G2J, T);
      break;
    }
    case G1H_LOAD: {
      g1s p;
      r28::g1h28 r;
      ldw(p, a);
      r28::g1h28_load(r, p);
      stw(o, r);
      break;
    }
    case G1H_ADD: case G1H_ADD_RA: case G1H_ADD_RB: {
      r28::g1h28 p, q, r;
      ldw(p, a);
      ldw(q, a + G1J);
      if (op == G1H_ADD) {
        r28::g1h28_add(r, p, q);
      } else if (op == G1H_ADD_RA) {
        r28::g1h28_add(p, p, q);
        r = p;
      } else {
        r28::g1h28_add(q, p, q);
        r = q;
      }
      stw(o, r);
      break;
    }
    case G1H_STORE: {
      r28::g1h28 p;
      g1s r;
      ldw(p, a);
      r28::g1h28_store(r, p);
      stw(o, r);
      break;
    }
    default: break;
  }
}

// the 68 events of the Miller loop from an affine Q (k_lines_lane28: T = (qx, qy, 1), a doubling
// per bit of |x| below the top and an addition where the bit is set); qx, qy are the caller's
HD void run_line_chain(uint32_t *o, const r28::fe2 &qx, const r28::fe2 &qy) {
  r28::g2h28 T;
  T.x = qx;
  T.y = qy;
  r28::f_one(T.z);
  for (int e = 0; e < EVENTS; e++) {
    uint32_t *d = o + (size_t)e * G2J;
    auto put = [&](int c, const r28::fe2 &v) { stw(d + (c >> 1) * FE2, v); };
    if (ev_is_dbl(e))
      r28::line_dbl28(T, put);
    else
      r28::line_add28(T, qx, qy, put);
  }
  stw(o + (size_t)EVENTS * G2J, T);
}

template <uint32_t op>
HD void run_clear(const uint32_t *rec, uint32_t *o) {
  const uint32_t *a = rec + 4;
  switch (op) {
    case CLEAR_MID: {  // pa, x1
      r28::g2a28 pa, t2a;
      r28::g2j28 x1, T;
      ldw(pa, a);
      ldw(x1, a + G2A);
      r28::clear_mid28(t2a, T, pa, x1);
      stw(o, t2a);
      stw(o + G2A, T);
      break;
    }
    case CLEAR_POST: {  // x2, T
      r28::g2j28 x2, T, h;
      ldw(x2, a);
      ldw(T, a + G2J);
      r28::clear_post28(h, x2, T);
      stw(o, h);
      break;
    }
    case CLEAR_STAGED: case CLEAR_FULL: {
      r28::g2j28 p, r;
      ldw(p, a);
      if (op == CLEAR_STAGED)
        r28::clear_cofactor28_staged(r, p);
      else
        r28::clear_cofactor28(r, p);
      stw(o, r);
      break;
    }
    default: break;
  }
}

HD void run_g1mul(const uint32_t *rec, uint32_t *o) {  // base (engine form, affine), the scalar in words 2, 3
  g1a base;
  ldw(base, rec + 4);
  const uint64_t k = (uint64_t)rec[2] | ((uint64_t)rec[3] << 32);
  r28::g1j28 t;
  r28::g1_mul_u64_w3_28(t, base, k);
  g1s r;
  r28::g1s_from_jac28(r, t);
  stw(o, r);
}

struct g2a28_lds {
  r28::g2a28 v;
  uint32_t pad;
};
static_assert(sizeof(g2a28_lds) == 57 * 4, "odd LDS stride");
struct fe2_lds {
  r28::fe2 v;
  uint32_t pad;
};
static_assert(sizeof(fe2_lds) == 29 * 4, "odd LDS stride");

// no barrier in any kernel: lanes of other ops and lanes past n return at once
#define CASE_OF(cond)                                          \
  const uint32_t i = blockIdx.x * LANES + threadIdx.x;         \
  if (i >= n) return;                                          \
  const uint32_t *rec = in + (size_t)IN_WORDS * i;             \
  const uint32_t op = rec[0];                                  \
  if (!(cond)) return;                                         \
  uint32_t *o = out + off[i]

#define POINT_OPS(X)                                                                                       \
  X(G2_DBL) X(G2_DBL_RP) X(G2_ADD) X(G2_ADD_RA) X(G2_MADD_T) X(G2_MADD_T_RA) X(G2_MADD_F) X(G2_MADD_F_RA)  \
  X(G2_NEG) X(G2_EQ) X(G1_DBL) X(G1_DBL_RP) X(G1_ADD) X(G1_ADD_RA) X(G1_NEG) X(G1_EQ) X(PSI) X(PSI2)     \
  X(OF_AFF) X(TO_AFF) X(FE2_INV) X(INV) X(HALF) X(FE2_HALF) X(MUL_3B) X(STORE12) X(LOAD12) X(G2J_RT)      \
  X(G2A_RT) X(G2J_IN) X(G2J_OUT) X(LINE_DBL) X(LINE_ADD) X(G1H_LOAD) X(G1H_ADD) X(G1H_ADD_RA)             \
  X(G1H_ADD_RB) X(G1H_STORE)
#define CLEAR_OPS(X) X(CLEAR_MID) X(CLEAR_POST) X(CLEAR_STAGED) X(CLEAR_FULL)

__global__ void __launch_bounds__(LANES) k_point(const uint32_t *in, const uint64_t *off, uint32_t n, uint32_t *out) {
  CASE_OF(op < LINE_CHAIN);
  switch (op) {
#define X(OP) case OP: run_point<OP>(rec, o); break;
    POINT_OPS(X)
#undef X
    default: break;
  }
}
__global__ void __launch_bounds__(LANES) k_line_chain(const uint32_t *in, const uint64_t *off, uint32_t n,
                                                      uint32_t *out) {
  CASE_OF(op == LINE_CHAIN);
  __shared__ fe2_lds qs[2 * LANES];
  r28::fe2 &qx = qs[threadIdx.x].v, &qy = qs[LANES + threadIdx.x].v;
  {
    r28::fe2 t;
    ldw(t, rec + 4);
    qx = t;
    ldw(t, rec + 4 + FE2);
    qy = t;
  }
  run_line_chain(o, qx, qy);
}
__global__ void __launch_bounds__(LANES) __attribute__((amdgpu_waves_per_eu(2, 2)))
k_xabs_lds(const uint32_t *in, const uint64_t *off, uint32_t n, uint32_t *out) {
  CASE_OF(op == XABS);
  __shared__ g2a28_lds bl[LANES];
  r28::g2a28 &b = bl[threadIdx.x].v;
  {
    r28::g2a28 t;
    ldw(t, rec + 4);
    b = t;
  }
  r28::g2j28 h;
  r28::g2_xabs_aff28(h, b);
  stw(o, h);
}
__global__ void __launch_bounds__(LANES) k_xabs_reg(const uint32_t *in, const uint64_t *off, uint32_t n,
                                                    uint32_t *out) {
  CASE_OF(op == XABS);
  r28::g2a28 b;
  ldw(b, rec + 4);
  r28::g2j28 h;
  r28::g2_xabs_aff28(h, b);
  stw(o + G2J, h);
}
__global__ void __launch_bounds__(LANES) k_in_group(const uint32_t *in, const uint64_t *off, uint32_t n,
                                                    uint32_t *out) {
  CASE_OF(op == IN_GROUP);
  __shared__ g2a28_lds bl[LANES];
  r28::g2a28 &b = bl[threadIdx.x].v;
  {
    r28::g2a28 t;
    ldw(t, rec + 4);
    b = t;
  }
  o[0] = r28::g2_in_group28(b) ? 1u : 0u;
}
__global__ void __launch_bounds__(LANES) k_clear(const uint32_t *in, const uint64_t *off, uint32_t n, uint32_t *out) {
  CASE_OF(op >= CLEAR_MID && op <= CLEAR_FULL);
  switch (op) {
#define X(OP) case OP: run_clear<OP>(rec, o); break;
    CLEAR_OPS(X)
#undef X
    default: break;
  }
}
__global__ void __launch_bounds__(LANES) k_g1mul(const uint32_t *in, const uint64_t *off, uint32_t n, uint32_t *out) {
  CASE_OF(op == G1MUL);
  run_g1mul(rec, o);
}

template <uint32_t OP>
static __attribute__((noinline)) void host_point(const uint32_t *rec, uint32_t *o) {
  run_point<OP>(rec, o);
}
template <uint32_t OP>
static __attribute__((noinline)) void host_clear(const uint32_t *rec, uint32_t *o) {
  run_clear<OP>(rec, o);
}
static void run_host(const uint32_t *rec, uint32_t *o) {
  const uint32_t op = rec[0];
  if (op < LINE_CHAIN) {
    switch (op) {
#define X(OP) case OP: host_point<OP>(rec, o); break;
      POINT_OPS(X)
#undef X
      default: break;
    }
  } else if (op == LINE_CHAIN) {
    r28::fe2 qx, qy;
    ldw(qx, rec + 4);
    ldw(qy, rec + 4 + FE2);
    run_line_chain(o, qx, qy);
  } else if (op == XABS) {
    r28::g2a28 b;
    ldw(b, rec + 4);
    r28::g2j28 h;
    r28::g2_xabs_aff28(h, b);
    stw(o, h);
    stw(o + G2J, h);
  } else if (op == IN_GROUP) {
    r28::g2a28 b;
    ldw(b, rec + 4);
    o[0] = r28::g2_in_group28(b) ? 1u : 0u;
  } else if (op == G1MUL) {
    run_g1mul(rec, o);
  } else {
    switch (op) {
#define X(OP) case OP: host_clear<OP>(rec, o); break;
      CLEAR_OPS(X)
#undef X
      default: break;
    }
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
    fprintf(stderr, "usage: curve28_check [--host] IN OUT\n");
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
    if (rec[0] >= OP_COUNT || rec[1] != 0) {
      fprintf(stderr, "case %u: unknown op %u / aux %u\n", i, rec[0], rec[1]);
      return 1;
    }
    off[i] = total;
    total += out_words(rec[0]);
  }
  std::vector<uint32_t> o(total, 0xeeeeeeeeu);
  if (host) {
    for (uint32_t i = 0; i < n; i++) run_host(&in[(size_t)i * IN_WORDS], &o[off[i]]);
  } else {
    uint32_t *din, *dout;
    uint64_t *doff;
    HIP_OK(hipMalloc(&din, in.size() * 4));
    HIP_OK(hipMalloc(&doff, off.size() * 8));
    HIP_OK(hipMalloc(&dout, total * 4));
    HIP_OK(hipMemcpy(din, in.data(), in.size() * 4, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(doff, off.data(), off.size() * 8, hipMemcpyHostToDevice));
    HIP_OK(hipMemset(dout, 0xee, total * 4));
    const uint32_t nb = (n + LANES - 1) / LANES;
    k_point<<<nb, LANES>>>(din, doff, n, dout);
    HIP_OK(hipGetLastError());
    k_line_chain<<<nb, LANES>>>(din, doff, n, dout);
    HIP_OK(hipGetLastError());
    k_xabs_lds<<<nb, LANES>>>(din, doff, n, dout);
    HIP_OK(hipGetLastError());
    k_xabs_reg<<<nb, LANES>>>(din, doff, n, dout);
    HIP_OK(hipGetLastError());
    k_in_group<<<nb, LANES>>>(din, doff, n, dout);
    HIP_OK(hipGetLastError());
    k_clear<<<nb, LANES>>>(din, doff, n, dout);
    HIP_OK(hipGetLastError());
    k_g1mul<<<nb, LANES>>>(din, doff, n, dout);
    HIP_OK(hipGetLastError());
    HIP_OK(hipDeviceSynchronize());
    HIP_OK(hipMemcpy(o.data(), dout, total * 4, hipMemcpyDeviceToHost));
  }
  f = fopen(argv[argc - 1], "wb");
  if (!f) return 1;
  if (fwrite(o.data(), 4, total, f) != total) return 1;
  if (fclose(f) != 0) return 1;
  printf("curve28_check: %u cases%s, %zu result words\n", n, host ? " (host)" : "", total);
  return 0;
}
