// bls_gang.h function by function on MI355X: `gang_check IN OUT` reads a case file written by
// tools/ubench/gang_vectors.py (an op code, a 64-bit scalar and the operands as RAW 12 x 32-bit
// Montgomery limb images, so the caller controls every limb), runs one DPP quad (4 lanes) or one
// DPP row (16 lanes) per case in work-groups of WG threads, as the engine's kernels do, and
// writes the results of EVERY lane of the gang (the header promises that all lanes end holding
// the same value; the kernels store from lane 0, lane c % 4 or lane c).  Chains also write every
// intermediate accumulator from lane 0.  It checks nothing itself beyond the HIP status:
// tests/test_gpu_gang.py recomputes every word with Python integers.
// Build: make -C tools/ubench
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../grandine_amd/csrc/gbls_common.h"
#define GBLS_GANG_LINES
#include "../../grandine_amd/csrc/bls_gang.h"
#include "../../grandine_amd/csrc/bls_pairing.h"

using namespace gbls;

// op codes (gang_vectors.py OPS); quad ops first, then row ops
enum : uint32_t {
  Q_FP2MUL = 0,      // r = a b, r fresh
  Q_FP2MUL_RA = 1,   // a = a b
  Q_FP2MUL_RB = 2,   // b = a b
  Q_FP2MUL_AA = 3,   // r = a a (a == b)
  Q_DBL = 4,         // gang_dbl, r fresh
  Q_DBL_RP = 5,      // r aliasing p
  Q_ADD = 6,         // gang_add, r fresh
  Q_ADD_RA = 7,      // r aliasing a
  Q1_DBL = 8,        // gang1_dbl
  Q1_DBL_RP = 9,
  Q1_ADD = 10,       // gang1_add
  Q1_ADD_RA = 11,
  Q_LINE_DBL = 12,   // gang_line_dbl: T, L0, L2, L3
  Q_LINE_ADD = 13,   // gang_line_add_aff
  Q_XABS = 14,       // gang_mul_by_xabs, every acc
  Q_G1MUL = 15,      // k_mv_g1mul's chain, every acc, then g1s_from_jac
  Q_G2MUL = 16,      // k_mv_g2mul's chain on half aux of the scalar, every acc
  Q_LINES = 17,      // k_lines' 68 events: every event's coefficients, the final T
  R_MUL4 = 18,       // row_mul4, four distinct products
  R_MUL4_ALIAS = 19, // outputs aliasing A0, B1, A2, B3
  R_MUL4_TXXX = 20,  // row_mul4(t, x, x, x, E, E, E, E, t, t, t, t)
  R_DBL = 21,
  R_DBL_RP = 22,
  R_ADD = 23,
  R_ADD_RA = 24,
  R_LINE_DBL = 25,
  R_LINE_ADD = 26,
  R_XABS = 27,
  R_LINES = 28,      // k_lines_row's 68 events
  OP_COUNT = 29
};
constexpr int IN_WORDS = 4 + 192;  // op, aux, scalar lo, scalar hi, then up to 8 Fp2 operands
constexpr int F1 = 12, F2 = 24, G1J = 36, G2J = 72, G2A = 48, LINE = 72;
constexpr int XABS_STEPS = 68;  // 63 doublings + 5 additions

static bool is_row(uint32_t op) { return op >= R_MUL4; }
// doublings + additions of the MSB-first chain on k (0: the identity comes out untouched)
static uint32_t chain_steps(uint64_t k) {
  if (k == 0) return 0;
  int top = 63;
  while (!((k >> top) & 1)) top--;
  return (uint32_t)top + (uint32_t)__builtin_popcountll(k) - 1;
}
static bool all_zero(const uint32_t *w, int n) {
  uint32_t acc = 0;
  for (int i = 0; i < n; i++) acc |= w[i];
  return acc == 0;
}
// words written from lane 0 before the per-lane blocks, and words per lane
static void out_shape(const uint32_t *rec, size_t &pre, size_t &per) {
  const uint32_t op = rec[0];
  const uint64_t r = (uint64_t)rec[2] | ((uint64_t)rec[3] << 32);
  pre = 0;
  switch (op) {
    case Q_FP2MUL: case Q_FP2MUL_RA: case Q_FP2MUL_RB: case Q_FP2MUL_AA: per = F2; break;
    case Q_DBL: case Q_DBL_RP: case Q_ADD: case Q_ADD_RA:
    case R_DBL: case R_DBL_RP: case R_ADD: case R_ADD_RA: per = G2J; break;
    case Q1_DBL: case Q1_DBL_RP: case Q1_ADD: case Q1_ADD_RA: per = G1J; break;
    case Q_LINE_DBL: case Q_LINE_ADD: case R_LINE_DBL: case R_LINE_ADD: per = G2J + LINE; break;
    case Q_XABS: case R_XABS: pre = (size_t)XABS_STEPS * G2J; per = G2J; break;
    case Q_G1MUL:
      pre = all_zero(rec + 4, 2 * F1) ? 0 : (size_t)chain_steps(r) * G1J;
      per = 2 * G1J;
      break;
    case Q_G2MUL:
      pre = all_zero(rec + 4, G2A) ? 0 : (size_t)chain_steps(rec[1] ? (r >> 32) : (r & 0xffffffffull)) * G2J;
      per = G2J;
      break;
    case Q_LINES: case R_LINES: per = (size_t)ML_EVENTS * LINE + G2J; break;
    case R_MUL4: case R_MUL4_ALIAS: per = 4 * F2; break;
    case R_MUL4_TXXX: per = 2 * F2; break;
    default: per = 0;
  }
}

// ---------------------------------------------------------------- operand images
__device__ __forceinline__ void ld(fp &r, const uint32_t *s) {
#pragma unroll
  for (int i = 0; i < 12; i++) r.l[i] = s[i];
}
__device__ __forceinline__ void ld(fp2 &r, const uint32_t *s) {
  ld(r.c0, s);
  ld(r.c1, s + F1);
}
template <class F>
__device__ __forceinline__ void ld(jac<F> &r, const uint32_t *s) {
  constexpr int W = sizeof(F) / 4;
  ld(r.x, s);
  ld(r.y, s + W);
  ld(r.z, s + 2 * W);
}
template <class F>
__device__ __forceinline__ void ld(aff<F> &r, const uint32_t *s) {
  constexpr int W = sizeof(F) / 4;
  ld(r.x, s);
  ld(r.y, s + W);
}
__device__ __forceinline__ void ld(g2h &r, const uint32_t *s) {
  ld(r.x, s);
  ld(r.y, s + F2);
  ld(r.z, s + 2 * F2);
}
__device__ __forceinline__ void st(uint32_t *d, const fp &a) {
#pragma unroll
  for (int i = 0; i < 12; i++) d[i] = a.l[i];
}
__device__ __forceinline__ void st(uint32_t *d, const fp2 &a) {
  st(d, a.c0);
  st(d + F1, a.c1);
}
template <class F>
__device__ __forceinline__ void st(uint32_t *d, const jac<F> &a) {
  constexpr int W = sizeof(F) / 4;
  st(d, a.x);
  st(d + W, a.y);
  st(d + 2 * W, a.z);
}
__device__ __forceinline__ void st(uint32_t *d, const g2h &a) {
  st(d, a.x);
  st(d + F2, a.y);
  st(d + 2 * F2, a.z);
}
__device__ __forceinline__ void st(uint32_t *d, const g1s &a) {
  st(d, a.x);
  st(d + F1, a.y);
  st(d + 2 * F1, a.c);
}
__device__ __forceinline__ void st_line(uint32_t *d, const g2h &T, const fp2 &L0, const fp2 &L2, const fp2 &L3) {
  st(d, T);
  st(d + G2J, L0);
  st(d + G2J + F2, L2);
  st(d + G2J + 2 * F2, L3);
}

// ---------------------------------------------------------------- one quad per case
__global__ void __launch_bounds__(WG) k_quad(const uint32_t *in, const uint64_t *off, uint32_t n, uint32_t *out) {
  uint32_t t = blockIdx.x * WG + threadIdx.x;
  uint32_t i = t >> 2;
  int q = (int)(t & 3);
  if (i >= n) return;  // whole quads only
  const uint32_t *rec = in + (size_t)IN_WORDS * i;
  const uint32_t *a = rec + 4;
  uint32_t *o = out + off[i];
  const uint32_t op = rec[0];  // quad-uniform
  const uint64_t sc = (uint64_t)rec[2] | ((uint64_t)rec[3] << 32);
  switch (op) {
    case Q_FP2MUL: case Q_FP2MUL_RA: case Q_FP2MUL_RB: case Q_FP2MUL_AA: {
      fp2 x, y, r;
      ld(x, a);
      ld(y, a + F2);
      if (op == Q_FP2MUL) {
        gang_fp2_mul(r, x, y, q);
      } else if (op == Q_FP2MUL_RA) {
        gang_fp2_mul(x, x, y, q);
        r = x;
      } else if (op == Q_FP2MUL_RB) {
        gang_fp2_mul(y, x, y, q);
        r = y;
      } else {
        gang_fp2_mul(r, x, x, q);
      }
      st(o + F2 * q, r);
      break;
    }
    case Q_DBL: case Q_DBL_RP: {
      g2j p, r;
      ld(p, a);
      if (op == Q_DBL) {
        gang_dbl(r, p, q);
      } else {
        gang_dbl(p, p, q);
        r = p;
      }
      st(o + G2J * q, r);
      break;
    }
    case Q_ADD: case Q_ADD_RA: {
      g2j x, y, r;
      ld(x, a);
      ld(y, a + G2J);
      if (op == Q_ADD) {
        gang_add(r, x, y, q);
      } else {
        gang_add(x, x, y, q);
        r = x;
      }
      st(o + G2J * q, r);
      break;
    }
    case Q1_DBL: case Q1_DBL_RP: {
      g1j p, r;
      ld(p, a);
      if (op == Q1_DBL) {
        gang1_dbl(r, p, q);
      } else {
        gang1_dbl(p, p, q);
        r = p;
      }
      st(o + G1J * q, r);
      break;
    }
    case Q1_ADD: case Q1_ADD_RA: {
      g1j x, y, r;
      ld(x, a);
      ld(y, a + G1J);
      if (op == Q1_ADD) {
        gang1_add(r, x, y, q);
      } else {
        gang1_add(x, x, y, q);
        r = x;
      }
      st(o + G1J * q, r);
      break;
    }
    case Q_LINE_DBL: case Q_LINE_ADD: {
      g2h T;
      g2a Q;
      fp2 L0, L2, L3;
      ld(T, a);
      ld(Q, a + G2J);
      if (op == Q_LINE_DBL)
        gang_line_dbl(T, L0, L2, L3, q);
      else
        gang_line_add_aff(T, Q, L0, L2, L3, q);
      st_line(o + (G2J + LINE) * q, T, L0, L2, L3);
      break;
    }
    case Q_XABS: {  // gang_mul_by_xabs, every acc from lane 0
      g2j p, acc;
      ld(p, a);
      acc = p;
      uint32_t *d = o;
      for (int b = 62; b >= 0; b--) {
        gang_dbl(acc, acc, q);
        if (q == 0) st(d, acc);
        d += G2J;
        if ((k::X_ABS >> b) & 1) {
          gang_add(acc, acc, p, q);
          if (q == 0) st(d, acc);
          d += G2J;
        }
      }
      g2j r;
      gang_mul_by_xabs(r, p, q);  // the header's own loop must end on the same words
      st(d + G2J * q, r);
      break;
    }
    case Q_G1MUL: {  // k_mv_g1mul
      g1a pk;
      ld(pk, a);
      uint64_t k = sc;
      g1j acc;
      jac_set_inf(acc);
      uint32_t *d = o;
      if (k != 0 && !aff_is_inf(pk)) {
        int top = 63;
        while (!((k >> top) & 1)) top--;
        g1j base;
        jac_from_aff(base, pk);
        acc = base;
        for (int b = top - 1; b >= 0; b--) {
          gang1_dbl(acc, acc, q);
          if (q == 0) st(d, acc);
          d += G1J;
          if ((k >> b) & 1) {
            gang1_add(acc, acc, base, q);
            if (q == 0) st(d, acc);
            d += G1J;
          }
        }
      }
      g1s s;
      g1s_from_jac(s, acc);
      st(d + 2 * G1J * q, acc);
      st(d + 2 * G1J * q + G1J, s);
      break;
    }
    case Q_G2MUL: {  // k_mv_g2mul, one 32-bit half per quad
      g2a base;
      ld(base, a);
      uint64_t k = rec[1] == 0 ? (sc & 0xffffffffull) : (sc >> 32);
      g2j acc;
      jac_set_inf(acc);
      uint32_t *d = o;
      if (k != 0 && !aff_is_inf(base)) {
        int top = 63;
        while (!((k >> top) & 1)) top--;
        g2j bj;
        jac_from_aff(bj, base);
        acc = bj;
        for (int b = top - 1; b >= 0; b--) {
          gang_dbl(acc, acc, q);
          if (q == 0) st(d, acc);
          d += G2J;
          if ((k >> b) & 1) {
            gang_add(acc, acc, bj, q);
            if (q == 0) st(d, acc);
            d += G2J;
          }
        }
      }
      st(d + G2J * q, acc);
      break;
    }
    case Q_LINES: {  // k_lines, events [0, ML_EVENTS)
      g2a Q;
      ld(Q, a);
      g2h T;
      fp2 L0, L2, L3;
      T.x = Q.x;
      T.y = Q.y;
      fp2_one(T.z);
      uint32_t *d = o + (size_t)(ML_EVENTS * LINE + G2J) * q;
      for (int e = 0; e < ML_EVENTS; e++) {
        if (ev_is_dbl(e))
          gang_line_dbl(T, L0, L2, L3, q);
        else
          gang_line_add_aff(T, Q, L0, L2, L3, q);
        st(d + LINE * e, L0);
        st(d + LINE * e + F2, L2);
        st(d + LINE * e + 2 * F2, L3);
      }
      st(d + ML_EVENTS * LINE, T);
      break;
    }
    default: break;
  }
}

// ---------------------------------------------------------------- one row per case
__global__ void __launch_bounds__(WG) k_row(const uint32_t *in, const uint64_t *off, uint32_t n, uint32_t *out) {
  uint32_t t = blockIdx.x * WG + threadIdx.x;
  uint32_t i = t >> 4;
  int l = (int)(t & 15);
  if (i >= n) return;  // whole rows
  const uint32_t *rec = in + (size_t)IN_WORDS * i;
  const uint32_t *a = rec + 4;
  uint32_t *o = out + off[i];
  const uint32_t op = rec[0];  // row-uniform
  switch (op) {
    case R_MUL4: case R_MUL4_ALIAS: {
      fp2 A0, A1, A2, A3, B0, B1, B2, B3;
      ld(A0, a);
      ld(A1, a + F2);
      ld(A2, a + 2 * F2);
      ld(A3, a + 3 * F2);
      ld(B0, a + 4 * F2);
      ld(B1, a + 5 * F2);
      ld(B2, a + 6 * F2);
      ld(B3, a + 7 * F2);
      uint32_t *d = o + 4 * F2 * l;
      if (op == R_MUL4) {
        fp2 R0, R1, R2, R3;
        row_mul4(R0, R1, R2, R3, A0, A1, A2, A3, B0, B1, B2, B3, l);
        st(d, R0);
        st(d + F2, R1);
        st(d + 2 * F2, R2);
        st(d + 3 * F2, R3);
      } else {
        row_mul4(A0, B1, A2, B3, A0, A1, A2, A3, B0, B1, B2, B3, l);
        st(d, A0);
        st(d + F2, B1);
        st(d + 2 * F2, A2);
        st(d + 3 * F2, B3);
      }
      break;
    }
    case R_MUL4_TXXX: {  // the last level of row_dbl / row_line_dbl
      fp2 E, tt, x;
      ld(E, a);
      ld(tt, a + F2);
      row_mul4(tt, x, x, x, E, E, E, E, tt, tt, tt, tt, l);
      st(o + 2 * F2 * l, tt);
      st(o + 2 * F2 * l + F2, x);
      break;
    }
    case R_DBL: case R_DBL_RP: {
      g2j p, r;
      ld(p, a);
      if (op == R_DBL) {
        row_dbl(r, p, l);
      } else {
        row_dbl(p, p, l);
        r = p;
      }
      st(o + G2J * l, r);
      break;
    }
    case R_ADD: case R_ADD_RA: {
      g2j x, y, r;
      ld(x, a);
      ld(y, a + G2J);
      if (op == R_ADD) {
        row_add(r, x, y, l);
      } else {
        row_add(x, x, y, l);
        r = x;
      }
      st(o + G2J * l, r);
      break;
    }
    case R_LINE_DBL: case R_LINE_ADD: {
      g2h T;
      g2a Q;
      fp2 L0, L2, L3;
      ld(T, a);
      ld(Q, a + G2J);
      if (op == R_LINE_DBL)
        row_line_dbl(T, L0, L2, L3, l);
      else
        row_line_add_aff(T, Q, L0, L2, L3, l);
      st_line(o + (G2J + LINE) * l, T, L0, L2, L3);
      break;
    }
    case R_XABS: {
      g2j p, acc;
      ld(p, a);
      acc = p;
      uint32_t *d = o;
      for (int b = 62; b >= 0; b--) {
        row_dbl(acc, acc, l);
        if (l == 0) st(d, acc);
        d += G2J;
        if ((k::X_ABS >> b) & 1) {
          row_add(acc, acc, p, l);
          if (l == 0) st(d, acc);
          d += G2J;
        }
      }
      g2j r;
      row_mul_by_xabs(r, p, l);
      st(d + G2J * l, r);
      break;
    }
    case R_LINES: {  // k_lines_row, events [0, ML_EVENTS)
      g2a Q;
      ld(Q, a);
      g2h T;
      fp2 L0, L2, L3;
      T.x = Q.x;
      T.y = Q.y;
      fp2_one(T.z);
      uint32_t *d = o + (size_t)(ML_EVENTS * LINE + G2J) * l;
      for (int e = 0; e < ML_EVENTS; e++) {
        if (ev_is_dbl(e))
          row_line_dbl(T, L0, L2, L3, l);
        else
          row_line_add_aff(T, Q, L0, L2, L3, l);
        st(d + LINE * e, L0);
        st(d + LINE * e + F2, L2);
        st(d + LINE * e + 2 * F2, L3);
      }
      st(d + ML_EVENTS * LINE, T);
      break;
    }
    default: break;
  }
}

#define HIP_OK(call)                                                              \
  do {                                                                            \
    const hipError_t err_ = (call);                                               \
    if (err_ != hipSuccess) {                                                     \
      fprintf(stderr, "%s: %s\n", #call, hipGetErrorString(err_));                \
      return 2;                                                                   \
    }                                                                             \
  } while (0)

int main(int argc, char **argv) {
  if (argc != 3) {
    fprintf(stderr, "usage: gang_check IN OUT\n");
    return 1;
  }
  FILE *f = fopen(argv[1], "rb");
  if (!f) return 1;
  uint32_t n = 0;
  if (fread(&n, 4, 1, f) != 1 || n == 0 || n > (1u << 16)) return 1;
  std::vector<uint32_t> in((size_t)n * IN_WORDS);
  if (fread(in.data(), 4, in.size(), f) != in.size()) return 1;
  fclose(f);
  // the cases of each kind keep their file order; the results are laid out in file order
  std::vector<uint32_t> inq, inr;
  std::vector<uint64_t> offq, offr;
  size_t total = 0;
  for (uint32_t i = 0; i < n; i++) {
    const uint32_t *rec = &in[(size_t)i * IN_WORDS];
    if (rec[0] >= OP_COUNT || rec[1] > 1) {
      fprintf(stderr, "case %u: unknown op %u / aux %u\n", i, rec[0], rec[1]);
      return 1;
    }
    size_t pre, per;
    out_shape(rec, pre, per);
    const bool row = is_row(rec[0]);
    (row ? inr : inq).insert((row ? inr : inq).end(), rec, rec + IN_WORDS);
    (row ? offr : offq).push_back(total);
    total += pre + per * (row ? 16 : 4);
  }
  const uint32_t nq = (uint32_t)offq.size(), nr = (uint32_t)offr.size();
  uint32_t *dout;
  HIP_OK(hipMalloc(&dout, total * 4));
  HIP_OK(hipMemset(dout, 0xee, total * 4));
  if (nq) {
    uint32_t *din;
    uint64_t *doff;
    HIP_OK(hipMalloc(&din, inq.size() * 4));
    HIP_OK(hipMalloc(&doff, offq.size() * 8));
    HIP_OK(hipMemcpy(din, inq.data(), inq.size() * 4, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(doff, offq.data(), offq.size() * 8, hipMemcpyHostToDevice));
    k_quad<<<nblk((size_t)nq * 4), WG>>>(din, doff, nq, dout);
    HIP_OK(hipGetLastError());
  }
  if (nr) {
    uint32_t *din;
    uint64_t *doff;
    HIP_OK(hipMalloc(&din, inr.size() * 4));
    HIP_OK(hipMalloc(&doff, offr.size() * 8));
    HIP_OK(hipMemcpy(din, inr.data(), inr.size() * 4, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(doff, offr.data(), offr.size() * 8, hipMemcpyHostToDevice));
    k_row<<<nblk((size_t)nr * 16), WG>>>(din, doff, nr, dout);
    HIP_OK(hipGetLastError());
  }
  HIP_OK(hipDeviceSynchronize());
  std::vector<uint32_t> o(total);
  HIP_OK(hipMemcpy(o.data(), dout, total * 4, hipMemcpyDeviceToHost));
  f = fopen(argv[2], "wb");
  if (!f) return 1;
  if (fwrite(o.data(), 4, total, f) != total) return 1;
  if (fclose(f) != 0) return 1;
  printf("gang_check: %u quad cases, %u row cases, %zu result words\n", nq, nr, total);
  return 0;
}
