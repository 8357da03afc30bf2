// gfx950 kernels: the call-local key table of local key sets (gbls_local.h,
// include/grandine_bls_gpu_local.h).  k_g1_local_decode turns a call's compressed keys pkb[n] into
// loc[n] in the registry's radix-32 form, with PublicKey::try_from semantics (an invalid key is
// stored all-zero, as gbls_registry_set stores one) and their statuses.  Two forms, the same bytes
// and statuses as k_g1_decompress(validate = 1) on every input:
//   k_g1_local_decode        one lane per key (the throughput form)
//   k_g1_local_decode_wave   one 64-lane wave per key on the W4 engine (bls_w4.h): a block's
//                            deposits and address changes are a handful of keys, and one lane's
//                            square root plus two 64-bit membership chains would be the longest
//                            kernel of the submission
#include "gbls_common.h"
#include "gbls_local.h"
#include "bls_w4.h"

namespace gbls {

__global__ void __launch_bounds__(WG) k_g1_local_decode(const uint8_t *in, uint32_t n, g1a *loc, int32_t *st) {
  const uint32_t i = blockIdx.x * WG + threadIdx.x;
  if (i >= n) return;
  g1a a;
  int32_t s = g1_decompress(a, in + 48u * i);
  if (s == ST_SUCCESS) {  // PublicKey::validate, public_key.rs:27
    if (aff_is_inf(a))
      s = ST_PK_IS_INFINITY;
    else if (!g1_in_group(a))
      s = ST_NOT_IN_GROUP;
  }
  if (s != ST_SUCCESS) {
    fp_zero(a.x);
    fp_zero(a.y);
  }
  loc[i] = a;
  st[i] = s;
}

// [|x|] acc for a base (bx, by) that acc starts from, affine on the curve the chain runs on (dbl1 and
// madd1 never read the curve's b)
__device__ __forceinline__ void w4_mul_by_xabs1(const w4::Ctx &c, w4::J1 &acc, uint32_t bx, uint32_t by) {
  acc = w4::J1{bx, by, c.one};
  for (int i = 62; i >= 0; i--) {
    w4::dbl1(c, acc, acc);
    if ((k::X_ABS >> i) & 1) w4::madd1(c, acc, acc, bx, by);
  }
}

// One wave per key.  The flag checks, the infinity encoding and x < p are lane-local and the same
// in all 64 lanes (every branch below is wave-uniform); x, x^3 + 4, the y^2 == rhs test and the
// sign choice are g1_decompress's own one-lane lines, so x and y are its canonical words.  On the
// rows: y = rhs^((p+1)/4) as rhs^((p-3)/4) rhs (dfp::pow_pm3d4), and the membership test
// [x^2]P == -phi(P) as two mul_by_xabs chains.  The second chain's base Q = [|x|]P = (X : Y : Z) is
// Jacobian, and madd1 adds an affine point, so the chain runs on the isomorphic curve
// y^2 = x^3 + 4 Z^6, where (X, Y) IS affine: its result (X' : Y' : Z') is the point
// (X' : Y' : Z' Z) of E.  No inversion: -phi(P) = (beta x, -y) is compared by cross-multiplication.
template <bool X>
__global__ void __launch_bounds__(64) k_g1_local_decode_wave(const uint8_t *in, uint32_t n, g1a *loc, int32_t *st) {
  if constexpr (X) w4::exclusive_simd();
  const uint32_t i = blockIdx.x;
  if (i >= n) return;  // whole waves
  const uint8_t *b = in + 48u * i;
  g1a a;
  fp_zero(a.x);
  fp_zero(a.y);
  int32_t s = ST_SUCCESS;
  const uint8_t b0 = b[0];
  bool point = false;
  fp x, rhs;
  if (!(b0 & 0x80)) {
    s = ST_BAD_ENCODING;
  } else if (b0 & 0x40) {  // the infinity encoding: a well-formed one is PK_IS_INFINITY
    uint32_t acc = b0 & 0x3f;
    for (int q = 1; q < 48; q++) acc |= b[q];
    s = acc ? ST_BAD_ENCODING : ST_PK_IS_INFINITY;
  } else {
    fp_from_be48(x, b);
    x.l[11] &= 0x1fffffffu;
    if (!limbs_lt(x.l, k::P)) {
      s = ST_BAD_ENCODING;
    } else {
      fp_to_mont(x, x);
      fp_sqr(rhs, x);
      fp_mul(rhs, rhs, x);
      fp_add(rhs, rhs, fp_const(k::B1_M));
      point = true;
    }
  }
  if (point) {
    w4::Ctx c;
    w4::init(c);
    const uint32_t rr = dfp::from_regs(rhs.l, c.t);
    const uint32_t yr = dfp::mul(dfp::pow_pm3d4(rr, c.t), rr, c.t);
    fp y, y2;
    dfp::to_words_all(y.l, yr, c.t);
    fp_sqr(y2, y);
    if (!fp_eq(y2, rhs)) {
      s = ST_NOT_ON_CURVE;
    } else {
      if (fp_lex_largest(y) != (bool)(b0 & 0x20)) fp_neg(y, y);
      if (fp_is_zero(x)) {  // (0, +-2) has order 3
        s = ST_NOT_IN_GROUP;
      } else {
        fp bx;
        fp_mul(bx, x, fp_const(k::BETA_M));
        const uint32_t px = dfp::from_regs(x.l, c.t), py = dfp::from_regs(y.l, c.t), pbx = dfp::from_regs(bx.l, c.t);
        w4::J1 q, t;
        w4_mul_by_xabs1(c, q, px, py);
        bool member = !(w4::zero4(c, q.z, q.z, q.z, q.z) & 1);  // an infinite [|x|]P: [x^2]P is infinite too
        if (member) {
          w4_mul_by_xabs1(c, t, q.x, q.y);
          uint32_t zt, zz, zzz, u, v, d0, d1;
          w4::mul4(c, zt, d0, d1, d1, t.z, q.z, t.z, q.z, t.z, q.z, t.z, q.z);
          w4::mul4(c, zz, d0, d1, d1, zt, zt, zt, zt, zt, zt, zt, zt);
          w4::mul4(c, u, zzz, d0, d1, pbx, zz, zz, zt, pbx, zz, pbx, zz);
          w4::mul4(c, v, d0, d1, d1, py, zzz, py, zzz, py, zzz, py, zzz);
          // X' == beta x Zt^2, Y' == -y Zt^3, Zt != 0
          const uint32_t zf = w4::zero4(c, w4::sub<1>(c, t.x, u), w4::add(t.y, v), zt, zt);
          member = (zf & 7) == 3;
        }
        if (member) {
          a.x = x;
          a.y = y;
        } else {
          s = ST_NOT_IN_GROUP;
        }
      }
    }
  }
  if (threadIdx.x == 0) {
    loc[i] = a;
    st[i] = s;
  }
}

void launch_g1_local_decode(hipStream_t st, const uint8_t *in, uint32_t n, g1a *loc, int32_t *status) {
  if (!n) return;
  if (n <= kLocalWaveMax)
    (n <= w4::kExclusiveMaxWaves ? k_g1_local_decode_wave<true> : k_g1_local_decode_wave<false>)<<<n, 64, 0, st>>>(
        in, n, loc, status);
  else
    k_g1_local_decode<<<nblk(n), WG, 0, st>>>(in, n, loc, status);
}

}  // namespace gbls
