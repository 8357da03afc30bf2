// gfx950 kernel: the last stage of the c = 5 bucket MSM (k_msm.hip) on the wave-per-point engine
// (bls_w4.h) -- per (segment, window) the weighted sum of its 16 bucket sums,
//   S(s, w) = sum_{b = 0..15} (b + 1) X(s, w, b),
// which pairs with -[2^(5 w)] g1: 13 extra Miller pairs per segment.  A bucket's X is the sum of
// its runs (the first chunk partial, then every kMsmFold-th: k_msm_fold).
#include "gbls_common.h"
#include "k_msm.h"
#include "bls_w4.h"

namespace gbls {

// One workgroup of kMsmW4Waves waves per window.  Wave v owns the buckets [lo, lo + BW),
// lo = v BW, and walks them downwards with the running sums T += X_b (run by run), A += T, so
// that T = sum X_b and A = sum (b - lo + 1) X_b; its share of S is A + lo T (double-and-add over
// the bits of lo).  The waves' shares are joined through LDS in a tree (the row-form registers as
// they are, as k_g2sum_final_w4), wave 0 stores S.
// Two waves: the dependent chain is 8 x (runs + 1) + 2 additions and 3 doublings (C2's buckets
// have two runs: 26 additions at ~9.5 us, 0.26 ms measured) and a 16-segment launch is 416 waves,
// within w4::kExclusiveMaxWaves.  Four waves for launches of up to 128 windows (single batches,
// C4's one segment) were measured and dropped: the kernel's own time fell to 0.23 ms with four
// runs per bucket, but neither C4 nor the one-batch-per-step leg gained: the signature side is
// not on a single batch's critical path.
// Every branch depends on the window's counts or on the wave index only: wave-uniform.
constexpr int kMsmW4Waves = 2;
constexpr int kMsmW4Buckets = 16;  // 2^(c-1), c = 5
template <bool X, bool R28>
__global__ void __launch_bounds__(64 * kMsmW4Waves) k_msm_windows_w4(const g2j *chunk, const uint32_t *cstart,
                                                                    uint32_t nwin, uint32_t W, uint32_t xb,
                                                                    const uint32_t *seg_off, int empty_is_error,
                                                                    g1s *P, g2a *H, int32_t *seg_err, g2j *Sj) {
  if constexpr (X) w4::exclusive_simd();
  constexpr int NW = kMsmW4Waves, BW = kMsmW4Buckets / NW;
  static_assert(NW >= 1 && (NW & (NW - 1)) == 0 && NW <= kMsmW4Buckets, "a power of two of waves");
  __shared__ uint32_t sh[NW > 1 ? NW / 2 : 1][6 * 64];  // a sending wave's share, word k of lane l at k * 64 + l
  const uint32_t t = blockIdx.x;
  if (t >= nwin) return;  // block-uniform
  const uint32_t v = threadIdx.x >> 6, lane = threadIdx.x & 63;
  w4::Ctx c;
  w4::init(c);
  w4::J T, A;
  w4::set_inf(c, T);
  w4::set_inf(c, A);
  const uint32_t lo = t * kMsmW4Buckets + v * BW;
  for (uint32_t b = lo + BW; b-- > lo;) {
    const uint32_t c0 = cstart[b], c1 = cstart[b + 1];
    for (uint32_t q = c0; q < c1; q += kMsmFold) {
      w4::J x;
      if constexpr (R28)
        w4::load28(c, x, chunk[q]);
      else
        w4::load(c, x, chunk[q]);
      w4::add(c, T, T, x);
    }
    w4::add(c, A, A, T);
  }
  if (v) {  // + lo T, lo = v BW < 16
    const uint32_t m = v * BW;
    w4::J D = T;
    for (int bit = 30 - __clz((int)m); bit >= 0; bit--) {  // below m's top bit
      w4::dbl(c, D, D);
      if ((m >> bit) & 1) w4::add(c, D, D, T);
    }
    w4::add(c, A, A, D);
  }
  for (uint32_t width = NW / 2; width > 0; width >>= 1) {
    __syncthreads();
    if (v >= width && v < 2 * width) {
      uint32_t *d = sh[v - width] + lane;
      const uint32_t s[6] = {A.x.c0, A.x.c1, A.y.c0, A.y.c1, A.z.c0, A.z.c1};
#pragma unroll
      for (int k = 0; k < 6; k++) d[64 * k] = s[k];
    }
    __syncthreads();
    if (v < width) {
      const uint32_t *d = sh[v] + lane;
      w4::J o;
      o.x = {d[0], d[64]};
      o.y = {d[128], d[192]};
      o.z = {d[256], d[320]};
      w4::add(c, A, A, o);
    }
  }
  if (v != 0) return;  // wave-uniform; no barrier follows
  if (Sj)
    w4::store_jac(c, Sj + t, A);  // the lines take it projectively (k_lines_w4j)
  else
    w4::store_affine(c, H + xb + t, A);
  if (threadIdx.x == 0) {
    const uint32_t s = t / W, w = t % W;
    g1s g;
    msm_weight(g, k::MSM_W5, kMsmW4Buckets * w);  // bucket 0 of window w: -[2^(5 w)] g1
    P[xb + t] = g;
    if (w == 0 && empty_is_error && seg_off[s + 1] == seg_off[s]) atomicOr(&seg_err[s], 1);
  }
}

void launch_msm_windows_w4(hipStream_t st, const g2j *chunk, const uint32_t *cstart, uint32_t nwin, uint32_t W,
                           bool r28, uint32_t xb, const uint32_t *seg_off, int empty_is_error, g1s *P, g2a *H,
                           int32_t *seg_err, g2j *Sj) {
  const bool x = nwin * kMsmW4Waves <= w4::kExclusiveMaxWaves;
  auto k = r28 ? (x ? k_msm_windows_w4<true, true> : k_msm_windows_w4<false, true>)
               : (x ? k_msm_windows_w4<true, false> : k_msm_windows_w4<false, false>);
  k<<<nwin, 64 * kMsmW4Waves, 0, st>>>(chunk, cstart, nwin, W, xb, seg_off, empty_is_error, P, H, seg_err, Sj);
}

}  // namespace gbls
