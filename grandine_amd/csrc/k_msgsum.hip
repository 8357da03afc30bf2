// gfx950 kernels: message groups (GBLS_INIT_DEDUP).  Sets of one segment that share a message m
// fold by bilinearity, prod_i e(r_i pk_i, H(m)) = e(sum_i r_i pk_i, H(m)): k_mv_g1mul writes the
// per-set points r_i pk_i as before, and k_g1s_msgsum forms each group's point, the G1 half of
// the group's one Miller pair.  The points are line-evaluation points (bls_pairing.h g1s), i.e.
// homogeneous projective, summed by the complete addition (g1s_add / r28::g1h28_add): no
// inversion, and a group whose sum is infinity is written all-zero (its lines evaluate to 1).
#include "gbls_common.h"
#include "bls_curve28.h"

namespace gbls {

namespace {

// the two arithmetic layers behind one interface (R28: bls_curve28.h, else bls_pairing.h)
template <bool R28>
struct Sum;
template <>
struct Sum<true> {
  typedef r28::g1h28 pt;
  static constexpr int kWords = 42;
  static __device__ __forceinline__ void inf(pt &a) { r28::g1h28_set_inf(a); }
  static __device__ __forceinline__ void load(pt &a, const g1s &p) { r28::g1h28_load(a, p); }
  static __device__ __forceinline__ void add(pt &a, const pt &b) { r28::g1h28_add(a, a, b); }
  static __device__ __forceinline__ void store(g1s &p, const pt &a) { r28::g1h28_store(p, a); }
  static __device__ __forceinline__ uint32_t &word(pt &a, int k) {
    return k < 14 ? a.x.l[k] : k < 28 ? a.y.l[k - 14] : a.c.l[k - 28];
  }
};
template <>
struct Sum<false> {
  typedef g1s pt;
  static constexpr int kWords = 36;
  static __device__ __forceinline__ void inf(pt &a) {
    fp_zero(a.x);
    fp_zero(a.y);
    fp_zero(a.c);
  }
  static __device__ __forceinline__ void load(pt &a, const g1s &p) { a = p; }
  static __device__ __forceinline__ void add(pt &a, const pt &b) { g1s_add(a, a, b); }
  static __device__ __forceinline__ void store(g1s &p, const pt &a) { p = a; }  // g1s_add zeroes infinity
  static __device__ __forceinline__ uint32_t &word(pt &a, int k) {
    return k < 12 ? a.x.l[k] : k < 24 ? a.y.l[k - 12] : a.c.l[k - 24];
  }
};

}  // namespace

// One lane per group (many small groups): the members in list order.
template <bool R28>
__global__ void __launch_bounds__(WG) k_g1s_msgsum(const g1s *Pset, const uint32_t *grp_off,
                                                   const uint32_t *grp_set, uint32_t ngrp, g1s *P) {
  typedef Sum<R28> S;
  const uint32_t gi = blockIdx.x * WG + threadIdx.x;
  if (gi >= ngrp) return;
  const uint32_t b = grp_off[gi], e = grp_off[gi + 1];
  typename S::pt acc, v;
  S::inf(acc);
#pragma unroll 1
  for (uint32_t j = b; j < e; j++) {
    S::load(v, Pset[grp_set[j]]);
    S::add(acc, v);
  }
  g1s o;
  S::store(o, acc);
  P[gi] = o;
}

// One wave per group (a 64-set gossip group, a 512-set sync-committee group): lane l sums the
// members l, l + 64, ..., then a tree through LDS joins the lanes, starting at the first level
// that has two operands (a group of g <= 64 sets costs ceil(log2 g) additions).  The LDS points
// lie kWords + 1 words apart when kWords is even: an odd stride, so that the 32 lanes of a store
// or load group fall on 32 different banks.
template <bool R28>
__global__ void __launch_bounds__(WG) k_g1s_msgsum_wave(const g1s *Pset, const uint32_t *grp_off,
                                                        const uint32_t *grp_set, uint32_t ngrp, g1s *P) {
  typedef Sum<R28> S;
  constexpr int kStride = S::kWords | 1;
  __shared__ uint32_t sh[(WG / 2) * kStride];
  const uint32_t gi = blockIdx.x, lane = threadIdx.x;
  if (gi >= ngrp) return;  // block-uniform (grid = ngrp)
  const uint32_t b = grp_off[gi], e = grp_off[gi + 1], cnt = e - b;
  typename S::pt acc, v;
  S::inf(acc);
#pragma unroll 1
  for (uint32_t j = b + lane; j < e; j += WG) {
    S::load(v, Pset[grp_set[j]]);
    S::add(acc, v);
  }
  uint32_t width = WG / 2;
  while (width >= cnt && width > 0) width >>= 1;  // lanes >= cnt hold infinity
#pragma unroll 1
  for (; width > 0; width >>= 1) {
    __syncthreads();
    if (lane >= width && lane < 2 * width) {
      uint32_t *d = sh + (lane - width) * kStride;
#pragma unroll
      for (int k = 0; k < S::kWords; k++) d[k] = S::word(acc, k);
    }
    __syncthreads();
    if (lane < width) {
      const uint32_t *d = sh + lane * kStride;
#pragma unroll
      for (int k = 0; k < S::kWords; k++) S::word(v, k) = d[k];
      S::add(acc, v);
    }
  }
  if (lane != 0) return;
  g1s o;
  S::store(o, acc);
  P[gi] = o;
}

void launch_g1s_msgsum(hipStream_t st, const g1s *Pset, const uint32_t *grp_off, const uint32_t *grp_set,
                       uint32_t ngrp, uint32_t max_group, g1s *P) {
  if (!ngrp) return;
  const bool wave = max_group >= g_msgsum_wave_min;
  if (wave && g_lane_r28)
    k_g1s_msgsum_wave<true><<<ngrp, WG, 0, st>>>(Pset, grp_off, grp_set, ngrp, P);
  else if (wave)
    k_g1s_msgsum_wave<false><<<ngrp, WG, 0, st>>>(Pset, grp_off, grp_set, ngrp, P);
  else if (g_lane_r28)
    k_g1s_msgsum<true><<<nblk(ngrp), WG, 0, st>>>(Pset, grp_off, grp_set, ngrp, P);
  else
    k_g1s_msgsum<false><<<nblk(ngrp), WG, 0, st>>>(Pset, grp_off, grp_set, ngrp, P);
}

}  // namespace gbls
