// gfx950 kernels: the random linear combination S = sum_i r_i sig_i of
// Signature::multi_verify (bls/src/signature.rs:117-126; blst accumulates it with one
// 64-bit POINTonE2_mult_w5 per set) as a bucket (Pippenger) multi-scalar multiplication,
// per segment of batches whose segments hold >= kMsmMinPerSeg sets (the C5-scale shards,
// coalesced C2 batches), where it replaces the per-set double-and-add of k_mv_g2mul and
// the chunk sums of k_g2sum: about W mixed additions per set instead of 64 doublings +
// 32 additions.
//
// Signed c-bit digits, W = 65 / c windows, B = 2^(c-1) buckets per window and segment
// (digit d != 0 adds sign(d) sig into bucket |d| - 1 of its segment's window):
//   1 k_msm_count    lane per set: bucket histogram (atomics), segment error flags
//   2 k_msm_scan     one workgroup: bucket starts, chunk starts (K entries per chunk), and
//                    per fold level l the bucket's pair starts (2^(l+1) chunks per pair)
//   3 k_msm_scatter  lane per set: (set | sign) into its buckets' lists
//   4 k_msm_chunk    lane per chunk: sum of <= K affine points (mixed additions), one partial
//   4b k_msm_fold    kMsmFoldLevels launches, lane per pair of one bucket's partials at
//                    level l: partial[j] += partial[j + 2^l] (full Jacobian additions), so
//                    each run of kMsmFold partials ends summed in its first; the bucket's
//                    reader adds the runs' sums (k_msm_windows_w4, msm_bucket_sum)
// (r05: the chunk kernel no longer folds its wave's partials through LDS -- log2(run) levels
// of additions at whole-wave cost with most lanes masked off; the fold levels are their own
// launches, every lane one addition, so K can be small: GBLS_MSM_K = 8 gives ~1.7k chunk
// waves against 884 at K = 16, VERDICT r04 item 4, at the same C2 rate)
// The window sums never go through a Horner chain of 60 doublings.  The window weights move
// to the G1 side of the pairing instead, where they are constants:
//   e(-g1, S) = prod_w e(-[2^(c w)] g1, S_w),   S_w = sum_b (b + 1) X_{w,b},
// so every window becomes one extra Miller pair of its segment, with a precomputed G1 point
// (bls_constants.h MSM_W5 entry 16 w / MSM_W13 entry w, tools/gen_constants.py).  With c = 5
// that is 13 pairs per segment, and the bucket weights (b + 1) are folded on the wave engine:
//   5 k_msm_windows_w4  (k_msm_w4.hip) workgroup per (segment, window): the buckets' partials
//                    added up and S_w by running sums, Jacobian for k_lines_w4j (or affine)
// (until r06 every bucket sum was a pair of its own, paired with -[(b+1) 2^(c w)] g1: 208
// pairs per segment whose lines ran 16 lanes per point on the whole GPU)
// With c = 13 (segments >= 2^16 sets, 4096 buckets per window) a per-window tree
// folds the weights (b + 1) into S_w:
//   5 k_msm_bucket   level-0 tree nodes (the buckets' partials added up)
//   6 k_msm_tree     per (segment, window), a binary tree over the buckets computing
//                    S_w = sum_b (b+1) X_b with nodes (T = sum X, A = sum (b - lo) X):
//                    T = T_L + T_R, A = A_L + A_R + 2^l T_R   (l = level)
//   7 k_msm_wpairs   lane per window: affine S_w = A + T, its pair
// Infinite signatures and zero scalars contribute nothing (blst skips infinite
// signatures; a zero scalar fails the batch through k_msm_count's flags).  An empty window sums
// to the point at infinity, whose Miller pair is the identity.  Bucket order is
// nondeterministic (atomics) but the sums are exact, so the verdict is too.
//
// r06: the chunk sums and the fold levels run in radix 2^28 (k_msm_chunk28 / k_msm_fold28,
// bls_curve28.h's lazy jac_add_aff28 / jac_add28): k_msm_count writes each scattered
// signature once in radix 2^28 (4 conversion products per set, against ~13 additions of it),
// partials are stored as radix-2^28 limbs in the engine layout (store12), and the bucket
// readers convert them: k_msm_windows_w4 straight to the wave engine's row form (w4::load28),
// k_msm_bucket back to engine form.
#include "gbls_common.h"
#include "k_msm.h"
#include "bls_gang.h"
#include "bls_curve28.h"

namespace gbls {


__device__ __forceinline__ int msm_digit(uint64_t k, int w, int c, uint32_t &carry) {
  uint64_t raw = (c * w < 64) ? (k >> (c * w)) & ((1ull << c) - 1) : 0;
  int d = (int)raw + (int)carry;
  if (d > (1 << (c - 1))) {
    d -= 1 << c;
    carry = 1;
  } else {
    carry = 0;
  }
  return d;
}
// segment of set i: the largest s with seg_off[s] <= i (seg_off has nseg + 1 entries)
__device__ __forceinline__ uint32_t msm_segment(const uint32_t *seg_off, uint32_t nseg, uint32_t i) {
  uint32_t lo = 0, hi = nseg;
  while (hi - lo > 1) {
    uint32_t mid = (lo + hi) >> 1;
    if (seg_off[mid] <= i)
      lo = mid;
    else
      hi = mid;
  }
  return lo;
}

// also the per-segment error flags: an infinite key, a zero scalar or a failed
// pre-check (key aggregation / signature group check) fails the set's segment
__global__ void __launch_bounds__(WGR) k_msm_count(const g2a *sigs, const uint64_t *rands, uint32_t n,
                                                   const uint32_t *seg_off, uint32_t nseg, int c,
                                                   int W, const g1a *pks, const int32_t *pre,
                                                   const int32_t *pre2, uint32_t *cnt,
                                                   int32_t *seg_err, g2a *sig28) {
  uint32_t i = blockIdx.x * WGR + threadIdx.x;
  if (i >= n) return;
  uint64_t k = rands[i];
  const uint32_t s = msm_segment(seg_off, nseg, i);
  if (aff_is_inf(pks[i]) || k == 0 || (pre && pre[i] != 0) || (pre2 && pre2[i] != 0))
    atomicOr(&seg_err[s], 1);
  const g2a sg = sigs[i];
  if (k == 0 || aff_is_inf(sg)) return;
  if (sig28) {  // the signature in radix 2^28 for k_msm_chunk28 (every scattered set)
    r28::g2a28 a;
    r28::from_fp(a.x.c0, sg.x.c0), r28::from_fp(a.x.c1, sg.x.c1);
    r28::from_fp(a.y.c0, sg.y.c0), r28::from_fp(a.y.c1, sg.y.c1);
    r28::g2a_store12(sig28[i], a);
  }
  const uint32_t B = 1u << (c - 1);
  const uint32_t base = s * (uint32_t)W * B;
  uint32_t carry = 0;
  for (int w = 0; w < W; w++) {
    int d = msm_digit(k, w, c, carry);
    if (d) atomicAdd(&cnt[base + w * B + (uint32_t)(d < 0 ? -d : d) - 1], 1u);
  }
}

// one workgroup of 1024 lanes: start[b] (exclusive scan of cnt), cur = start,
// cstart[b] (exclusive scan of ceil(cnt / K)), fstart[l][b] (exclusive scan of the bucket's
// level-l fold pairs, floor((ceil(cnt / K) + 2^l - 1) / 2^(l+1)) -- pairs whose second
// partial exists); start/cstart/fstart[l] have nb + 1 entries
struct MsmFoldStarts {
  uint32_t *l[kMsmFoldLevels];
};
__global__ void __launch_bounds__(1024) k_msm_scan(const uint32_t *cnt, uint32_t nb, uint32_t K,
                                                   uint32_t *start, uint32_t *cur,
                                                   uint32_t *cstart, MsmFoldStarts fs) {
  constexpr int NS = 2 + kMsmFoldLevels;
  __shared__ uint32_t sv[NS][1024];
  __shared__ uint32_t base[NS];
  if (threadIdx.x < NS) base[threadIdx.x] = 0;
  __syncthreads();
  for (uint32_t off = 0; off < nb; off += 1024) {
    uint32_t b = off + threadIdx.x;
    uint32_t v[NS];
    v[0] = b < nb ? cnt[b] : 0;
    v[1] = (v[0] + K - 1) / K;
#pragma unroll
    for (int l = 0; l < kMsmFoldLevels; l++) v[2 + l] = (v[1] + (1u << l) - 1) >> (l + 1);
#pragma unroll
    for (int q = 0; q < NS; q++) sv[q][threadIdx.x] = v[q];
    __syncthreads();
    for (uint32_t d = 1; d < 1024; d <<= 1) {  // inclusive Hillis-Steele scans
      uint32_t x[NS];
#pragma unroll
      for (int q = 0; q < NS; q++) x[q] = threadIdx.x >= d ? sv[q][threadIdx.x - d] : 0;
      __syncthreads();
#pragma unroll
      for (int q = 0; q < NS; q++) sv[q][threadIdx.x] += x[q];
      __syncthreads();
    }
    if (b < nb) {
      const uint32_t sa = base[0] + sv[0][threadIdx.x] - v[0];
      start[b] = sa;
      cur[b] = sa;
      cstart[b] = base[1] + sv[1][threadIdx.x] - v[1];
#pragma unroll
      for (int l = 0; l < kMsmFoldLevels; l++) fs.l[l][b] = base[2 + l] + sv[2 + l][threadIdx.x] - v[2 + l];
    }
    __syncthreads();
    if (threadIdx.x < NS) base[threadIdx.x] += sv[threadIdx.x][1023];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    start[nb] = base[0];
    cstart[nb] = base[1];
#pragma unroll
    for (int l = 0; l < kMsmFoldLevels; l++) fs.l[l][nb] = base[2 + l];
  }
}

__global__ void __launch_bounds__(WGR) k_msm_scatter(const g2a *sigs, const uint64_t *rands,
                                                     uint32_t n, const uint32_t *seg_off,
                                                     uint32_t nseg, int c, int W, uint32_t *cur,
                                                     uint32_t *list) {
  uint32_t i = blockIdx.x * WGR + threadIdx.x;
  if (i >= n) return;
  uint64_t k = rands[i];
  if (k == 0 || aff_is_inf(sigs[i])) return;
  const uint32_t B = 1u << (c - 1);
  const uint32_t base = msm_segment(seg_off, nseg, i) * (uint32_t)W * B;
  uint32_t carry = 0;
  for (int w = 0; w < W; w++) {
    int d = msm_digit(k, w, c, carry);
    if (!d) continue;
    uint32_t pos = atomicAdd(&cur[base + w * B + (uint32_t)(d < 0 ? -d : d) - 1], 1u);
    list[pos] = i | (d < 0 ? 0x80000000u : 0u);
  }
}

// the largest b with tab[b] <= j (tab has nb + 1 nondecreasing entries, tab[0] = 0)
__device__ __forceinline__ uint32_t msm_owner(const uint32_t *tab, uint32_t nb, uint32_t j) {
  uint32_t lo = 0, hi = nb;
  while (hi - lo > 1) {
    uint32_t mid = (lo + hi) >> 1;
    if (tab[mid] <= j)
      lo = mid;
    else
      hi = mid;
  }
  return lo;
}

// chunk j: sum of <= K affine points of one bucket (found by binary search over cstart), one
// partial per chunk
__global__ void __launch_bounds__(WG) k_msm_chunk(const g2a *sigs, const uint32_t *list,
                                                  const uint32_t *start, const uint32_t *cstart,
                                                  uint32_t nb, uint32_t max_chunks, uint32_t K,
                                                  g2j *chunk) {
  const uint32_t j = blockIdx.x * WG + threadIdx.x;
  if (j >= max_chunks || j >= cstart[nb]) return;
  const uint32_t b = msm_owner(cstart, nb, j);
  const uint32_t e0 = start[b] + (j - cstart[b]) * K;
  const uint32_t e1 = min(e0 + K, start[b + 1]);
  g2j acc;
  jac_set_inf(acc);
  // the next point's loads are issued before this point's addition: at one wave per SIMD the
  // chain otherwise waits on every random-address load
  uint32_t vn = list[e0];
  g2a pn = sigs[vn & 0x7fffffffu];
  for (uint32_t e = e0; e < e1; e++) {
    const uint32_t v = vn;
    g2a p = pn;
    if (e + 1 < e1) {
      vn = list[e + 1];
      pn = sigs[vn & 0x7fffffffu];
    }
    if (v >> 31) fp2_neg(p.y, p.y);
    jac_add_aff(acc, acc, p);
  }
  chunk[j] = acc;
}

// fold level l, pair t of bucket b = owner: partial[j] += partial[j + 2^l] for
// j = cstart[b] + (t - fstart[b]) 2^(l+1) (only pairs whose second partial exists are counted)
__global__ void __launch_bounds__(WG) k_msm_fold(const uint32_t *cstart, const uint32_t *fstart,
                                                 uint32_t nb, uint32_t max_pairs, int l,
                                                 g2j *chunk) {
  const uint32_t t = blockIdx.x * WG + threadIdx.x;
  if (t >= max_pairs || t >= fstart[nb]) return;
  const uint32_t b = msm_owner(fstart, nb, t);
  const uint32_t j = cstart[b] + ((t - fstart[b]) << (l + 1));
  g2j x = chunk[j], y = chunk[j + (1u << l)];
  jac_add(x, x, y);
  chunk[j] = x;
}

// k_msm_chunk in radix 2^28: the bucket's points from sig28 (radix-2^28 limbs, never infinite:
// k_msm_scatter lists finite signatures only), the partial stored as radix-2^28 limbs
__global__ void __launch_bounds__(WG) k_msm_chunk28(const g2a *sig28, const uint32_t *list,
                                                    const uint32_t *start, const uint32_t *cstart,
                                                    uint32_t nb, uint32_t max_chunks, uint32_t K,
                                                    g2j *chunk) {
  const uint32_t j = blockIdx.x * WG + threadIdx.x;
  if (j >= max_chunks || j >= cstart[nb]) return;
  const uint32_t b = msm_owner(cstart, nb, j);
  const uint32_t e0 = start[b] + (j - cstart[b]) * K;
  const uint32_t e1 = min(e0 + K, start[b + 1]);
  r28::g2j28 acc;
  uint32_t vn = list[e0];
  g2a pn = sig28[vn & 0x7fffffffu];
  for (uint32_t e = e0; e < e1; e++) {
    const uint32_t v = vn;
    r28::g2a28 q;
    r28::g2a_load12(q, pn);
    if (e + 1 < e1) {
      vn = list[e + 1];
      pn = sig28[vn & 0x7fffffffu];
    }
    if (v >> 31) r28::f_neg(q.y, q.y);
    if (e == e0) {
      acc.x = q.x;
      acc.y = q.y;
      r28::f_one(acc.z);
    } else {
      r28::jac_add_aff28<false>(acc, acc, q);
    }
  }
  r28::g2j_store12(chunk[j], acc);
}
__global__ void __launch_bounds__(WG) k_msm_fold28(const uint32_t *cstart, const uint32_t *fstart,
                                                   uint32_t nb, uint32_t max_pairs, int l,
                                                   g2j *chunk) {
  const uint32_t t = blockIdx.x * WG + threadIdx.x;
  if (t >= max_pairs || t >= fstart[nb]) return;
  const uint32_t b = msm_owner(fstart, nb, t);
  const uint32_t j = cstart[b] + ((t - fstart[b]) << (l + 1));
  r28::g2j28 x, y;
  r28::g2j_load12(x, chunk[j]);
  r28::g2j_load12(y, chunk[j + (1u << l)]);
  jac_add(x, x, y);
  r28::g2j_store12(chunk[j], x);
}

// sum of bucket b: its fold groups' sums (k_msm_fold), at every kMsmFold-th chunk partial of
// the bucket's chunk range
// (R28: the partials are radix-2^28 limbs, summed in radix 2^28 and converted to engine form)
template <bool R28>
__device__ __forceinline__ void msm_bucket_sum(g2j &x, const g2j *chunk, const uint32_t *cstart,
                                               uint32_t b) {
  const uint32_t c0 = cstart[b], c1 = cstart[b + 1];
  if (c1 == c0) {
    jac_set_inf(x);
    return;
  }
  if constexpr (R28) {
    r28::g2j28 s, y;
    r28::g2j_load12(s, chunk[c0]);
    for (uint32_t w = c0 + kMsmFold; w < c1; w += kMsmFold) {
      r28::g2j_load12(y, chunk[w]);
      jac_add(s, s, y);
    }
    r28::g2j_out(x, s);
  } else {
    x = chunk[c0];
    for (uint32_t w = c0 + kMsmFold; w < c1; w += kMsmFold) {
      g2j y = chunk[w];
      jac_add(x, x, y);
    }
  }
}

// level-0 tree nodes: T = X_b (the bucket's folded first chunk, or infinity), A = inf
template <bool R28>
__global__ void __launch_bounds__(WG) k_msm_bucket(const g2j *chunk, const uint32_t *cstart,
                                                   uint32_t nb, g2j *T, g2j *A) {
  uint32_t b = blockIdx.x * WG + threadIdx.x;
  if (b >= nb) return;
  g2j x, inf;
  msm_bucket_sum<R28>(x, chunk, cstart, b);
  jac_set_inf(inf);
  T[b] = x;
  A[b] = inf;
}

// tree level l: nodes (T, A) of ranges of 2^l buckets -> ranges of 2^(l+1); per
// (segment, window) group g the level has m = B >> (l+1) output nodes: inputs at
// g * 2m + 2q (+1), output at g * m + q.
__global__ void __launch_bounds__(WG) k_msm_tree(const g2j *Tin, const g2j *Ain, uint32_t groups,
                                                 uint32_t m, int l, g2j *Tout, g2j *Aout) {
  uint32_t t = blockIdx.x * WG + threadIdx.x;
  if (t >= groups * m) return;
  uint32_t g = t / m, k2 = t % m;
  size_t li = (size_t)g * 2 * m + 2 * k2;
  g2j TL = Tin[li], TR = Tin[li + 1], AL = Ain[li], AR = Ain[li + 1];
  jac_add(AL, AL, AR);
  g2j x = TR;
  for (int i = 0; i < l; i++) jac_dbl(x, x);
  jac_add(AL, AL, x);
  jac_add(TL, TL, TR);
  Tout[t] = TL;
  Aout[t] = AL;
}

// c = 13: lane per (segment, window) t = s * W + w: S_w = A_w + T_w (weights b + 1),
// affine, paired with -[2^(c w)] g1 at pair n + t
__global__ void __launch_bounds__(WG) k_msm_wpairs(const g2j *T, const g2j *A, uint32_t nw,
                                                   uint32_t W, uint32_t n, const uint32_t *seg_off,
                                                   int empty_is_error, g1s *P, g2a *H,
                                                   int32_t *seg_err) {
  uint32_t t = blockIdx.x * WG + threadIdx.x;
  if (t >= nw) return;
  uint32_t s = t / W, w = t % W;
  g2j a = A[t], b = T[t];
  jac_add(a, a, b);
  g2a o;
  jac_to_aff(o, a);
  g1s g;
  msm_weight(g, k::MSM_W13, w);
  P[n + t] = g;
  H[n + t] = o;
  if (w == 0 && empty_is_error && seg_off[s + 1] == seg_off[s]) atomicOr(&seg_err[s], 1);
}

// ---------------------------------------------------------------- host side
// Window widths dividing 65 (64-bit scalars + the signed-digit carry), so that no window
// is nearly empty (a 2-bit top window would pile every set into two buckets): c = 5
// (13 windows, 16 buckets each, summed per window on the wave engine) for segments up to 2^16
// sets, else c = 13 (5 windows of 4096 buckets, per-window trees); one pair per window.
MsmPlan msm_plan(uint32_t n, uint32_t nseg) {
  uint32_t avg = nseg ? n / nseg : n;
  MsmPlan p;
  p.nseg = nseg;
  p.c = avg >= (1u << 16) ? 13 : 5;
  p.W = 65 / p.c;
  p.tree = p.c == 13;
  p.extra = (uint32_t)p.W;
  p.nb = nseg * ((uint32_t)p.W << (p.c - 1));
  // chunks of <= K points (GBLS_MSM_K; else kMsmChunkSmall below 4096 sets per segment,
  // kMsmChunk from there), fold groups of kMsmFold chunk partials
  p.K = g_msm_k ? g_msm_k : (avg < 4096 ? kMsmChunkSmall : kMsmChunk);
  p.max_chunks = (uint32_t)(((uint64_t)p.W * n + p.K - 1) / p.K) + p.nb;
  p.max_folds = p.max_chunks / 2 + p.nb;
  size_t o = 0;
  auto take = [&](size_t bytes) {
    size_t at = o;
    o += (bytes + 255) & ~(size_t)255;
    return at;
  };
  p.o_cnt = take(p.nb * 4);
  p.o_start = take((p.nb + 1) * 4);
  p.o_cur = take(p.nb * 4);
  p.o_cstart = take((p.nb + 1) * 4);
  for (int l = 0; l < kMsmFoldLevels; l++) p.o_fstart[l] = take((p.nb + 1) * 4);
  p.o_list = take((size_t)p.W * n * 4);
  p.o_chunk = take((size_t)p.max_chunks * sizeof(g2j));
  const size_t tn = p.tree ? p.nb : 0;
  p.o_t0 = take(tn * sizeof(g2j));
  p.o_a0 = take(tn * sizeof(g2j));
  p.o_t1 = take((tn / 2 + 1) * sizeof(g2j));
  p.o_a1 = take((tn / 2 + 1) * sizeof(g2j));
  p.r28 = g_msm_r28 != 0;
  p.o_sig28 = take(p.r28 ? (size_t)n * sizeof(g2a) : 0);
  p.bytes = o;
  return p;
}

void launch_msm(hipStream_t st, const MsmPlan &p, uint8_t *ws, const g2a *sigs,
                const uint64_t *rands, const g1a *pks, const int32_t *pre, const int32_t *pre2,
                uint32_t n, const uint32_t *seg_off, int empty_is_error, g2a *H, g1s *P,
                int32_t *seg_err, uint32_t xbase, g2j *Sj) {
  // the pair kernels' `n` is only the index of the first extra pair
  const uint32_t xb = xbase == NONE ? n : xbase;
  uint32_t *cnt = reinterpret_cast<uint32_t *>(ws + p.o_cnt);
  uint32_t *start = reinterpret_cast<uint32_t *>(ws + p.o_start);
  uint32_t *cur = reinterpret_cast<uint32_t *>(ws + p.o_cur);
  uint32_t *cstart = reinterpret_cast<uint32_t *>(ws + p.o_cstart);
  MsmFoldStarts fs;
  for (int l = 0; l < kMsmFoldLevels; l++) fs.l[l] = reinterpret_cast<uint32_t *>(ws + p.o_fstart[l]);
  uint32_t *list = reinterpret_cast<uint32_t *>(ws + p.o_list);
  g2j *chunk = reinterpret_cast<g2j *>(ws + p.o_chunk);
  (void)hipMemsetAsync(cnt, 0, p.nb * 4, st);
  (void)hipMemsetAsync(seg_err, 0, p.nseg * 4, st);
  g2a *sig28 = p.r28 ? reinterpret_cast<g2a *>(ws + p.o_sig28) : nullptr;
  k_msm_count<<<nblk(n, WGR), WGR, 0, st>>>(sigs, rands, n, seg_off, p.nseg, p.c, p.W, pks, pre,
                                            pre2, cnt, seg_err, sig28);
  k_msm_scan<<<1, 1024, 0, st>>>(cnt, p.nb, p.K, start, cur, cstart, fs);
  k_msm_scatter<<<nblk(n, WGR), WGR, 0, st>>>(sigs, rands, n, seg_off, p.nseg, p.c, p.W, cur,
                                              list);
  if (p.r28)
    k_msm_chunk28<<<nblk(p.max_chunks), WG, 0, st>>>(sig28, list, start, cstart, p.nb, p.max_chunks,
                                                     p.K, chunk);
  else
    k_msm_chunk<<<nblk(p.max_chunks), WG, 0, st>>>(sigs, list, start, cstart, p.nb, p.max_chunks,
                                                   p.K, chunk);
  for (int l = 0; l < kMsmFoldLevels; l++) {
    const uint32_t mp = (p.max_folds >> l) + p.nb;
    if (p.r28)
      k_msm_fold28<<<nblk(mp), WG, 0, st>>>(cstart, fs.l[l], p.nb, mp, l, chunk);
    else
      k_msm_fold<<<nblk(mp), WG, 0, st>>>(cstart, fs.l[l], p.nb, mp, l, chunk);
  }
  if (!p.tree) {
    launch_msm_windows_w4(st, chunk, cstart, p.nseg * (uint32_t)p.W, (uint32_t)p.W, p.r28, xb, seg_off,
                          empty_is_error, P, H, seg_err, Sj);
    return;
  }
  g2j *T[2] = {reinterpret_cast<g2j *>(ws + p.o_t0), reinterpret_cast<g2j *>(ws + p.o_t1)};
  g2j *A[2] = {reinterpret_cast<g2j *>(ws + p.o_a0), reinterpret_cast<g2j *>(ws + p.o_a1)};
  if (p.r28)
    k_msm_bucket<true><<<nblk(p.nb), WG, 0, st>>>(chunk, cstart, p.nb, T[0], A[0]);
  else
    k_msm_bucket<false><<<nblk(p.nb), WG, 0, st>>>(chunk, cstart, p.nb, T[0], A[0]);
  int src = 0;
  const uint32_t B = 1u << (p.c - 1), groups = p.nseg * (uint32_t)p.W;
  for (int l = 0; (1u << (l + 1)) <= B; l++) {
    uint32_t m = B >> (l + 1);
    k_msm_tree<<<nblk((size_t)groups * m), WG, 0, st>>>(T[src], A[src], groups, m, l, T[1 - src],
                                                         A[1 - src]);
    src = 1 - src;
  }
  k_msm_wpairs<<<nblk(groups), WG, 0, st>>>(T[src], A[src], groups, (uint32_t)p.W, xb, seg_off,
                                            empty_is_error, P, H, seg_err);
}

}  // namespace gbls
