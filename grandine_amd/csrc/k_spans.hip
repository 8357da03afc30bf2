// gfx950 kernels: per-set keys of span sets (gbls_multi_verify_spans, gbls_g1_aggregate_spans).
// An attestation since EIP-7549 is (committee_bits, one aggregation bit string over the named
// committees, signature): up to 64 committees of about 500 members per set and 8 such sets in a
// block.  One lane or one row per SET would leave a block's keys to 8 chains of 64 committees
// each, so the work is cut into PIECES, one per (set, committee) pair (gbls_spans.h):
//   k_g1_span_pieces  one lane or one 16-lane row per piece: its committee's contribution
//                     C - S, S or C, in that committee's cheaper direction, as a Jacobian point
//   k_g1_span_keys    one lane or one row per set: the string checked over all M members, the
//                     pieces' flags ORed, their contributions folded, one inversion
//
// Radix-32 arithmetic as k_g1_bits_keys: the registry is stored in that form and the affine bytes
// equal those of every other key path.
#include "gbls_common.h"
#include "gbls_spans.h"
#include "gbls_rowfold.h"

namespace gbls {

// ROW = false: one lane per piece.  ROW = true: one 16-lane DPP row per piece, lane r taking
// members j = r (mod 16) of the committee (list entries for a plain piece), folded as in
// k_g1_bits_keys; the row's lane 0 writes the contribution.  Every lane of a row counts the
// committee's whole window, so the direction is the same in all 16 lanes without an exchange.
template <bool ROW>
__global__ void __launch_bounds__(WG) k_g1_span_pieces(const g1a *reg, uint32_t nreg, const g1a *tab,
                                                       uint32_t ntab, const SpanPiece *pieces,
                                                       const SpanSet *sets, const uint32_t *rows, uint32_t np,
                                                       g1j *contrib, uint32_t *pflags) {
  const uint32_t t = blockIdx.x * WG + threadIdx.x;
  const uint32_t q = ROW ? t >> 4 : t, r = ROW ? t & 15 : 0, lanes = ROW ? 16 : 1;
  if (q >= np) return;  // whole rows
  const SpanPiece d = pieces[q];
  const bool committee = d.slot != kNoCommittee;
  const uint32_t m = d.list ? d.cnt : 0;
  const uint32_t *row = rows;
  uint32_t nw = 0, p = 0;
  bool subtract = false;
  if (committee) {
    const SpanSet s = sets[d.set];
    row = rows + s.row;
    nw = bits_row_words(s.nbytes);
    p = span_count(row, nw, d.bit, m);
    subtract = committee_subtracts(m, p);
  }
  // a committee piece walks the words of its window (each lane its own bits of every word), a
  // plain piece its list
  const uint32_t end = committee ? (m + 31) / 32 : m, step = committee ? 1 : lanes;
  uint32_t bad = 0;
  g1j acc;
  jac_set_inf(acc);
#pragma unroll 1
  for (uint32_t i = committee ? 0 : r; i < end; i += step) {
    uint32_t sel = committee ? bits_select(span_window(row, nw, d.bit, i), m, i, subtract, r, lanes) : 1u;
    const uint32_t base = committee ? 32 * i : i;
#pragma unroll 1
    while (sel) {
      const uint32_t v = d.list[base + bits_ctz(sel)];
      sel &= sel - 1;
      if (v >= nreg || aff_is_inf(reg[v]))  // out of range / invalid slot
        bad = 1;
      else
        jac_add_aff(acc, acc, reg[v]);
    }
  }
  if constexpr (ROW) {  // whole rows reach every fold, whatever their lanes added
    jac_row_fold<1>(acc, bad);
    jac_row_fold<2>(acc, bad);
    jac_row_fold<4>(acc, bad);
    jac_row_fold<8>(acc, bad);
    if (r != 0) return;
  }
  uint32_t flags;
  if (committee) {
    g1a C;
    fp_zero(C.x);
    fp_zero(C.y);
    if (d.slot < ntab) C = tab[d.slot];  // past the table: stays all-zero, an invalid slot
    g1j out;
    flags = span_contribution(out, C, acc, d.list != nullptr, subtract, p, bad);
    acc = out;
  } else {
    flags = SP_PLAIN | (bad ? SP_BAD_INDEX : 0u) | (m == 0 ? SP_EMPTY : 0u);
  }
  contrib[q] = acc;
  pflags[q] = flags;
}

// ROW = false: one lane per set.  ROW = true: one 16-lane row per set, lane r folding the set's
// pieces first + r (mod 16); lane 0 checks the set's string and finishes.  The folds
// are the complete addition: twin committees double, opposite contributions cancel.
template <bool ROW>
__global__ void __launch_bounds__(WG) k_g1_span_keys(const SpanSet *sets, const uint32_t *rows,
                                                     const g1j *contrib, const uint32_t *pflags, uint32_t n,
                                                     g1a *out, int32_t *st) {
  const uint32_t t = blockIdx.x * WG + threadIdx.x;
  const uint32_t s = ROW ? t >> 4 : t, r = ROW ? t & 15 : 0, lanes = ROW ? 16 : 1;
  if (s >= n) return;  // whole rows
  const SpanSet d = sets[s];
  uint32_t flags = 0;
  g1j acc;
  jac_set_inf(acc);
#pragma unroll 1
  for (uint32_t i = r; i < d.npieces; i += lanes) {
    flags |= pflags[d.first + i];
    jac_add(acc, acc, contrib[d.first + i]);
  }
  if constexpr (ROW) {
    jac_row_fold<1>(acc, flags);
    jac_row_fold<2>(acc, flags);
    jac_row_fold<4>(acc, flags);
    jac_row_fold<8>(acc, flags);
    if (r != 0) return;
  }
  uint32_t p = 0;
  const bool ok = (flags & SP_PLAIN) || bits_check(rows + d.row, d.nbytes, d.M, &p);
  g1a key;
  st[s] = span_key(key, acc, d.npieces, flags, ok);
  out[s] = key;
}

void launch_g1_span_keys(hipStream_t st, const g1a *reg, uint32_t nreg, const g1a *tab, uint32_t ntab,
                         const void *pieces, const void *sets, const uint32_t *rows, uint32_t np, uint32_t n,
                         uint32_t max_work, uint32_t max_pieces, void *contrib, uint32_t *pflags, g1a *out,
                         int32_t *status) {
  if (!n) return;
  constexpr uint32_t kRowFormMax = 1u << 28;  // 16 lanes per item: the thread index stays 32-bit
  const SpanPiece *pp = static_cast<const SpanPiece *>(pieces);
  const SpanSet *ss = static_cast<const SpanSet *>(sets);
  g1j *cj = static_cast<g1j *>(contrib);
  if (np) {
    if (max_work >= g_committee_row_min && np < kRowFormMax)
      k_g1_span_pieces<true><<<nblk(16 * (size_t)np), WG, 0, st>>>(reg, nreg, tab, ntab, pp, ss, rows, np, cj, pflags);
    else
      k_g1_span_pieces<false><<<nblk(np), WG, 0, st>>>(reg, nreg, tab, ntab, pp, ss, rows, np, cj, pflags);
  }
  if (max_pieces >= kSpanFoldRowMin && n < kRowFormMax)
    k_g1_span_keys<true><<<nblk(16 * (size_t)n), WG, 0, st>>>(ss, rows, cj, pflags, n, out, status);
  else
    k_g1_span_keys<false><<<nblk(n), WG, 0, st>>>(ss, rows, cj, pflags, n, out, status);
}

// Local key sets (gbls_local.h): the head pieces [0, np - np_local) read the registry, the tail
// reads the call's own table; a set's pieces lie wholly in one of the two, and the finish runs over
// all sets as it does above.
void launch_g1_span_keys_local(hipStream_t st, const g1a *reg, uint32_t nreg, const g1a *tab, uint32_t ntab,
                               const g1a *loc, uint32_t nloc, const void *pieces, const void *sets,
                               const uint32_t *rows, uint32_t np, uint32_t np_local, uint32_t n, uint32_t max_work,
                               uint32_t max_work_local, uint32_t max_pieces, void *contrib, uint32_t *pflags,
                               g1a *out, int32_t *status) {
  if (!n) return;
  constexpr uint32_t kRowFormMax = 1u << 28;
  const SpanPiece *pp = static_cast<const SpanPiece *>(pieces);
  const SpanSet *ss = static_cast<const SpanSet *>(sets);
  g1j *cj = static_cast<g1j *>(contrib);
  auto run = [&](const g1a *keys, uint32_t nkeys, uint32_t first, uint32_t cnt, uint32_t work) {
    if (!cnt) return;
    if (work >= g_committee_row_min && cnt < kRowFormMax)
      k_g1_span_pieces<true><<<nblk(16 * (size_t)cnt), WG, 0, st>>>(keys, nkeys, tab, ntab, pp + first, ss, rows, cnt,
                                                                   cj + first, pflags + first);
    else
      k_g1_span_pieces<false><<<nblk(cnt), WG, 0, st>>>(keys, nkeys, tab, ntab, pp + first, ss, rows, cnt, cj + first,
                                                        pflags + first);
  };
  run(reg, nreg, 0, np - np_local, max_work);
  run(loc, nloc, np - np_local, np_local, max_work_local);
  if (max_pieces >= kSpanFoldRowMin && n < kRowFormMax)
    k_g1_span_keys<true><<<nblk(16 * (size_t)n), WG, 0, st>>>(ss, rows, cj, pflags, n, out, status);
  else
    k_g1_span_keys<false><<<nblk(n), WG, 0, st>>>(ss, rows, cj, pflags, n, out, status);
}

}  // namespace gbls
