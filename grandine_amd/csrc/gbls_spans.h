// Span sets: the per-piece and per-set steps of k_g1_span_pieces and k_g1_span_keys (k_spans.hip),
// as __host__ __device__ text so that tests/native/spans_harness.cpp compiles the same lines for
// the CPU.
//
// Since EIP-7549 an attestation names up to 64 committees (committee_bits) and carries ONE bit
// string, the concatenation of the named committees' aggregation bits in ascending committee
// order.  The unit of work is a PIECE: one (set, committee) pair, or a plain set's index list.  The
// host resolves committee_bits to pieces (span_pieces below); a piece reads its window of the set's
// repacked bit row (gbls_bits.h) at an arbitrary bit offset and contributes C - S, S or C as a
// Jacobian point, in the direction committee_subtracts picks for ITS committee; the set's key is
// the fold of its pieces' contributions, one inversion per set.
#pragma once
#include "gbls_bits.h"

namespace gbls {

// one piece of a launch.  list/cnt: the committee's resident members (list == nullptr: the slot
// is past the table or keeps no members), a plain set's registry indices.  slot: kNoCommittee for
// a plain set's piece.  set: the piece's set.  bit: where the committee's bits start in the
// set's row, the sum of the member counts of the committees named before it.
struct SpanPiece {
  const uint32_t *list;
  uint32_t cnt, slot, set, bit;
};
// one set of a launch: its pieces [first, first + npieces), the word offset and byte length of its
// repacked bit string, and M, the member counts of its named committees summed.  A plain set has
// one piece and no string.
struct SpanSet {
  uint32_t first, npieces, row, nbytes, M;
};

// what a piece tells its set beside its contribution
enum : uint32_t {
  SP_BAD_INDEX = 1,  // a member or listed index is past the registry or names an invalid key
  SP_BAD_SLOT = 2,   // the slot is past the table, invalid (all-zero sum) or keeps no members
  SP_EMPTY = 4,      // a committee without a participant; a plain set's empty list
  SP_PLAIN = 8,      // the piece is a plain set's list
};
// the finish folds a set's contributions in one lane up to this many pieces and in a 16-lane row
// from there on: a chain of k additions against ceil(k / 16) + 4
constexpr uint32_t kSpanFoldRowMin = 8;
// a set whose committees hold more members than this is rejected (M and every bit offset stay
// 32-bit, m + 31 does not wrap)
constexpr uint64_t kSpanMaxMembers = 0xffffff00ull;

// Word w of the window that starts at bit `bit` of a row of nw words: bits bit + 32 w .. + 31, a
// funnel of two row words.  A word index from nw on reads as zero, so a window never reaches the
// next set's row or the buffer's end, whatever the string's length.  No shift by 32: an aligned
// window is the row word itself.
HD uint32_t span_window(const uint32_t *row, uint32_t nw, uint32_t bit, uint32_t w) {
  const uint32_t i = (bit >> 5) + w, sh = bit & 31;  // (bit <= kSpanMaxMembers: no wrap)
  const uint32_t lo = i < nw ? row[i] : 0u;
  if (sh == 0) return lo;
  const uint32_t hi = i + 1 < nw ? row[i + 1] : 0u;
  return (lo >> sh) | (hi << (32 - sh));
}

// the committee's participants: the set bits among the m that start at `bit`
HD uint32_t span_count(const uint32_t *row, uint32_t nw, uint32_t bit, uint32_t m) {
  uint32_t p = 0;
  for (uint32_t wi = 0; wi < (m + 31) / 32; wi++) p += bits_popc(span_window(row, nw, bit, wi) & bits_member_mask(m, wi));
  return p;
}

// A committee piece's contribution from its accumulated sum S and the slot's cached sum C:
// C - S when it added the absentees, else S, and C itself when everyone participates (S is then
// infinite: nothing was added).  Jacobian, no inversion.  Returns the piece's flags: an invalid
// slot counts in either direction (the participants' sum does not read C, the slot must be valid
// all the same), a committee without a participant rejects its set.
HD uint32_t span_contribution(g1j &out, const g1a &C, const g1j &S, bool has_members, bool subtract, uint32_t p,
                              uint32_t bad) {
  uint32_t flags = bad ? SP_BAD_INDEX : 0u;
  if (!has_members || aff_is_inf(C)) flags |= SP_BAD_SLOT;
  if (p == 0) flags |= SP_EMPTY;
  out = S;
  if (subtract) {
    jac_neg(out, S);
    jac_add_aff(out, out, C);  // complete: S = -C doubles, S = C is the identity
  }
  return flags;
}

// The set's key from the fold T of its contributions and the OR of its pieces' flags.  ok: a span
// set's string passed bits_check over M (true for a plain set).  Returns the status; the key is
// all-zero on a rejection and for an infinite sum.
//   span set   BAD_ENCODING: no committee named, any flag, a malformed string
//   plain set  as in k_g1_committee_keys: a bad index is BAD_ENCODING, an empty list
//              AGGR_TYPE_MISMATCH
HD int32_t span_key(g1a &key, const g1j &T, uint32_t npieces, uint32_t flags, bool ok) {
  int32_t status = ST_SUCCESS;
  if (flags & SP_PLAIN) {
    if (flags & SP_BAD_INDEX)
      status = ST_BAD_ENCODING;
    else if (flags & SP_EMPTY)
      status = ST_AGGR_TYPE_MISMATCH;
  } else if (!npieces || !ok || (flags & (SP_BAD_INDEX | SP_BAD_SLOT | SP_EMPTY))) {
    status = ST_BAD_ENCODING;
  }
  g1j t = T;
  if (status != ST_SUCCESS) jac_set_inf(t);
  jac_to_aff(key, t);  // infinity: all-zero
  return status;
}

// host: committee_bits as it arrives (SSZ Bitvector[64]: bit c is cbits[c >> 3] >> (c & 7) & 1)
inline bool span_named(const uint8_t *cbits, uint32_t c) { return (cbits[c >> 3] >> (c & 7)) & 1u; }
inline bool span_mask_empty(const uint8_t *cbits) {
  uint8_t any = 0;
  for (int i = 0; i < 8; i++) any |= cbits[i];
  return any == 0;
}
inline uint32_t span_mask_count(const uint8_t *cbits) {
  uint32_t k = 0;
  for (int i = 0; i < 8; i++) k += bits_popc(cbits[i]);
  return k;
}

// host: the pieces of span set `set`: one per set bit c of cbits, ascending, naming slot com + c
// (formed in 64 bits: a base near 2^32 does not wrap into the table).  members(slot, &list, &cnt)
// says whether the slot keeps members and where.  A slot that keeps none gives a piece without a
// list, which rejects the set.  Writes up to 64 pieces, returns their number; *M: the named
// committees' member counts summed.  A set over more than kSpanMaxMembers members is rejected the
// same way (every piece without a list, M = 0).
template <class Members>
inline uint32_t span_pieces(uint32_t set, uint32_t com, const uint8_t *cbits, Members &&members, SpanPiece *out,
                            uint32_t *M) {
  uint32_t k = 0;
  uint64_t at = 0;
  for (uint32_t c = 0; c < 64; c++) {
    if (!span_named(cbits, c)) continue;
    const uint64_t slot = (uint64_t)com + c;
    SpanPiece &p = out[k++];
    p.list = nullptr;
    p.cnt = 0;
    p.slot = slot < kNoCommittee ? (uint32_t)slot : kNoCommittee - 1;  // (never a plain piece's mark)
    p.set = set;
    p.bit = (uint32_t)at;
    if (slot < kNoCommittee && at <= kSpanMaxMembers && !members((uint32_t)slot, &p.list, &p.cnt)) {
      p.list = nullptr;
      p.cnt = 0;
    }
    at += p.cnt;
  }
  if (at > kSpanMaxMembers) {
    for (uint32_t i = 0; i < k; i++) {
      out[i].list = nullptr;
      out[i].cnt = out[i].bit = 0;
    }
    at = 0;
  }
  *M = (uint32_t)at;
  return k;
}

// host: the keys a piece's lane-form chain adds, min(p, m - p) with ties to the participants (not
// validated: only the launch form depends on it)
inline uint32_t span_work(const uint32_t *row, uint32_t nbytes, uint32_t bit, uint32_t m) {
  const uint32_t p = span_count(row, bits_row_words(nbytes), bit, m);
  return committee_subtracts(m, p) ? m - p : p;
}

}  // namespace gbls
