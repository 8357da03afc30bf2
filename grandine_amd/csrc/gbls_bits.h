// Aggregation-bit sets: the per-set step of k_g1_bits_keys (k_bits.hip), as __host__ __device__
// text so that tests/native/bits_harness.cpp compiles the same lines for the CPU.
//
// A committee set names a table slot whose m members are resident on the device and carries the
// attestation's own bit string (SSZ bit order: bit j is byte j >> 3, bit j & 7).  The host repacks
// every string into a row of 32-bit words (bits_repack: little-endian, zero padded), so the kernel
// never loads across an unaligned or short buffer end and bit j is  row[j >> 5] >> (j & 31) & 1.
// The key is the sum of the members whose bit is set, formed from the cached sum C minus the
// members whose bit is CLEAR when those are the fewer (committee_subtracts, gbls_committees.h).
#pragma once
#include <cstring>

#include "gbls_committees.h"

namespace gbls {

// one set of a launch.  list/cnt: a committee set's resident members (list == nullptr: the slot is
// past the table or keeps no members), a plain set's registry indices.  slot: kNoCommittee for a
// plain set.  row: the word offset of a committee set's repacked bit string, nbytes its length.
struct BitSet {
  const uint32_t *list;
  uint32_t cnt, slot, row, nbytes;
};

HD uint32_t bits_popc(uint32_t w) {
#if defined(__HIP_DEVICE_COMPILE__)
  return (uint32_t)__popc(w);
#else
  return (uint32_t)__builtin_popcount(w);
#endif
}
HD uint32_t bits_ctz(uint32_t w) {  // w != 0
#if defined(__HIP_DEVICE_COMPILE__)
  return (uint32_t)(__ffs((int)w) - 1);
#else
  return (uint32_t)__builtin_ctz(w);
#endif
}

HD uint32_t bits_row_words(uint32_t nbytes) { return (nbytes + 3) / 4; }
// the bits of word wi that name members (positions below m); wi < ceil(m / 32)
HD uint32_t bits_member_mask(uint32_t m, uint32_t wi) {
  const uint32_t left = m - 32 * wi;
  return left >= 32 ? 0xffffffffu : (1u << left) - 1u;
}

// A committee's bit string of nbytes bytes over m members, in either SSZ encoding, told apart
// without a flag:
//   Bitvector[m]  ceil(m / 8) bytes, every bit from m on zero
//   Bitlist       m / 8 + 1 bytes, the delimiter bit at position m set, every bit above it zero
// (when m % 8 != 0 the lengths coincide and bit m decides).  Returns false for anything else:
// another length, a stray bit, the long form without its delimiter.  *p: the members whose bit is
// set.  `row` holds bits_row_words(nbytes) words, zero past the string's end.
HD bool bits_check(const uint32_t *row, uint32_t nbytes, uint32_t m, uint32_t *p) {
  *p = 0;
  const uint32_t len_v = (m + 7) / 8, len_l = m / 8 + 1;
  if (nbytes != len_v && nbytes != len_l) return false;
  const uint32_t nw = bits_row_words(nbytes), mw = (m + 31) / 32;
  uint32_t total = 0, part = 0;
  for (uint32_t wi = 0; wi < nw; wi++) {
    const uint32_t w = row[wi];
    total += bits_popc(w);
    if (wi < mw) part += bits_popc(w & bits_member_mask(m, wi));
  }
  // bit m lies inside the string exactly when it has the long form's length
  const uint32_t delim = nbytes == len_l ? (row[m >> 5] >> (m & 31)) & 1u : 0u;
  if (nbytes != len_v && !delim) return false;  // the long form without its delimiter
  if (total != part + delim) return false;      // a bit past the members that is not the delimiter
  *p = part;
  return true;
}

// The members of word wi (value w) that lane r of `lanes` adds: the clear bits when the set
// subtracts its absentees, else the set bits; never a position from m on (the inverted padding
// selects nobody).  lanes == 16: lane r takes members j = r (mod 16), bits r and r + 16 of a word.
HD uint32_t bits_select(uint32_t w, uint32_t m, uint32_t wi, bool subtract, uint32_t r, uint32_t lanes) {
  uint32_t sel = (subtract ? ~w : w) & bits_member_mask(m, wi);
  if (lanes == 16) sel &= 0x00010001u << r;
  return sel;
}

// The set's key from its accumulated sum S; `bad`: a malformed bit string, a slot without members,
// a member or listed index that is past the registry or names an invalid key.  Returns the status.
//   committee set  BAD_ENCODING also for an invalid (all-zero) cached sum, in either direction;
//                  no participant at all: infinity, a SUCCESS written all-zero (as committee_key)
//   plain set      as in k_g1_committee_keys: an empty list is AGGR_TYPE_MISMATCH
HD int32_t bits_key(g1a &key, const g1a &C, const g1j &S, bool committee, bool subtract, uint32_t m,
                    uint32_t p, uint32_t bad) {
  uint32_t flags = bad ? CK_BAD_INDEX : 0u;
  if (!committee)
    flags |= m == 0 ? CK_EMPTY : 0u;
  else if (subtract)
    flags |= CK_COMMITTEE | (p == m ? CK_EMPTY : 0u);
  else if (aff_is_inf(C))  // the participants' sum does not read C: the slot must be valid all the same
    flags |= CK_BAD_INDEX;
  return committee_key(key, C, S, flags);
}

// host: a bit string of nbytes bytes at any alignment -> its row of bits_row_words(nbytes) words
inline void bits_repack(uint32_t *row, const uint8_t *bits, uint32_t nbytes) {
  const uint32_t nw = bits_row_words(nbytes);
  if (!nw) return;
  row[nw - 1] = 0;
  // the engine's hosts and gfx950 are little-endian: byte i holds bits 8 i .. 8 i + 7 of the row
  std::memcpy(row, bits, nbytes);
}
// host: the keys a committee set's lane-form chain adds, min(p, m - p) with ties to the
// participants, from its repacked row (not validated: only the launch form depends on it)
inline uint32_t bits_work(const uint32_t *row, uint32_t nbytes, uint32_t m) {
  const uint32_t nw = bits_row_words(nbytes), mw = (m + 31) / 32 < nw ? (m + 31) / 32 : nw;
  uint32_t p = 0;
  for (uint32_t wi = 0; wi < mw; wi++) p += bits_popc(row[wi] & bits_member_mask(m, wi));
  return committee_subtracts(m, p) ? m - p : p;
}

}  // namespace gbls
