// Local key sets (include/grandine_bls_gpu_local.h): sets whose keys the caller holds only as
// compressed bytes, in a table that lives for one call.  Host-compilable text, as gbls_spans.h is: the
// argument rules and the layout of a launch's pieces, so that tests/native/local_harness.cpp
// compiles the same lines for the CPU.
//
// A call's table pkb[npkb] is decoded on the device into loc[npkb], in the registry's form (an
// invalid key all-zero, as gbls_registry_set stores one: k_local.hip).  A local set is then ONE
// plain piece (gbls_spans.h) whose list holds positions into loc instead of registry indices, so
// nothing after the decode is new: the piece kernel runs twice, over the head of the piece array
// with the registry and over the tail with loc.  A shard of a sharded batch decodes the WHOLE
// table, not only the keys its sets name: the table is small by design (a block's deposits and
// address changes), and the positions then need no rebasing per shard.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "gbls_spans.h"

namespace gbls {

constexpr uint32_t kLocalKeys = 0xfffffffeu;  // com[i] of a local set (GBLS_LOCAL_KEYS)
// tables up to this many keys are decoded one wave per key (k_g1_local_decode_wave), larger ones
// one lane per key.  Measured (the whole key call): the wave form takes ~605 us
// up to 256 keys and 951 us at 2048, where the lane form takes 1905 - 2200 us and 1964 us; at 8192
// keys the lane form wins (2032 us against 3004 us).  Not a run-time knob; an experiment build
// (make BUILD=build_x LIB=lib_x EXTRA=-DGBLS_LOCAL_WAVE_MAX=0) shows the other form at a size.
#ifdef GBLS_LOCAL_WAVE_MAX
constexpr uint32_t kLocalWaveMax = GBLS_LOCAL_WAVE_MAX;
#else
constexpr uint32_t kLocalWaveMax = 2048;
#endif

// pieces [0, np_span) belong to span and plain sets, in set order; [np_span, np_span + np_local)
// to the local sets, in set order (SpanSet::first is free, so a set's pieces lie anywhere)
struct LocalLayout {
  uint32_t np_span = 0, np_local = 0;
};
inline bool local_is(const uint32_t *com, size_t i) { return com[i] == kLocalKeys; }
inline uint32_t local_set_pieces(const uint32_t *com, const uint8_t (*cbits)[8], size_t i) {
  return com[i] == kNoCommittee || com[i] == kLocalKeys ? 1u : span_mask_count(cbits[i]);
}
// The layout of sets [b, e) (a shard's slice): first[i - b] is where set i's pieces start.  The
// counts are formed in 64 bits; returns false when they do not fit 32.
inline bool local_layout(const uint32_t *com, const uint8_t (*cbits)[8], size_t b, size_t e, uint32_t *first,
                         LocalLayout *out) {
  uint64_t ns = 0, nl = 0;
  for (size_t i = b; i < e; i++) (local_is(com, i) ? nl : ns) += local_set_pieces(com, cbits, i);
  if (ns + nl > 0xffffffffull) return false;
  uint32_t s = 0, l = (uint32_t)ns;
  for (size_t i = b; i < e; i++) {
    uint32_t &at = local_is(com, i) ? l : s;
    first[i - b] = at;
    at += local_set_pieces(com, cbits, i);
  }
  out->np_span = (uint32_t)ns;
  out->np_local = (uint32_t)nl;
  return true;
}
// A plain or local set's piece: `list` holds the shard's slice of pk_idx (entries
// [off[b], off[e]), nullptr without ranges), set i's range starts at off[i] - off[b].  A local
// piece is a plain piece: only the table its kernel launch reads differs.
inline void local_list_piece(SpanPiece &p, uint32_t set, const uint32_t *list, const uint32_t *off, size_t b, size_t i) {
  p.list = nullptr;
  p.cnt = p.bit = 0;
  p.slot = kNoCommittee;
  p.set = set;
  if (off) {
    p.list = list + (off[i] - off[b]);
    p.cnt = off[i + 1] - off[i];
  }
}

inline bool local_offsets_ok(const uint32_t *off, size_t n) {
  if (!off || off[0] != 0) return false;
  for (size_t i = 0; i < n; i++)
    if (off[i + 1] < off[i]) return false;
  return true;
}
// The arguments of a span | local key source: what grandine_bls_gpu_spans.h asks of span and plain
// sets, and of a local set zero committee_bits, an empty bit string and a range of pk_off (so
// pk_off itself).  pkb may be null only for an empty table; npkb and the pieces fit 32 bits.
inline bool local_args_ok(const uint32_t *com, const uint8_t (*cbits)[8], const uint8_t *bits, const uint32_t *bits_off,
                          const uint32_t *pk_idx, const uint32_t *pk_off, const void *pkb, size_t npkb, size_t n) {
  if (!com || !cbits || n > 0xfffffffeull || (uint64_t)npkb > 0xffffffffull || (npkb && !pkb)) return false;
  if (!local_offsets_ok(bits_off, n) || (pk_off && !local_offsets_ok(pk_off, n))) return false;
  if ((bits_off[n] && !bits) || (pk_off && pk_off[n] && !pk_idx)) return false;
  uint64_t np = 0;
  for (size_t i = 0; i < n; i++) {
    const bool plain = com[i] == kNoCommittee, local = com[i] == kLocalKeys;
    if (local && !pk_off) return false;
    if ((plain || local) && (bits_off[i + 1] != bits_off[i] || !span_mask_empty(cbits[i]))) return false;
    if (!plain && !local && pk_off && pk_off[i + 1] != pk_off[i]) return false;
    np += local_set_pieces(com, cbits, i);
  }
  return np <= 0xffffffffull;
}

}  // namespace gbls
