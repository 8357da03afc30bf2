// gfx950 kernels of the message line cache (gbls_msgcache.h): copies between the cache table and a
// submission's line buffer.
//
// The table is slot-major: slot s holds its message's 68 x 72 line words contiguously, in
// line_word order (word w = (e * 6 + c) * 12 + limb).  The line buffer is word-major: word w of
// the pair at column cp is L[w * ncol + cp] (bls_pairing.h line_word).  A copy is therefore a
// transpose, done through an LDS tile of kTile pairs x kTile words by a workgroup of four waves:
//   table side   one wave per pair, lane = word: 64 consecutive words of one slot, a whole
//                256-byte run (slots are 19 584 B apart, so runs start on 128-byte lines);
//   buffer side  one wave per word, lane = pair: the pairs' columns of one word row.  The tables
//                number a segment's pairs so that neighbouring pairs sit in neighbouring columns
//                (gbls_tables.h), so these are runs as long as the hits are neighbours.
// The tile's rows are kTile + 1 words apart: the lanes of the transposed access (stride 65 words)
// fall on 64 different LDS banks, and the row-wise access is stride 1.
#include "gbls_common.h"

namespace gbls {

namespace {
constexpr uint32_t kTile = 64;
constexpr uint32_t kLcWG = 256;
constexpr uint32_t kSlotWords = ML_EVENTS * 72;
constexpr uint32_t kWordTiles = (kSlotWords + kTile - 1) / kTile;  // 77 (the last one half full)
}  // namespace

// pairs [first, first + count): pair first + i from slot[i]
__global__ void __launch_bounds__(kLcWG) k_linecache_load(const uint32_t *tab, const uint32_t *slot,
                                                          uint32_t first, uint32_t count, LineCols lc,
                                                          uint32_t *L) {
  __shared__ uint32_t tile[kTile][kTile + 1];
  const uint32_t p0 = blockIdx.x * kTile, w0 = blockIdx.y * kTile;
  const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  for (uint32_t k = wv; k < kTile; k += kLcWG / 64) {
    const uint32_t i = p0 + k;
    if (i < count && w0 + lane < kSlotWords) tile[k][lane] = tab[(size_t)slot[i] * kSlotWords + w0 + lane];
  }
  __syncthreads();
  const uint32_t i = p0 + lane;
  if (i >= count) return;
  const uint32_t pair = first + i, cp = lc.col ? lc.col[pair] : pair;
  for (uint32_t w = wv; w < kTile; w += kLcWG / 64)
    if (w0 + w < kSlotWords) L[(size_t)(w0 + w) * lc.ncol + cp] = tile[lane][w];
}

// entries [0, count): the lines of pair pairs[i] to slot[i]
__global__ void __launch_bounds__(kLcWG) k_linecache_store(uint32_t *tab, const uint32_t *pairs,
                                                           const uint32_t *slot, uint32_t count, LineCols lc,
                                                           const uint32_t *L) {
  __shared__ uint32_t tile[kTile][kTile + 1];
  const uint32_t p0 = blockIdx.x * kTile, w0 = blockIdx.y * kTile;
  const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  if (p0 + lane < count) {
    const uint32_t pair = pairs[p0 + lane], cp = lc.col ? lc.col[pair] : pair;
    for (uint32_t w = wv; w < kTile; w += kLcWG / 64)
      if (w0 + w < kSlotWords) tile[lane][w] = L[(size_t)(w0 + w) * lc.ncol + cp];
  }
  __syncthreads();
  for (uint32_t k = wv; k < kTile; k += kLcWG / 64) {
    const uint32_t i = p0 + k;
    if (i < count && w0 + lane < kSlotWords) tab[(size_t)slot[i] * kSlotWords + w0 + lane] = tile[k][lane];
  }
}

void launch_linecache_load(hipStream_t st, const uint32_t *tab, const uint32_t *slot, uint32_t first,
                           uint32_t count, LineCols lc, uint32_t *lines) {
  if (!count) return;
  k_linecache_load<<<dim3(nblk(count, kTile), kWordTiles), kLcWG, 0, st>>>(tab, slot, first, count, lc, lines);
}

void launch_linecache_store(hipStream_t st, uint32_t *tab, const uint32_t *pairs, const uint32_t *slot,
                            uint32_t count, LineCols lc, const uint32_t *lines) {
  if (!count) return;
  k_linecache_store<<<dim3(nblk(count, kTile), kWordTiles), kLcWG, 0, st>>>(tab, pairs, slot, count, lc, lines);
}

}  // namespace gbls
