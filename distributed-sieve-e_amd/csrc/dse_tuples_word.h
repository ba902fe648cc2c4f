// dse_tuples_word.h -- the per-word body of the constellations as numbers (dse_tuples.hip).
//
// A range's candidates are numbered 0 .. nbits - 1 from its start ("positions"); behind them
// come above_bits <= 31 candidates of the caller's, the bits of `above` from bit above_shift on.
// Together they are the visible candidates; position i is visible when i < nbits + above_bits.
//
// A pattern is (require, forbid), require with bit 0 set, require & forbid == 0; its span is the
// bit length of require | forbid. Position i < nbits matches when i + span <= nbits + above_bits,
// every candidate i + j, j a set bit of require, is an entry and every candidate i + j, j a set
// bit of forbid, is not.
//
// A thread (or the host loop of dse_debug_tuples_host) holds one word `w` of the visible
// candidates and the low half `nx` of the word after it; the match word of w is decided from the
// 96-bit window {nx : w} with the funnel shift of the statistics (stats_shift):
//   tuples_visible_word  positions [64 wi, 64 wi + 64) of the visible candidates; `above` is read
//                        only for the words that reach past nbits (at most two);
//   tuples_match_word    the AND over require's set bits, and of the complement over forbid's, of
//                        the shifted window, cut where a span would leave the visible candidates;
//   tuples_word          that, cut to the range's own positions: bit b = position 64 wi + b matches.
// The functions are __host__ __device__: the kernels and dse_debug_tuples_host (tests, on the
// host) run the same code.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dse_mask.h"
#include "dse_stats_word.h"

namespace dse {

constexpr uint32_t kTuplesMaxAbove = 31;

struct TupleSrc {
  MaskRange r;
  const uint64_t* above;
  uint32_t above_shift, above_bits;
  uint32_t require, forbid;
};

__host__ __device__ __forceinline__ uint32_t tuples_span(uint32_t require, uint32_t forbid) {
  return 32u - (uint32_t)__builtin_clz(require | forbid);  // require has bit 0 set
}

// the candidates above the range as a number: bit k = position nbits + k (above_bits > 0); reads
// the whole words that cover the string, one or two
__host__ __device__ __forceinline__ uint64_t tuples_above(const TupleSrc& s) {
  uint64_t v = s.above[0] >> s.above_shift;
  if (s.above_shift + s.above_bits > 64u) v |= s.above[1] << (64u - s.above_shift);
  return v & ((1ull << s.above_bits) - 1ull);
}

// positions [64 wi, 64 wi + 64) of the visible candidates, 0 past them
__host__ __device__ __forceinline__ uint64_t tuples_visible_word(const TupleSrc& s, uint64_t wi) {
  uint64_t v = mask_word(s.r, wi);
  const uint64_t pos0 = wi * 64ull, nb = s.r.nbits;
  if (s.above_bits && pos0 + 64ull > nb && pos0 < nb + s.above_bits) {
    const uint64_t a = tuples_above(s);
    v |= pos0 <= nb ? a << (nb - pos0) : a >> (pos0 - nb);  // both shifts < 64
  }
  return v;
}

// The starts in w whose pattern matches inside the window {nx : w}; vis = the visible positions
// from w's bit 0 on (any number, also 0): a start whose span reaches past them is no match.
__host__ __device__ __forceinline__ uint64_t tuples_match_word(uint64_t w, uint32_t nx, uint32_t require,
                                                               uint32_t forbid, uint64_t vis) {
  const uint32_t span = tuples_span(require, forbid);
  if (vis < span) return 0ull;
  uint64_t m = w;
  for (uint32_t r = require & ~1u; r; r &= r - 1) m &= stats_shift(w, nx, (uint32_t)__builtin_ctz(r));
  for (uint32_t f = forbid; f; f &= f - 1) m &= ~stats_shift(w, nx, (uint32_t)__builtin_ctz(f));
  const uint64_t n = vis - span + 1;  // starts whose span is visible
  return n >= 64 ? m : m & ((1ull << n) - 1ull);
}

// The match word of word wi: w, nx = tuples_visible_word of wi and the low half of that of wi + 1.
__host__ __device__ __forceinline__ uint64_t tuples_word(const TupleSrc& s, uint64_t wi, uint64_t w, uint32_t nx) {
  const uint64_t pos0 = wi * 64ull, nb = s.r.nbits;
  if (pos0 >= nb) return 0ull;
  const uint64_t m = tuples_match_word(w, nx, s.require, s.forbid, nb + s.above_bits - pos0);
  return nb - pos0 >= 64 ? m : m & ((1ull << (nb - pos0)) - 1ull);  // a match starts in the range
}

}  // namespace dse
