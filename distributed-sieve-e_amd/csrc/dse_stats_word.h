// dse_stats_word.h -- the per-word bodies of the mask statistics (dse_stats.hip).
//
// A range's candidates are numbered 0 .. nbits - 1 from its start ("positions");
// word wi holds the positions [64 wi, 64 wi + 64). A thread (or the host loop of
// dse_debug_stats_host) holds one word `w` and the low half `nx` of the word
// after it, both with the bits past nbits dropped, so everything that starts in
// w and reaches at most 31 places past its end is decided from the 96-bit
// window {nx : w}:
//   stats_pattern_word  matches of a constellation pattern that start in w;
//   stats_small_gaps    the gaps of 1 .. kStatsSmall places whose lower prime is
//                       in w, counted bit-parallel (no loop over the primes),
//                       and the primes of w whose gap is longer than that;
//   stats_inword_large  the longer gaps whose two primes both lie in w;
//   stats_cross         the longer gap that ends at w's first prime (the prime
//                       before it comes from the caller: a workgroup scan on the
//                       device, the loop's carry on the host);
//   stats_small_best    the largest short gap of w and its lower prime, for
//                       ranges in which no longer gap exists.
// Every gap is seen exactly once: the short ones (<= kStatsSmall places) only by
// stats_small_gaps, wherever their primes lie, the longer ones only by the other
// paths. The functions are __host__ __device__: the kernels and
// dse_debug_stats_host (tests, on the host) run the same code.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dse_mask.h"

namespace dse {

constexpr uint32_t kStatsSmall = 16;    // gaps of up to this many places are counted bit-parallel
constexpr uint32_t kStatsBins = 1024;   // DSE_STATS_GAP_BINS
constexpr uint64_t kStatsNone = ~0ull;  // DSE_STATS_NONE
static_assert(kStatsSmall >= 1 && kStatsSmall <= 31, "a short gap is decided inside the 96-bit window");

__host__ __device__ __forceinline__ uint32_t stats_ctz64(uint64_t x) { return (uint32_t)__builtin_ctzll(x); }
__host__ __device__ __forceinline__ uint32_t stats_msb64(uint64_t x) { return 63u - (uint32_t)__builtin_clzll(x); }
__host__ __device__ __forceinline__ uint32_t stats_pop64(uint64_t x) { return (uint32_t)__builtin_popcountll(x); }

// positions [s, s + 64) of the range as one word (bit k = position s + k; 0 past nbits)
__host__ __device__ __forceinline__ uint64_t stats_bits64(const MaskRange& r, uint64_t s) {
  const uint64_t wi = s >> 6;
  const uint32_t sh = (uint32_t)(s & 63);
  uint64_t v = mask_word(r, wi) >> sh;
  if (sh) v |= mask_word(r, wi + 1) << (64 - sh);
  return v;
}

// bits [j, j + 64) of the window {nx : w}, 1 <= j <= 31 (two funnel shifts)
__host__ __device__ __forceinline__ uint64_t stats_shift(uint64_t w, uint32_t nx, uint32_t j) {
  const uint32_t w0 = (uint32_t)w, w1 = (uint32_t)(w >> 32);
  const uint32_t lo = (w0 >> j) | (w1 << (32 - j)), hi = (w1 >> j) | (nx << (32 - j));
  return lo | ((uint64_t)hi << 32);
}

// matches of pat (bit 0 set, span <= 32) that start in w
__host__ __device__ __forceinline__ uint32_t stats_pattern_word(uint64_t w, uint32_t nx, uint32_t pat) {
  uint64_t m = w;
  for (uint32_t r = pat & ~1u; r; r &= r - 1) m &= stats_shift(w, nx, (uint32_t)__builtin_ctz(r));
  return stats_pop64(m);
}

// cnt[d - 1] += the gaps of d places whose lower prime is in w, d <= kStatsSmall.
// Returns the primes of w that have no prime within kStatsSmall places above them.
template <typename C>
__host__ __device__ __forceinline__ uint64_t stats_small_gaps(uint64_t w, uint32_t nx, C* cnt) {
  uint64_t seen = 0;  // bit i: a prime within the places i + 1 .. i + d
#pragma unroll
  for (uint32_t d = 1; d <= kStatsSmall; ++d) {
    const uint64_t xs = stats_shift(w, nx, d);
    cnt[d - 1] += (C)stats_pop64(w & xs & ~seen);
    seen |= xs;
  }
  return w & ~seen;
}

// The gaps of more than kStatsSmall places between two primes of w: put(d, position
// of the lower prime), in increasing position. rem = stats_small_gaps' result.
template <typename Sink>
__host__ __device__ __forceinline__ void stats_inword_large(uint64_t w, uint64_t rem, uint64_t pos0, Sink&& put) {
  if (!rem) return;
  uint64_t it = rem & ~(1ull << stats_msb64(w));  // w's last prime has its successor in a later word
  while (it) {
    const uint32_t i = stats_ctz64(it);
    it &= it - 1;
    put((uint64_t)(1u + stats_ctz64(w >> (i + 1))), pos0 + i);
  }
}

// The gap from the prime before a word's first prime (prev1 = its position + 1,
// not 0) to that prime at position f, when it is a long one.
template <typename Sink>
__host__ __device__ __forceinline__ void stats_cross(uint64_t f, uint64_t prev1, Sink&& put) {
  const uint64_t d = f - (prev1 - 1);
  if (d > kStatsSmall) put(d, prev1 - 1);
}

// (d, i) comes before (bd, bi) as the maximal gap: strictly longer, or as long and lower
__host__ __device__ __forceinline__ bool stats_better(uint64_t d, uint64_t i, uint64_t bd, uint64_t bi) {
  return d > bd || (d == bd && i < bi);
}

// The longest short gap whose lower prime is in w and the lowest such prime, merged into (bd, bi).
__host__ __device__ __forceinline__ void stats_small_best(uint64_t w, uint32_t nx, uint64_t pos0, uint64_t& bd,
                                                          uint64_t& bi) {
  uint64_t seen = 0, gm = 0;
  uint32_t gd = 0;
  for (uint32_t d = 1; d <= kStatsSmall; ++d) {
    const uint64_t xs = stats_shift(w, nx, d);
    const uint64_t m = w & xs & ~seen;
    if (m) {
      gm = m;
      gd = d;
    }
    seen |= xs;
  }
  if (gd && stats_better(gd, pos0 + stats_ctz64(gm), bd, bi)) {
    bd = gd;
    bi = pos0 + stats_ctz64(gm);
  }
}

}  // namespace dse
