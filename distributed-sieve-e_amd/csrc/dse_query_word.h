// dse_query_word.h -- the per-word and per-tile bodies of rank and select on a
// prime mask (dse_query.hip), __host__ __device__: the kernel runs them on the
// words a lane holds, dse_debug_query_host (dse_query_host.cpp) on the host
// over a whole tile.
//
// An entry is a set bit of the range [g_start, g_start + nbits); the entry at
// position i (bit i of the range) has the value 3 + 2 (g_start + i). Every
// query on a value x starts from its lead: how many positions of the range
// hold a value <= x. RANK(x) is the number of entries among them.
#pragma once
#include <stdint.h>

#include "dse_mask.h"

namespace dse {

constexpr uint64_t kQueryNone = ~0ull;
constexpr uint32_t kQueryRank = 0, kQuerySelect = 1, kQueryNext = 2, kQueryPrev = 3, kQueryTest = 4;
constexpr uint32_t kQueryKinds = 5;

__host__ __device__ __forceinline__ uint32_t query_pop64(uint64_t x) { return (uint32_t)__builtin_popcountll(x); }

// The positions of the range whose value is <= x, in 0..nbits. The candidates
// 0 .. c - 1 have a value <= x for c = (x - 1) / 2 (x >= 3; none below): c is
// below 2^63 for every x, so nothing wraps.
__host__ __device__ __forceinline__ uint64_t query_lead(uint64_t x, uint64_t g_start, uint64_t nbits) {
  const uint64_t c = x < 3 ? 0ull : (x - 1) / 2;
  if (c <= g_start) return 0ull;
  return c - g_start < nbits ? c - g_start : nbits;
}

// the value of the entry at position pos of the range (g_start + pos <= 2^62)
__host__ __device__ __forceinline__ uint64_t query_value(uint64_t g_start, uint64_t pos) {
  return 3ull + 2ull * (g_start + pos);
}

// rank inside a word: its set bits below bit b, b in 0..64
__host__ __device__ __forceinline__ uint32_t query_rank64(uint64_t w, uint32_t b) {
  return b >= 64 ? query_pop64(w) : query_pop64(w & ((1ull << b) - 1));
}

// select inside a word: the bit index of its k-th set bit (k = 0 the lowest), k < popcount(w).
// Six halvings: the low half holds the bit exactly when it has more than k set bits.
__host__ __device__ __forceinline__ uint32_t query_select64(uint64_t w, uint32_t k) {
  uint32_t pos = 0;
#pragma unroll
  for (uint32_t h = 32; h > 0; h >>= 1) {
    const uint32_t c = query_pop64(w & ((1ull << h) - 1));
    if (k >= c) {
      k -= c;
      w >>= h;
      pos += h;
    }
  }
  return pos;
}

// Rank in a run of kN words of a tile, the run's first word being the tile's
// word j0 and load(i) its word i: the set bits of the run at tile positions
// below p.
template <uint32_t kN, typename Load>
__host__ __device__ __forceinline__ uint32_t query_rank_words(Load&& load, uint32_t j0, uint32_t p) {
  uint32_t c = 0;
#pragma unroll
  for (uint32_t i = 0; i < kN; ++i) {
    const uint32_t lo = (j0 + i) * 64;
    if (p > lo) c += query_rank64(load(i), p - lo);
  }
  return c;
}

// the set bits of the run
template <uint32_t kN, typename Load>
__host__ __device__ __forceinline__ uint32_t query_pop_words(Load&& load) {
  uint32_t c = 0;
#pragma unroll
  for (uint32_t i = 0; i < kN; ++i) c += query_pop64(load(i));
  return c;
}

// Select in the run: the position inside the run (64 i + bit) of its r-th set
// bit, r < query_pop_words.
template <uint32_t kN, typename Load>
__host__ __device__ __forceinline__ uint32_t query_select_words(Load&& load, uint32_t r) {
  uint32_t pos = 0;
  bool found = false;
#pragma unroll
  for (uint32_t i = 0; i < kN; ++i) {
    const uint64_t w = load(i);
    const uint32_t c = query_pop64(w);
    if (!found && r < c) {
      pos = i * 64 + query_select64(w, r);
      found = true;
    }
    if (!found) r -= c;
  }
  return pos;
}

// TEST: 1 when x is the value of an entry of the range
__host__ __device__ __forceinline__ uint64_t query_test(const MaskRange& m, uint64_t x) {
  if (x < 3 || !(x & 1)) return 0ull;
  const uint64_t g = (x - 3) / 2;
  if (g < m.g_start || g - m.g_start >= m.nbits) return 0ull;
  const uint64_t pos = g - m.g_start;
  return (mask_word(m, pos >> 6) >> (pos & 63)) & 1ull;
}

}  // namespace dse
