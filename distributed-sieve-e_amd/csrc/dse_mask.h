// dse_mask.h -- a range of a prime mask and its words, shared by everything
// that turns a device-resident mask into something else: the device finish
// (dse_finish.hip), primes as numbers (dse_primes.hip), the statistics
// (dse_stats.hip), rank and select (dse_query.hip), the Goldbach partitions
// (dse_goldbach.hip), the residue classes and races (dse_race.hip), the constellations as numbers
// (dse_tuples.hip) and their host sides.
//
// A range is the odd indices [g_start, g_start + nbits), one bit each, in
// `words` 64-bit words; the kernels walk it in tiles of kMaskTileWords words,
// one word per thread of a 256-thread workgroup. The functions are
// __host__ __device__: the kernels and the debug hooks of the host layer
// (tests, on the host) run the same code.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dse {

constexpr uint32_t kMaskTileWords = 256;
constexpr uint32_t kMaskTileBits = kMaskTileWords * 64;

struct MaskRange {
  const uint64_t* mask;
  uint64_t g_start, nbits, words;
};

__host__ __device__ inline MaskRange mask_range(const uint64_t* mask, uint64_t g_start, uint64_t nbits) {
  return MaskRange{mask, g_start, nbits, (nbits + 63) / 64};
}

// tiles of a range of nbits candidates
__host__ __device__ inline uint64_t mask_tiles(uint64_t nbits) {
  return (nbits + kMaskTileBits - 1) / kMaskTileBits;
}

// word wi of the range: bits past nbits dropped, 0 past the last word
__host__ __device__ __forceinline__ uint64_t mask_word(const MaskRange& r, uint64_t wi) {
  if (wi >= r.words) return 0ull;
  uint64_t b = r.mask[wi];
  if (wi == r.words - 1 && (r.nbits & 63)) b &= (1ull << (r.nbits & 63)) - 1;
  return b;
}

}  // namespace dse
