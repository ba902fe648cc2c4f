// dse_rank_emit.h -- the tile bodies of an ordered compaction by rank window
// (device only), shared by primes as numbers (dse_primes.hip) and the
// constellations as numbers (dse_tuples.hip). Each unit brings its word source:
// the 64 entries-or-not of mask word w (the mask word itself, or its match
// word); the entry of bit b of word w has the value 3 + 2 (g_start + 64 w + b).
//
//   rank_tile_size    a tile's entries into sums[tile] (the size launch);
//   launch_rank_scan  (dse_internal.h, one kernel in dse_primes.hip) turns the
//                     sums into each tile's first rank and writes the totals;
//   rank_tile_window  a tile's rank interval cut to the call's rank window;
//   rank_tile_emit    the tile's entries inside it, placed by rank into an LDS
//                     staging window and stored to out[rank - first] with
//                     wave-contiguous 8-byte stores.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dse_block.h"
#include "dse_mask.h"
#include "dse_primes_word.h"

namespace dse {

constexpr uint32_t kRankThreads = kMaskTileWords;  // one mask word per thread
constexpr uint32_t kRankWaves = kRankThreads / 64;
// LDS staging window, in entries (16 KiB). A tile of a prime mask near 1e9 holds
// about 1,600 entries; an all-ones tile holds 16,384 and takes 8 windows.
constexpr uint32_t kRankWindow = 2048;

// s_wave: kRankWaves elements of LDS
__device__ __forceinline__ void rank_tile_size(uint64_t bits, uint32_t* s_wave, unsigned long long* __restrict__ sums) {
  const uint32_t t = block_sum<kRankThreads>((uint32_t)__popcll(bits), s_wave);
  if (threadIdx.x == 0) sums[blockIdx.x] = t;
}

// tile t's ranks [r0, r1) cut to the window [first, end): [lo, hi), the same in every thread;
// false for a tile outside the window, which has read only those two sums
__device__ __forceinline__ bool rank_tile_window(const unsigned long long* __restrict__ sums, uint64_t t, uint64_t first,
                                                 uint64_t end, uint64_t& r0, uint64_t& lo, uint64_t& hi) {
  r0 = sums[t];
  const uint64_t r1 = sums[t + 1];
  lo = max(r0, first);
  hi = min(r1, end);
  return lo < hi;
}

// bits: this thread's word of tile t; gw: the odd index of its bit 0. s_val: kRankWindow elements
// of LDS, s_wave: kRankWaves. Every thread of the workgroup calls it.
__device__ __forceinline__ void rank_tile_emit(uint64_t bits, uint64_t gw, uint64_t r0, uint64_t lo, uint64_t hi,
                                               uint64_t first, uint64_t* __restrict__ out, uint64_t* s_val,
                                               uint32_t* s_wave) {
  const uint32_t tid = threadIdx.x;
  const uint32_t c = (uint32_t)__popcll(bits);
  uint32_t tile;
  uint64_t rank = r0 + (block_scan<kRankThreads>(c, s_wave, &tile) - c);  // of this word's lowest set bit

  for (uint64_t b = lo; b < hi; b += kRankWindow) {
    const uint64_t e = min(b + (uint64_t)kRankWindow, hi);
    // this word's entries of ranks [b, e) into the staging window by rank
    primes_word(bits, rank, gw, b, e, [&](uint64_t r, uint64_t v) { s_val[(uint32_t)(r - b)] = v; });
    __syncthreads();
    // the window to out[b - first ...]: lane i of a wave stores element i, 512 contiguous bytes
    const uint32_t n = (uint32_t)(e - b);
    uint64_t* const dst = out + (b - first);
    for (uint32_t i = tid; i < n; i += kRankThreads) dst[i] = s_val[i];
    __syncthreads();
  }
}

}  // namespace dse
