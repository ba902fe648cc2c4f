// dse_tuples.hip -- constellations as numbers (gfx950): the positions of a
// device-resident prime mask at which a pattern (require, forbid) of span <= 32
// matches, as little-endian uint64 values 3 + 2 (g_start + position) of the
// lowest member, in increasing order.
//
// The count / scan / emit launches of primes as numbers (dse_primes.hip) on the
// tile bodies of dse_rank_emit.h; the word a thread hands them is not its mask
// word but that word's match word (dse_tuples_word.h), made on the fly:
//   tuples_size_kernel  per tile: its matches;
//   launch_rank_scan    dse_primes.hip's scan kernel, as it is;
//   tuples_emit_kernel  per tile inside the rank window: its matches by rank
//                       through the LDS staging window to out[rank - first].
// A thread loads its own word of the visible candidates once; the low half of
// the next word comes from the lane above it (one cross-lane move), and only a
// wave's last lane, which has no such neighbour, loads it from memory. The
// candidates above the range are read by the threads of the last one or two
// words alone. No workgroup waits on another: the launches are the only ordering.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dse_internal.h"
#include "dse_rank_emit.h"
#include "dse_tuples_word.h"

namespace dse {
namespace {

struct TuArgs {
  TupleSrc s;
  uint64_t first, end;  // the rank window [first, end)
};

// the match word of word w, w = this thread's word of a tile; every lane of the wave calls it
__device__ __forceinline__ uint64_t tu_match_word(const TuArgs& a, uint64_t w) {
  const uint64_t x = tuples_visible_word(a.s, w);
  uint32_t nx = __shfl_down((uint32_t)x, 1);
  if ((threadIdx.x & 63u) == 63u) nx = (uint32_t)tuples_visible_word(a.s, w + 1);
  return tuples_word(a.s, w, x, nx);
}

__global__ __launch_bounds__(kRankThreads) void tuples_size_kernel(TuArgs a, unsigned long long* __restrict__ sums) {
  __shared__ uint32_t s_wave[kRankWaves];
  const uint64_t w = (uint64_t)blockIdx.x * kMaskTileWords + threadIdx.x;
  rank_tile_size(tu_match_word(a, w), s_wave, sums);
}

__global__ __launch_bounds__(kRankThreads) void tuples_emit_kernel(TuArgs a, const unsigned long long* __restrict__ sums,
                                                                   uint64_t tile0, uint64_t* __restrict__ out) {
  __shared__ uint64_t s_val[kRankWindow];
  __shared__ uint32_t s_wave[kRankWaves];
  const uint64_t t = tile0 + blockIdx.x;
  uint64_t r0, lo, hi;
  if (!rank_tile_window(sums, t, a.first, a.end, r0, lo, hi)) return;
  const uint64_t w = t * kMaskTileWords + threadIdx.x;
  rank_tile_emit(tu_match_word(a, w), a.s.r.g_start + w * 64ull, r0, lo, hi, a.first, out, s_val, s_wave);
}

TuArgs tu_args(uint64_t g_start, uint64_t nbits, const uint64_t* mask, const TuplePattern& p, uint64_t first,
               uint64_t out_cap) {
  return TuArgs{TupleSrc{mask_range(mask, g_start, nbits), p.above, p.above_shift, p.above_bits, p.require, p.forbid},
                first, primes_window_end(first, out_cap)};
}

bool tu_valid(const TuplePattern& p) {
  return (p.require & 1u) && !(p.require & p.forbid) && p.above_bits <= kTuplesMaxAbove && p.above_shift < 64 &&
         (p.above || !p.above_bits);
}

}  // namespace

hipError_t launch_tuples_scan(uint64_t g_start, uint64_t nbits, const uint64_t* mask, const TuplePattern& p,
                              uint64_t first, uint64_t out_cap, unsigned long long* totals, void* tile_sums,
                              hipStream_t stream) {
  const uint64_t ntiles = mask_tiles(nbits);
  if (ntiles > 0x7FFFFFFFull || !tu_valid(p)) return hipErrorInvalidValue;
  if (ntiles)
    hipLaunchKernelGGL(tuples_size_kernel, dim3((uint32_t)ntiles), dim3(kRankThreads), 0, stream,
                       tu_args(g_start, nbits, mask, p, first, out_cap),
                       reinterpret_cast<unsigned long long*>(tile_sums));
  return launch_rank_scan(tile_sums, ntiles, first, out_cap, totals, stream);
}

hipError_t launch_tuples_emit(uint64_t g_start, uint64_t nbits, const uint64_t* mask, const TuplePattern& p,
                              uint64_t first, uint64_t* out, uint64_t out_cap, const void* tile_sums, uint64_t tile0,
                              uint64_t tiles, hipStream_t stream) {
  const uint64_t ntiles = mask_tiles(nbits);
  if (tile0 > ntiles || tiles > ntiles - tile0 || ntiles > 0x7FFFFFFFull || !tu_valid(p)) return hipErrorInvalidValue;
  if (!tiles || !out_cap) return hipSuccess;
  hipLaunchKernelGGL(tuples_emit_kernel, dim3((uint32_t)tiles), dim3(kRankThreads), 0, stream,
                     tu_args(g_start, nbits, mask, p, first, out_cap),
                     reinterpret_cast<const unsigned long long*>(tile_sums), tile0, out);
  return hipGetLastError();
}

}  // namespace dse
