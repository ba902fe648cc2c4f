// dse_primes.hip -- primes as numbers (gfx950): ordered stream compaction of a
// device-resident prime mask into little-endian uint64 values 3 + 2 (g_start +
// bit index), in increasing order.
//
// Three launches on the caller's stream, the count / scan / write shape of the
// base-prime compaction (dse_base.hip) and of the device finish (dse_finish.hip);
// the tile bodies are dse_rank_emit.h's, which dse_tuples.hip instantiates with
// match words, and the scan launch (launch_rank_scan) serves both:
//   primes_size_kernel  per tile of kMaskTileWords mask words: its entries (set bits);
//   rank_scan_kernel    one workgroup: 64-bit exclusive scan of the tile counts in
//                       place (the total behind them), and the call's totals;
//   primes_emit_kernel  per tile: its entries whose rank lies in the call's rank
//                       window [first, first + out_cap), placed by rank into an LDS
//                       staging window and stored to out[rank - first] with
//                       wave-contiguous 8-byte stores.
// A tile's rank interval is [sums[t], sums[t + 1]); a tile outside the window
// returns after reading those two values, so the host entry points launch the
// emit per slab of ranks over the tiles that hold them (launch_primes_emit's
// tile range). No workgroup waits on another: the launches are the only ordering.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dse_internal.h"
#include "dse_rank_emit.h"

namespace dse {
namespace {

struct PrArgs {
  MaskRange r;
  uint64_t first, end;  // the rank window [first, end)
};

__global__ __launch_bounds__(kRankThreads) void primes_size_kernel(PrArgs a, unsigned long long* __restrict__ sums) {
  __shared__ uint32_t s_wave[kRankWaves];
  const uint64_t w = (uint64_t)blockIdx.x * kMaskTileWords + threadIdx.x;
  rank_tile_size(mask_word(a.r, w), s_wave, sums);
}

// exclusive scan of the ntiles counts in place, sums[ntiles] = their total;
// totals[0] = entries of the range, totals[1] = entries inside the rank window
__global__ __launch_bounds__(kSliceThreads) void rank_scan_kernel(unsigned long long* __restrict__ sums, uint32_t ntiles,
                                                         uint64_t first, uint64_t out_cap,
                                                         unsigned long long* __restrict__ totals) {
  __shared__ uint64_t s_wave[kSliceThreads / 64];
  const ScanSlice<uint64_t> s = slice_scan(ntiles, s_wave, [&](uint32_t b) { return sums[b]; });
  uint64_t r = s.start;
  for (uint32_t b = s.b0; b < s.b1; ++b) {
    const uint64_t v = sums[b];
    sums[b] = r;
    r += v;
  }
  if (threadIdx.x == 0) {
    const uint64_t C = s.total;
    sums[ntiles] = C;
    totals[0] = C;
    totals[1] = C > first ? min(out_cap, C - first) : 0ull;
  }
}

__global__ __launch_bounds__(kRankThreads) void primes_emit_kernel(PrArgs a, const unsigned long long* __restrict__ sums,
                                                                   uint64_t tile0, uint64_t* __restrict__ out) {
  __shared__ uint64_t s_val[kRankWindow];
  __shared__ uint32_t s_wave[kRankWaves];
  const uint64_t t = tile0 + blockIdx.x;
  uint64_t r0, lo, hi;
  if (!rank_tile_window(sums, t, a.first, a.end, r0, lo, hi)) return;
  const uint64_t w = t * kMaskTileWords + threadIdx.x;
  rank_tile_emit(mask_word(a.r, w), a.r.g_start + w * 64ull, r0, lo, hi, a.first, out, s_val, s_wave);
}

PrArgs pr_args(uint64_t g_start, uint64_t nbits, const uint64_t* mask, uint64_t first, uint64_t out_cap) {
  return PrArgs{mask_range(mask, g_start, nbits), first, primes_window_end(first, out_cap)};
}

}  // namespace

uint64_t primes_scratch_bytes(uint64_t nbits) { return (mask_tiles(nbits) + 1) * sizeof(unsigned long long); }

hipError_t launch_rank_scan(void* tile_sums, uint64_t ntiles, uint64_t first, uint64_t out_cap,
                            unsigned long long* totals, hipStream_t stream) {
  if (ntiles > 0x7FFFFFFFull) return hipErrorInvalidValue;
  hipLaunchKernelGGL(rank_scan_kernel, dim3(1), dim3(kSliceThreads), 0, stream,
                     reinterpret_cast<unsigned long long*>(tile_sums), (uint32_t)ntiles, first, out_cap, totals);
  return hipGetLastError();
}

hipError_t launch_primes_scan(uint64_t g_start, uint64_t nbits, const uint64_t* mask, uint64_t first,
                              uint64_t out_cap, unsigned long long* totals, void* tile_sums, hipStream_t stream) {
  const uint64_t ntiles = mask_tiles(nbits);
  if (ntiles > 0x7FFFFFFFull) return hipErrorInvalidValue;
  unsigned long long* sums = reinterpret_cast<unsigned long long*>(tile_sums);
  if (ntiles)
    hipLaunchKernelGGL(primes_size_kernel, dim3((uint32_t)ntiles), dim3(kRankThreads), 0, stream,
                       pr_args(g_start, nbits, mask, first, out_cap), sums);
  return launch_rank_scan(sums, ntiles, first, out_cap, totals, stream);
}

hipError_t launch_primes_emit(uint64_t g_start, uint64_t nbits, const uint64_t* mask, uint64_t first, uint64_t* out,
                              uint64_t out_cap, const void* tile_sums, uint64_t tile0, uint64_t tiles,
                              hipStream_t stream) {
  const uint64_t ntiles = mask_tiles(nbits);
  if (tile0 > ntiles || tiles > ntiles - tile0 || ntiles > 0x7FFFFFFFull) return hipErrorInvalidValue;
  if (!tiles || !out_cap) return hipSuccess;
  hipLaunchKernelGGL(primes_emit_kernel, dim3((uint32_t)tiles), dim3(kRankThreads), 0, stream,
                     pr_args(g_start, nbits, mask, first, out_cap),
                     reinterpret_cast<const unsigned long long*>(tile_sums), tile0, out);
  return hipGetLastError();
}

}  // namespace dse
