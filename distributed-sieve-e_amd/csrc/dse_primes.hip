// dse_primes.hip -- primes as numbers (gfx950): ordered stream compaction of a
// device-resident prime mask into little-endian uint64 values 3 + 2 (g_start +
// bit index), in increasing order.
//
// Three launches on the caller's stream, the count / scan / write shape of the
// base-prime compaction (dse_base.hip) and of the device finish (dse_finish.hip):
//   primes_size_kernel  per tile of kMaskTileWords mask words: its entries (set bits);
//   primes_scan_kernel  one workgroup: 64-bit exclusive scan of the tile counts in
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

#include "dse_block.h"
#include "dse_internal.h"
#include "dse_primes_word.h"

namespace dse {
namespace {

constexpr uint32_t kPrThreads = kMaskTileWords;  // one mask word per thread
constexpr uint32_t kPrWaves = kPrThreads / 64;
// LDS staging window, in entries (16 KiB). A tile of a prime mask near 1e9 holds
// about 1,600 entries; an all-ones tile holds 16,384 and takes 8 windows.
constexpr uint32_t kPrWindow = 2048;

struct PrArgs {
  MaskRange r;
  uint64_t first, end;  // the rank window [first, end)
};

__global__ __launch_bounds__(kPrThreads) void primes_size_kernel(PrArgs a, unsigned long long* __restrict__ sums) {
  __shared__ uint32_t s_wave[kPrWaves];
  const uint64_t w = (uint64_t)blockIdx.x * kMaskTileWords + threadIdx.x;
  const uint32_t t = block_sum<kPrThreads>((uint32_t)__popcll(mask_word(a.r, w)), s_wave);
  if (threadIdx.x == 0) sums[blockIdx.x] = t;
}

// exclusive scan of the ntiles counts in place, sums[ntiles] = their total;
// totals[0] = entries of the range, totals[1] = entries inside the rank window
__global__ __launch_bounds__(kSliceThreads) void primes_scan_kernel(unsigned long long* __restrict__ sums, uint32_t ntiles,
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

__global__ __launch_bounds__(kPrThreads) void primes_emit_kernel(PrArgs a, const unsigned long long* __restrict__ sums,
                                                                 uint64_t tile0, uint64_t* __restrict__ out) {
  __shared__ uint64_t s_val[kPrWindow];
  __shared__ uint32_t s_wave[kPrWaves];
  const uint32_t tid = threadIdx.x;
  const uint64_t t = tile0 + blockIdx.x;
  // the tile's ranks [r0, r1) cut to the window: [lo, hi), the same in every thread
  const uint64_t r0 = sums[t], r1 = sums[t + 1];
  const uint64_t lo = max(r0, a.first), hi = min(r1, a.end);
  if (lo >= hi) return;

  const uint64_t w = t * kMaskTileWords + tid;
  uint64_t bits = mask_word(a.r, w);
  const uint32_t c = (uint32_t)__popcll(bits);
  uint32_t tile;
  uint64_t rank = r0 + (block_scan<kPrThreads>(c, s_wave, &tile) - c);  // of this word's lowest set bit
  const uint64_t gw = a.r.g_start + w * 64ull;

  for (uint64_t b = lo; b < hi; b += kPrWindow) {
    const uint64_t e = min(b + (uint64_t)kPrWindow, hi);
    // this word's entries of ranks [b, e) into the staging window by rank
    primes_word(bits, rank, gw, b, e, [&](uint64_t r, uint64_t v) { s_val[(uint32_t)(r - b)] = v; });
    __syncthreads();
    // the window to out[b - first ...]: lane i of a wave stores element i, 512 contiguous bytes
    const uint32_t n = (uint32_t)(e - b);
    uint64_t* const dst = out + (b - a.first);
    for (uint32_t i = tid; i < n; i += kPrThreads) dst[i] = s_val[i];
    __syncthreads();
  }
}

PrArgs pr_args(uint64_t g_start, uint64_t nbits, const uint64_t* mask, uint64_t first, uint64_t out_cap) {
  return PrArgs{mask_range(mask, g_start, nbits), first, primes_window_end(first, out_cap)};
}

}  // namespace

uint64_t primes_scratch_bytes(uint64_t nbits) { return (mask_tiles(nbits) + 1) * sizeof(unsigned long long); }

hipError_t launch_primes_scan(uint64_t g_start, uint64_t nbits, const uint64_t* mask, uint64_t first,
                              uint64_t out_cap, unsigned long long* totals, void* tile_sums, hipStream_t stream) {
  const uint64_t ntiles = mask_tiles(nbits);
  if (ntiles > 0x7FFFFFFFull) return hipErrorInvalidValue;
  unsigned long long* sums = reinterpret_cast<unsigned long long*>(tile_sums);
  if (ntiles)
    hipLaunchKernelGGL(primes_size_kernel, dim3((uint32_t)ntiles), dim3(kPrThreads), 0, stream,
                       pr_args(g_start, nbits, mask, first, out_cap), sums);
  hipLaunchKernelGGL(primes_scan_kernel, dim3(1), dim3(kSliceThreads), 0, stream, sums, (uint32_t)ntiles, first, out_cap,
                     totals);
  return hipGetLastError();
}

hipError_t launch_primes_emit(uint64_t g_start, uint64_t nbits, const uint64_t* mask, uint64_t first, uint64_t* out,
                              uint64_t out_cap, const void* tile_sums, uint64_t tile0, uint64_t tiles,
                              hipStream_t stream) {
  const uint64_t ntiles = mask_tiles(nbits);
  if (tile0 > ntiles || tiles > ntiles - tile0 || ntiles > 0x7FFFFFFFull) return hipErrorInvalidValue;
  if (!tiles || !out_cap) return hipSuccess;
  hipLaunchKernelGGL(primes_emit_kernel, dim3((uint32_t)tiles), dim3(kPrThreads), 0, stream,
                     pr_args(g_start, nbits, mask, first, out_cap),
                     reinterpret_cast<const unsigned long long*>(tile_sums), tile0, out);
  return hipGetLastError();
}

}  // namespace dse
