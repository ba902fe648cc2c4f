// dse_slab.h -- the two-launch slab reduction of the units that turn a whole mask
// range into one small struct (dse_stats.hip, dse_goldbach.hip, dse_gaps.hip, dse_consec.hip; dse_race.hip puts a
// count launch over the same runs in front). Main launch: `grid`
// workgroups, each walking its own contiguous run of tiles (dse_mask.h) and ending
// with one slab of plain stores: scalars of the unit's own, the number of histogram
// bins it filled (word kSlBins) and those bins (from word kSlHist). Closing launch:
// one workgroup per kSlabCloseBins bins sums them over the slabs (dse_gaps.hip: takes their minimum; dse_consec.hip:
// the 64 bins of the row it writes, slab_sum_bins_at); workgroup 0 also
// reduces the scalars, one slab per thread. dse_sums.hip has no bins: its slabs hold multi-limb integers, which its one
// closing workgroup adds with slab_add_limbs / slab_fold_limbs. The launches are the only ordering.
// Slab and result layouts and the per-word bodies stay with each unit; so do the
// main kernels' flush of their register counters and slab stores, which a helper
// here compiled to another instruction stream (profiles/r14/slab_layer_codegen.txt).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dse_block.h"
#include "dse_mask.h"

namespace dse {

constexpr uint32_t kSlabCloseThreads = 1024;  // the closing kernel: one thread per slab
constexpr uint32_t kSlabCloseBins = 64;       // and 64 bins per workgroup

// Tiles after which a main kernel with one mask word per thread (dse_stats.hip, dse_race.hip,
// dse_goldbach.hip) empties its 32-bit register counters into LDS. A counter grows by at most 64 per
// tile (the bits of the thread's word), and the flush sums it over a wave in 32 bits first (wave_sum),
// so it is the wave's sum that must fit: 64 lanes x 64 x tiles <= 2^32 - 1, tiles <= 1,048,575. (2^20
// tiles is one too many: an all-ones run's wave sum is 2^32 exactly and wraps to 0.)
constexpr uint32_t kSlabFlushTiles = 0xFFFFFFFFu / (64u * 64u);
static_assert(64ull * 64ull * kSlabFlushTiles <= 0xFFFFFFFFull, "a wave's sum of the counters fits 32 bits");

// Workgroups of the main launch: every workgroup walks one fixed run of tiles, so the grid is one
// resident round of per_cu workgroups per compute unit (what the main kernel's registers admit,
// make resources), at most max_grid, 0 exactly for an empty range. grid_cap > 0: the tests' cap.
inline uint32_t slab_grid(uint64_t nbits, uint32_t per_cu, int num_cus, uint32_t grid_cap, uint32_t max_grid) {
  const uint64_t ntiles = mask_tiles(nbits);
  uint64_t cap = grid_cap ? grid_cap : (uint64_t)per_cu * (uint64_t)(num_cus > 0 ? num_cus : 1);
  if (cap > max_grid) cap = max_grid;
  if (ntiles <= cap) return (uint32_t)ntiles;
  const uint64_t per = (ntiles + cap - 1) / cap;
  return (uint32_t)((ntiles + per - 1) / per);
}

inline uint64_t slab_bytes(uint32_t grid, uint32_t slab_words) {
  return (uint64_t)(grid ? grid : 1u) * slab_words * sizeof(uint64_t);
}

// the runs of a launch; slab_run is false when `grid` is no grid of nbits candidates
struct SlabRun {
  uint64_t ntiles, tiles_per_wg;
};
inline bool slab_run(uint64_t nbits, uint32_t grid, SlabRun* r) {
  r->ntiles = mask_tiles(nbits);
  if ((r->ntiles != 0) != (grid != 0)) return false;
  r->tiles_per_wg = grid ? (r->ntiles + grid - 1) / grid : 0;
  return true;
}

// this workgroup's tiles [t0, t1)
__device__ __forceinline__ void slab_tiles(const SlabRun& r, uint64_t& t0, uint64_t& t1) {
  t0 = (uint64_t)blockIdx.x * r.tiles_per_wg;
  t1 = min(r.ntiles, t0 + r.tiles_per_wg);
}

// The closing kernel's column sum into s_bins[0 .. kSlabCloseBins), which the caller zeroes and
// fences with barriers of its own: 16 slabs at a time, 512 contiguous bytes of each.
// slab_sum_bins_at: the bins bin0 .. bin0 + kSlabCloseBins of a workgroup's own choice.
template <uint32_t kSlabWords, uint32_t kSlBins, uint32_t kSlHist>
__device__ __forceinline__ void slab_sum_bins_at(const unsigned long long* slabs, uint32_t nslabs, uint32_t bin0,
                                                 unsigned long long* s_bins) {
  const uint32_t grp = threadIdx.x >> 6, lane = threadIdx.x & 63u, bin = bin0 + lane;
  uint64_t acc = 0;
  for (uint32_t s = grp; s < nslabs; s += kSlabCloseThreads / 64) {
    const unsigned long long* const sl = slabs + (uint64_t)s * kSlabWords;
    if (bin < sl[kSlBins]) acc += sl[kSlHist + bin];
  }
  if (acc) atomicAdd(&s_bins[lane], (unsigned long long)acc);
}
template <uint32_t kSlabWords, uint32_t kSlBins, uint32_t kSlHist>
__device__ __forceinline__ void slab_sum_bins(const unsigned long long* slabs, uint32_t nslabs,
                                              unsigned long long* s_bins) {
  slab_sum_bins_at<kSlabWords, kSlBins, kSlHist>(slabs, nslabs, blockIdx.x * kSlabCloseBins, s_bins);
}

// The column minimum of a unit whose bins hold positions (~0: none), into s_bins[0 .. kSlabCloseBins),
// which the caller fills with ~0 and fences with barriers of its own: slab_sum_bins' walk.
template <uint32_t kSlabWords, uint32_t kSlBins, uint32_t kSlHist>
__device__ __forceinline__ void slab_min_bins(const unsigned long long* slabs, uint32_t nslabs,
                                              unsigned long long* s_bins) {
  const uint32_t grp = threadIdx.x >> 6, lane = threadIdx.x & 63u, bin = blockIdx.x * kSlabCloseBins + lane;
  uint64_t acc = ~0ull;
  for (uint32_t s = grp; s < nslabs; s += kSlabCloseThreads / 64) {
    const unsigned long long* const sl = slabs + (uint64_t)s * kSlabWords;
    if (bin < sl[kSlBins]) acc = min(acc, (uint64_t)sl[kSlHist + bin]);
  }
  if (acc != ~0ull) atomicMin(&s_bins[lane], (unsigned long long)acc);
}

// The sum over a workgroup of one multi-limb integer per thread (kLimbs little-endian uint64 limbs;
// dse_sums.hip: a thread's register accumulators in the main kernel, a slab's column in the closing
// one). Every limb goes as two 32-bit halves, each summed per wave and added to s_half[2 kLimbs],
// which the caller zeroes and fences with barriers of its own: a sum of 1024 halves stays below 2^42,
// so the order of the additions cannot matter. slab_fold_limbs then carries the halves into limbs.
template <uint32_t kLimbs>
__device__ __forceinline__ void slab_add_limbs(const uint64_t (&x)[kLimbs], unsigned long long* s_half) {
#pragma unroll
  for (uint32_t k = 0; k < 2 * kLimbs; ++k) {
    const uint64_t h = (k & 1u) ? x[k >> 1] >> 32 : x[k >> 1] & 0xFFFFFFFFull;
    const uint64_t r = wave_sum(h);
    if ((threadIdx.x & 63u) == 0 && r) atomicAdd(&s_half[k], (unsigned long long)r);
  }
}
template <uint32_t kLimbs>
__host__ __device__ __forceinline__ void slab_fold_limbs(const unsigned long long* s_half, uint64_t (&out)[kLimbs]) {
  uint64_t c = 0;  // what the halves below carry into this one: below 2^11
#pragma unroll
  for (uint32_t k = 0; k < kLimbs; ++k) {
    const uint64_t lo = s_half[2 * k] + c;
    const uint64_t hi = s_half[2 * k + 1] + (lo >> 32);
    out[k] = (lo & 0xFFFFFFFFull) | (hi << 32);
    c = hi >> 32;
  }
}

// the main launch unless the range is empty, then the closing launch over `bins` histogram bins
template <typename Args>
inline hipError_t slab_launch(void (*main_kernel)(Args, unsigned long long*),
                              void (*close_kernel)(Args, const unsigned long long*, uint32_t, unsigned long long*),
                              const Args& a, uint32_t grid, uint32_t main_threads, uint32_t bins, void* slabs,
                              uint64_t* out, hipStream_t stream) {
  unsigned long long* const sl = reinterpret_cast<unsigned long long*>(slabs);
  if (grid) hipLaunchKernelGGL(main_kernel, dim3(grid), dim3(main_threads), 0, stream, a, sl);
  hipLaunchKernelGGL(close_kernel, dim3(bins / kSlabCloseBins), dim3(kSlabCloseThreads), 0, stream, a, sl, grid,
                     reinterpret_cast<unsigned long long*>(out));
  return hipGetLastError();
}

}  // namespace dse
