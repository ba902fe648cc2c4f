// dse_goldbach.hip -- minimal Goldbach partitions of a device-resident prime mask
// (gfx950): for every even 6 + 2c of a range the smallest rank i whose small prime
// P_i has 6 + 2c - P_i prime too, as one dse_goldbach (include/dse.h) in device
// memory: the histogram of the ranks, the largest of them and the unresolved evens.
//
// Two launches on the caller's stream; the launches are the only ordering and no
// workgroup waits on another:
//   gb_main_kernel   every workgroup walks its own contiguous run of tiles
//                    (kMaskTileBits candidates, one mask word of 64 evens per
//                    thread). A tile's line -- its 256 words and the kGbLowWords
//                    words below it, from the mask, from `below` or zeros
//                    (gb_bits64) -- is staged in LDS, the next tile's words already
//                    loaded; two lines in turn, so one barrier per tile. A thread
//                    walks the ranks upwards over the set U of its unresolved evens
//                    (dse_goldbach_word.h): the first kGbRegRanks ranks unrolled,
//                    their counts in registers (half of all evens resolve within
//                    four primes: one LDS atomic per hit would serialise on one
//                    address); the later ranks in a loop that reads h_i from
//                    constant memory (wave-uniform, scalar loads), counts the few
//                    hits by LDS atomics and leaves when the wave has nothing
//                    unresolved. The workgroup ends by storing a slab with plain
//                    stores: unresolved, first unresolved, the maximum, and the
//                    histogram bins up to it.
//   gb_close_kernel  32 workgroups, each summing 64 histogram bins over the slabs;
//                    workgroup 0 also sums the unresolved evens, reduces the first
//                    of them and the maximum and writes the scalar members.
// The maximum is tracked only in the loop over the later ranks. A run of tiles whose
// evens all resolve within kGbRegRanks primes (synthetic masks, small nprimes) is
// walked a second time with the tracking on.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dse_block.h"
#include "dse_goldbach_word.h"
#include "dse_internal.h"

namespace dse {
namespace {

constexpr uint32_t kGbThreads = kMaskTileWords;  // one mask word per thread
constexpr uint32_t kGbWaves = kGbThreads / 64;
// workgroups per compute unit of the one resident round the grid is: 4 with the 16 register counters of
// the production build (93 VGPRs; kGbMaxGrid holds 4 x 256 CUs), 3 for A/B builds with more (make resources)
constexpr uint32_t kGbGridPerCu = kGbRegRanks > 16 ? 3 : 4;
// the register counters are 32 bits wide and grow by at most 64 per tile: summed into LDS this often
constexpr uint32_t kGbFlushTiles = 1u << 20;
static_assert(kGbLineWords <= 2 * kGbThreads, "a thread stages at most two words of a line");
static_assert(kGbRegRanks <= kGbPrimes && kGbTable.h(kGbRegRanks - 1) <= 64 * kGbLowWords,
              "the unrolled windows stay in the line");

// a workgroup's slab, in uint64 words
constexpr uint32_t kSlUnres = 0, kSlFirst = 1, kSlMaxR = 2, kSlMaxC = 3, kSlBins = 4, kSlHist = 8,
                   kSlabWords = kSlHist + kGbPrimes;
// the closing kernel: one thread per slab, 64 bins per workgroup
constexpr uint32_t kClThreads = 1024, kClBins = 64, kClGroups = kGbPrimes / kClBins;
static_assert(kGbMaxGrid <= kClThreads, "the closing kernel reads one slab per thread");

// dse_goldbach as uint64 words
constexpr uint32_t kOutGStart = 0, kOutNbits = 1, kOutNprimes = 2, kOutResolved = 3, kOutUnres = 4, kOutFirst = 5,
                   kOutMaxR = 6, kOutMaxC = 7, kOutHist = 8;
static_assert(kOutHist + kGbPrimes == kGbWords, "dse_goldbach is kGbWords words");

// the table the loop over the later ranks reads: constant memory, the index wave-uniform
__constant__ GbTable c_gb_table = gb_make_table();

struct GbArgs {
  GbSrc s;
  uint64_t g_start, ntiles, tiles_per_wg;
  uint32_t nprimes;
};

// the workgroup's best (rank, candidate) in every thread (two barriers)
template <uint32_t kWaves>
__device__ __forceinline__ void gb_block_best(uint64_t& br, uint64_t& bc, unsigned long long* s_r,
                                              unsigned long long* s_c) {
  for (uint32_t o = 32; o > 0; o >>= 1) {
    const uint64_t r = (uint64_t)__shfl_xor((unsigned long long)br, o);
    const uint64_t c = (uint64_t)__shfl_xor((unsigned long long)bc, o);
    if (r != kGbNone && gb_better(r, c, br, bc)) {
      br = r;
      bc = c;
    }
  }
  __syncthreads();  // the arrays' last readers
  if ((threadIdx.x & 63u) == 0) {
    s_r[threadIdx.x >> 6] = br;
    s_c[threadIdx.x >> 6] = bc;
  }
  __syncthreads();
  br = s_r[0];
  bc = s_c[0];
  for (uint32_t i = 1; i < kWaves; ++i)
    if (s_r[i] != kGbNone && gb_better(s_r[i], s_c[i], br, bc)) {
      br = s_r[i];
      bc = s_c[i];
    }
}

__global__ __launch_bounds__(kGbThreads) void gb_main_kernel(GbArgs a, unsigned long long* __restrict__ slabs) {
  __shared__ unsigned long long s_hist[kGbPrimes];
  __shared__ uint64_t s_line[2][kGbLineWords + 1];  // + 1: the window of h = 0 loads (and drops) one 32-bit word more
  __shared__ unsigned long long s_unres, s_first;
  __shared__ unsigned long long s_r[kGbWaves], s_c[kGbWaves];
  const uint32_t tid = threadIdx.x, lane = tid & 63u;
  const uint32_t n = a.nprimes;

  for (uint32_t i = tid; i < kGbPrimes; i += kGbThreads) s_hist[i] = 0ull;
  if (tid == 0) {
    s_unres = 0ull;
    s_first = kGbNone;
  }
  __syncthreads();

  uint32_t cnt[kGbRegRanks];
#pragma unroll
  for (uint32_t i = 0; i < kGbRegRanks; ++i) cnt[i] = 0;
  uint64_t unres = 0, first = kGbNone;  // this thread's unresolved evens and the first of them
  uint64_t br = kGbNone, bc = kGbNone;  // its largest minimal rank and the lowest candidate that has it

  const uint64_t t0 = (uint64_t)blockIdx.x * a.tiles_per_wg;
  const uint64_t t1 = min(a.ntiles, t0 + a.tiles_per_wg);
  // word k of tile t's line: the positions from 64 (256 t - kGbLowWords + k) on
  auto fetch = [&](uint64_t t, uint32_t k) {
    return gb_bits64(a.s, ((int64_t)(t * kMaskTileWords) - (int64_t)kGbLowWords + (int64_t)k) * 64);
  };
  const bool two = tid + kGbThreads < kGbLineWords;
  const uint32_t d0 = 2u * (kGbLowWords + tid);  // this thread's word, in 32-bit words of the line

  // One walk over the run. track: the second walk, which only looks for the maximum among the
  // first kGbRegRanks ranks; the first walk does everything else.
  auto walk = [&](const bool track) {
    uint64_t x0 = 0, x1 = 0;
    if (t0 < t1) {
      x0 = fetch(t0, tid);
      if (two) x1 = fetch(t0, tid + kGbThreads);
    }
    uint32_t since = 0;
    for (uint64_t t = t0; t < t1; ++t) {
      uint64_t* const line = s_line[(uint32_t)(t - t0) & 1u];
      line[tid] = x0;
      if (two) line[tid + kGbThreads] = x1;
      __syncthreads();  // also: every thread is done with the other line
      if (t + 1 < t1) {
        x0 = fetch(t + 1, tid);
        if (two) x1 = fetch(t + 1, tid + kGbThreads);
      }
      const uint32_t* const l32 = reinterpret_cast<const uint32_t*>(line);
      auto ld = [&](uint32_t k) { return l32[k]; };
      const uint64_t wi = t * kMaskTileWords + tid;
      const uint64_t pos0 = wi * 64ull;
      uint64_t U = gb_evens(a.s.nbits, wi);
      if (track) {
        gb_search(U, c_gb_table, 0u, min(n, kGbRegRanks), d0, ld, [](uint64_t) { return true; },
                  [&](uint32_t i, uint64_t hit) {
                    if (hit && gb_better(i, pos0 + (uint32_t)__builtin_ctzll(hit), br, bc)) {
                      br = i;
                      bc = pos0 + (uint32_t)__builtin_ctzll(hit);
                    }
                  });
        continue;
      }
      U = gb_search_first<kGbRegRanks>(U, n, d0, ld, [&](uint32_t i, uint64_t hit) {
        cnt[i] += (uint32_t)__builtin_popcountll(hit);
      });
      U = gb_search(
          U, c_gb_table, kGbRegRanks, n, d0, ld, [](uint64_t u) { return __any(u != 0ull) != 0; },
          [&](uint32_t i, uint64_t hit) {
            if (hit) {
              atomicAdd(&s_hist[i], (unsigned long long)__builtin_popcountll(hit));
              const uint64_t c = pos0 + (uint32_t)__builtin_ctzll(hit);
              if (gb_better(i, c, br, bc)) {
                br = i;
                bc = c;
              }
            }
          });
      if (U) {
        unres += (uint32_t)__builtin_popcountll(U);
        if (first == kGbNone) first = pos0 + (uint32_t)__builtin_ctzll(U);  // the tiles come in increasing order
      }
      if (++since == kGbFlushTiles || t + 1 == t1) {
#pragma unroll
        for (uint32_t i = 0; i < kGbRegRanks; ++i) {
          const uint32_t r = wave_sum(cnt[i]);
          if (lane == 0 && r) atomicAdd(&s_hist[i], (unsigned long long)r);
          cnt[i] = 0;
        }
        since = 0;
      }
    }
  };

  walk(false);
  {
    const uint64_t u = wave_sum(unres);
    if (lane == 0 && u) atomicAdd(&s_unres, (unsigned long long)u);
    if (first != kGbNone) atomicMin(&s_first, (unsigned long long)first);
  }
  gb_block_best<kGbWaves>(br, bc, s_r, s_c);  // its barriers also make the LDS sums final
  if (br == kGbNone) {
    // nothing resolved at a later rank in the whole run: the maximum is among the first ranks
    walk(true);  // (the reduction's barriers: the first walk's last line is read no more)
    gb_block_best<kGbWaves>(br, bc, s_r, s_c);
  }

  unsigned long long* const sl = slabs + (uint64_t)blockIdx.x * kSlabWords;
  const uint32_t nb = br == kGbNone ? 0u : (uint32_t)br + 1u;  // bins above the maximum are 0
  for (uint32_t i = tid; i < nb; i += kGbThreads) sl[kSlHist + i] = s_hist[i];
  if (tid == 0) {
    sl[kSlUnres] = s_unres;
    sl[kSlFirst] = s_first;
    sl[kSlMaxR] = br;
    sl[kSlMaxC] = bc;
    sl[kSlBins] = nb;
  }
}

__global__ __launch_bounds__(kClThreads) void gb_close_kernel(GbArgs a, const unsigned long long* __restrict__ slabs,
                                                              uint32_t nslabs, unsigned long long* __restrict__ out) {
  __shared__ unsigned long long s_bins[kClBins];
  __shared__ unsigned long long s_unres, s_first;
  __shared__ unsigned long long s_r[kClThreads / 64], s_c[kClThreads / 64];
  const uint32_t tid = threadIdx.x, lane = tid & 63u;
  const uint32_t bin0 = blockIdx.x * kClBins;

  if (tid < kClBins) s_bins[tid] = 0ull;
  if (tid == 0) {
    s_unres = 0ull;
    s_first = kGbNone;
  }
  __syncthreads();
  // this workgroup's 64 bins over the slabs: 16 slabs at a time, 512 contiguous bytes of each
  {
    const uint32_t grp = tid >> 6, bin = bin0 + lane;
    uint64_t acc = 0;
    for (uint32_t s = grp; s < nslabs; s += kClThreads / 64) {
      const unsigned long long* const sl = slabs + (uint64_t)s * kSlabWords;
      if (bin < sl[kSlBins]) acc += sl[kSlHist + bin];
    }
    if (acc) atomicAdd(&s_bins[lane], (unsigned long long)acc);
  }
  __syncthreads();
  if (tid < kClBins) out[kOutHist + bin0 + tid] = s_bins[tid];
  if (blockIdx.x != 0) return;

  // workgroup 0: the scalar members
  const bool have = tid < nslabs;
  const unsigned long long* const my = slabs + (uint64_t)(have ? tid : 0u) * kSlabWords;
  {
    const uint64_t u = wave_sum(have ? (uint64_t)my[kSlUnres] : 0ull);
    if (lane == 0 && u) atomicAdd(&s_unres, (unsigned long long)u);
    if (have && my[kSlFirst] != kGbNone) atomicMin(&s_first, my[kSlFirst]);
  }
  uint64_t br = have ? (uint64_t)my[kSlMaxR] : kGbNone, bc = have ? (uint64_t)my[kSlMaxC] : kGbNone;
  gb_block_best<kClThreads / 64>(br, bc, s_r, s_c);  // its barriers also order the sums above
  if (tid == 0) {
    out[kOutGStart] = a.g_start;
    out[kOutNbits] = a.s.nbits;
    out[kOutNprimes] = a.nprimes;
    out[kOutResolved] = a.s.nbits - s_unres;
    out[kOutUnres] = s_unres;
    out[kOutFirst] = s_first == kGbNone ? kGbNone : a.g_start + s_first;
    out[kOutMaxR] = br;
    out[kOutMaxC] = br == kGbNone ? kGbNone : a.g_start + bc;
  }
}

}  // namespace

uint32_t goldbach_grid(uint64_t nbits, int num_cus, uint32_t grid_cap) {
  const uint64_t ntiles = mask_tiles(nbits);
  // every workgroup walks one fixed run of tiles, so the grid is one resident round
  uint64_t cap = grid_cap ? grid_cap : (uint64_t)kGbGridPerCu * (uint64_t)(num_cus > 0 ? num_cus : 1);
  if (cap > kGbMaxGrid) cap = kGbMaxGrid;
  if (ntiles <= cap) return (uint32_t)ntiles;
  const uint64_t per = (ntiles + cap - 1) / cap;
  return (uint32_t)((ntiles + per - 1) / per);
}

uint64_t goldbach_scratch_bytes(uint32_t grid) {
  return (uint64_t)(grid ? grid : 1u) * kSlabWords * sizeof(uint64_t);
}

hipError_t launch_goldbach(uint64_t g_start, uint64_t nbits, const uint64_t* mask, uint32_t mask_shift,
                           const uint64_t* below, uint32_t below_shift, uint64_t below_bits, uint32_t nprimes,
                           uint64_t* out, void* slabs, uint32_t grid, hipStream_t stream) {
  if (nprimes < 1 || nprimes > kGbPrimes || grid > kGbMaxGrid || mask_shift > 63 || below_shift > 63)
    return hipErrorInvalidValue;
  GbArgs a;
  a.s = GbSrc{mask, below, nbits, below_bits, mask_shift, below_shift};
  a.g_start = g_start;
  a.nprimes = nprimes;
  a.ntiles = mask_tiles(nbits);
  if ((a.ntiles != 0) != (grid != 0)) return hipErrorInvalidValue;
  a.tiles_per_wg = grid ? (a.ntiles + grid - 1) / grid : 0;
  unsigned long long* const sl = reinterpret_cast<unsigned long long*>(slabs);
  if (grid) hipLaunchKernelGGL(gb_main_kernel, dim3(grid), dim3(kGbThreads), 0, stream, a, sl);
  hipLaunchKernelGGL(gb_close_kernel, dim3(kClGroups), dim3(kClThreads), 0, stream, a, sl, grid,
                     reinterpret_cast<unsigned long long*>(out));
  return hipGetLastError();
}

}  // namespace dse
