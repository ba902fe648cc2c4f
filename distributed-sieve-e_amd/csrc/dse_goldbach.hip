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

#include "dse_goldbach_word.h"
#include "dse_internal.h"
#include "dse_slab.h"

namespace dse {
namespace {

constexpr uint32_t kGbThreads = kMaskTileWords;  // one mask word per thread
constexpr uint32_t kGbWaves = kGbThreads / 64;
// workgroups per compute unit of the one resident round the grid is: 4 with the 16 register counters of
// the production build (93 VGPRs; kGbMaxGrid holds 4 x 256 CUs), 3 for A/B builds with more (make resources)
constexpr uint32_t kGbGridPerCu = kGbRegRanks > 16 ? 3 : 4;
// the register counters are 32 bits wide and grow by at most 64 per tile; they are summed per wave in 32 bits
// and then into LDS this often, so that a wave's sum cannot wrap (kSlabFlushTiles, dse_slab.h)
constexpr uint32_t kGbFlushTiles = kSlabFlushTiles;
static_assert(kGbLineWords <= 2 * kGbThreads, "a thread stages at most two words of a line");
static_assert(kGbRegRanks <= kGbPrimes && kGbTable.h(kGbRegRanks - 1) <= 64 * kGbLowWords,
              "the unrolled windows stay in the line");

// a workgroup's slab, in uint64 words
constexpr uint32_t kSlUnres = 0, kSlFirst = 1, kSlMaxR = 2, kSlMaxC = 3, kSlBins = 4, kSlHist = 8,
                   kSlabWords = kSlHist + kGbPrimes;
constexpr uint32_t kClThreads = kSlabCloseThreads, kClBins = kSlabCloseBins;
static_assert(kGbMaxGrid <= kClThreads, "the closing kernel reads one slab per thread");

// dse_goldbach as uint64 words
constexpr uint32_t kOutGStart = 0, kOutNbits = 1, kOutNprimes = 2, kOutResolved = 3, kOutUnres = 4, kOutFirst = 5,
                   kOutMaxR = 6, kOutMaxC = 7, kOutHist = 8;
static_assert(kOutHist + kGbPrimes == kGbWords, "dse_goldbach is kGbWords words");

// the table the loop over the later ranks reads: constant memory, the index wave-uniform
__constant__ GbTable c_gb_table = gb_make_table();

struct GbArgs {
  GbSrc s;
  uint64_t g_start;
  SlabRun run;
  uint32_t nprimes;
};

// block_best's order: a maximum beats none (gb_better alone would let kGbNone win by r > br). Two
// returns: as one && expression it compiles to selects, another stream than the one measured.
__device__ __forceinline__ bool gb_best_better(uint64_t r, uint64_t c, uint64_t br, uint64_t bc) {
  if (r != kGbNone && gb_better(r, c, br, bc)) return true;
  return false;
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

  uint64_t t0, t1;
  slab_tiles(a.run, t0, t1);
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
  block_best<kGbWaves>(br, bc, s_r, s_c, gb_best_better);  // its barriers also make the LDS sums final
  if (br == kGbNone) {
    // nothing resolved at a later rank in the whole run: the maximum is among the first ranks
    walk(true);  // (the reduction's barriers: the first walk's last line is read no more)
    block_best<kGbWaves>(br, bc, s_r, s_c, gb_best_better);
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
  slab_sum_bins<kSlabWords, kSlBins, kSlHist>(slabs, nslabs, s_bins);
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
  block_best<kClThreads / 64>(br, bc, s_r, s_c, gb_best_better);  // its barriers also order the sums above
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
  return slab_grid(nbits, kGbGridPerCu, num_cus, grid_cap, kGbMaxGrid);
}

uint64_t goldbach_scratch_bytes(uint32_t grid) { return slab_bytes(grid, kSlabWords); }

hipError_t launch_goldbach(uint64_t g_start, uint64_t nbits, const uint64_t* mask, uint32_t mask_shift,
                           const uint64_t* below, uint32_t below_shift, uint64_t below_bits, uint32_t nprimes,
                           uint64_t* out, void* slabs, uint32_t grid, hipStream_t stream) {
  if (nprimes < 1 || nprimes > kGbPrimes || grid > kGbMaxGrid || mask_shift > 63 || below_shift > 63)
    return hipErrorInvalidValue;
  GbArgs a;
  a.s = GbSrc{mask, below, nbits, below_bits, mask_shift, below_shift};
  a.g_start = g_start;
  a.nprimes = nprimes;
  if (!slab_run(nbits, grid, &a.run)) return hipErrorInvalidValue;
  return slab_launch(gb_main_kernel, gb_close_kernel, a, grid, kGbThreads, kGbPrimes, slabs, out, stream);
}

}  // namespace dse
