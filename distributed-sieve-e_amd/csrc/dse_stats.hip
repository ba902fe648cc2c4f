// dse_stats.hip -- statistics of a device-resident prime mask (gfx950): the
// matches of up to 8 constellation patterns, the histogram of the prime gaps
// and the maximal gap, as one dse_stats (include/dse.h) in device memory.
//
// Two launches on the caller's stream; the launches are the only ordering and
// no workgroup waits on another:
//   stats_main_kernel   every workgroup walks its own contiguous run of tiles
//                       (kMaskTileBits candidates, one mask word per thread;
//                       the words of the next three tiles are already in flight).
//                       A thread holds its word and the low half of the word
//                       after it (a plain global load, also across tile and
//                       workgroup seams), so patterns and the gaps of up to
//                       kStatsSmall places need no seam pass: both are counted
//                       bit-parallel into registers (dse_stats_word.h) and
//                       reach LDS once per workgroup, already summed per wave.
//                       Only the longer gaps take an LDS atomic each: inside a
//                       word by a loop over its few primes that have one, from
//                       word to word by a workgroup scan of "last prime so
//                       far", from tile to tile by a carry in registers. The
//                       workgroup ends by storing a slab with plain stores:
//                       counts, first and last prime, maximal gap, and the
//                       histogram bins up to its longest gap.
//   stats_close_kernel  16 workgroups, each summing 64 histogram bins over the
//                       slabs. Every one scans the slabs' first/last primes for
//                       the gaps that cross workgroup seams (the last prime is
//                       carried across empty runs); workgroup 0 also sums the
//                       counts, reduces the maximal gap (longest, then lowest)
//                       and writes the scalar members, head and tail.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dse_internal.h"
#include "dse_slab.h"
#include "dse_stats_word.h"

namespace dse {
namespace {

constexpr uint32_t kStThreads = kMaskTileWords;  // one mask word per thread
constexpr uint32_t kStWaves = kStThreads / 64;
constexpr uint32_t kStDepth = 3;  // tiles loaded together, one group ahead of the one worked on
// per-thread counters are 32 bits wide and grow by at most 64 per tile; they are summed per wave in 32
// bits and then into LDS this often, so that a wave's sum cannot wrap (kSlabFlushTiles, dse_slab.h)
constexpr uint32_t kStFlushTiles = kSlabFlushTiles;

// a workgroup's slab, in uint64 words
constexpr uint32_t kSlPrimes = 0, kSlFirst = 1, kSlLast1 = 2, kSlMaxD = 3, kSlMaxI = 4, kSlOverflow = 5, kSlBins = 6,
                   kSlMatches = 8, kSlHist = 16, kSlabWords = kSlHist + kStatsBins;
constexpr uint32_t kClThreads = kSlabCloseThreads, kClBins = kSlabCloseBins;
static_assert(kStatsMaxGrid <= kClThreads, "the closing kernel scans one slab per thread");

// dse_stats as uint64 words
constexpr uint32_t kOutGStart = 0, kOutNbits = 1, kOutPrimes = 2, kOutFirst = 3, kOutLast = 4, kOutHead = 5,
                   kOutTail = 6, kOutNPat = 7, kOutPat = 8, kOutMatches = 16, kOutMaxGap = 24, kOutMaxGapG = 25,
                   kOutOverflow = 26, kOutGaps = 27;
static_assert(kOutGaps + kStatsBins == kStatsWords, "dse_stats is kStatsWords words");

struct StArgs {
  MaskRange r;
  SlabRun run;
  uint64_t last_mask;  // the bits of the last word that lie inside the range
  uint32_t npat;
  uint32_t pat[8];
};

// Word wi of the range from v = mask[min(wi, words - 1)]: mask_word's result without a branch.
// The main kernel's tuned variant of the shared load: its raw loads are issued tiles ahead of
// their use, and the clipping works on what they brought with a precomputed last_mask.
__device__ __forceinline__ uint64_t st_fix(const StArgs& a, uint64_t wi, uint64_t v) {
  return wi < a.r.words ? v & (wi == a.r.words - 1 ? a.last_mask : ~0ull) : 0ull;
}

__global__ __launch_bounds__(kStThreads, 3) void stats_main_kernel(StArgs a, unsigned long long* __restrict__ slabs) {
  __shared__ unsigned long long s_hist[kStatsBins + 1];  // [kStatsBins]: the gaps of kStatsBins places and more
  __shared__ unsigned long long s_acc[9];                // matches[8], primes
  __shared__ unsigned long long s_first;                 // position of the run's first prime
  __shared__ unsigned long long s_bd[kStWaves], s_bi[kStWaves];
  __shared__ uint32_t s_wave[2][kStWaves];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;

  for (uint32_t i = tid; i <= kStatsBins; i += kStThreads) s_hist[i] = 0ull;
  if (tid < 9) s_acc[tid] = 0ull;
  if (tid == 0) s_first = kStatsNone;
  __syncthreads();

  uint32_t sm[kStatsSmall], mt[8], pc = 0;
#pragma unroll
  for (uint32_t d = 0; d < kStatsSmall; ++d) sm[d] = 0;
#pragma unroll
  for (uint32_t p = 0; p < 8; ++p) mt[p] = 0;
  uint64_t bd = 0, bi = kStatsNone;  // this thread's maximal long gap, in places, and its lower prime
  uint64_t carry = 0;                // position + 1 of the run's last prime so far (the same in every thread)

  auto put = [&](uint64_t d, uint64_t i) {
    atomicAdd(&s_hist[d < kStatsBins ? d : kStatsBins], 1ull);
    if (stats_better(d, i, bd, bi)) {
      bd = d;
      bi = i;
    }
  };
  // the register counters into LDS, summed per wave first
  auto flush = [&]() {
#pragma unroll
    for (uint32_t d = 0; d < kStatsSmall; ++d) {
      const uint32_t r = wave_sum(sm[d]);
      if (lane == 0 && r) atomicAdd(&s_hist[d + 1], (unsigned long long)r);
      sm[d] = 0;
    }
#pragma unroll
    for (uint32_t p = 0; p < 8; ++p) {
      const uint32_t r = wave_sum(mt[p]);
      if (lane == 0 && r) atomicAdd(&s_acc[p], (unsigned long long)r);
      mt[p] = 0;
    }
    const uint32_t r = wave_sum(pc);
    if (lane == 0 && r) atomicAdd(&s_acc[8], (unsigned long long)r);
    pc = 0;
  };

  uint64_t t0, t1;
  slab_tiles(a.run, t0, t1);
  // This thread's word of each of the tiles t .. t + kStDepth - 1 and the low half of the word
  // after it, as they lie in memory: plain loads at clamped addresses with no use behind them, so
  // all of them stay in flight; tile() drops what lies outside the range (st_fix).
  auto load_group = [&](uint64_t t, uint64_t(&W)[kStDepth], uint32_t(&X)[kStDepth]) {
    const uint64_t lastw = a.r.words - 1;
#pragma unroll
    for (uint32_t j = 0; j < kStDepth; ++j) {
      const uint64_t wi = min(t + j, t1 - 1) * kMaskTileWords + tid;
      W[j] = a.r.mask[min(wi, lastw)];
      X[j] = reinterpret_cast<const uint32_t*>(a.r.mask)[2 * min(wi + 1, lastw)];
    }
  };
  uint32_t since = 0;
  auto tile = [&](uint64_t t, uint64_t wraw, uint32_t xraw) {
    const uint64_t wi = t * kMaskTileWords + tid;
    const uint64_t pos0 = wi * 64ull;
    const uint64_t w = st_fix(a, wi, wraw);
    const uint32_t nx = (uint32_t)st_fix(a, wi + 1, xraw);

    pc += stats_pop64(w);
#pragma unroll
    for (uint32_t p = 0; p < 8; ++p)
      if (p < a.npat) mt[p] += stats_pattern_word(w, nx, a.pat[p]);
    const uint64_t rem = stats_small_gaps(w, nx, sm);

    // exclusive scan (maximum) of "tile position + 1 of the last prime so far"
    const uint32_t x = wave_scan(w ? tid * 64u + stats_msb64(w) + 1u : 0u, ScanMax());
    uint32_t ex = __shfl_up(x, 1);
    if (lane == 0) ex = 0;
    // the waves' maxima through LDS: two sets by tile parity, so one barrier per tile orders them
    uint32_t* const sw = s_wave[(uint32_t)(t - t0) & 1u];
    if (lane == 63) sw[wave] = x;
    __syncthreads();
    uint32_t tot = 0;
    for (uint32_t i = 0; i < kStWaves; ++i) {
      const uint32_t u = sw[i];
      if (i < wave) ex = max(ex, u);
      tot = max(tot, u);
    }
    const uint64_t tile0 = t * (uint64_t)kMaskTileBits;
    const uint64_t prev1 = ex ? tile0 + ex : carry;
    if (w) {
      const uint64_t f = pos0 + stats_ctz64(w);
      if (prev1)
        stats_cross(f, prev1, put);
      else
        s_first = f;  // one thread of the workgroup, once
    }
    stats_inword_large(w, rem, pos0, put);
    if (tot) carry = tile0 + tot;
    if (++since == kStFlushTiles) {
      flush();
      since = 0;
    }
  };

  if (t0 < t1) {
    // two register sets in turn: a group's loads are issued a whole group of work before their first use
    uint64_t Wa[kStDepth], Wb[kStDepth];
    uint32_t Xa[kStDepth], Xb[kStDepth];
    auto work = [&](uint64_t t, const uint64_t(&W)[kStDepth], const uint32_t(&X)[kStDepth]) {
#pragma unroll
      for (uint32_t j = 0; j < kStDepth; ++j)
        if (t + j < t1) tile(t + j, W[j], X[j]);
    };
    load_group(t0, Wa, Xa);
    for (uint64_t t = t0; t < t1; t += 2 * kStDepth) {
      load_group(t + kStDepth, Wb, Xb);
      work(t, Wa, Xa);
      load_group(t + 2 * kStDepth, Wa, Xa);
      work(t + kStDepth, Wb, Xb);
    }
  }
  flush();
  block_best<kStWaves>(bd, bi, s_bd, s_bi, stats_better);

  if (bd == 0 && carry != 0) {
    // no gap of more than kStatsSmall places in the whole run (synthetic masks, tiny
    // ranges): its maximal gap is a short one, found by a second walk
    bi = kStatsNone;
    for (uint64_t t = t0; t < t1; ++t) {
      const uint64_t wi = t * kMaskTileWords + tid;
      stats_small_best(mask_word(a.r, wi), (uint32_t)mask_word(a.r, wi + 1), wi * 64ull, bd, bi);
    }
    block_best<kStWaves>(bd, bi, s_bd, s_bi, stats_better);
  }

  // the slab: the barriers above made every LDS sum final
  unsigned long long* const sl = slabs + (uint64_t)blockIdx.x * kSlabWords;
  const uint32_t nb = bd < kStatsBins ? (uint32_t)bd + 1u : kStatsBins;  // bins above the longest gap are 0
  for (uint32_t i = tid; i < nb; i += kStThreads) sl[kSlHist + i] = s_hist[i];
  if (tid < 8) sl[kSlMatches + tid] = s_acc[tid];
  if (tid == 0) {
    sl[kSlPrimes] = s_acc[8];
    sl[kSlFirst] = s_first;
    sl[kSlLast1] = carry;
    sl[kSlMaxD] = bd;
    sl[kSlMaxI] = bi;
    sl[kSlOverflow] = s_hist[kStatsBins];
    sl[kSlBins] = nb;
  }
}

__global__ __launch_bounds__(kClThreads) void stats_close_kernel(StArgs a, const unsigned long long* __restrict__ slabs,
                                                                 uint32_t nslabs,
                                                                 unsigned long long* __restrict__ out) {
  __shared__ unsigned long long s_scan[kClThreads];
  __shared__ unsigned long long s_bins[kClBins + 1];  // [kClBins]: seam gaps of kStatsBins places and more
  __shared__ unsigned long long s_acc[11];            // matches[8], primes, overflow, first
  __shared__ unsigned long long s_bd[kClThreads / 64], s_bi[kClThreads / 64];
  const uint32_t tid = threadIdx.x, lane = tid & 63u;
  const uint32_t bin0 = blockIdx.x * kClBins;
  const bool lead = blockIdx.x == 0;

  if (tid <= kClBins) s_bins[tid] = 0ull;
  if (tid < 10) s_acc[tid] = 0ull;
  if (tid == 10) s_acc[10] = kStatsNone;
  const bool have = tid < nslabs;
  const unsigned long long* const my = slabs + (uint64_t)(have ? tid : 0u) * kSlabWords;
  const uint64_t first = have ? my[kSlFirst] : kStatsNone;
  s_scan[tid] = have ? my[kSlLast1] : 0ull;
  __syncthreads();
  // inclusive scan (maximum) of the slabs' "position + 1 of the last prime": carries it across empty slabs
  for (uint32_t o = 1; o < kClThreads; o <<= 1) {
    const uint64_t y = tid >= o ? s_scan[tid - o] : 0ull;
    __syncthreads();
    if (y > s_scan[tid]) s_scan[tid] = y;
    __syncthreads();
  }
  const uint64_t prev1 = tid ? s_scan[tid - 1] : 0ull;
  const uint64_t last1 = s_scan[kClThreads - 1];

  // the gap that crosses into this slab, when it is a long one (short ones were counted by the main kernel)
  uint64_t bd = 0, bi = kStatsNone;
  if (first != kStatsNone && prev1) {
    const uint64_t d = first - (prev1 - 1);
    if (d > kStatsSmall) {
      bd = d;
      bi = prev1 - 1;
      if (d >= kStatsBins) {
        if (lead) atomicAdd(&s_bins[kClBins], 1ull);
      } else if (d >= bin0 && d < bin0 + kClBins) {
        atomicAdd(&s_bins[(uint32_t)d - bin0], 1ull);
      }
    }
  }

  slab_sum_bins<kSlabWords, kSlBins, kSlHist>(slabs, nslabs, s_bins);
  __syncthreads();
  if (tid < kClBins) out[kOutGaps + bin0 + tid] = s_bins[tid];
  if (!lead) return;

  // workgroup 0: the scalar members
#pragma unroll
  for (uint32_t k = 0; k < 10; ++k) {
    const uint32_t src = k < 8 ? kSlMatches + k : k == 8 ? kSlPrimes : kSlOverflow;
    const uint64_t r = wave_sum(have ? my[src] : 0ull);
    if (lane == 0 && r) atomicAdd(&s_acc[k], (unsigned long long)r);
  }
  if (first != kStatsNone) atomicMin(&s_acc[10], (unsigned long long)first);
  if (have && stats_better(my[kSlMaxD], my[kSlMaxI], bd, bi)) {
    bd = my[kSlMaxD];
    bi = my[kSlMaxI];
  }
  block_best<kClThreads / 64>(bd, bi, s_bd, s_bi, stats_better);  // its barriers also order the sums above
  if (tid == 0) {
    out[kOutGStart] = a.r.g_start;
    out[kOutNbits] = a.r.nbits;
    out[kOutPrimes] = s_acc[8];
    out[kOutFirst] = s_acc[10] == kStatsNone ? kStatsNone : a.r.g_start + s_acc[10];
    out[kOutLast] = last1 ? a.r.g_start + (last1 - 1) : kStatsNone;
    const uint64_t head = stats_bits64(a.r, 0);
    out[kOutHead] = head;
    out[kOutTail] = a.r.nbits >= 64  ? stats_bits64(a.r, a.r.nbits - 64)
                    : a.r.nbits == 0 ? 0ull
                                     : head << (64 - a.r.nbits);
    out[kOutNPat] = a.npat;
    for (uint32_t p = 0; p < 8; ++p) {
      out[kOutPat + p] = p < a.npat ? a.pat[p] : 0u;
      out[kOutMatches + p] = s_acc[p];
    }
    out[kOutMaxGap] = 2ull * bd;
    out[kOutMaxGapG] = bd ? a.r.g_start + bi : kStatsNone;
    out[kOutOverflow] = s_acc[9] + s_bins[kClBins];
  }
}

}  // namespace

uint32_t stats_grid(uint64_t nbits, int num_cus, uint32_t grid_cap) {
  return slab_grid(nbits, 3, num_cus, grid_cap, kStatsMaxGrid);  // stats_main_kernel's registers admit 3 per CU
}

uint64_t stats_scratch_bytes(uint32_t grid) { return slab_bytes(grid, kSlabWords); }

hipError_t launch_stats(uint64_t g_start, uint64_t nbits, const uint64_t* mask, const uint32_t* patterns,
                        uint32_t npatterns, uint64_t* stats, void* slabs, uint32_t grid, hipStream_t stream) {
  if (npatterns > 8 || grid > kStatsMaxGrid) return hipErrorInvalidValue;
  StArgs a;
  a.r = mask_range(mask, g_start, nbits);
  a.last_mask = (nbits & 63) ? (1ull << (nbits & 63)) - 1 : ~0ull;
  if (!slab_run(nbits, grid, &a.run)) return hipErrorInvalidValue;
  a.npat = npatterns;
  for (uint32_t p = 0; p < 8; ++p) a.pat[p] = p < npatterns ? patterns[p] : 0u;
  return slab_launch(stats_main_kernel, stats_close_kernel, a, grid, kStThreads, kStatsBins, slabs, stats, stream);
}

}  // namespace dse
