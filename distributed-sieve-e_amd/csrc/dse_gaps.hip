// dse_gaps.hip -- where the prime gaps of a device-resident mask are (gfx950): the
// first occurrence of every gap, the first and last prime, the prime count and
// the maximal gap, as one dse_gaps (include/dse.h) in device memory.
//
// Two launches of the slab reduction (dse_slab.h) on the caller's stream; the
// launches are the only ordering and no workgroup waits on another:
//   gaps_main_kernel   every workgroup walks its own contiguous run of tiles with
//                      stats_main_kernel's structure (one mask word per thread and
//                      the low half of the word after it, the words of the next
//                      three tiles in flight; word to word by a workgroup scan of
//                      "last prime so far", tile to tile by a register carry) and
//                      keeps its run's table in LDS: per gap size the lowest
//                      position, lowered by "read the entry, 64-bit LDS minimum
//                      if mine is lower". Once per tile every wave turns the
//                      entries of the bins below kGapsSettled into a uniform
//                      bitmap of settled bins (dse_gaps_word.h): an entry below
//                      the lowest position the run can still produce. With every
//                      short bin settled a tile is one OR-of-shifts by doubling,
//                      a scan, and the rare long gaps that are not settled yet.
//                      An entry only ever holds a position where that gap is, so
//                      "entry < floor" means the same whichever wave wrote it and
//                      whenever: waves a barrier apart cannot mislead each other.
//                      The workgroup ends by storing a slab with plain stores:
//                      prime count, first and last prime, maximal gap (the
//                      highest bin of the table, or the longest gap of
//                      kGapsBins places and more, tracked in registers), a
//                      bitmap of the bins it found, and the table up to its
//                      longest gap.
//   gaps_close_kernel  16 workgroups, each taking the minimum of 64 bins over the
//                      slabs. Every one scans the slabs' first/last primes for the
//                      long gaps that cross workgroup seams (the last prime is
//                      carried across empty runs); workgroup 0 also sums the
//                      count, ORs the found bitmaps, reduces the maximal gap
//                      (longest, then lowest) and writes the scalar members.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dse_gaps_word.h"
#include "dse_internal.h"
#include "dse_slab.h"

namespace dse {
namespace {

constexpr uint32_t kGpThreads = kMaskTileWords;  // one mask word per thread
constexpr uint32_t kGpWaves = kGpThreads / 64;
constexpr uint32_t kGpDepth = 3;  // tiles loaded together, one group ahead of the one worked on

// a workgroup's slab, in uint64 words
constexpr uint32_t kSlPrimes = 0, kSlFirst = 1, kSlLast1 = 2, kSlMaxD = 3, kSlMaxI = 4, kSlOverflow = 5, kSlBins = 6,
                   kSlFound = 8, kSlTab = kSlFound + kGapsBins / 64, kSlabWords = kSlTab + kGapsBins;
constexpr uint32_t kClThreads = kSlabCloseThreads, kClBins = kSlabCloseBins;
static_assert(kGapsMaxGrid <= kClThreads, "the closing kernel scans one slab per thread");
static_assert(kGapsBins % kGpThreads == 0, "the slab's found bitmap: whole steps of one bin per thread");

// dse_gaps as uint64 words
constexpr uint32_t kOutGStart = 0, kOutNbits = 1, kOutPrimes = 2, kOutFirst = 3, kOutLast = 4, kOutFound = 5,
                   kOutMaxGap = 6, kOutMaxGapG = 7, kOutOverflow = 8, kOutTab = 9;
static_assert(kOutTab + kGapsBins == kGapsWords, "dse_gaps is kGapsWords words");

struct GpArgs {
  MaskRange r;
  SlabRun run;
  uint64_t last_mask;  // the bits of the last word that lie inside the range
};

// Word wi of the range from v = mask[min(wi, words - 1)]: mask_word's result without a branch.
__device__ __forceinline__ uint64_t gp_fix(const GpArgs& a, uint64_t wi, uint64_t v) {
  return wi < a.r.words ? v & (wi == a.r.words - 1 ? a.last_mask : ~0ull) : 0ull;
}

__global__ __launch_bounds__(kGpThreads, 4) void gaps_main_kernel(GpArgs a, unsigned long long* __restrict__ slabs) {
  __shared__ unsigned long long s_tab[kGapsBins + 1];  // [kGapsBins]: the first gap of kGapsBins places and more
  __shared__ unsigned long long s_first;               // position of the run's first prime
  __shared__ unsigned long long s_primes;
  __shared__ unsigned long long s_bd[kGpWaves], s_bi[kGpWaves];
  __shared__ uint32_t s_wave[2][kGpWaves];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;

  for (uint32_t i = tid; i <= kGapsBins; i += kGpThreads) s_tab[i] = kGapsNone;
  if (tid == 0) {
    s_first = kGapsNone;
    s_primes = 0ull;
  }
  __syncthreads();

  uint64_t pc = 0;
  uint64_t bd = 0, bi = kGapsNone;  // this thread's maximal gap of kGapsBins places and more, and its lower prime
  uint64_t carry = 0;               // position + 1 of the run's last prime so far (the same in every thread)
  GapsSettled st = {0ull, 0ull};    // the same in every thread of a wave

  auto put = [&](uint64_t d, uint64_t i) {
    unsigned long long* const e = &s_tab[d < kGapsBins ? d : kGapsBins];
    if (i < *e) atomicMin(e, (unsigned long long)i);
    if (d >= kGapsBins && stats_better(d, i, bd, bi)) {
      bd = d;
      bi = i;
    }
  };

  // The short gaps: the loop over d is uniform, so the lanes that arrive here together hold the
  // same d, and of them the lowest lane holds the lowest position: it alone goes to the table.
  // A lane that finds another d in the lowest lane goes itself, so any grouping gives the minimum.
  auto put_small = [&](uint64_t d, uint64_t i) {
    const uint32_t low = stats_ctz64(__ballot(1));
    if (lane == low || (uint32_t)__shfl((int)d, (int)low) != (uint32_t)d) put(d, i);
  };

  uint64_t t0, t1;
  slab_tiles(a.run, t0, t1);
  // This thread's word of each of the tiles t .. t + kGpDepth - 1 and the low half of the word
  // after it, as they lie in memory: plain loads at clamped addresses with no use behind them, so
  // all of them stay in flight; tile() drops what lies outside the range (gp_fix).
  auto load_group = [&](uint64_t t, uint64_t(&W)[kGpDepth], uint32_t(&X)[kGpDepth]) {
    const uint64_t lastw = a.r.words - 1;
#pragma unroll
    for (uint32_t j = 0; j < kGpDepth; ++j) {
      const uint64_t wi = min(t + j, t1 - 1) * kMaskTileWords + tid;
      W[j] = a.r.mask[min(wi, lastw)];
      X[j] = reinterpret_cast<const uint32_t*>(a.r.mask)[2 * min(wi + 1, lastw)];
    }
  };
  auto tile = [&](uint64_t t, uint64_t wraw, uint32_t xraw) {
    const uint64_t wi = t * kMaskTileWords + tid;
    const uint64_t pos0 = wi * 64ull;
    const uint64_t w = gp_fix(a, wi, wraw);
    const uint32_t nx = (uint32_t)gp_fix(a, wi + 1, xraw);

    pc += stats_pop64(w);
    // the short gaps, under the settled bits of the tile before: this tile's floor is higher
    const uint64_t rem = gaps_small(w, nx, pos0, st.lo, put_small);

    // exclusive scan (maximum) of "tile position + 1 of the last prime so far"
    const uint32_t x = wave_scan(w ? tid * 64u + stats_msb64(w) + 1u : 0u, ScanMax());
    uint32_t ex = __shfl_up(x, 1);
    if (lane == 0) ex = 0;
    // the waves' maxima through LDS: two sets by tile parity, so one barrier per tile orders them
    uint32_t* const sw = s_wave[(uint32_t)(t - t0) & 1u];
    if (lane == 63) sw[wave] = x;
    __syncthreads();
    uint32_t tot = 0;
    for (uint32_t i = 0; i < kGpWaves; ++i) {
      const uint32_t u = sw[i];
      if (i < wave) ex = max(ex, u);
      tot = max(tot, u);
    }
    const uint64_t tile0 = t * (uint64_t)kMaskTileBits;
    // The settled bits of this tile: whatever a wave ahead or behind has written by now, an entry
    // below this tile's floor is a position that no put of this tile or a later one can beat.
    const uint64_t floor = gaps_floor(tile0, carry);
    st.lo = __ballot(gaps_settled_bit(s_tab[lane], floor));
    st.hi = __ballot(gaps_settled_bit(s_tab[64u + lane], floor));

    const uint64_t prev1 = ex ? tile0 + ex : carry;
    if (w) {
      const uint64_t f = pos0 + stats_ctz64(w);
      if (prev1)
        gaps_cross(f, prev1, st, put);
      else
        s_first = f;  // one thread of the workgroup, once
    }
    gaps_inword_large(w, rem, pos0, st, put);
    if (tot) carry = tile0 + tot;
  };

  if (t0 < t1) {
    // two register sets in turn: a group's loads are issued a whole group of work before their first use
    uint64_t Wa[kGpDepth], Wb[kGpDepth];
    uint32_t Xa[kGpDepth], Xb[kGpDepth];
    auto work = [&](uint64_t t, const uint64_t(&W)[kGpDepth], const uint32_t(&X)[kGpDepth]) {
#pragma unroll
      for (uint32_t j = 0; j < kGpDepth; ++j)
        if (t + j < t1) tile(t + j, W[j], X[j]);
    };
    load_group(t0, Wa, Xa);
    for (uint64_t t = t0; t < t1; t += 2 * kGpDepth) {
      load_group(t + kGpDepth, Wb, Xb);
      work(t, Wa, Xa);
      load_group(t + 2 * kGpDepth, Wa, Xa);
      work(t + kGpDepth, Wb, Xb);
    }
  }
  {
    const uint64_t r = wave_sum(pc);
    if (lane == 0 && r) atomicAdd(&s_primes, (unsigned long long)r);
  }
  __syncthreads();  // the table is final

  // the bins this run found, 64 per wave and step, and the highest of them as the maximal gap
  unsigned long long* const sl = slabs + (uint64_t)blockIdx.x * kSlabWords;
#pragma unroll
  for (uint32_t k = 0; k < kGapsBins / kGpThreads; ++k) {
    const uint32_t bin = k * kGpThreads + tid;
    const uint64_t e = s_tab[bin];
    const uint64_t m = __ballot(e != kGapsNone);
    if (lane == 0) sl[kSlFound + k * kGpWaves + wave] = m;
    if (e != kGapsNone && stats_better(bin, e, bd, bi)) {
      bd = bin;
      bi = e;
    }
  }
  block_best<kGpWaves>(bd, bi, s_bd, s_bi, stats_better);

  const uint32_t nb = bd < kGapsBins ? (uint32_t)bd + 1u : kGapsBins;  // bins above the longest gap are empty
  for (uint32_t i = tid; i < nb; i += kGpThreads) sl[kSlTab + i] = s_tab[i];
  if (tid == 0) {
    sl[kSlPrimes] = s_primes;
    sl[kSlFirst] = s_first;
    sl[kSlLast1] = carry;
    sl[kSlMaxD] = bd;
    sl[kSlMaxI] = bi;
    sl[kSlOverflow] = s_tab[kGapsBins];
    sl[kSlBins] = nb;
  }
}

__global__ __launch_bounds__(kClThreads) void gaps_close_kernel(GpArgs a, const unsigned long long* __restrict__ slabs,
                                                                uint32_t nslabs,
                                                                unsigned long long* __restrict__ out) {
  __shared__ unsigned long long s_scan[kClThreads];
  __shared__ unsigned long long s_bins[kClBins + 1];  // [kClBins]: seam gaps of kGapsBins places and more
  __shared__ unsigned long long s_found[kGapsBins / 64];
  __shared__ unsigned long long s_acc[3];  // primes, overflow, first
  __shared__ unsigned long long s_bd[kClThreads / 64], s_bi[kClThreads / 64];
  const uint32_t tid = threadIdx.x, lane = tid & 63u;
  const uint32_t bin0 = blockIdx.x * kClBins;
  const bool lead = blockIdx.x == 0;

  if (tid <= kClBins) s_bins[tid] = kGapsNone;
  if (tid < kGapsBins / 64) s_found[tid] = 0ull;
  if (tid == 0) s_acc[0] = 0ull;
  if (tid == 1 || tid == 2) s_acc[tid] = kGapsNone;
  const bool have = tid < nslabs;
  const unsigned long long* const my = slabs + (uint64_t)(have ? tid : 0u) * kSlabWords;
  const uint64_t first = have ? my[kSlFirst] : kGapsNone;
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

  // the gap that crosses into this slab, when it is a long one (short ones were put by the main kernel)
  uint64_t bd = 0, bi = kGapsNone;
  if (first != kGapsNone && prev1) {
    const uint64_t d = first - (prev1 - 1);
    if (d > kGapsSmall) {
      bd = d;
      bi = prev1 - 1;
      if (d >= kGapsBins) {
        if (lead) atomicMin(&s_bins[kClBins], (unsigned long long)bi);
      } else {
        if (d >= bin0 && d < bin0 + kClBins) atomicMin(&s_bins[(uint32_t)d - bin0], (unsigned long long)bi);
        if (lead) atomicOr(&s_found[d >> 6], 1ull << (d & 63));
      }
    }
  }

  slab_min_bins<kSlabWords, kSlBins, kSlTab>(slabs, nslabs, s_bins);
  __syncthreads();
  if (tid < kClBins) {
    const uint64_t e = s_bins[tid];
    out[kOutTab + bin0 + tid] = e == kGapsNone ? kGapsNone : a.r.g_start + e;
  }
  if (!lead) return;

  // workgroup 0: the scalar members
  {
    const uint64_t r = wave_sum(have ? (uint64_t)my[kSlPrimes] : 0ull);
    if (lane == 0 && r) atomicAdd(&s_acc[0], (unsigned long long)r);
  }
  if (have) {
    if (my[kSlOverflow] != kGapsNone) atomicMin(&s_acc[1], my[kSlOverflow]);
    for (uint32_t k = 0; k < kGapsBins / 64; ++k) {
      const uint64_t m = my[kSlFound + k];
      if (m) atomicOr(&s_found[k], (unsigned long long)m);
    }
  }
  if (first != kGapsNone) atomicMin(&s_acc[2], (unsigned long long)first);
  if (have && stats_better(my[kSlMaxD], my[kSlMaxI], bd, bi)) {
    bd = my[kSlMaxD];
    bi = my[kSlMaxI];
  }
  block_best<kClThreads / 64>(bd, bi, s_bd, s_bi, stats_better);  // its barriers also order the atomics above
  if (tid == 0) {
    out[kOutGStart] = a.r.g_start;
    out[kOutNbits] = a.r.nbits;
    out[kOutPrimes] = s_acc[0];
    out[kOutFirst] = s_acc[2] == kGapsNone ? kGapsNone : a.r.g_start + s_acc[2];
    out[kOutLast] = last1 ? a.r.g_start + (last1 - 1) : kGapsNone;
    uint64_t found = 0;
    for (uint32_t k = 0; k < kGapsBins / 64; ++k) found += stats_pop64(s_found[k]);
    out[kOutFound] = found;
    out[kOutMaxGap] = 2ull * bd;
    out[kOutMaxGapG] = bd ? a.r.g_start + bi : kGapsNone;
    const uint64_t ov = min((uint64_t)s_acc[1], (uint64_t)s_bins[kClBins]);
    out[kOutOverflow] = ov == kGapsNone ? kGapsNone : a.r.g_start + ov;
  }
}

}  // namespace

uint32_t gaps_grid(uint64_t nbits, int num_cus, uint32_t grid_cap) {
  return slab_grid(nbits, 4, num_cus, grid_cap, kGapsMaxGrid);  // gaps_main_kernel's registers and LDS admit 4 per CU
}

uint64_t gaps_scratch_bytes(uint32_t grid) { return slab_bytes(grid, kSlabWords); }

hipError_t launch_gaps(uint64_t g_start, uint64_t nbits, const uint64_t* mask, uint64_t* out, void* slabs,
                       uint32_t grid, hipStream_t stream) {
  if (grid > kGapsMaxGrid) return hipErrorInvalidValue;
  GpArgs a;
  a.r = mask_range(mask, g_start, nbits);
  a.last_mask = (nbits & 63) ? (1ull << (nbits & 63)) - 1 : ~0ull;
  if (!slab_run(nbits, grid, &a.run)) return hipErrorInvalidValue;
  return slab_launch(gaps_main_kernel, gaps_close_kernel, a, grid, kGpThreads, kGapsBins, slabs, out, stream);
}

}  // namespace dse
