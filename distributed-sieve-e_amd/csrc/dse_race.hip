// dse_race.hip -- residue-class counts and a prime race of a device-resident prime
// mask (gfx950): pi(x; q, r) for every r, and for two classes a and b the running
// difference D (+1 at an entry = a mod q, -1 at one = b mod q): who leads how often,
// where the lead is first taken, the extrema of D and where they are first attained,
// as one dse_race (include/dse.h) in device memory.
//
// D at an entry depends on every entry before it. Three launches on the caller's
// stream; the launches are the only ordering and no workgroup waits on another:
//   race_count_kernel  every workgroup walks its own contiguous run of tiles
//                      (kMaskTileBits candidates, one mask word per thread) and counts
//                      the entries per position class g mod T (dse_race_word.h): T
//                      popcounts of the word under a shifted comb, into registers
//                      (instantiated for T <= 4, 16 and 64: the class index is a
//                      compile-time one, the array stays in registers), summed per
//                      wave into LDS at the end. Its slab gets the T sums.
//   race_main_kernel   the same grid and runs. A workgroup sums the class-a minus
//                      class-b counts of the slabs before its own, adds d_start and so
//                      knows D at its first tile. Per tile a workgroup scan of the
//                      words' deltas gives D at every word's start, the tile's total
//                      goes into a register carry (one barrier per tile). A word whose
//                      D cannot reach 0 and cannot set an extremum adds its steps to
//                      the leading side; any other word is walked step by step
//                      (race_word). Its slab gets the scalars.
//   race_close_kernel  one workgroup: sums the class bins over the slabs, maps the
//                      position classes to residues, reduces the scalars (one slab per
//                      thread) and writes the struct.
// With a == b only the counts are wanted and the main launch is left out.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dse_internal.h"
#include "dse_race_word.h"
#include "dse_slab.h"

namespace dse {
namespace {

constexpr uint32_t kRcThreads = kMaskTileWords;  // one mask word per thread
constexpr uint32_t kRcWaves = kRcThreads / 64;
constexpr uint32_t kRcGridPerCu = 4;  // workgroups per compute unit of the one resident round the grid is
// the count kernel's register counters are 32 bits wide and grow by at most 64 per tile; they are summed per wave in
// 32 bits and then into LDS after this many tiles, so that a wave's sum cannot wrap (kSlabFlushTiles, dse_slab.h)
constexpr uint32_t kRcFlushTiles = kSlabFlushTiles;

// a workgroup's slab, in uint64 words: the scalars are the main kernel's, the bins the count kernel's
constexpr uint32_t kSlAAhead = 0, kSlBAhead = 1, kSlFirstA = 2, kSlFirstB = 3, kSlMaxD = 4, kSlMaxG = 5, kSlMinD = 6,
                   kSlMinG = 7, kSlBins = 8, kSlHist = 16, kSlabWords = kSlHist + kRaceMaxModulus;
constexpr uint32_t kClThreads = kSlabCloseThreads, kClBins = kSlabCloseBins;
static_assert(kRaceMaxGrid <= kClThreads, "the closing kernel reads one slab per thread");
static_assert(kRaceMaxModulus == kClBins, "one closing workgroup sums every class bin");

// dse_race as uint64 words
constexpr uint32_t kOutGStart = 0, kOutNbits = 1, kOutQ = 2, kOutA = 3, kOutB = 4, kOutDStart = 5, kOutDEnd = 6,
                   kOutSteps = 7, kOutAAhead = 8, kOutBAhead = 9, kOutTies = 10, kOutFirstA = 11, kOutFirstB = 12,
                   kOutMaxD = 13, kOutMaxG = 14, kOutMinD = 15, kOutMinG = 16, kOutCounts = 17;
static_assert(kOutCounts + kRaceMaxModulus == kRaceWords, "dse_race is kRaceWords words");

struct RaceArgs {
  MaskRange r;
  SlabRun run;
  uint64_t comb;     // race_comb(T)
  int64_t d_start;
  uint32_t q, a, b;  // a == b: counts only
  uint32_t T;        // race_period(q)
  uint32_t ca, cb;   // race_class_pos of a and b
  uint32_t step;     // kMaskTileBits mod T: the phase from a tile to the next
};

// the phase g mod T of this thread's word of tile t
__device__ __forceinline__ uint32_t rc_phase(const RaceArgs& a, uint64_t t) {
  const uint64_t pos = (t * kMaskTileWords + threadIdx.x) * 64ull;
  return (uint32_t)((a.r.g_start % a.T + pos % a.T) % a.T);
}

template <uint32_t kBound>
__global__ __launch_bounds__(kRcThreads) void race_count_kernel(RaceArgs a, unsigned long long* __restrict__ slabs) {
  __shared__ unsigned long long s_cnt[kRaceMaxModulus];
  const uint32_t tid = threadIdx.x, lane = tid & 63u;
  if (tid < kRaceMaxModulus) s_cnt[tid] = 0ull;
  __syncthreads();

  uint32_t cnt[kBound];
#pragma unroll
  for (uint32_t c = 0; c < kBound; ++c) cnt[c] = 0;
  uint64_t t0, t1;
  slab_tiles(a.run, t0, t1);
  if (t0 < t1) {
    uint32_t ph = rc_phase(a, t0);
    uint64_t next = mask_word(a.r, t0 * kMaskTileWords + tid);
    for (uint64_t tb = t0; tb < t1; tb += kRcFlushTiles) {
      const uint64_t te = min(t1, tb + kRcFlushTiles);
      for (uint64_t t = tb; t < te; ++t) {
        const uint64_t w = next;
        if (t + 1 < t1) next = mask_word(a.r, (t + 1) * kMaskTileWords + tid);  // in flight over this tile's work
        race_count_word<kBound>(w, a.comb, a.T, ph, cnt);
        ph = race_phase_add(ph, a.step, a.T);
      }
      // the register counters into LDS, summed per wave first; by race_count_word's groups
      constexpr uint32_t kGroup = race_count_group(kBound);
#pragma unroll
      for (uint32_t c0 = 0; c0 < kBound; c0 += kGroup)
        if (c0 < a.T) {
#pragma unroll
          for (uint32_t c = c0; c < c0 + kGroup; ++c) {
            const uint32_t r = wave_sum(cnt[c]);
            if (lane == 0 && r) atomicAdd(&s_cnt[c], (unsigned long long)r);
            cnt[c] = 0;
          }
        }
    }
  }
  __syncthreads();

  unsigned long long* const sl = slabs + (uint64_t)blockIdx.x * kSlabWords;
  if (tid < kRaceMaxModulus) sl[kSlHist + tid] = tid < a.T ? s_cnt[tid] : 0ull;  // a last group's classes >= T hold no count
  if (tid == 0) sl[kSlBins] = kRaceMaxModulus;
}

__global__ __launch_bounds__(kRcThreads) void race_main_kernel(RaceArgs a, unsigned long long* __restrict__ slabs) {
  __shared__ long long s_sum[kRcWaves];
  __shared__ int32_t s_wave[2][kRcWaves];
  __shared__ unsigned long long s_acc[2], s_first[2];
  __shared__ unsigned long long s_d[kRcWaves], s_g[kRcWaves];
  const uint32_t tid = threadIdx.x, lane = tid & 63u;

  if (tid < 2) {
    s_acc[tid] = 0ull;
    s_first[tid] = kRaceNone;
  }
  // D at this workgroup's first tile: d_start and the steps of the slabs before its own
  long long before = 0;
  for (uint32_t s = tid; s < blockIdx.x; s += kRcThreads) {
    const unsigned long long* const sl = slabs + (uint64_t)s * kSlabWords + kSlHist;
    if (a.ca != kRaceNoClass) before += (long long)sl[a.ca];
    if (a.cb != kRaceNoClass) before -= (long long)sl[a.cb];
  }
  int64_t carry = a.d_start + (int64_t)block_sum<kRcThreads>(before, s_sum);  // its barrier also orders the stores above

  RaceAcc acc;
  uint64_t t0, t1;
  slab_tiles(a.run, t0, t1);
  if (t0 < t1) {
    uint32_t ph = rc_phase(a, t0);
    uint64_t next = mask_word(a.r, t0 * kMaskTileWords + tid);
    for (uint64_t t = t0; t < t1; ++t) {
      const uint64_t w = next;
      if (t + 1 < t1) next = mask_word(a.r, (t + 1) * kMaskTileWords + tid);
      const uint64_t A = w & race_class_mask(a.comb, a.T, a.ca, ph);
      const uint64_t B = w & race_class_mask(a.comb, a.T, a.cb, ph);
      ph = race_phase_add(ph, a.step, a.T);
      const int32_t delta = (int32_t)__builtin_popcountll(A) - (int32_t)__builtin_popcountll(B);
      // two sets of wave totals by tile parity, so the scan's one barrier per tile orders them
      int32_t total;
      const int32_t incl = block_scan<kRcThreads>(delta, s_wave[(uint32_t)(t - t0) & 1u], &total);
      race_word(A, B, carry + (int64_t)(incl - delta), (t * kMaskTileWords + tid) * 64ull, acc);
      carry += (int64_t)total;
    }
  }

  {
    const uint64_t x = wave_sum(acc.a_ahead), y = wave_sum(acc.b_ahead);
    if (lane == 0 && x) atomicAdd(&s_acc[0], (unsigned long long)x);
    if (lane == 0 && y) atomicAdd(&s_acc[1], (unsigned long long)y);
    if (acc.first_a != kRaceNone) atomicMin(&s_first[0], (unsigned long long)acc.first_a);
    if (acc.first_b != kRaceNone) atomicMin(&s_first[1], (unsigned long long)acc.first_b);
  }
  uint64_t xd = (uint64_t)acc.max_d, xg = acc.max_g, nd = (uint64_t)acc.min_d, ng = acc.min_g;
  block_best<kRcWaves>(xd, xg, s_d, s_g, race_max_better);  // its barriers also make the LDS sums final
  block_best<kRcWaves>(nd, ng, s_d, s_g, race_min_better);
  if (tid == 0) {
    unsigned long long* const sl = slabs + (uint64_t)blockIdx.x * kSlabWords;
    sl[kSlAAhead] = s_acc[0];
    sl[kSlBAhead] = s_acc[1];
    sl[kSlFirstA] = s_first[0];
    sl[kSlFirstB] = s_first[1];
    sl[kSlMaxD] = xd;
    sl[kSlMaxG] = xg;
    sl[kSlMinD] = nd;
    sl[kSlMinG] = ng;
  }
}

__global__ __launch_bounds__(kClThreads) void race_close_kernel(RaceArgs a, const unsigned long long* __restrict__ slabs,
                                                                uint32_t nslabs, unsigned long long* __restrict__ out) {
  __shared__ unsigned long long s_bins[kClBins];
  __shared__ unsigned long long s_acc[2], s_first[2];
  __shared__ unsigned long long s_d[kClThreads / 64], s_g[kClThreads / 64];
  const uint32_t tid = threadIdx.x, lane = tid & 63u;
  const bool race = a.a != a.b;

  if (tid < kClBins) s_bins[tid] = 0ull;
  if (tid < 2) {
    s_acc[tid] = 0ull;
    s_first[tid] = kRaceNone;
  }
  __syncthreads();
  slab_sum_bins<kSlabWords, kSlBins, kSlHist>(slabs, nslabs, s_bins);
  __syncthreads();
  if (tid < kRaceMaxModulus) {
    const uint32_t c = tid < a.q ? race_class_pos(a.q, tid) : kRaceNoClass;
    out[kOutCounts + tid] = c == kRaceNoClass ? 0ull : s_bins[c];
  }

  // the scalar members: one slab per thread; without a race the main kernel has not written them
  const bool have = race && tid < nslabs;
  const unsigned long long* const my = slabs + (uint64_t)(have ? tid : 0u) * kSlabWords;
  {
    const uint64_t x = wave_sum(have ? (uint64_t)my[kSlAAhead] : 0ull), y = wave_sum(have ? (uint64_t)my[kSlBAhead] : 0ull);
    if (lane == 0 && x) atomicAdd(&s_acc[0], (unsigned long long)x);
    if (lane == 0 && y) atomicAdd(&s_acc[1], (unsigned long long)y);
    if (have && my[kSlFirstA] != kRaceNone) atomicMin(&s_first[0], my[kSlFirstA]);
    if (have && my[kSlFirstB] != kRaceNone) atomicMin(&s_first[1], my[kSlFirstB]);
  }
  uint64_t xd = have ? (uint64_t)my[kSlMaxD] : 0ull, xg = have ? (uint64_t)my[kSlMaxG] : kRaceNone;
  uint64_t nd = have ? (uint64_t)my[kSlMinD] : 0ull, ng = have ? (uint64_t)my[kSlMinG] : kRaceNone;
  auto at = [&](uint64_t pos) { return pos == kRaceNone ? kRaceNone : a.r.g_start + pos; };
  block_best<kClThreads / 64>(xd, xg, s_d, s_g, race_max_better);  // its barriers also order the sums above
  // stored before the second reduction: the waves' 16 pairs of one reduction are not kept in registers over the other
  if (tid == 0) {
    out[kOutMaxD] = xg == kRaceNone ? (uint64_t)a.d_start : xd;
    out[kOutMaxG] = at(xg);
  }
  block_best<kClThreads / 64>(nd, ng, s_d, s_g, race_min_better);
  if (tid == 0) {
    const uint64_t na = race && a.ca != kRaceNoClass ? s_bins[a.ca] : 0ull;
    const uint64_t nb = race && a.cb != kRaceNoClass ? s_bins[a.cb] : 0ull;
    out[kOutGStart] = a.r.g_start;
    out[kOutNbits] = a.r.nbits;
    out[kOutQ] = a.q;
    out[kOutA] = a.a;
    out[kOutB] = a.b;
    out[kOutDStart] = (uint64_t)a.d_start;
    out[kOutDEnd] = (uint64_t)(a.d_start + (int64_t)na - (int64_t)nb);
    out[kOutSteps] = na + nb;
    out[kOutAAhead] = s_acc[0];
    out[kOutBAhead] = s_acc[1];
    out[kOutTies] = na + nb - s_acc[0] - s_acc[1];
    out[kOutFirstA] = at(s_first[0]);
    out[kOutFirstB] = at(s_first[1]);
    out[kOutMinD] = ng == kRaceNone ? (uint64_t)a.d_start : nd;
    out[kOutMinG] = at(ng);
  }
}

}  // namespace

uint32_t race_grid(uint64_t nbits, int num_cus, uint32_t grid_cap) {
  return slab_grid(nbits, kRcGridPerCu, num_cus, grid_cap, kRaceMaxGrid);
}

uint64_t race_scratch_bytes(uint32_t grid) { return slab_bytes(grid, kSlabWords); }

hipError_t launch_race(uint64_t g_start, uint64_t nbits, const uint64_t* mask, uint32_t q, uint32_t a, uint32_t b,
                       int64_t d_start, uint64_t* out, void* slabs, uint32_t grid, hipStream_t stream) {
  if (q < 3 || q > kRaceMaxModulus || a >= q || b >= q || (a == b && d_start) || grid > kRaceMaxGrid)
    return hipErrorInvalidValue;
  RaceArgs ra;
  ra.r = mask_range(mask, g_start, nbits);
  if (!slab_run(nbits, grid, &ra.run)) return hipErrorInvalidValue;
  ra.T = race_period(q);
  ra.comb = race_comb(ra.T);
  ra.d_start = d_start;
  ra.q = q;
  ra.a = a;
  ra.b = b;
  ra.ca = race_class_pos(q, a);
  ra.cb = race_class_pos(q, b);
  ra.step = kMaskTileBits % ra.T;
  auto count = ra.T <= 4 ? race_count_kernel<4> : ra.T <= 16 ? race_count_kernel<16> : race_count_kernel<64>;
  if (a == b) return slab_launch(count, race_close_kernel, ra, grid, kRcThreads, kClBins, slabs, out, stream);
  if (grid)
    hipLaunchKernelGGL(count, dim3(grid), dim3(kRcThreads), 0, stream, ra, reinterpret_cast<unsigned long long*>(slabs));
  return slab_launch(race_main_kernel, race_close_kernel, ra, grid, kRcThreads, kClBins, slabs, out, stream);
}

}  // namespace dse
