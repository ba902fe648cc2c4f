// dse_consec.hip -- the residue pairs of consecutive primes of a device-resident mask
// (gfx950): for a modulus q the q x q matrix N(a, b) of the pairs of consecutive
// entries with the lower value = a and the upper = b (mod q), as one dse_consec
// (include/dse.h) in device memory.
//
// Two launches of the slab reduction (dse_slab.h) on the caller's stream; the
// launches are the only ordering and no workgroup waits on another. The pairs are
// counted by position class (c, c'), c = g mod T (dse_consec_word.h), every pair
// exactly once by one of three paths:
//   consec_main_kernel  every workgroup walks its own contiguous run of tiles, one
//                       mask word per thread, the next tile's word in flight.
//                       In-word pairs (both primes in the thread's word): for
//                       T <= kConsecBitMaxT the bit-parallel body into T^2 register
//                       counters (instantiated for every such T: the indices are
//                       compile-time ones, the array stays in registers), otherwise
//                       the per-entry body, one 32-bit LDS add per pair.
//                       Cross-word pairs: the word that holds the upper prime, its
//                       first entry, counts the pair with one LDS add. The lower
//                       prime comes from gaps_main_kernel's scan: a workgroup scan
//                       (maximum) of "last prime so far" by tile parity, one barrier
//                       per tile, carried from tile to tile in a register together
//                       with its class, so any number of empty tiles is no case of
//                       its own. The class of a position is (tile's phase + position
//                       in the tile) mod T; the tile's phase is the 64-bit remainder
//                       at the run's first tile, stepped by kMaskTileBits mod T.
//                       The 32-bit counters are emptied into the slab's 64-bit bins
//                       every flush_tiles tiles and at the end (a thread owns its
//                       bins of its workgroup's slab: the first time it stores,
//                       later it adds). The slab also gets the run's entry count,
//                       its first prime and its last prime + 1.
//   consec_close_kernel 64 workgroups, one per row a of the result. Every one scans
//                       the slabs' first / last primes (the last prime is carried
//                       across empty runs) and the workgroup whose row is the class
//                       of a seam's lower prime counts that seam's pair; it sums its
//                       row c = race_class_pos(q, a) of position classes over the
//                       slabs and writes counts[a * 64 + b] for every b, zeros for a
//                       residue without a class. Workgroup 0 also writes the scalars.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dse_consec_word.h"
#include "dse_internal.h"
#include "dse_slab.h"

namespace dse {
namespace {

constexpr uint32_t kCsThreads = kMaskTileWords;  // one mask word per thread
constexpr uint32_t kCsWaves = kCsThreads / 64;
constexpr uint32_t kCsGridPerCu = 4;  // workgroups per compute unit of the one resident round the grid is

// a workgroup's slab, in uint64 words
constexpr uint32_t kSlPrimes = 0, kSlFirst = 1, kSlLast1 = 2, kSlBins = 3, kSlHist = 8,
                   kSlabWords = kSlHist + kConsecBins;
constexpr uint32_t kClThreads = kSlabCloseThreads, kClBins = kSlabCloseBins;
static_assert(kConsecMaxGrid <= kClThreads, "the closing kernel reads one slab per thread");
static_assert(kConsecStride == kClBins && kConsecMaxModulus == kConsecBins / kClBins,
              "one closing workgroup per row of the result, a row of position classes per workgroup");

// dse_consec as uint64 words
constexpr uint32_t kOutGStart = 0, kOutNbits = 1, kOutQ = 2, kOutPrimes = 3, kOutPairs = 4, kOutFirst = 5,
                   kOutLast = 6, kOutCounts = 7;
static_assert(kOutCounts + kConsecBins == kConsecWords, "dse_consec is kConsecWords words");

struct ConsecArgs {
  MaskRange r;
  SlabRun run;
  uint64_t comb;         // race_comb(T)
  uint32_t q, T;         // T = race_period(q)
  uint32_t magic;        // consec_magic(T)
  uint32_t step;         // kMaskTileBits mod T: the phase from a tile to the next
  uint32_t word_step;    // 64 mod T: from a word to the next
  uint32_t flush_tiles;  // 1 .. kConsecFlushTiles
};

// the position class of a position of the range (any distance from its start)
__device__ __forceinline__ uint32_t cs_class(const ConsecArgs& a, uint64_t pos) {
  return (uint32_t)((a.r.g_start % a.T + pos % a.T) % a.T);
}

// kBound > 0: the bit-parallel body for T <= kBound; 0: the per-entry body
template <uint32_t kBound>
__global__ __launch_bounds__(kCsThreads, kCsGridPerCu) void consec_main_kernel(ConsecArgs a,
                                                                                unsigned long long* __restrict__ slabs) {
  __shared__ uint32_t s_hist[kConsecBins];
  __shared__ unsigned long long s_first;  // position of the run's first prime
  __shared__ unsigned long long s_primes;
  __shared__ uint32_t s_wave[2][kCsWaves];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint32_t T = a.T, nb = T * kConsecStride;  // bins c * kConsecStride + c' below nb

  for (uint32_t i = tid; i < nb; i += kCsThreads) s_hist[i] = 0u;
  if (tid == 0) {
    s_first = kConsecNone;
    s_primes = 0ull;
  }
  __syncthreads();

  constexpr uint32_t kRegs = kBound ? kBound * kBound : 1;
  uint32_t cnt[kRegs];
#pragma unroll
  for (uint32_t i = 0; i < kRegs; ++i) cnt[i] = 0;

  unsigned long long* const sl = slabs + (uint64_t)blockIdx.x * kSlabWords;
  bool flushed = false;  // the slab's bins hold this run's counts so far
  uint64_t pc = 0;
  uint64_t carry = 0;      // position + 1 of the run's last prime so far (the same in every thread)
  uint32_t carry_cls = 0;  // and its position class
  uint64_t t0, t1;
  slab_tiles(a.run, t0, t1);
  if (t0 < t1) {
    uint32_t php = cs_class(a, t0 * (uint64_t)kMaskTileBits);  // the phase of the tile's first candidate
    uint64_t next = mask_word(a.r, t0 * kMaskTileWords + tid);
    for (uint64_t tb = t0; tb < t1; tb += a.flush_tiles) {
      const uint64_t te = min(t1, tb + a.flush_tiles);
      for (uint64_t t = tb; t < te; ++t) {
        const uint64_t w = next;
        if (t + 1 < t1) next = mask_word(a.r, (t + 1) * kMaskTileWords + tid);  // in flight over this tile's work
        const uint32_t ph = consec_mod(php + tid * a.word_step, T, a.magic);   // of this thread's word
        pc += (uint64_t)__builtin_popcountll(w);

        // the in-word pairs
        if constexpr (kBound != 0) {
          consec_count_word<kBound>(w, a.comb, T, ph, cnt);
        } else {
          consec_walk_word(w, T, a.magic, ph,
                           [&](uint32_t c, uint32_t c2) { atomicAdd(&s_hist[c * kConsecStride + c2], 1u); });
        }

        // exclusive scan (maximum) of "tile position + 1 of the last prime so far"
        const uint32_t x =
            wave_scan(w ? tid * 64u + (63u - (uint32_t)__builtin_clzll(w)) + 1u : 0u, ScanMax());
        uint32_t ex = __shfl_up(x, 1);
        if (lane == 0) ex = 0;
        // the waves' maxima through LDS: two sets by tile parity, so one barrier per tile orders them
        uint32_t* const sw = s_wave[(uint32_t)(t - t0) & 1u];
        if (lane == 63) sw[wave] = x;
        __syncthreads();
        uint32_t tot = 0;
#pragma unroll
        for (uint32_t i = 0; i < kCsWaves; ++i) {
          const uint32_t u = sw[i];
          if (i < wave) ex = max(ex, u);
          tot = max(tot, u);
        }

        // the cross-word pair whose upper prime is this word's first entry
        if (w) {
          const uint32_t f = (uint32_t)__builtin_ctzll(w);
          if (ex || carry) {
            const uint32_t cl = ex ? consec_mod(php + ex - 1u, T, a.magic) : carry_cls;
            const uint32_t cu = consec_mod(ph + f, T, a.magic);
            atomicAdd(&s_hist[cl * kConsecStride + cu], 1u);
          } else {
            s_first = (t * kMaskTileWords + tid) * 64ull + f;  // one thread of the workgroup, once
          }
        }
        if (tot) {
          carry = t * (uint64_t)kMaskTileBits + tot;
          carry_cls = consec_mod(php + tot - 1u, T, a.magic);
        }
        php = race_phase_add(php, a.step, T);
      }

      // the 32-bit counters into the slab's 64-bit bins
      if constexpr (kBound != 0) {
#pragma unroll
        for (uint32_t c = 0; c < kBound; ++c)
          if (c < T) {
#pragma unroll
            for (uint32_t c2 = 0; c2 < kBound; ++c2) {
              const uint32_t r = wave_sum(cnt[c * kBound + c2]);
              if (lane == 0 && r && c2 < T) atomicAdd(&s_hist[c * kConsecStride + c2], r);
              cnt[c * kBound + c2] = 0;
            }
          }
      }
      __syncthreads();  // every add of these tiles has landed
      for (uint32_t i = tid; i < nb; i += kCsThreads) {
        uint64_t v = s_hist[i];
        s_hist[i] = 0u;
        if (flushed) v += sl[kSlHist + i];
        sl[kSlHist + i] = v;
      }
      flushed = true;
      __syncthreads();  // the bins are empty before the next tiles add to them
    }
  }
  {
    const uint64_t r = wave_sum(pc);
    if (lane == 0 && r) atomicAdd(&s_primes, (unsigned long long)r);
  }
  __syncthreads();
  if (tid == 0) {
    sl[kSlPrimes] = s_primes;
    sl[kSlFirst] = s_first;
    sl[kSlLast1] = carry;
    sl[kSlBins] = flushed ? nb : 0u;
  }
}

__global__ __launch_bounds__(kClThreads) void consec_close_kernel(ConsecArgs a,
                                                                  const unsigned long long* __restrict__ slabs,
                                                                  uint32_t nslabs, unsigned long long* __restrict__ out) {
  __shared__ unsigned long long s_scan[kClThreads];
  __shared__ unsigned long long s_bins[kClBins];
  __shared__ unsigned long long s_acc[2];  // primes, first
  const uint32_t tid = threadIdx.x, lane = tid & 63u;
  const uint32_t row = blockIdx.x;  // the residue a of the lower prime
  const uint32_t c = row < a.q ? race_class_pos(a.q, row) : kRaceNoClass;
  const bool lead = row == 0;

  if (tid < kClBins) s_bins[tid] = 0ull;
  if (tid == 0) s_acc[0] = 0ull;
  if (tid == 1) s_acc[1] = kConsecNone;
  const bool have = tid < nslabs;
  const unsigned long long* const my = slabs + (uint64_t)(have ? tid : 0u) * kSlabWords;
  const uint64_t first = have ? my[kSlFirst] : kConsecNone;
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

  // the pair that crosses into this slab, in the row of its lower prime
  if (c != kRaceNoClass && first != kConsecNone && prev1 && cs_class(a, prev1 - 1) == c)
    atomicAdd(&s_bins[cs_class(a, first)], 1ull);
  if (c != kRaceNoClass) slab_sum_bins_at<kSlabWords, kSlBins, kSlHist>(slabs, nslabs, c * kConsecStride, s_bins);
  __syncthreads();
  if (tid < kClBins) {
    const uint32_t c2 = c != kRaceNoClass && tid < a.q ? race_class_pos(a.q, tid) : kRaceNoClass;
    out[kOutCounts + row * kConsecStride + tid] = c2 == kRaceNoClass ? 0ull : s_bins[c2];
  }
  if (!lead) return;

  // workgroup 0: the scalar members
  {
    const uint64_t r = wave_sum(have ? (uint64_t)my[kSlPrimes] : 0ull);
    if (lane == 0 && r) atomicAdd(&s_acc[0], (unsigned long long)r);
  }
  if (first != kConsecNone) atomicMin(&s_acc[1], (unsigned long long)first);
  __syncthreads();
  if (tid == 0) {
    const uint64_t primes = s_acc[0];
    out[kOutGStart] = a.r.g_start;
    out[kOutNbits] = a.r.nbits;
    out[kOutQ] = a.q;
    out[kOutPrimes] = primes;
    out[kOutPairs] = primes ? primes - 1 : 0ull;
    out[kOutFirst] = s_acc[1] == kConsecNone ? kConsecNone : a.r.g_start + s_acc[1];
    out[kOutLast] = last1 ? a.r.g_start + (last1 - 1) : kConsecNone;
  }
}

}  // namespace

uint32_t consec_grid(uint64_t nbits, int num_cus, uint32_t grid_cap) {
  return slab_grid(nbits, kCsGridPerCu, num_cus, grid_cap, kConsecMaxGrid);
}

uint64_t consec_scratch_bytes(uint32_t grid) { return slab_bytes(grid, kSlabWords); }

hipError_t launch_consec(uint64_t g_start, uint64_t nbits, const uint64_t* mask, uint32_t q, uint64_t* out,
                         void* slabs, uint32_t grid, uint32_t flush_tiles, uint32_t body, hipStream_t stream) {
  if (q < 3 || q > kConsecMaxModulus || grid > kConsecMaxGrid || flush_tiles > kConsecFlushTiles || body > 2)
    return hipErrorInvalidValue;
  ConsecArgs a;
  a.r = mask_range(mask, g_start, nbits);
  if (!slab_run(nbits, grid, &a.run)) return hipErrorInvalidValue;
  a.q = q;
  a.T = race_period(q);
  a.comb = race_comb(a.T);
  a.magic = consec_magic(a.T);
  a.step = kMaskTileBits % a.T;
  a.word_step = 64u % a.T;
  a.flush_tiles = flush_tiles ? flush_tiles : kConsecFlushTiles;
  const uint32_t bit_max = body == 1 ? kConsecBitBuiltT : body == 2 ? 0u : kConsecBitMaxT;
  static_assert(kConsecBitMaxT <= kConsecBitBuiltT && kConsecBitBuiltT == 6, "the instantiations below");
  using Main = void (*)(ConsecArgs, unsigned long long*);
  static const Main kBit[kConsecBitBuiltT + 1] = {nullptr,  // T >= 2
                                                  nullptr,
                                                  consec_main_kernel<2>,
                                                  consec_main_kernel<3>,
                                                  consec_main_kernel<4>,
                                                  consec_main_kernel<5>,
                                                  consec_main_kernel<6>};
  const Main main = a.T > bit_max ? consec_main_kernel<0> : kBit[a.T];
  return slab_launch(main, consec_close_kernel, a, grid, kCsThreads, kConsecBins, slabs, out, stream);
}

}  // namespace dse
