// dse_gaps_word.h -- the per-word bodies of the first-occurrence table of the
// prime gaps (dse_gaps.hip).
//
// Positions, words and the 96-bit window {nx : w} are those of dse_stats_word.h,
// whose bit helpers this header shares by including it. A gap of d places whose
// lower prime is at position i is one call put(d, i); the caller's table keeps
// the minimum per d. Every gap is seen exactly once:
//   gaps_small         the gaps of 1 .. kGapsSmall places whose lower prime is in
//                      w, wherever the next word lies: per d only the lowest
//                      such prime of w is put (the others cannot be the first);
//   gaps_inword_large  the longer gaps whose two primes both lie in w;
//   gaps_cross         the longer gap that ends at w's first prime (the prime
//                      before it comes from the caller).
// Pruning. A table entry below `floor`, the lowest position the caller can still
// put (gaps_floor), can never be lowered again: the bin is settled. GapsSettled
// holds that as one bit per bin d < kGapsSettled, refreshed by the caller once
// per tile (gaps_settled_bit: one bin's bit from its entry). gaps_small skips a
// settled d; with every short bin settled it collapses to gaps_far, the OR of
// the 31 shifts by doubling, and with the bins 1 .. 16 settled it adds one
// term per open bin above them. The long paths ask gaps_is_settled before they
// touch the table. A settled bit only ever suppresses a put that could not
// change the table, so the result is the same with any subset of the true bits.
// The functions are __host__ __device__: the kernels and dse_debug_gaps_host
// (tests, on the host) run the same code.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dse_mask.h"
#include "dse_stats_word.h"

namespace dse {

constexpr uint32_t kGapsSmall = 31;      // gaps of up to this many places are decided inside the window
constexpr uint32_t kGapsBins = 1024;     // DSE_GAPS_BINS
constexpr uint64_t kGapsNone = ~0ull;    // DSE_GAPS_NONE
constexpr uint32_t kGapsSettled = 128;   // bins with a settled bit
constexpr uint64_t kGapsSmallAll = 0xFFFFFFFEull;  // the bits 1 .. kGapsSmall
constexpr uint64_t kGapsSmallLow = 0x0001FFFEull;  // the bits 1 .. 16
static_assert(kGapsSmall == 31, "gaps_far's doubling and kGapsSmallAll are written for 31 places");

struct GapsSettled {
  uint64_t lo, hi;  // bit d of {hi : lo}: bin d holds a position that nothing later can beat
};

// The lowest position a walk can still put when it enters the tile at tile0 with the last
// prime before it at carry1 - 1 (carry1 = 0: none): that prime's gap is still open.
__host__ __device__ __forceinline__ uint64_t gaps_floor(uint64_t tile0, uint64_t carry1) {
  return carry1 ? carry1 - 1 : tile0;
}

__host__ __device__ __forceinline__ bool gaps_settled_bit(uint64_t entry, uint64_t floor) { return entry < floor; }

__host__ __device__ __forceinline__ bool gaps_is_settled(const GapsSettled& s, uint64_t d) {
  return d < kGapsSettled && (((d < 64 ? s.lo : s.hi) >> (d & 63)) & 1ull);
}

// The shifts 1 .. 16 of the window ORed together by doubling (1, 1..2, 1..4, 1..8, 1..16), as
// the 96 bits {hi : lo}: bit i is right where i + 16 <= 95.
struct GapsNear {
  uint64_t lo;
  uint32_t hi;
};
__host__ __device__ __forceinline__ GapsNear gaps_near16(uint64_t w, uint32_t nx) {
  GapsNear o = {(w >> 1) | ((uint64_t)nx << 63), nx >> 1};
#pragma unroll
  for (uint32_t k = 1; k <= 8; k <<= 1) {
    o.lo |= (o.lo >> k) | ((uint64_t)o.hi << (64 - k));
    o.hi |= o.hi >> k;
  }
  return o;
}
// bits [k, k + 64) of o, k <= 15
__host__ __device__ __forceinline__ uint64_t gaps_near_shift(const GapsNear& o, uint32_t k) {
  return (o.lo >> k) | (((uint64_t)o.hi << 32) << (32 - k));
}

// The primes of w that have no prime within kGapsSmall places above them: the OR of the
// shifts 1 .. 31 of the window, 1 .. 16 by doubling and 15 more.
__host__ __device__ __forceinline__ uint64_t gaps_far(uint64_t w, uint32_t nx) {
  const GapsNear o = gaps_near16(w, nx);
  return w & ~(o.lo | gaps_near_shift(o, 15));
}

// put(d, position) for the lowest prime of w whose gap is d places, every d <= kGapsSmall that
// is not settled. Returns gaps_far(w, nx). Three paths by what is settled: every short bin (the
// steady state): gaps_far alone; the bins 1 .. 16 (after a tile or two of real primes): gaps_far
// and, per open bin d > 16, the primes with a prime d places above and none within d - 1, the
// latter from the 1 .. 16 OR and its shift by d - 17; otherwise all 31 shifts in turn.
template <typename Sink>
__host__ __device__ __forceinline__ uint64_t gaps_small(uint64_t w, uint32_t nx, uint64_t pos0, uint64_t settled_lo,
                                                        Sink&& put) {
  if ((settled_lo & kGapsSmallLow) == kGapsSmallLow) {
    const GapsNear o = gaps_near16(w, nx);
    for (uint32_t open = (uint32_t)(~settled_lo & (kGapsSmallAll & ~kGapsSmallLow)); open; open &= open - 1) {
      const uint32_t d = (uint32_t)__builtin_ctz(open);
      const uint64_t m = w & stats_shift(w, nx, d) & ~(o.lo | gaps_near_shift(o, d - 17));
      if (m) put((uint64_t)d, pos0 + stats_ctz64(m));
    }
    return w & ~(o.lo | gaps_near_shift(o, 15));
  }
  uint64_t seen = 0;  // bit i: a prime within the places i + 1 .. i + d
  for (uint32_t d = 1; d <= kGapsSmall; ++d) {
    const uint64_t xs = stats_shift(w, nx, d);
    if (!((settled_lo >> d) & 1ull)) {
      const uint64_t m = w & xs & ~seen;
      if (m) put((uint64_t)d, pos0 + stats_ctz64(m));
    }
    seen |= xs;
  }
  return w & ~seen;
}

// The gaps of more than kGapsSmall places between two primes of w, in increasing position.
// rem = gaps_small's result.
template <typename Sink>
__host__ __device__ __forceinline__ void gaps_inword_large(uint64_t w, uint64_t rem, uint64_t pos0,
                                                           const GapsSettled& s, Sink&& put) {
  if (!rem) return;
  uint64_t it = rem & ~(1ull << stats_msb64(w));  // w's last prime has its successor in a later word
  while (it) {
    const uint32_t i = stats_ctz64(it);
    it &= it - 1;
    const uint64_t d = 1u + stats_ctz64(w >> (i + 1));
    if (!gaps_is_settled(s, d)) put(d, pos0 + i);
  }
}

// The gap from the prime before a word's first prime (prev1 = its position + 1, not 0) to that
// prime at position f, when it is a long one.
template <typename Sink>
__host__ __device__ __forceinline__ void gaps_cross(uint64_t f, uint64_t prev1, const GapsSettled& s, Sink&& put) {
  const uint64_t d = f - (prev1 - 1);
  if (d > kGapsSmall && !gaps_is_settled(s, d)) put(d, prev1 - 1);
}

}  // namespace dse
