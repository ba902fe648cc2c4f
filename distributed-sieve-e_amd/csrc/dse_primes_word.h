// dse_primes_word.h -- the per-word body of the prime-value extractor (dse_primes.hip).
//
// A mask word's set bits are entries of the range, ranked in increasing bit
// order: the word's lowest set bit has rank `rank`, the next rank + 1, ... The
// entry of bit b has the value 3 + 2 (g_word_start + b), g_word_start being the
// odd index of the word's bit 0. primes_word hands the entries whose rank lies
// in [lo, hi) to a sink put(rank, value), in increasing rank, and keeps its
// place in (bits, rank), so a caller that fills one window after another (the
// emit kernel's LDS staging windows) goes on where the window before ended.
// The function is __host__ __device__: the emit kernel and
// dse_debug_primes_word (tests, on the host) run the same code.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dse {

__host__ __device__ __forceinline__ uint32_t primes_ctz64(uint64_t x) {
#if defined(__HIP_DEVICE_COMPILE__)
  return (uint32_t)__ffsll((long long)x) - 1u;
#else
  return (uint32_t)__builtin_ctzll(x);
#endif
}

// bits: the word's entries not yet consumed (bits past the range's end already
// dropped); rank: the rank of its lowest set bit. Entries below lo are dropped,
// entries in [lo, hi) go to the sink, entries from hi on stay in `bits`.
// Returns the number of entries handed to the sink.
template <typename Sink>
__host__ __device__ __forceinline__ uint32_t primes_word(uint64_t& bits, uint64_t& rank, uint64_t g_word_start,
                                                         uint64_t lo, uint64_t hi, Sink&& put) {
  uint32_t n = 0;
  const uint64_t c = (uint64_t)__builtin_popcountll(bits);
  if (rank + c <= lo) {  // the whole word lies below the window
    rank += c;
    bits = 0;
    return 0;
  }
  while (bits && rank < hi) {
    if (rank >= lo) {
      put(rank, 3ull + 2ull * (g_word_start + primes_ctz64(bits)));
      ++n;
    }
    bits &= bits - 1;
    ++rank;
  }
  return n;
}

// [first, first + cap) as a rank interval that cannot wrap
__host__ __device__ __forceinline__ uint64_t primes_window_end(uint64_t first, uint64_t cap) {
  return cap > ~0ull - first ? ~0ull : first + cap;
}

}  // namespace dse
