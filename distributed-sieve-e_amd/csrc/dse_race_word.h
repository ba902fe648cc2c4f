// dse_race_word.h -- the per-word bodies of the residue-class counts and the prime
// race (dse_race.hip).
//
// The value of candidate g is 3 + 2 g, so its class mod q depends only on g mod T,
// T = q / gcd(q, 2) <= 63: the class of residue r is the one position c_r mod T
// (race_class_pos), or no candidate at all (q even, r even). Inside a word whose
// first candidate has the phase ph = g mod T, the candidates of position class c are
// the comb of period T (race_comb) shifted by (c - ph) mod T (race_class_mask).
//   race_count_word   the entries of a word per position class: T popcounts;
//   race_same_sign    the fast-path test: no step of the word can bring D to 0;
//   race_word         one word of the race: its steps are the set bits of A (+1) and
//                     B (-1); D0 = D at the word's start. With the sign decided and
//                     no new extremum possible the word's steps are added to the
//                     side that leads and no bit is walked; otherwise its steps are
//                     walked exactly, in increasing order;
//   race_max_better, race_min_better   the order of the extrema: largest (smallest)
//                     D, then lowest position; one without a position is none.
// A caller hands race_word its words in increasing order of position, so "first" is
// "not yet set". The functions are __host__ __device__: the kernels and
// dse_debug_race_host (tests, on the host) run the same code.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dse_mask.h"

namespace dse {

constexpr uint32_t kRaceMaxModulus = 64;             // DSE_RACE_MAX_MODULUS
constexpr uint32_t kRaceWords = 17 + kRaceMaxModulus;  // DSE_RACE_WORDS
constexpr uint64_t kRaceNone = ~0ull;                // DSE_RACE_NONE
constexpr uint32_t kRaceNoClass = ~0u;               // race_class_pos of a residue that holds no candidate
constexpr int64_t kRaceDMin = INT64_MIN, kRaceDMax = INT64_MAX;  // extrema not yet attained

// the period of the classes in candidates
__host__ __device__ __forceinline__ uint32_t race_period(uint32_t q) { return (q & 1u) ? q : q / 2; }

// bits 0, T, 2T, ... of a word
__host__ __device__ inline uint64_t race_comb(uint32_t T) {
  uint64_t c = 0;
  for (uint32_t k = 0; k < 64; k += T) c |= 1ull << k;
  return c;
}

// the g mod T of the candidates whose value is r mod q (r < q); kRaceNoClass if there is none
__host__ __device__ inline uint32_t race_class_pos(uint32_t q, uint32_t r) {
  const uint32_t m = (r + 2 * q - 3) % q;  // 2 g mod q
  if (q & 1u) return (uint32_t)((uint64_t)m * ((q + 1) / 2) % q);
  return (m & 1u) ? kRaceNoClass : m / 2;
}

// the candidates of position class c in a word whose first candidate has the phase ph (both < T)
__host__ __device__ __forceinline__ uint64_t race_class_mask(uint64_t comb, uint32_t T, uint32_t c, uint32_t ph) {
  if (c == kRaceNoClass) return 0ull;
  // (c - ph) mod T from the difference and its sign: no c + T per class to keep (the count kernel has 64 classes)
  const int32_t d = (int32_t)c - (int32_t)ph;
  return comb << (uint32_t)(d + ((d >> 31) & (int32_t)T));
}

// the phase of the word 256 words (one tile) on
__host__ __device__ __forceinline__ uint32_t race_phase_add(uint32_t ph, uint32_t step, uint32_t T) {
  ph += step;
  return ph >= T ? ph - T : ph;
}

// cnt[c] += entries of w in position class c, c < T <= kBound. The classes are taken in groups of
// race_count_group(kBound), one test of T per group: cnt[c] of a c >= T in the last group gets a
// number nobody reads (its shift stays below 64), and no per-class condition has to be kept.
constexpr uint32_t race_count_group(uint32_t bound) { return bound >= 64 ? 8 : bound >= 16 ? 4 : bound; }

template <uint32_t kBound, typename C>
__host__ __device__ __forceinline__ void race_count_word(uint64_t w, uint64_t comb, uint32_t T, uint32_t ph,
                                                         C (&cnt)[kBound]) {
  constexpr uint32_t kGroup = race_count_group(kBound);
  static_assert(kBound % kGroup == 0 && kBound <= 64, "whole groups");
#pragma unroll
  for (uint32_t c0 = 0; c0 < kBound; c0 += kGroup)
    if (c0 < T) {
#pragma unroll
      for (uint32_t c = c0; c < c0 + kGroup; ++c)
        cnt[c] += (C)__builtin_popcountll(w & race_class_mask(comb, T, c, ph));
    }
}

// D stays above 0 (below 0) through a word of na steps up and nb steps down that starts at D0
__host__ __device__ __forceinline__ bool race_same_sign(int64_t D0, uint32_t na, uint32_t nb) {
  return D0 > (int64_t)nb || -D0 > (int64_t)na;
}

__host__ __device__ __forceinline__ bool race_max_better(uint64_t d, uint64_t g, uint64_t bd, uint64_t bg) {
  if (g == kRaceNone) return false;
  if (bg == kRaceNone) return true;
  return (int64_t)d > (int64_t)bd || (d == bd && g < bg);
}
__host__ __device__ __forceinline__ bool race_min_better(uint64_t d, uint64_t g, uint64_t bd, uint64_t bg) {
  if (g == kRaceNone) return false;
  if (bg == kRaceNone) return true;
  return (int64_t)d < (int64_t)bd || (d == bd && g < bg);
}

// what one walker (a thread, the host loop) has seen of the race; positions count from the range's start
struct RaceAcc {
  uint64_t a_ahead = 0, b_ahead = 0;
  uint64_t first_a = kRaceNone, first_b = kRaceNone;
  int64_t max_d = kRaceDMin, min_d = kRaceDMax;
  uint64_t max_g = kRaceNone, min_g = kRaceNone;
};

__host__ __device__ __forceinline__ void race_word(uint64_t A, uint64_t B, int64_t D0, uint64_t pos0, RaceAcc& s) {
  uint64_t S = A | B;
  if (!S) return;
  const uint32_t na = (uint32_t)__builtin_popcountll(A), nb = (uint32_t)__builtin_popcountll(B);
  const bool extremum = D0 + (int64_t)na > s.max_d || D0 - (int64_t)nb < s.min_d;
  if (race_same_sign(D0, na, nb) && !extremum) {
    const uint64_t first = pos0 + (uint32_t)__builtin_ctzll(S);
    if (D0 > 0) {
      s.a_ahead += na + nb;
      if (s.first_a == kRaceNone) s.first_a = first;
    } else {
      s.b_ahead += na + nb;
      if (s.first_b == kRaceNone) s.first_b = first;
    }
    return;
  }
  int64_t D = D0;
  while (S) {
    const uint32_t k = (uint32_t)__builtin_ctzll(S);
    S &= S - 1;
    const uint64_t pos = pos0 + k;
    D += ((A >> k) & 1ull) ? 1 : -1;
    if (D > 0) {
      ++s.a_ahead;
      if (s.first_a == kRaceNone) s.first_a = pos;
    } else if (D < 0) {
      ++s.b_ahead;
      if (s.first_b == kRaceNone) s.first_b = pos;
    }
    if (D > s.max_d) {
      s.max_d = D;
      s.max_g = pos;
    }
    if (D < s.min_d) {
      s.min_d = D;
      s.min_g = pos;
    }
  }
}

}  // namespace dse
