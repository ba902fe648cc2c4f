// dse_consec_word.h -- the per-word bodies of the residue pairs of consecutive
// primes (dse_consec.hip).
//
// The class mod q of candidate g depends only on g mod T, T = race_period(q) <= 63
// (dse_race_word.h), so the pairs are counted by position class (c, c'), c = g mod T
// of the lower prime and c' of the upper, in bin c * kConsecStride + c'; the closing
// kernel maps position classes to residues. A pair whose two primes lie in one word
// is an in-word pair, counted by one of two bodies:
//   consec_count_word  bit-parallel. For a lower class c with the candidates M_c
//                      (race_class_mask), S_c = (~w + ((w & M_c) << 1)) & w is the set
//                      of entries of w whose predecessor entry in w lies in class c:
//                      the 1 injected above an entry of class c ripples through the
//                      non-entries (the ones of ~w) and lands on the next entry (a
//                      zero of ~w), where it stops; two injections cannot meet, since
//                      the lower one stops at or below the upper one's entry. A carry
//                      out of bit 63 is the word's last entry, whose successor is not
//                      in w. Then cnt[c][c'] += popcount(S_c & M_c'): about T (and,
//                      shift, add, and) + T^2 (and, popcount) operations per word,
//                      into registers.
//   consec_walk_word   per entry. The set bits of w in increasing order, the class
//                      of each (ph + k) mod T by a multiplication (consec_mod), one
//                      add(c, c') per pair.
// The first entry of a word is the upper prime of a cross-word pair, which the caller
// counts from its scan of "last prime so far". The functions are __host__ __device__:
// the kernels and dse_debug_consec_host (tests, on the host) run the same code.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dse_race_word.h"

namespace dse {

constexpr uint32_t kConsecMaxModulus = 64;                                          // DSE_CONSEC_MAX_MODULUS
constexpr uint32_t kConsecStride = kConsecMaxModulus;                               // bins of a lower class
constexpr uint32_t kConsecBins = kConsecMaxModulus * kConsecStride;
constexpr uint32_t kConsecWords = 7 + kConsecBins;                                  // DSE_CONSEC_WORDS
constexpr uint64_t kConsecNone = ~0ull;                                             // DSE_CONSEC_NONE
// The bit-parallel body is taken up to T = kConsecBitMaxT, the per-entry body above: at N = 1e11 on the
// MI355X it wins by 55%, 48%, 18% and 2% for T = 2, 3, 4, 5 and loses by 17% for T = 6, by 46% and 72% for
// 7 and 8 (profiles/r20/ab_consec_threshold.txt). It is built for every T up to kConsecBitBuiltT, one
// past the threshold, so that the bench tool can show the crossing.
constexpr uint32_t kConsecBitMaxT = 5;
constexpr uint32_t kConsecBitBuiltT = 6;

// x mod T for x < 2^26 / T by one multiplication: M = consec_magic(T) = floor(2^32 / T) + 1, so
// M T = 2^32 + e with 1 <= e <= T, and floor(x M / 2^32) = floor(x / T) while x e < 2^32.
__host__ __device__ __forceinline__ uint32_t consec_magic(uint32_t T) { return (uint32_t)((1ull << 32) / T) + 1u; }
__host__ __device__ __forceinline__ uint32_t consec_mod(uint32_t x, uint32_t T, uint32_t M) {
  return x - (uint32_t)(((uint64_t)x * M) >> 32) * T;
}

// the entries of w whose predecessor entry in w is one of the candidates Mc
__host__ __device__ __forceinline__ uint64_t consec_succ(uint64_t w, uint64_t Mc) {
  return (~w + ((w & Mc) << 1)) & w;
}

// cnt[c * kBound + c'] += in-word pairs of w of the position classes (c, c'), c, c' < T <= kBound; ph
// is the phase of the word's first candidate. Rows c >= T are skipped; cnt[c][c'] of a c' >= T gets
// a number nobody reads (race_class_mask's shift stays below 64).
template <uint32_t kBound, typename C>
__host__ __device__ __forceinline__ void consec_count_word(uint64_t w, uint64_t comb, uint32_t T, uint32_t ph,
                                                           C (&cnt)[kBound * kBound]) {
  static_assert(kBound <= 64, "a class per bit of the period at most");
  uint64_t M[kBound];
#pragma unroll
  for (uint32_t c = 0; c < kBound; ++c) M[c] = w & race_class_mask(comb, T, c, ph);
#pragma unroll
  for (uint32_t c = 0; c < kBound; ++c)
    if (c < T) {
      const uint64_t S = (~w + (M[c] << 1)) & w;  // consec_succ(w, M_c)
#pragma unroll
      for (uint32_t c2 = 0; c2 < kBound; ++c2) cnt[c * kBound + c2] += (C)__builtin_popcountll(S & M[c2]);
    }
}

// add(c, c') for every in-word pair of w, in increasing order; M = consec_magic(T)
template <typename Add>
__host__ __device__ __forceinline__ void consec_walk_word(uint64_t w, uint32_t T, uint32_t M, uint32_t ph, Add&& add) {
  if (!w) return;
  uint32_t c = consec_mod(ph + (uint32_t)__builtin_ctzll(w), T, M);
  w &= w - 1;
  while (w) {
    const uint32_t c2 = consec_mod(ph + (uint32_t)__builtin_ctzll(w), T, M);
    w &= w - 1;
    add(c, c2);
    c = c2;
  }
}

}  // namespace dse
