// dse_sums_word.h -- the per-word and per-entry bodies of the power and reciprocal sums
// (dse_sums.hip). Every sum is an exact integer of little-endian uint64 limbs, so results are
// equal bit for bit whatever the grid and merge by plain addition.
//
// The match word of a mask word is dse_tuples_word.h's (tuples_word). Positions count from the
// range's start; a match at position p has the value B + 2p, B = 3 + 2 g_start.
//   sums_word_power   one match word at position pos (a multiple of 64) into a SumsPower: n, the
//                     sum of p and the sum of p^2 over its matches, from popcounts under fixed
//                     combs: no loop over the matches;
//   sums_power_close  a SumsPower and B into sum1 = n B + 2 P1 and sum2 = n B^2 + 4 B P1 + 4 P2,
//                     once per result;
//   sums_recip        floor(2^126 / v) for any v >= 3, exactly, without a 128-bit divide:
//                     three quotient digits from the f64 reciprocal, each an underestimate, and
//                     the remainder 2^126 - q v kept in 128-bit integers, which settles the last
//                     place;
//   sums_entry_recip  a match's required members into a 192-bit sum.
// Bounds of one call: p < 2^44 and at most 2^44 matches, so P1 < 2^88 (two limbs) and P2 < 2^132
// (three); a value is below 2^63 + 2 (the odd-index bound 2^62), so sum1 < 2^108 and sum2 < 2^171; a
// quotient is below 2^125 and 2^44 matches of 32 members stay below 2^174. No limb of an
// accumulator can overflow.
// The functions are __host__ __device__: the kernels and dse_debug_sums_host (tests, on the
// host) run the same code.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dse_stats_word.h"
#include "dse_tuples_word.h"

namespace dse {

constexpr uint32_t kSumsPower = 1u, kSumsRecip = 2u;  // DSE_SUMS_POWER, DSE_SUMS_RECIP
constexpr uint32_t kSumsRecipShift = 126;             // DSE_SUMS_RECIP_SHIFT
constexpr uint64_t kSumsNone = ~0ull;                 // DSE_SUMS_NONE

typedef unsigned __int128 sums_u128;

// a += x over little-endian limbs, kX <= kA, with explicit carries; the carry out of the top limb
// is dropped (the callers' bounds say there is none)
template <uint32_t kA, uint32_t kX>
__host__ __device__ __forceinline__ void limbs_add(uint64_t (&a)[kA], const uint64_t (&x)[kX]) {
  static_assert(kX <= kA, "the addend is no longer than the sum");
  uint64_t c = 0;
#pragma unroll
  for (uint32_t i = 0; i < kA; ++i) {
    const uint64_t xi = i < kX ? x[i] : 0ull;
    const uint64_t s = a[i] + xi;
    const uint64_t t = s + c;
    c = (uint64_t)(s < xi) | (uint64_t)(t < s);
    a[i] = t;
  }
}

// a *= m
template <uint32_t kA>
__host__ __device__ __forceinline__ void limbs_mul64(uint64_t (&a)[kA], uint64_t m) {
  uint64_t c = 0;
#pragma unroll
  for (uint32_t i = 0; i < kA; ++i) {
    const sums_u128 p = (sums_u128)a[i] * m + c;
    a[i] = (uint64_t)p;
    c = (uint64_t)(p >> 64);
  }
}

struct SumsPower {
  uint64_t n;      // matches
  uint64_t p1[2];  // sum of their positions
  uint64_t p2[3];  // sum of the squares of their positions
};

// the bits of a word whose place i has bit k set, k < 6
__host__ __device__ __forceinline__ uint64_t sums_comb(uint32_t k) {
  return k == 0 ? 0xAAAAAAAAAAAAAAAAull
       : k == 1 ? 0xCCCCCCCCCCCCCCCCull
       : k == 2 ? 0xF0F0F0F0F0F0F0F0ull
       : k == 3 ? 0xFF00FF00FF00FF00ull
       : k == 4 ? 0xFFFF0000FFFF0000ull
                : 0xFFFFFFFF00000000ull;
}

// The matches m of the word at position pos: i = sum_k 2^k [bit k of i], so the sum of i over m's
// bits is sum_k 2^k pop(m & comb_k) and the sum of i^2 is sum_{k, l} 2^(k + l) pop(m & comb_k & comb_l).
__host__ __device__ __forceinline__ void sums_word_power(uint64_t m, uint64_t pos, SumsPower& acc) {
  if (!m) return;
  const uint64_t n = stats_pop64(m);
  uint64_t s1 = 0, s2 = 0;
#pragma unroll
  for (uint32_t k = 0; k < 6; ++k) {
    const uint64_t mk = m & sums_comb(k);
    const uint64_t ck = stats_pop64(mk);
    s1 += ck << k;
    s2 += ck << (2 * k);
#pragma unroll
    for (uint32_t l = k + 1; l < 6; ++l) s2 += (uint64_t)stats_pop64(mk & sums_comb(l)) << (k + l + 1);
  }
  acc.n += n;
  // sum of (pos + i) = n pos + s1 < 2^51; sum of (pos + i)^2 = n pos^2 + 2 pos s1 + s2 < 2^95
  const uint64_t d1[1] = {n * pos + s1};
  limbs_add(acc.p1, d1);
  const sums_u128 t = (sums_u128)pos * pos * n + (sums_u128)(2 * pos) * s1 + s2;
  const uint64_t d2[2] = {(uint64_t)t, (uint64_t)(t >> 64)};
  limbs_add(acc.p2, d2);
}

// sum1 (two limbs) and sum2 (three) of the matches in `acc` whose positions count from the value B
__host__ __device__ inline void sums_power_close(const SumsPower& acc, uint64_t B, uint64_t (&sum1)[2],
                                                 uint64_t (&sum2)[3]) {
  // n B + 2 P1
  const sums_u128 nb = (sums_u128)acc.n * B;
  sum1[0] = (uint64_t)nb;
  sum1[1] = (uint64_t)(nb >> 64);
  uint64_t t2[2] = {acc.p1[0], acc.p1[1]};
  limbs_mul64(t2, 2);
  limbs_add(sum1, t2);
  // n B^2 + 4 B P1 + 4 P2
  const sums_u128 bb = (sums_u128)B * B;
  sum2[0] = (uint64_t)bb;
  sum2[1] = (uint64_t)(bb >> 64);
  sum2[2] = 0;
  limbs_mul64(sum2, acc.n);
  uint64_t t3[3] = {acc.p1[0], acc.p1[1], 0ull};
  limbs_mul64(t3, B);
  limbs_mul64(t3, 4);
  limbs_add(sum2, t3);
  uint64_t u3[3] = {acc.p2[0], acc.p2[1], acc.p2[2]};
  limbs_mul64(u3, 4);
  limbs_add(sum2, u3);
}

// floor(2^126 / v), 3 <= v < 2^64: q[0] low, q[1] high (below 2^125).
//
// r = 2^126 - q v is kept exactly. A step takes est = r * inv in f64, inv = (1 - 2^-46) / v: the
// conversions of r and v, the division and the product are five roundings of 2^-53 each, so
// est < r / v, and floor(est) v <= r: r never goes negative. With qi >= est - 1 and
// est >= (r / v)(1 - 2^-45) a step leaves r' <= r 2^-45 + v: 2^81 + v, then 2^36 + 2^19 + v, then
// less than 2 v. The closing loop therefore runs at most once, and it makes the result exact
// whatever the estimates were: it ends with 0 <= r < v and q v + r = 2^126.
__host__ __device__ __forceinline__ void sums_recip(uint64_t v, uint64_t (&q)[2]) {
  const double inv = (1.0 - 0x1p-46) / (double)v;
  sums_u128 r = (sums_u128)1 << kSumsRecipShift, acc = 0;
#pragma unroll
  for (uint32_t k = 0; k < 3; ++k) {
    const double rd = (double)(uint64_t)(r >> 64) * 0x1p64 + (double)(uint64_t)r;
    const double est = rd * inv;
    // floor(est) as two words: est 2^-64 is exact, and so is what its floor leaves of est
    const uint64_t eh = (uint64_t)(est * 0x1p-64);
    const uint64_t el = (uint64_t)(est - (double)eh * 0x1p64);
    const sums_u128 qi = ((sums_u128)eh << 64) | el;
    acc += qi;
    r -= qi * v;
  }
  while (r >= v) {
    ++acc;
    r -= v;
  }
  q[0] = (uint64_t)acc;
  q[1] = (uint64_t)(acc >> 64);
}

// acc += sum over the set bits j of require of floor(2^126 / (v + 2j)), v a match's value
__host__ __device__ __forceinline__ void sums_entry_recip(uint64_t v, uint32_t require, uint64_t (&acc)[3]) {
  for (uint32_t r = require; r; r &= r - 1) {
    uint64_t q[2];
    sums_recip(v + 2ull * (uint32_t)__builtin_ctz(r), q);
    limbs_add(acc, q);
  }
}

}  // namespace dse
