// dse_goldbach_word.h -- the per-word bodies of the minimal Goldbach partitions
// (dse_goldbach.hip) and the table of the small primes.
//
// A range's candidates are numbered 0 .. nbits - 1 from its start ("positions");
// the candidates the caller supplies below it have the positions -below_bits .. -1.
// The even of position c is 6 + 2 (g_start + c); its partition with the small
// prime P_i = 3 + 2 h_i holds iff position c - h_i is a visible entry. A thread
// (or the host loop of dse_debug_goldbach_host) owns the 64 evens of one mask
// word as the set U of those still unresolved, and walks the ranks i upwards:
//   gb_bits64   the visible entries of 64 positions, from the mask, from `below`
//               or zeros: the one function every word of a tile's line comes from;
//   gb_window   the 64 positions from c0 - h_i on, from three 32-bit words of the
//               line by two funnel shifts (the shift is the same for every word
//               of a tile: (-h_i) mod 32);
//   gb_search   the ranks [i0, i1) of one word: the three line words slide down
//               as h_i grows, so a rank costs a load only when h_i crosses a
//               multiple of 32; leaves when `any` says nothing is unresolved.
// The functions are __host__ __device__: the kernels and dse_debug_goldbach_host
// (tests, on the host) run the same code.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dse_mask.h"

namespace dse {

constexpr uint32_t kGbPrimes = 2048;    // DSE_GOLDBACH_PRIMES
constexpr uint32_t kGbReachMax = 8939;  // h of the last of them, 17881
constexpr uint64_t kGbNone = ~0ull;     // DSE_GOLDBACH_NONE
// words of a tile's line below the tile: position c0 - h lies at most this many words below c0
constexpr uint32_t kGbLowWords = (kGbReachMax + 63) / 64;
constexpr uint32_t kGbLineWords = kGbLowWords + kMaskTileWords;

// ranks searched by gb_search_first, their hits counted in registers by the kernel
#ifndef DSE_GB_REG_RANKS
#define DSE_GB_REG_RANKS 16
#endif
constexpr uint32_t kGbRegRanks = DSE_GB_REG_RANKS;
static_assert(kGbRegRanks % 4 == 0, "gb_search starts at a multiple of 4");

// h_i = (P_i - 3) / 2 of the first kGbPrimes odd primes
// (16 bits each, four to a 64-bit word: the kernel reads them with scalar loads, which have no
// 16-bit form, one load ahead of the four ranks it is for)
struct GbTable {
  uint64_t pk[kGbPrimes / 4];
  uint32_t count;  // odd primes up to 3 + 2 kGbReachMax: kGbPrimes exactly
  __host__ __device__ constexpr uint32_t h(uint32_t i) const {
    return (uint32_t)(pk[i >> 2] >> (16u * (i & 3u))) & 0xFFFFu;
  }
};

constexpr GbTable gb_make_table() {
  GbTable t{};
  bool comp[kGbReachMax + 1] = {};  // comp[j]: 3 + 2j is composite
  for (uint32_t j = 0; j <= kGbReachMax; ++j) {
    if (comp[j]) continue;
    if (t.count < kGbPrimes) t.pk[t.count >> 2] |= (uint64_t)j << (16u * (t.count & 3u));
    ++t.count;
    const uint32_t p = 3 + 2 * j;
    for (uint32_t m = (p * p - 3) / 2; m <= kGbReachMax; m += p) comp[m] = true;
  }
  return t;
}
constexpr GbTable kGbTable = gb_make_table();
static_assert(kGbTable.count == kGbPrimes && kGbTable.h(kGbPrimes - 1) == kGbReachMax && kGbTable.h(0) == 0 &&
                  kGbTable.h(1023) == (8167 - 3) / 2,
              "the first 2048 odd primes end at 17881");

// What a call sees: the range's mask and the candidates below it, each a bit string
// that starts `shift` bits into its first word.
struct GbSrc {
  const uint64_t* mask;
  const uint64_t* below;
  uint64_t nbits, below_bits;
  uint32_t mask_shift, below_shift;  // mask_shift < 64 (0 for a caller's mask), below_shift < 64
};

// bits [b, b + 64) of a bit string; words past `last` are not read (their bits come back 0)
__host__ __device__ __forceinline__ uint64_t gb_str64(const uint64_t* s, uint64_t last, uint64_t b) {
  const uint64_t w = b >> 6;
  const uint32_t sh = (uint32_t)(b & 63);
  uint64_t v = w <= last ? s[w] >> sh : 0ull;
  if (sh && w < last) v |= s[w + 1] << (64 - sh);
  return v;
}

// The visible entries of the positions [s, s + 64), s a multiple of 64 (negative: below the
// range). Bit k = position s + k; 0 past nbits, below -below_bits and for what is not an entry.
__host__ __device__ __forceinline__ uint64_t gb_bits64(const GbSrc& a, int64_t s) {
  if (s >= 0) {
    if ((uint64_t)s >= a.nbits) return 0ull;
    const uint64_t left = a.nbits - (uint64_t)s;
    const uint64_t v = gb_str64(a.mask, (a.mask_shift + a.nbits - 1) >> 6, a.mask_shift + (uint64_t)s);
    return left < 64 ? v & ((1ull << left) - 1) : v;
  }
  const int64_t j0 = (int64_t)a.below_bits + s;  // bit 0 is candidate j0 of `below`
  if (j0 <= -64 || a.below_bits == 0) return 0ull;
  const uint64_t last = (a.below_shift + a.below_bits - 1) >> 6;
  if (j0 >= 0) return gb_str64(a.below, last, a.below_shift + (uint64_t)j0);
  // the lowest -j0 positions lie below `below`; what the shift pushes out lies past its end
  return gb_str64(a.below, last, a.below_shift) << (uint32_t)(-j0);
}

// the evens of word wi of a range of nbits: one bit per candidate inside the range
__host__ __device__ __forceinline__ uint64_t gb_evens(uint64_t nbits, uint64_t wi) {
  const uint64_t c0 = wi * 64ull;
  if (c0 >= nbits) return 0ull;
  return nbits - c0 < 64 ? (1ull << (nbits - c0)) - 1 : ~0ull;
}

// bits [s, s + 64) of the 96 bits {c : b : a}, s < 32
__host__ __device__ __forceinline__ uint64_t gb_window(uint32_t a, uint32_t b, uint32_t c, uint32_t s) {
#if defined(__HIP_DEVICE_COMPILE__)
  return (uint64_t)__builtin_amdgcn_alignbit(b, a, s) | ((uint64_t)__builtin_amdgcn_alignbit(c, b, s) << 32);
#else
  const uint64_t lo = (uint64_t)a | ((uint64_t)b << 32);
  return s ? (lo >> s) | ((uint64_t)c << (64 - s)) : lo;
#endif
}

// 32-bit words below word d0 of the line at which the window of h starts, and its shift
__host__ __device__ __forceinline__ uint32_t gb_back(uint32_t h) { return (h + 31u) >> 5; }
__host__ __device__ __forceinline__ uint32_t gb_shift(uint32_t h) { return (0u - h) & 31u; }

// The ranks [i0, i1) for the evens U of the word whose first candidate is bit 0 of the line's
// 32-bit word d0: ld(k) = 32-bit word k of the line (k >= d0 - gb_back(h of rank i1 - 1), k <= d0 + 2).
// on_hit(i, hit) gets the evens whose minimal rank is i (hit may be 0). Returns what is left
// of U. The words a, b, c slide: xp = gb_back of the rank before (the same in every word of a
// tile, so the reloads are wave-uniform branches on the device).
struct GbSlide {
  uint32_t a = 0, b = 0, c = 0, xp = 0;
  bool have = false;
};

// one rank of gb_search: slide to h and return the window of the 64 positions from c0 - h on
template <typename Ld>
__host__ __device__ __forceinline__ uint64_t gb_rank(GbSlide& w, uint32_t h, uint32_t d0, Ld&& ld) {
  const uint32_t x = gb_back(h), dl = x - w.xp, k = d0 - x;
  if (!w.have || dl > 2) {
    w.a = ld(k);
    w.b = ld(k + 1);
    w.c = ld(k + 2);
    w.have = true;
  } else if (dl == 1) {
    w.c = w.b;
    w.b = w.a;
    w.a = ld(k);
  } else if (dl == 2) {
    w.c = w.a;
    w.b = ld(k + 1);
    w.a = ld(k);
  }
  w.xp = x;
  return gb_window(w.a, w.b, w.c, gb_shift(h));
}

template <typename Ld, typename Any, typename Hit>
__host__ __device__ __forceinline__ uint64_t gb_search(uint64_t U, const GbTable& h, uint32_t i0, uint32_t i1,
                                                       uint32_t d0, Ld&& ld, Any&& any, Hit&& on_hit) {
  GbSlide w;
  uint64_t nxt = h.pk[i0 >> 2];  // i0 is a multiple of 4
  for (uint32_t i = i0; i < i1; i += 4) {
    const uint64_t quad = nxt;
    nxt = h.pk[i + 4 < kGbPrimes ? (i >> 2) + 1 : i >> 2];  // in flight while these four ranks run
#pragma unroll
    for (uint32_t j = 0; j < 4; ++j) {
      if (i + j >= i1 || !any(U)) return U;
      const uint64_t hit = U & gb_rank(w, (uint32_t)(quad >> (16u * j)) & 0xFFFFu, d0, ld);
      U ^= hit;
      on_hit(i + j, hit);
    }
  }
  return U;
}

// The ranks [0, min(kRanks, n)) the same way with everything about the rank a compile-time
// constant (kGbTable): no table read, no reload test, and on_hit's i indexes registers. It
// does not leave early (on real primes nearly every word has evens left at these ranks) and
// it slides through all kRanks windows: past rank n they hit nothing.
template <uint32_t kRanks, typename Ld, typename Hit>
__host__ __device__ __forceinline__ uint64_t gb_search_first(uint64_t U, uint32_t n, uint32_t d0, Ld&& ld,
                                                             Hit&& on_hit) {
  GbSlide w;
#pragma unroll
  for (uint32_t i = 0; i < kRanks; ++i) {
    const uint64_t hit = U & gb_rank(w, kGbTable.h(i), d0, ld) & (i < n ? ~0ull : 0ull);
    U ^= hit;
    on_hit(i, hit);
  }
  return U;
}

// (r, c) comes before (br, bc) as the range's maximum: a higher rank, or the same at a lower
// candidate; kGbNone as br: no maximum yet
__host__ __device__ __forceinline__ bool gb_better(uint64_t r, uint64_t c, uint64_t br, uint64_t bc) {
  return br == kGbNone || r > br || (r == br && c < bc);
}

}  // namespace dse
