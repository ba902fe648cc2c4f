// dse_finish_fmt.h -- the per-value formatter of the device finish (dse_finish.hip).
//
// One entry of a primes{k}.txt file (sieve.clj:82-108) is
//   [", " unless it opens a line]  <value>  ["\n" when it is the line's tenth]
// with <value> printed as a Java Long (plain decimal) or, for chunk 1, as
// java.lang.Double.toString prints an integer-valued double below 2^53:
// "<digits>.0" below 10^7, otherwise d0 "." d1..d(sig-1) "E" (len-1) with the
// trailing zeros of the digit string trimmed (sig digits kept, "0" after the
// point when only d0 is left). The functions are __host__ __device__: the
// emit kernel and dse_debug_finish_format (tests, on the host) run the same
// code. Characters go through a sink put(pos, ch), so the kernel can clip an
// entry to its LDS window without a private byte array.
//
// Digits come from at most three pieces of nine digits, v = hi*10^18 +
// mid*10^9 + lo, split once with multiply-high by constants; a piece p < 10^9
// is turned into the 7.57 fixed-point fraction p * ceil(2^57 / 10^8), whose
// integer part is the leading digit and which yields the next digit with each
// multiplication by ten (error < 0.2415 * 10^9 * 10^8 < 2^57 after the eight
// multiplications, so every digit is exact).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dse {

// = DSE_FINISH_* of include/dse.h
constexpr uint32_t kFinishDoubles = 1u;
constexpr uint32_t kFinishHack = 2u;
constexpr uint32_t kFinishLast = 4u;

__host__ __device__ __forceinline__ uint64_t fin_mulhi64(uint64_t a, uint64_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __umul64hi(a, b);
#else
  return (uint64_t)(((unsigned __int128)a * b) >> 64);
#endif
}

// floor(v / 10^9), any 64-bit v: 10^9 = 2^9 * 5^9, and for x = v >> 9 < 2^55
// floor(x / 5^9) = mulhi(x, M) >> 11 with M = ceil(2^75 / 5^9)
// (M * 5^9 - 2^75 = 1,474,639 <= 2^75 / 2^55).
__host__ __device__ __forceinline__ uint64_t fin_div1e9(uint64_t v) {
  return fin_mulhi64(v >> 9, 0x44B82FA09B5A53ull) >> 11;
}

__host__ __device__ __forceinline__ uint64_t fin_pow10(uint32_t k) {
  const uint64_t t[20] = {1ull,
                          10ull,
                          100ull,
                          1000ull,
                          10000ull,
                          100000ull,
                          1000000ull,
                          10000000ull,
                          100000000ull,
                          1000000000ull,
                          10000000000ull,
                          100000000000ull,
                          1000000000000ull,
                          10000000000000ull,
                          100000000000000ull,
                          1000000000000000ull,
                          10000000000000000ull,
                          100000000000000000ull,
                          1000000000000000000ull,
                          10000000000000000000ull};
  return t[k];
}

// decimal digits of v (1 for v = 0)
__host__ __device__ __forceinline__ uint32_t fin_ndigits(uint64_t v) {
  const uint32_t bits = 64u - (uint32_t)__builtin_clzll(v | 1ull);
  const uint32_t t = (bits * 1233u) >> 12;  // floor(bits * log10(2)) for bits <= 64
  return t + 1u - (v < fin_pow10(t) ? 1u : 0u);
}

// Bytes of <value> when no trailing zero is trimmed (sig == len). The size
// pass of the finish kernels may assume that: every value printed from a mask
// bit is 3 + 2g, odd, so its last digit is not 0 and Double.toString keeps
// all len digits; the hack literals 2, 3, 5, 7 are below 10^7, where nothing
// is trimmed either. Monotone in v for either printing.
__host__ __device__ __forceinline__ uint32_t fin_value_len(uint64_t v, bool doubles) {
  const uint32_t len = fin_ndigits(v);
  if (!doubles) return len;
  if (v < 10000000ull) return len + 2u;         // "<digits>.0"
  return len + 2u + (len > 10u ? 2u : 1u);      // "." and "E" and a 1- or 2-digit exponent
}

// Print <value> at pos through put(pos, ch); returns its length. General:
// even values are trimmed as Double.toString trims them.
template <class Sink>
__host__ __device__ __forceinline__ uint32_t fin_format_value(uint64_t v, bool doubles, uint32_t pos, Sink&& put) {
  const uint32_t len = fin_ndigits(v);
  const uint64_t q1 = fin_div1e9(v);
  const uint32_t lo = (uint32_t)(v - q1 * 1000000000ull);
  const uint32_t hi = (uint32_t)fin_div1e9(q1);
  const uint32_t mid = (uint32_t)(q1 - (uint64_t)hi * 1000000000ull);
  const bool sci = doubles && v >= 10000000ull;
  uint32_t sig = len;
  if (sci && !(v & 1ull)) {  // trailing zeros of the digit string (never for a value printed from a bit)
    uint32_t p = lo, tz = 0;
    if (p == 0) {
      tz = 9;
      p = mid;
      if (p == 0) {
        tz = 18;
        p = hi;
      }
    }
    while (p % 10u == 0u) {
      p /= 10u;
      ++tz;
    }
    sig = len - tz;
  }
  // digit i (0 = most significant) is frame digit i + 27 - len of the 27-digit frame hi|mid|lo;
  // it lands at pos + i, or one further right behind the point of the E form
  const uint32_t lead = 27u - len;
  auto piece = [&](uint32_t p, uint32_t k0) {
    uint64_t t = (uint64_t)p * 1441151881ull;  // ceil(2^57 / 10^8)
#pragma unroll
    for (uint32_t j = 0; j < 9; ++j) {
      const uint32_t d = (uint32_t)(t >> 57);
      t = (t & ((1ull << 57) - 1)) * 10ull;
      const uint32_t i = k0 + j - lead;  // wraps for the frame's leading zeros
      if (i < sig) put(pos + i + ((sci && i) ? 1u : 0u), (char)('0' + d));
    }
  };
  if (len > 18u) piece(hi, 0u);
  if (len > 9u) piece(mid, 9u);
  piece(lo, 18u);
  if (!doubles) return len;
  if (!sci) {
    put(pos + len, '.');
    put(pos + len + 1u, '0');
    return len + 2u;
  }
  put(pos + 1u, '.');
  uint32_t n = sig + 1u;
  if (sig == 1u) put(pos + n++, '0');
  put(pos + n++, 'E');
  const uint32_t e = len - 1u;  // 7..19
  if (e >= 10u) put(pos + n++, '1');
  put(pos + n++, (char)('0' + (e >= 10u ? e - 10u : e)));
  return n;
}

// Separator and line-end bytes of the entries of ranks [0, R): a full line of
// ten carries nine ", " and one "\n"; m entries of a partial line carry m-1 ", ".
__host__ __device__ __forceinline__ uint64_t fin_sep_bytes(uint64_t R) {
  const uint64_t q = R / 10u, m = R - q * 10u;
  return 19u * q + (m ? 2u * (m - 1u) : 0u);
}

// One whole entry whose rank is r10 mod 10, at pos; returns its length.
template <class Sink>
__host__ __device__ __forceinline__ uint32_t fin_format_entry(uint64_t v, bool doubles, uint32_t r10, uint32_t pos,
                                                              Sink&& put) {
  uint32_t n = 0;
  if (r10) {
    put(pos, ',');
    put(pos + 1u, ' ');
    n = 2u;
  }
  n += fin_format_value(v, doubles, pos + n, put);
  if (r10 == 9u) put(pos + n++, '\n');
  return n;
}

}  // namespace dse
