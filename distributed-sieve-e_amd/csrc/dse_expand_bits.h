// dse_expand_bits.h -- the expand phase's block transform: the 8 plane words
// of one image block (composite bits, 32 periods each) to the block's 15
// output words (prime bits of 480 odd candidates), in registers.
//
// Output bit 15k + slot_i is set exactly when bit k of plane i is clear, with
// slot_i = (rho_i - 1)/2 the odd slot of plane i's residue rho_i inside a
// period of 30. The slots depend only on V0 mod 30, which is even: variant
// T = (V0 mod 30)/2 in [0, 15), and the slot of plane i is the i-th smallest
// of {((r - 1)/2 - T) mod 15 : r in kR30} (rho = (r - V0) mod 30 ascends with
// its slot).
//
// A period's 15-bit field is thus its 8 plane bits moved to fixed positions:
// with the complemented plane words as rows Z[slot_i] of a 16-row matrix (the
// other 8 rows zero), a 16 x 16 bit transpose turns row = slot, column =
// period into row = period, column = slot. It runs on both 16-bit halves of
// the registers at once (stages S = 8, 4, 2, 1), so afterwards register c
// holds the field of period c in bits 0..14 and that of period c + 16 in bits
// 16..30. Which rows are zero is known per variant and stage (ExpandPlan), so
// a swap with one zero row takes 3 operations instead of 4 and one between two
// zero rows none. Field k belongs at output bit 15k, and 15 * 16 = 240 = 16
// (mod 32): one rotate of register c by 15c mod 32 puts both of its fields at
// their in-word positions, where each takes one AND with a constant and an OR
// into its word, and one more for the 15 fields that straddle two words.
//
// Host and device share the body; only the full swap has a device form
// (v_bfi_b32, which the compiler does not pick for the C expression).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dse_internal.h"

namespace dse {

constexpr int kExpandVariants = 15;

struct ExpandPlan {
  uint8_t slot[8];  // row (odd slot) of plane i
  uint16_t nz[5];   // bit r: row r may be non-zero before stage st (nz[4]: after the last)
};

constexpr ExpandPlan make_expand_plan(int T) {
  ExpandPlan p{};
  bool used[15] = {};
  for (int j = 0; j < 8; ++j) used[((int)(kR30[j] - 1) / 2 + 15 - T) % 15] = true;
  int n = 0;
  uint32_t nz = 0;
  for (int s = 0; s < 15; ++s)
    if (used[s]) {
      p.slot[n++] = (uint8_t)s;
      nz |= 1u << s;
    }
  p.nz[0] = (uint16_t)nz;
  for (int st = 0; st < 4; ++st) {
    const int S = 8 >> st;
    uint32_t next = 0;
    for (int r = 0; r < 16; ++r)
      if (!(r & S) && ((nz >> r | nz >> (r + S)) & 1u)) next |= 1u << r | 1u << (r + S);
    nz = next;
    p.nz[st + 1] = (uint16_t)nz;
  }
  return p;
}

// The stages' column masks (the columns with bit S clear). A full swap's
// v_bfi_b32 takes its mask from an SGPR; the device form of expand_masks()
// hides the constants from the optimiser, so they occupy SGPRs from the call
// on (the kernel calls it per segment, before its block loop) and not across
// the whole kernel.
struct ExpandMasks {
  uint32_t m8, m4, m2, m1;
};
__host__ __device__ __forceinline__ ExpandMasks expand_masks() {
  ExpandMasks k{0x00FF00FFu, 0x0F0F0F0Fu, 0x33333333u, 0x55555555u};
#if defined(__HIP_DEVICE_COMPILE__)
  asm volatile("" : "+s"(k.m8), "+s"(k.m4), "+s"(k.m2), "+s"(k.m1));
#endif
  return k;
}

// Rows a (row index bit S clear) and b = a + S trade a's columns with bit S
// set for b's columns with bit S clear.
template <int S, bool NZA, bool NZB>
__host__ __device__ __forceinline__ void expand_row_swap(uint32_t& a, uint32_t& b, const ExpandMasks& k) {
  constexpr uint32_t m = S == 8 ? 0x00FF00FFu : S == 4 ? 0x0F0F0F0Fu : S == 2 ? 0x33333333u : 0x55555555u;
  const uint32_t x = a, y = b;
  if (NZA && NZB) {
#if defined(__HIP_DEVICE_COMPILE__)
    const uint32_t ms = S == 8 ? k.m8 : S == 4 ? k.m4 : S == 2 ? k.m2 : k.m1;
    // (x & m) | (y & ~m); both with m, so a stage keeps one mask in an SGPR
    asm("v_bfi_b32 %0, %1, %2, %3" : "=v"(b) : "s"(ms), "v"(x >> S), "v"(y));
    asm("v_bfi_b32 %0, %1, %2, %3" : "=v"(a) : "s"(ms), "v"(x), "v"(y << S));
#else
    (void)k;
    b = ((x >> S) & m) | (y & ~m);
    a = ((y << S) & ~m) | (x & m);
#endif
  } else if (NZA) {
    a = x & m;
    b = (x >> S) & m;
  } else if (NZB) {
    a = (y << S) & ~m;
    b = y & ~m;
  }
}

template <int T, int ST, int R>
__host__ __device__ __forceinline__ void expand_stage_row(uint32_t (&Z)[16], const ExpandMasks& k) {
  constexpr ExpandPlan plan = make_expand_plan(T);
  constexpr int S = 8 >> ST;
  if constexpr (!(R & S))
    expand_row_swap<S, (plan.nz[ST] >> R & 1) != 0, (plan.nz[ST] >> (R + S) & 1) != 0>(Z[R], Z[R + S], k);
  if constexpr (R + 1 < 16) expand_stage_row<T, ST, R + 1>(Z, k);
}

// P[i]: plane i's word of the block (bit k set: period k's candidate is
// composite). o[0..15): the block's output words (bit set: prime). k:
// expand_masks().
template <int T>
__host__ __device__ __forceinline__ void expand_block(const uint32_t (&P)[8], uint32_t (&o)[15],
                                                      const ExpandMasks& k) {
  static_assert(T >= 0 && T < kExpandVariants, "variant = (V0 mod 30) / 2");
  constexpr ExpandPlan plan = make_expand_plan(T);
  uint32_t Z[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) Z[r] = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) Z[plan.slot[i]] = ~P[i];
  expand_stage_row<T, 0, 0>(Z, k);
  expand_stage_row<T, 1, 0>(Z, k);
  expand_stage_row<T, 2, 0>(Z, k);
  expand_stage_row<T, 3, 0>(Z, k);
#pragma unroll
  for (int w = 0; w < 15; ++w) o[w] = 0;
#pragma unroll
  for (int c = 0; c < 16; ++c) {
    const int rot = (15 * c) & 31;
    const uint32_t r = rot ? (Z[c] << rot) | (Z[c] >> (32 - rot)) : Z[c];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int pos = 15 * (c + 16 * h), w = pos >> 5, p = pos & 31;
      o[w] |= r & (0x7FFFu << p);
      if (p > 17) o[w + 1] |= r & ((1u << (p - 17)) - 1u);
    }
  }
}

// Host dispatch over the variants (the kernel switches once per segment
// around its block loop instead). False for a variant outside [0, 15).
inline bool expand_block_variant(int variant, const uint32_t (&P)[8], uint32_t (&o)[15]) {
  const ExpandMasks k = expand_masks();
  switch (variant) {
    case 0: expand_block<0>(P, o, k); return true;
    case 1: expand_block<1>(P, o, k); return true;
    case 2: expand_block<2>(P, o, k); return true;
    case 3: expand_block<3>(P, o, k); return true;
    case 4: expand_block<4>(P, o, k); return true;
    case 5: expand_block<5>(P, o, k); return true;
    case 6: expand_block<6>(P, o, k); return true;
    case 7: expand_block<7>(P, o, k); return true;
    case 8: expand_block<8>(P, o, k); return true;
    case 9: expand_block<9>(P, o, k); return true;
    case 10: expand_block<10>(P, o, k); return true;
    case 11: expand_block<11>(P, o, k); return true;
    case 12: expand_block<12>(P, o, k); return true;
    case 13: expand_block<13>(P, o, k); return true;
    case 14: expand_block<14>(P, o, k); return true;
    default: return false;
  }
}

}  // namespace dse
