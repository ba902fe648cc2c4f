// dse_wheel_kernel.h -- template <bool BK> wheel_segments_kernel, the mod-30
// wheel segment kernel, with its mark helpers and its A, B1, B2 and L units.
// Geometry, image layout and arguments: dse_wheel_geometry.h. Three units
// instantiate it: dse_wheel.hip <true> (bucketed passes), dse_wheel_plain.hip
// <false> and dse_wheel_half.hip <false> with 2^16 periods per segment.
//
// One workgroup of 1024 threads per CU, segments blockIdx.x + t*gridDim.x.
// Per segment:
//   1. mark (ds_or_b32), units taken from one LDS counter:
//      A  (79 < p <= TA): one prime per wave; lane (plane i, c = 0..7) takes
//         the hits n of its plane with n mod 256 in [32c, 32c+32), by class
//         n mod 256: a class's hits sit 256p periods apart, same bit, so each
//         further mark is one v_add; the 4 lanes of a plane in a half-wave
//         are 32p periods apart, i.e. in blocks c*p mod 4: distinct banks;
//      B1 (TA < p <= TB1): one prime per half-wave; lane (plane i, j = 0..3)
//         takes the hits n with n mod 128 in [32j, 32j+32), by class n mod
//         128 to the segment end (one v_add per further mark, the marks past
//         the segment dropped), again 32p periods apart: conflict-free;
//      B2 (TB1 < p <= TB): one prime per quarter-wave; lane (plane i, j =
//         0..1) takes the hits n with n mod 64 in [32j, 32j+32), by class to
//         the segment end as B1; a 32-lane group holds two primes, so a bank
//         has at most two lanes;
//      L  (p > TB): one prime per lane, its 8 planes in a lane-rotated order,
//         starts from the table's wheel offsets with one reduction;
//   2. expand: lane reads one block (two ds_read_b128) and turns its 8 plane
//      words (composite bits) into the block's 15 output words (prime bits at
//      the 15 odd slots of each period) in registers: a 16 x 16 bit transpose
//      with the planes as rows at their slots, then a rotate and masked ORs
//      per register (dse_expand_bits.h; one static body per V0 mod 30, chosen
//      once per segment); fixes the small primes 3..79, masks the range end,
//      popcounts, stores; then each wave inits (patterns of 7..79) the blocks
//      it expanded, for the next segment.
// See DESIGN.md section 4 for the rooflines.
#pragma once
#include <type_traits>

#include "dse_expand_bits.h"
#include "dse_wheel_geometry.h"

namespace dse {
namespace {

// 32-bit LDS byte address of a __shared__ pointer.
__device__ __forceinline__ uint32_t lds_addr(const uint32_t* p) {
  return (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) uint32_t*)p;
}

// Every mark is issued as asm: the compiler's waitcnt pass does not see it,
// so callers drain lgkmcnt before a barrier (lds_drain); and it does not
// unroll loops around it, so runs are unrolled by hand.
__device__ __forceinline__ void lds_drain() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }

// Keeps a value opaque to the optimiser (loop strength reduction splits a
// marking offset into several induction variables; lane-derived constants get
// hoisted out of the segment loop and spilled).
__device__ __forceinline__ uint32_t opaque(uint32_t x) {
  asm volatile("" : "+v"(x));
  return x;
}

constexpr uint32_t kBlockMask = ~31u;  // period index -> its block's byte address
#ifndef DSE_FAKE_CF_L
#define DSE_FAKE_CF_L 0
#endif
// profiling knockout (DSE_FAKE_CF_L): the L marks' blocks forced to lane-distinct banks (wrong marks)
constexpr uint32_t kBlockMaskL = DSE_FAKE_CF_L ? ~127u : kBlockMask;
#ifndef DSE_FAKE_CF_INIT
#define DSE_FAKE_CF_INIT 0
#endif
#ifndef DSE_SHORT_TAIL
#define DSE_SHORT_TAIL 16
#endif
// MODE-0 L sets whose tail after the n_min run is at most this many steps mark
// it unconditionally (past the segment: dropped) instead of in mark_tail's loop
constexpr uint32_t kShortTail = DSE_SHORT_TAIL;
// Odd primes <= TB: the table index where the L list (and its sets of 64
// primes) starts whenever the table reaches past TB.
constexpr uint32_t odd_primes_upto(uint32_t x) {
  uint32_t c = 0;
  for (uint32_t v = 3; v <= x; v += 2) {
    bool pr = true;
    for (uint32_t d = 3; d * d <= v; d += 2)
      if (v % d == 0) { pr = false; break; }
    c += pr;
  }
  return c;
}
constexpr uint32_t kL0 = odd_primes_upto(TB);
// The marking plan of a set of 64 large primes pmin..pmax (unit_L), fixed by
// the primes and the segment geometry, so the table carries it (pl[] words
// p | plan << 20, wheel_offsets_kernel) instead of each set deriving it per
// segment with two divisions (~40 instructions): bits 0-1 MODE (2: pmin > KP,
// one mark per plane; 1: pmin > KP/2, two; 0: runs), bit 2 a tail loop
// follows the run, bits 3.. the run length: ceil(KP / pmin) (every lane's hit
// count is at most that; the marks past the segment are dropped), or
// floor(KP / pmax) (every lane's minimum) when the two differ by more than
// kShortTail. A set's plan comes from the pmin and pmax of all its 64 table
// primes, but the kernel's L list may end inside the set (i_big), so the plan
// must also be valid for every smaller pmax: see wheel_offsets_kernel
// (dse_wheel.hip).
// pl[] word -> p. Bit 31 is not a plan bit: it marks a lane past the table
// end (load_L), so a plan has at most 11 bits (asserted below).
constexpr uint32_t kLPrimeMask = 0x800FFFFFu;
// The unit queue's first claimed position in the instantiations without bucket
// units: positions below it are pre-assigned, two to each of the workgroup's
// NT / 64 waves (mark_segment). The bucket instantiation claims every position
// (0): with its first positions pre-assigned the 1e18 window ran 0.6% slower
// (profiles/r20/window_parts.txt).
template <bool BK>
constexpr uint32_t kFirstClaim = BK ? 0u : 2 * (NT / 64);
static_assert(kWheelMaxPrime <= (1u << 20), "pl[] words: the L primes (odd, <= kWheelMaxPrime) are below 2^20");
__host__ __device__ constexpr uint32_t l_plan(uint32_t pmin, uint32_t pmax, uint32_t kp) {
  if (pmin > kp) return 2;
  if (pmin > kp / 2) return 1;
  const uint32_t n_min = pmax >= kp ? 0u : kp / pmax;
  const uint32_t n_all = (kp + pmin - 1) / pmin;
  return n_all - n_min <= kShortTail ? n_all << 3 : 4u | n_min << 3;
}
// the longest run is that of the smallest L primes; both geometries' plans go into every table
static_assert(l_plan(TB + 2, TB + 2, 1u << 17) < (1u << 11) && l_plan(TB + 2, TB + 2, 1u << 16) < (1u << 11),
              "the plan fits bits 20..30 of a pl[] word (bit 31: kLPrimeMask's dead-lane flag)");
static_assert(odd_primes_upto(kQMax) + kMidCap >= kL0, "the L list starts at kL0 whenever it exists");

// Mark period k (< KP) of the plane whose byte base is pb4 (image + 4 plane):
// address (k & ~31) | pb4 in one v_and_or, bit 1 << (k & 31) (the shift reads
// the low 5 bits itself). 2 VALU.
__device__ __forceinline__ void mark_k(uint32_t pb4, uint32_t k, uint32_t one) {
  uint32_t a, b;
  asm volatile(
      "v_and_or_b32 %0, %2, %3, %4\n\t"
      "v_lshlrev_b32 %1, %2, %5\n\t"
      "ds_or_b32 %0, %1 offset:" DSE_IMG_OFF_S
      : "=&v"(a), "=&v"(b)
      : "v"(k), "s"(kBlockMask), "v"(pb4), "v"(one)
      : "memory");
}

// mark_k and advance k by p, in one asm block (written as mark_k + an add,
// the loop-carried index costs a v_mov per mark). 3 VALU.
__device__ __forceinline__ void mark_k_step(uint32_t pb4, uint32_t& k, uint32_t p, uint32_t one) {
  uint32_t a, b;
  asm volatile(
      "v_and_or_b32 %0, %2, %3, %4\n\t"
      "v_lshlrev_b32 %1, %2, %6\n\t"
      "ds_or_b32 %0, %1 offset:" DSE_IMG_OFF_S "\n\t"
      "v_add_u32 %2, %2, %5"
      : "=&v"(a), "=&v"(b), "+v"(k)
      : "s"(kBlockMask), "v"(pb4), "v"(p), "v"(one)
      : "memory");
}

// Four mark_k_steps in one asm block. Between two asm blocks the compiler
// puts a wait state (s_nop 0, or a filler) whenever the second reads a VGPR
// the first wrote -- it cannot see that no instruction in them needs one --
// so back-to-back mark_k_steps cost an s_nop per mark.
__device__ __forceinline__ void mark_k_step4(uint32_t pb4, uint32_t& k, uint32_t p, uint32_t one) {
  uint32_t a0, b0, a1, b1;
  asm volatile(
      "v_and_or_b32 %0, %4, %5, %6\n\t"
      "v_lshlrev_b32 %1, %4, %8\n\t"
      "v_add_u32 %4, %4, %7\n\t"
      "ds_or_b32 %0, %1 offset:" DSE_IMG_OFF_S "\n\t"
      "v_and_or_b32 %2, %4, %5, %6\n\t"
      "v_lshlrev_b32 %3, %4, %8\n\t"
      "v_add_u32 %4, %4, %7\n\t"
      "ds_or_b32 %2, %3 offset:" DSE_IMG_OFF_S "\n\t"
      "v_and_or_b32 %0, %4, %5, %6\n\t"
      "v_lshlrev_b32 %1, %4, %8\n\t"
      "v_add_u32 %4, %4, %7\n\t"
      "ds_or_b32 %0, %1 offset:" DSE_IMG_OFF_S "\n\t"
      "v_and_or_b32 %2, %4, %5, %6\n\t"
      "v_lshlrev_b32 %3, %4, %8\n\t"
      "v_add_u32 %4, %4, %7\n\t"
      "ds_or_b32 %2, %3 offset:" DSE_IMG_OFF_S
      : "=&v"(a0), "=&v"(b0), "=&v"(a1), "=&v"(b1), "+v"(k)
      : "s"(kBlockMask), "v"(pb4), "v"(p), "v"(one)
      : "memory");
}


// n unconditional marks k, k + p, ... (by 4: three SALU of loop control per
// mark otherwise); returns the index after the run.
__device__ __forceinline__ uint32_t mark_run(uint32_t pb4, uint32_t k, uint32_t p, uint32_t n, uint32_t one) {
  uint32_t h = 0;
  for (; h + 4 <= n; h += 4) mark_k_step4(pb4, k, p, one);
  for (; h < n; ++h) mark_k_step(pb4, k, p, one);
  return k;
}

// The rest of a lane's walk: k, k + p, ... while k < KP, as one asm loop
// that narrows exec as lanes finish (v_cmpx) and restores it once: 4 VALU
// and one branch per step (the compiler's loop keeps a mask of finished
// lanes: 2 more SALU per step; 1e11 -0.3%). All exec writes are inside the
// block. The branches only decide whether to run another step: exec only
// narrows, every mark is predicated by the exec the v_cmpx left, and a step
// run with an empty exec changes nothing, so even a branch that read exec
// from before the v_cmpx could not mark anything wrong, only run one empty
// step (and k grows by p every step, so the loop ends).
__device__ __forceinline__ void mark_tail(uint32_t pb4, uint32_t k, uint32_t p, uint32_t one) {
  uint64_t sv;
  uint32_t a, b;
  asm volatile(
      "s_mov_b64 %3, exec\n\t"
      "v_cmpx_gt_u32_e32 vcc, %5, %2\n\t"
      "s_cbranch_execz 2f\n"
      "1:\n\t"
      "v_and_or_b32 %0, %2, %6, %7\n\t"
      "v_lshlrev_b32 %1, %2, %8\n\t"
      "v_add_u32 %2, %2, %4\n\t"
      "ds_or_b32 %0, %1 offset:" DSE_IMG_OFF_S "\n\t"
      "v_cmpx_gt_u32_e32 vcc, %5, %2\n\t"
      "s_cbranch_execnz 1b\n"
      "2:\n\t"
      "s_mov_b64 exec, %3"
      : "=&v"(a), "=&v"(b), "+v"(k), "=&s"(sv)
      : "v"(p), "s"(KP), "s"(kBlockMask), "v"(pb4), "v"(one)
      : "memory", "vcc");
}

// ds_or_b32 at a precomputed LDS byte address.
__device__ __forceinline__ void mark_at(uint32_t a, uint32_t bit) {
  asm volatile("ds_or_b32 %0, %1 offset:" DSE_IMG_OFF_S : : "v"(a), "v"(bit) : "memory");
}

// The hits k + (r + 32 t) p, r = 0..31, t < K, of a lane that walks one
// plane from k with step p: class r's hits sit D = 32 S p periods apart (S =
// 4 for B1's lanes, which take 32 of every 128 hits, 2 for B2's, 32 of every
// 64), so they share their bit and their byte addresses step by D (a period
// index is its block's byte address): 3 VALU of setup per class, then one
// v_add per mark (mark_k_step: 3 VALU per mark).
// Four classes per asm block and loop iteration (.rept: the K - 1 further
// marks of a class, and two pairs of classes): one class per iteration pays
// three SALU of loop control per class, a third of the instructions of a class
// of two marks. The scratch pairs alternate between classes, as in
// mark_k_step4.
#define DSE_CLASS(A, B)                                  \
  "v_and_or_b32 " A ", %4, %5, %6\n\t"                   \
  "v_lshlrev_b32 " B ", %4, %7\n\t"                      \
  "v_add_u32 %4, %4, %8\n\t"                             \
  "ds_or_b32 " A ", " B " offset:" DSE_IMG_OFF_S "\n\t"  \
  ".rept %c10\n\t"                                       \
  "v_add_u32 " A ", " A ", %9\n\t"                       \
  "ds_or_b32 " A ", " B " offset:" DSE_IMG_OFF_S "\n\t"  \
  ".endr\n\t"
template <int K>
__device__ __forceinline__ void class_marks(uint32_t pb4, uint32_t k, uint32_t p, uint32_t D, uint32_t one) {
#pragma unroll 1
  for (uint32_t r = 0; r < 32; r += 4) {
    uint32_t a0, b0, a1, b1;
    asm volatile(".rept 2\n\t" DSE_CLASS("%0", "%1") DSE_CLASS("%2", "%3") ".endr"
                 : "=&v"(a0), "=&v"(b0), "=&v"(a1), "=&v"(b1), "+v"(k)
                 : "s"(kBlockMask), "v"(pb4), "v"(one), "v"(p), "v"(D), "n"(K - 1)
                 : "memory");
  }
}
// K wave-uniform in 1..kClassMarksMax (B1: floor(floor((KP - 1) / pmin) /
// 128) + 1, B2: the same with 64; the last mark of a class is dropped where
// its hit lies past the segment)
__device__ __forceinline__ void class_marks_k(uint32_t K, uint32_t pb4, uint32_t k, uint32_t p, uint32_t D,
                                              uint32_t one) {
  switch (K) {
    case 0: return;
    case 1: class_marks<1>(pb4, k, p, D, one); return;
    case 2: class_marks<2>(pb4, k, p, D, one); return;
    case 3: class_marks<3>(pb4, k, p, D, one); return;
    case 4: class_marks<4>(pb4, k, p, D, one); return;
    case 5: class_marks<5>(pb4, k, p, D, one); return;
    case 6: class_marks<6>(pb4, k, p, D, one); return;
    case 7: class_marks<7>(pb4, k, p, D, one); return;
    case 8: class_marks<8>(pb4, k, p, D, one); return;
    case 9: class_marks<9>(pb4, k, p, D, one); return;
    case 10: class_marks<10>(pb4, k, p, D, one); return;
    case 11: class_marks<11>(pb4, k, p, D, one); return;
    default: __builtin_unreachable();
  }
}

// x mod p for x < 2^63 with m = floor((2^64-1)/p).
__host__ __device__ __forceinline__ uint32_t mod_barrett(uint64_t x, uint32_t p, uint64_t m) {
#if defined(__HIP_DEVICE_COMPILE__)
  uint64_t q = __umul64hi(x, m);
#else
  uint64_t q = (uint64_t)(((unsigned __int128)x * m) >> 64);
#endif
  uint64_t r = x - q * p;
  if (r >= p) r -= p;
  if (r >= p) r -= p;
  return (uint32_t)r;
}

// floor((2^64-1)/p) for 2 <= p < 2^32 without a 64-bit division: a double
// quotient (relative error 2^-52, so off by < 2^11) corrected by the exact
// remainder, itself below 2^43 in magnitude and so exact in a double.
__device__ __forceinline__ uint64_t barrett_factor(uint32_t p) {
  const double dp = (double)p;
  uint64_t m = (uint64_t)(18446744073709551615.0 / dp);        // rounds 2^64-1 up to 2^64: may overshoot
  if (m > ~0ull / 2) m = ~0ull / 2;                              // p >= 2: the true m < 2^63
  int64_t r = (int64_t)(~0ull - m * (uint64_t)p);                // true remainder + (true m - m) * p
  m += (int64_t)__builtin_floor((double)r / dp);
  r = (int64_t)(~0ull - m * (uint64_t)p);
  while (r < 0) { --m; r += p; }
  while (r >= (int64_t)p) { ++m; r -= p; }
  return m;
}

__device__ __forceinline__ float fast_rcp(float x) { return __builtin_amdgcn_rcpf(x); }

// ceil(t / p), t < 2^24
__device__ __forceinline__ uint32_t div_ceil_small(uint32_t t, uint32_t p, float invp) {
  uint32_t q = (uint32_t)((float)t * invp);
  q = q * p > t ? q - 1 : q;
  q = (q + 1) * p <= t ? q + 1 : q;  // q = floor(t/p)
  return q + (q * p != t ? 1u : 0u);
}

// floor(t / p), t < 2^24
__device__ __forceinline__ uint32_t div_small(uint32_t t, uint32_t p, float invp) {
  uint32_t q = (uint32_t)((float)t * invp);
  q = q * p > t ? q - 1 : q;
  q = (q + 1) * p <= t ? q + 1 : q;
  return q;
}

// x*y mod p for x, y < p <= 2^14
__device__ __forceinline__ uint32_t mulmod_small(uint32_t x, uint32_t y, uint32_t p, float invp) {
  const uint32_t xy = x * y;
  uint32_t q = (uint32_t)((float)xy * invp);
  int32_t r = (int32_t)(xy - q * p);
  r = r < 0 ? r + (int32_t)p : r;
  r = r < 0 ? r + (int32_t)p : r;
  r = r >= (int32_t)p ? r - (int32_t)p : r;
  r = r >= (int32_t)p ? r - (int32_t)p : r;
  return (uint32_t)r;
}

// 30^{-1} mod p for p coprime to 30: (p*a + 1)/30 with p*a = -1 (mod 30);
// a = 2*nibble + 1, nibble indexed by (p mod 30)/2.
__host__ __device__ __forceinline__ uint64_t inv30_of(uint64_t p) {
  constexpr uint64_t T = (14ull << 0) | (8ull << 12) | (9ull << 20) | (11ull << 24) | (3ull << 32) | (5ull << 36) |
                         (6ull << 44) | (0ull << 56);
  const uint32_t r = (uint32_t)(p % 30u);
  const uint64_t a = 2 * ((T >> (4 * (r >> 1))) & 15) + 1;
  return (p * a + 1) / 30;
}

// First k >= 0 with p | Vs + rho + 30k, given Xs = Vs mod p (p in (61, 2^14]).
__device__ __forceinline__ uint32_t plane_first(uint32_t Xs, uint32_t rho, uint32_t p, uint32_t inv30,
                                                float invp) {
  uint32_t t = Xs + rho;
  t = t >= p ? t - p : t;
  const uint32_t u = t ? p - t : 0u;
  return mulmod_small(u, inv30, p, invp);
}

// First k >= start with k = kp (mod p); kp < p, start < 2^23.
__device__ __forceinline__ uint32_t first_at_or_after(uint32_t kp, uint32_t start, uint32_t p, float invp) {
  if (start <= kp) return kp;
  return kp + p * div_ceil_small(start - kp, p, invp);
}

// Smallest plane index k whose value Vs + rho + 30k is >= p^2, given D = p^2 - Vs > 0.
__device__ __forceinline__ uint32_t kmin_for(uint32_t D, uint32_t rho) {
  return D > rho ? (D - rho + 29u) / 30u : 0u;
}

// ---- work units of the mark phase ----------------------------------------

// A, by hit class: lane (plane, c) owns the hits n of its plane with n mod
// 256 = 32c + r, r = 0..31; class r's hits k0 + 256p t share their bit and
// their byte addresses step by the wave-uniform 256p, so after 3 VALU of class
// setup each further mark is one v_add. k0 = kp + (32c + r) p < 256p, so
// every class has K = floor(KP / 256p) or K + 1 hits: K + 1 marks, the last
// dropped past the image (address >= IMG_BYTES, see kImgOff). k = the class-0
// hit of the lane.
template <int K>
__device__ __forceinline__ void a_classes(uint32_t pb4, uint32_t k, uint32_t p, uint32_t one) {
  const uint32_t D = p << 8;  // 256 p periods = bytes
#pragma unroll 1
  for (uint32_t r = 0; r < 32; ++r) {
    uint32_t a, bit;
    asm volatile(
        "v_and_or_b32 %0, %2, %3, %4\n\t"
        "v_lshlrev_b32 %1, %2, %5"
        : "=&v"(a), "=&v"(bit)
        : "v"(k), "s"(kBlockMask), "v"(pb4), "v"(one));
#pragma unroll
    for (int t = 0; t < K; ++t) {
      mark_at(a, bit);
      a += D;
    }
    mark_at(a, bit);  // past the image (a >= IMG_BYTES): dropped
    k = opaque(k + p);
  }
}

// Vs mod p of the staged mid primes, carried from segment to segment: a
// workgroup's next segment starts G W integers later (G workgroups), so the
// unit that uses x[i] for this segment leaves (x[i] + inc[i]) mod p there,
// inc[i] = G W mod p. `have`: x holds this segment's residues (the
// workgroup's previous segment was of the same range and every mid unit ran
// in it); otherwise a 64-bit Barrett reduction (the workgroup's first
// segment, a range change, segments below TB^2).
struct MidRes {
  uint32_t* x;
  const uint32_t* inc;
  bool have;
};
__device__ __forceinline__ uint32_t mid_residue(const MidRes& mr, uint32_t i, uint32_t p, uint64_t m, uint64_t Vs,
                                                bool writer) {
  const uint32_t xs = mr.have ? mr.x[i] : mod_barrett(Vs, p, m);
  if (writer) {
    const uint32_t t = xs + mr.inc[i];
    mr.x[i] = min(t, t - p);
  }
  return xs;
}

// A: one mid prime (kQMax < p <= TA) per wave; lane (plane L & 7, c = L >> 3).
// Lanes 0-31 have c = 0..3: a plane's four lanes mark 32p periods apart at
// every step (same class r, same t), i.e. in blocks c p (mod 4) apart -- four
// distinct banks for odd p.
__device__ __forceinline__ void unit_A(uint32_t img0, uint32_t pi, uint64_t m, const MidRes& mr, uint32_t idx,
                                       uint64_t Vs, uint64_t rho_pack, uint32_t lane, uint32_t one) {
  const uint32_t p = pi & 0xFFFFu, inv30 = pi >> 16;  // wave-uniform
  const uint64_t p2 = (uint64_t)p * p;
  const uint32_t Xs = __builtin_amdgcn_readfirstlane(mid_residue(mr, idx, p, m, Vs, lane == 0));
  const float invp = fast_rcp((float)p);
  const uint32_t pl = lane & 7, c = lane >> 3;
  const uint32_t rho = (uint32_t)(rho_pack >> (5 * pl)) & 31u;
  const uint32_t kp = plane_first(Xs, rho, p, inv30, invp);
  const uint32_t pb4 = img0 + 4 * pl;
  const uint32_t k = kp + 32 * c * p;                   // class 0 of the lane: hit n = 32c
  if (p2 <= Vs) {
    switch (KP / (256 * p)) {  // K (wave-uniform): 2..6 for kQMax < p <= TA (1..3 for the half geometry)
      case 1: a_classes<1>(pb4, k, p, one); return;
      case 2: a_classes<2>(pb4, k, p, one); return;
      case 3: a_classes<3>(pb4, k, p, one); return;
      case 4: a_classes<4>(pb4, k, p, one); return;
      case 5: a_classes<5>(pb4, k, p, one); return;
      case 6: a_classes<6>(pb4, k, p, one); return;
      case 7: a_classes<7>(pb4, k, p, one); return;
      default: __builtin_unreachable();
    }
  }
  // p^2 inside the segment (its first segments only): the lane's hits with
  // k >= kmin, one at a time
  const uint32_t kmin = kmin_for((uint32_t)(p2 - Vs), rho);
  for (uint32_t r = 0; r < 32; ++r)
    for (uint32_t kk = k + r * p; kk < KP; kk += 256 * p)
      if (kk >= kmin) mark_k(pb4, kk, one);
}

// B1: two mid primes (TA < p <= TB1), one per half-wave; lane (plane L & 7,
// j = (L >> 3) & 3) owns the hits n with n mod 128 = 32j + r, r = 0..31. The
// four lanes of a plane are 32p periods apart: distinct banks, as in A. Every
// class r is marked to the segment end (class_marks), one mark more than the
// hits every lane has, dropped where it lies past the segment, as in A: no
// in-order walk of a last, partly filled block of 128 hits.
__device__ __forceinline__ void unit_B1(uint32_t img0, const uint32_t* __restrict__ s_mid_p,
                                        const uint64_t* __restrict__ s_mid_m, const MidRes& mr, uint32_t j0,
                                        uint32_t nj, uint64_t Vs, uint64_t rho_pack, uint32_t lane, uint32_t one) {
  const uint32_t h = lane >> 5, pl = lane & 7, j = (lane >> 3) & 3;
  if (h >= nj) return;  // the unit's second half-wave when the list ends
  const uint32_t pi = s_mid_p[j0 + h];
  const uint32_t p = pi & 0xFFFFu, inv30 = pi >> 16;
  const uint64_t m = s_mid_m[j0 + h];
  const float invp = fast_rcp((float)p);
  const uint32_t rho = (uint32_t)(rho_pack >> (5 * pl)) & 31u;
  const uint32_t kp = plane_first(mid_residue(mr, j0 + h, p, m, Vs, (lane & 31) == 0), rho, p, inv30, invp);
  const uint32_t pb4 = img0 + 4 * pl;
  uint32_t k = kp + 32 * j * p;                          // hit n = 32j
  const uint64_t p2 = (uint64_t)p * p;
  if (p2 > Vs) {  // p^2 inside the segment: one at a time from kmin
    const uint32_t kmin = kmin_for((uint32_t)min(p2 - Vs, (uint64_t)0xFFFFFFFFu), rho);
    for (; k < KP; k += 96 * p)
      for (uint32_t r = 0; r < 32 && k < KP; ++r, k += p)
        if (k >= kmin) mark_k(pb4, k, one);
    return;
  }
  // class by class (hits 32j + r + 128t: 128p periods apart, one bit): 1
  // VALU per mark where walking them takes 3. A hit of either prime has k =
  // kp + n p <= KP - 1, so n <= floor((KP - 1) / pmin) < 128 T: T marks per
  // class reach every hit, and the marks whose hit does not exist have k >=
  // KP (below 128 T pmax < 2 KP + 128 pmax) and are dropped (kImgOff). The
  // unit's first live lane holds pmin (the list ascends).
  const uint32_t pmin = __builtin_amdgcn_readfirstlane(p);
  const uint32_t T = __builtin_amdgcn_readfirstlane(div_small(KP - 1, pmin, fast_rcp((float)pmin))) / 128 + 1;
  class_marks_k(T, pb4, k, p, 128 * p, one);
}

// B2: four mid primes (TB1 < p <= TB), one per quarter-wave; lane (prime
// L >> 4, plane L & 7, j = (L >> 3) & 1) owns the hits n with n mod 64 = 32j
// + r, r = 0..31, and marks every class r to the segment end as B1 does: T2 =
// floor(floor((KP - 1) / pmin) / 64) + 1 marks 64p periods apart, the ones
// past the segment dropped. The two lanes of a prime and plane are 32p
// periods apart, p blocks: different blocks mod 4 for odd p. A 32-lane group
// holds two primes, so a bank has at most two lanes (dse_wheel_geometry.h):
// 1.6 conflict cycles per ds_or where four unrelated primes per plane and
// half-wave had 3.2.
__device__ __forceinline__ void unit_B2(uint32_t img0, const uint32_t* __restrict__ s_mid_p,
                                        const uint64_t* __restrict__ s_mid_m, const MidRes& mr, uint32_t j0,
                                        uint32_t nj, uint64_t Vs, uint64_t rho_pack, uint32_t lane, uint32_t one) {
  const uint32_t h = lane >> 4, pl = lane & 7, j = (lane >> 3) & 1;
  if (h >= nj) return;  // the quarter-waves past the list end mark nothing
  const uint32_t pi = s_mid_p[j0 + h];
  const uint32_t p = pi & 0xFFFFu, inv30 = pi >> 16;
  const uint64_t m = s_mid_m[j0 + h];
  const float invp = fast_rcp((float)p);
  const uint32_t rho = (uint32_t)(rho_pack >> (5 * pl)) & 31u;
  const uint32_t kp = plane_first(mid_residue(mr, j0 + h, p, m, Vs, (lane & 15) == 0), rho, p, inv30, invp);
  const uint32_t pb4 = img0 + 4 * pl;
  uint32_t k = kp + 32 * j * p;                          // hit n = 32j
  // the list ascends: pmax decides for the wave whether some p^2 lies inside
  // the segment
  const uint32_t pmax = __builtin_amdgcn_readfirstlane(s_mid_p[j0 + nj - 1]) & 0xFFFFu;
  if ((uint64_t)pmax * pmax > Vs) {  // one at a time from kmin (0 for the primes with p^2 <= Vs)
    const uint64_t p2 = (uint64_t)p * p;
    const uint32_t kmin = p2 > Vs ? kmin_for((uint32_t)min(p2 - Vs, (uint64_t)0xFFFFFFFFu), rho) : 0u;
    for (; k < KP; k += 32 * p)
      for (uint32_t r = 0; r < 32 && k < KP; ++r, k += p)
        if (k >= kmin) mark_k(pb4, k, one);
    return;
  }
  // a hit has k = kp + n p <= KP - 1, so n <= floor((KP - 1) / pmin) < 64 T2;
  // lane 0 holds pmin
  const uint32_t pmin = __builtin_amdgcn_readfirstlane(p);
  const uint32_t T2 = __builtin_amdgcn_readfirstlane(div_small(KP - 1, pmin, fast_rcp((float)pmin))) / 64 + 1;
  class_marks_k(T2, pb4, k, p, 64 * p, one);
}

// Operands of one large unit, loaded ahead of use. The table row of prime i
// holds its 8 wheel offsets rotated by i mod 8, so lane L (i = 64u + L) reads
// a[(q + L) & 7] at position q with two aligned 16-byte loads.
struct LargeOps {
  uint32_t p;
  uint64_t m;
  uint32_t a[8];
};

__device__ __forceinline__ void load_L(LargeOps& o, const uint32_t* __restrict__ P, const uint64_t* __restrict__ M,
                                       const uint32_t* __restrict__ A, uint32_t il, uint32_t np, bool need_m) {
  const uint32_t ic = min(il, np - 1);  // past the table end: load the last row, mark nothing
  // p | plan << 20 (table pl[]); past the table end bit 31 marks the lane dead
  // (a load under exec into the preset register: a select after an
  // unconditional load would wait for the load right here)
  o.p = il < np ? *reinterpret_cast<const uint32_t*>(reinterpret_cast<const char*>(P) + (ic << 2)) : 0xFFFFFFFFu;
  o.m = need_m ? M[ic] : 0ull;  // the Barrett factor: only for Kb >= 2^38 (unit_L); 1e12: -1.9%
  // 32-bit byte offset from the table's base (one VALU, no 64-bit address math)
  const uint4* row = reinterpret_cast<const uint4*>(reinterpret_cast<const char*>(A) + (ic << 5));
  const uint4 lo = row[0], hi = row[1];
  o.a[0] = lo.x; o.a[1] = lo.y; o.a[2] = lo.z; o.a[3] = lo.w;
  o.a[4] = hi.x; o.a[5] = hi.y; o.a[6] = hi.z; o.a[7] = hi.w;
}

// Operand registers whose contents are dead: left undefined (an empty asm
// that "writes" them), so the compiler keeps no copy of what they held.
__device__ __forceinline__ void undef_ops(LargeOps& o) {
  asm volatile("" : "=v"(o.p), "=v"(o.m), "=v"(o.a[0]), "=v"(o.a[1]), "=v"(o.a[2]), "=v"(o.a[3]), "=v"(o.a[4]),
               "=v"(o.a[5]), "=v"(o.a[6]), "=v"(o.a[7]));
}

// Mark a bucketed hit: entry = LDS word index << 5 | bit (bucket_entry), so
// the address is img0 + (e >> 5) * 4 and the bit 1 << (e & 31) (the shift
// reads the low 5 bits itself): 3 VALU.
__device__ __forceinline__ void mark_entry(uint32_t img0, uint32_t e, uint32_t one) {
  uint32_t a, b;
  asm volatile(
      "v_lshrrev_b32 %0, 3, %2\n\t"
      "v_and_or_b32 %0, %0, -4, %4\n\t"
      "v_lshlrev_b32 %1, %2, %3\n\t"
      "ds_or_b32 %0, %1 offset:" DSE_IMG_OFF_S
      : "=&v"(a), "=&v"(b)
      : "v"(e), "v"(one), "v"(img0)
      : "memory");
}

// Kb mod p by float quotients (unit_L): p > TB bounds the quotients.
constexpr uint64_t kQuotBits = 22;                                 // Kb < 2^32: q < 2^32 / (TB + 1) < 2^22
constexpr uint64_t kQuotErr38 = (1ull << (38 - 22)) / (TB + 1) + 1;  // Kb < 2^38: |q error| < 2^16 / (TB + 1) + 1
static_assert((1ull << 32) / (TB + 1) < (1ull << kQuotBits), "Kb < 2^32: float quotient within 1 (and < 2^24 for __umul24)");
static_assert((kQuotErr38 + 2) * kWheelMaxPrime < (1ull << 31), "Kb < 2^38: the rest Kb - q p must be exact in int32");
static_assert(kWheelMaxPrime < (1ull << 23), "__mul24 / __umul24 operands and float-exact p");
static_assert((uint64_t)(kWheelMaxPrime + 1) * (kWheelMaxPrime + 1) / 30 < (1ull << 38),
              "ranges without bucketed primes never need the Barrett path (unit_L<false>)");

// kb mod p for kb < 2^32 (values below 1.29e11), TB < p <= kWheelMaxPrime,
// invp = fast_rcp((float)p). A float quotient is within one of the true one:
// its relative error is below 2^-22 (kb rounded to float 2^-24, the rcp
// 2^-23, the product 2^-24) and q < 2^32 / p < 2^22 for p > TB (kQuotBits), so
// |error| < 1, and the truncation adds at most one more: kb - q p is in
// [-p, 2p), corrected by two unsigned min steps.
__device__ __forceinline__ uint32_t kb_mod_p_f32(uint32_t kb, uint32_t p, float invp) {
  const uint32_t q = (uint32_t)((float)kb * invp);
  // q p by v_mul_u32_u24 as asm: written as __umul24 the compiler merged it
  // with the other path's product into one quarter-rate v_mul_lo_u32
  uint32_t qp;
  asm("v_mul_u32_u24 %0, %1, %2" : "=v"(qp) : "v"(q), "v"(p));
  uint32_t x = kb - qp;  // in [-p, 2p) as a signed value; p < 2^24
  x = min(x, x + p);
  return min(x, x - p);
}

// Kb mod p for Kb < 2^38 (values below 8.2e12), p and invp as above: the float
// quotient of Kb is within kQuotErr38 of the true one (relative error <
// 2^-22, Kb / p < 2^38 / (TB + 1)), so Kb - q p is exact in 32 bits (|.| <
// (kQuotErr38 + 1) p < 2^31, asserted above); one more float quotient of that
// rest leaves it in [-p, 2p). 12 VALU where the 64-bit Barrett reduction
// takes ~24.
__device__ __forceinline__ uint32_t kb_mod_p_f38(uint64_t Kb, uint32_t p, float invp) {
  const uint32_t q = (uint32_t)((float)Kb * invp);
  const int32_t r = (int32_t)((uint32_t)Kb - q * p);
  const int32_t q2 = (int32_t)((float)r * invp);
  uint32_t x = (uint32_t)(r - __mul24(q2, (int32_t)p));
  x = min(x, x + p);
  return min(x, x - p);
}

// Kb mod p as unit_L takes it (Kb is wave-uniform there): one float quotient
// while Kb < 2^32, two below 2^38, and above that, which only a launch with
// bucketed primes meets (BARRETT), the 64-bit Barrett reduction with m =
// floor((2^64-1)/p). Without BARRETT m is not read and Kb must be below 2^38.
// dse_arith_probe.hip runs these three functions against exact integers
// (tests/test_gpu_wheel_arith.py).
template <bool BARRETT>
__device__ __forceinline__ uint32_t kb_mod_p(uint64_t Kb, uint32_t p, float invp, uint64_t m) {
  if (Kb < (1ull << 32)) return kb_mod_p_f32((uint32_t)Kb, p, invp);
  if (!BARRETT || Kb < (1ull << 38)) return kb_mod_p_f38(Kb, p, invp);
  return mod_barrett(Kb, p, m);
}

// L: 64 large primes (p > TB), one per lane; at step q lane L handles the
// absolute residue (q + L) & 7 (a half-wave spreads over all 8 planes). The
// per-plane hit count is at most ceil(KP / pmin): units whose primes all
// exceed KP (resp. KP/2) take one (two) predicated marks per plane, no loop.
// Per-segment, per-lane constants of the L units: at step q the lane handles
// absolute residue (q + i) & 7, whose plane byte base (pb) and -e (ne) are
// the same for every unit of the segment.
struct PlaneSteps {
  uint32_t pb[8];
  uint32_t ne[8];
  uint32_t one;  // 1 in a VGPR (shl1)
};

// Plane start (a - Kb - e) mod p = min(t, t + p), t = a + (-Kb mod p) + (-e)
// as one v_add3 (left to itself the compiler forms a - (kbm + e): 4 VALU).
__device__ __forceinline__ uint32_t plane_start(uint32_t a, uint32_t nKbm, uint32_t ne, uint32_t p) {
  uint32_t t, u;
  asm("v_add3_u32 %0, %2, %3, %4\n\t"
      "v_add_u32 %1, %0, %5\n\t"
      "v_min_u32 %0, %0, %1"
      : "=&v"(t), "=&v"(u)
      : "v"(a), "v"(nKbm), "v"(ne), "v"(p));
  return t;
}

// Branch-free body of an L unit whose 64 primes are all live and past p^2
// (the common case): the mark count per plane is decided once per unit.
// MODE 2: pmin > KP, one mark per plane; MODE 1: pmin > KP/2, two; MODE 0:
// n_min unconditional marks per plane and a short loop for the rest. Marks
// past the segment's end are dropped by the LDS (kImgOff), so MODE 1/2 and
// short MODE-0 tails need no compare and no exec masking.
// MODE 1/2: four planes per asm block, each a plane start (a - Kb - e) mod p
// and its NM = 1 or 2 marks kk, kk + p: 5 VALU + one ds_or per mark (round
// 5 predicated each mark with v_cmpx and restored exec after each plane: 2
// instructions more per plane and one per block). One block of four planes,
// not one per plane: between two asm blocks the compiler places an s_nop when
// the second reads a VGPR the first wrote.
#define DSE_PLANE_START(A, NE)                                       \
  "v_add3_u32 %0, " A ", %15, " NE "\n\t" /* t = a - Kb mod p - e */ \
  "v_add_u32 %1, %0, %16\n\t"                                        \
  "v_min_u32 %0, %0, %1\n\t" /* kk = (a - Kb - e) mod p */
#define DSE_PLANE_MARK(PB)               \
  "v_and_or_b32 %1, %0, %17, " PB "\n\t" \
  "v_lshlrev_b32 %2, %0, %18\n\t"        \
  "ds_or_b32 %1, %2 offset:" DSE_IMG_OFF_S "\n\t"
#define DSE_PLANE_NEXT "v_add_u32 %0, %0, %16\n\t"
template <int NM>
__device__ __forceinline__ void start_marks4(const uint32_t* a, const uint32_t* ne, const uint32_t* pb, uint32_t nKbm,
                                             uint32_t p, uint32_t one) {
  uint32_t t, u, b;
  if (NM == 1)
    asm volatile(
        DSE_PLANE_START("%3", "%7") DSE_PLANE_MARK("%11")
        DSE_PLANE_START("%4", "%8") DSE_PLANE_MARK("%12")
        DSE_PLANE_START("%5", "%9") DSE_PLANE_MARK("%13")
        DSE_PLANE_START("%6", "%10") DSE_PLANE_MARK("%14")
        : "=&v"(t), "=&v"(u), "=&v"(b)
        : "v"(a[0]), "v"(a[1]), "v"(a[2]), "v"(a[3]), "v"(ne[0]), "v"(ne[1]), "v"(ne[2]), "v"(ne[3]), "v"(pb[0]),
          "v"(pb[1]), "v"(pb[2]), "v"(pb[3]), "v"(nKbm), "v"(p), "s"(kBlockMaskL), "v"(one)
        : "memory");
  else
    asm volatile(
        DSE_PLANE_START("%3", "%7") DSE_PLANE_MARK("%11") DSE_PLANE_NEXT DSE_PLANE_MARK("%11")
        DSE_PLANE_START("%4", "%8") DSE_PLANE_MARK("%12") DSE_PLANE_NEXT DSE_PLANE_MARK("%12")
        DSE_PLANE_START("%5", "%9") DSE_PLANE_MARK("%13") DSE_PLANE_NEXT DSE_PLANE_MARK("%13")
        DSE_PLANE_START("%6", "%10") DSE_PLANE_MARK("%14") DSE_PLANE_NEXT DSE_PLANE_MARK("%14")
        : "=&v"(t), "=&v"(u), "=&v"(b)
        : "v"(a[0]), "v"(a[1]), "v"(a[2]), "v"(a[3]), "v"(ne[0]), "v"(ne[1]), "v"(ne[2]), "v"(ne[3]), "v"(pb[0]),
          "v"(pb[1]), "v"(pb[2]), "v"(pb[3]), "v"(nKbm), "v"(p), "s"(kBlockMaskL), "v"(one)
        : "memory");
}

#ifndef DSE_LOCKSTEP
#define DSE_LOCKSTEP 1
#endif
// One mark in each of the 8 planes, k[q] += p: 32 instructions in one block
// (two scratch pairs alternate, as in mark_k_step4, so a ds_or's operands are
// not rewritten by the next instruction).
#define DSE_MARK8_ONE(A, B, K, PB)                   \
  "v_and_or_b32 " A ", " K ", %21, " PB "\n\t"     \
  "v_lshlrev_b32 " B ", " K ", %22\n\t"             \
  "v_add_u32 " K ", " K ", %20\n\t"                 \
  "ds_or_b32 " A ", " B " offset:" DSE_IMG_OFF_S "\n\t"
__device__ __forceinline__ void mark8(uint32_t (&k)[8], const uint32_t* pb, uint32_t p, uint32_t one) {
  uint32_t a0, b0, a1, b1;
  asm volatile(DSE_MARK8_ONE("%0", "%1", "%4", "%12") DSE_MARK8_ONE("%2", "%3", "%5", "%13")
                   DSE_MARK8_ONE("%0", "%1", "%6", "%14") DSE_MARK8_ONE("%2", "%3", "%7", "%15")
                       DSE_MARK8_ONE("%0", "%1", "%8", "%16") DSE_MARK8_ONE("%2", "%3", "%9", "%17")
                           DSE_MARK8_ONE("%0", "%1", "%10", "%18") DSE_MARK8_ONE("%2", "%3", "%11", "%19")
               : "=&v"(a0), "=&v"(b0), "=&v"(a1), "=&v"(b1), "+v"(k[0]), "+v"(k[1]), "+v"(k[2]), "+v"(k[3]),
                 "+v"(k[4]), "+v"(k[5]), "+v"(k[6]), "+v"(k[7])
               : "v"(pb[0]), "v"(pb[1]), "v"(pb[2]), "v"(pb[3]), "v"(pb[4]), "v"(pb[5]), "v"(pb[6]), "v"(pb[7]),
                 "v"(p), "s"(kBlockMaskL), "v"(one)
               : "memory");
}

// MODE 0: n_run marks per plane (TAIL false: n_min + the tail, the ones past
// the segment dropped), or n_run = n_min marks and a loop for the rest (TAIL
// true: sets whose primes spread over a wide range of hit counts).
template <int MODE, bool TAIL = false>
__device__ __forceinline__ void unit_L_fast(const LargeOps& o, uint32_t p, uint32_t nKbm, const PlaneSteps& ps,
                                            uint32_t n_run) {
  if (MODE != 0) {
    constexpr int NM = MODE == 2 ? 1 : 2;  // marks per plane
    start_marks4<NM>(o.a, ps.ne, ps.pb, nKbm, p, ps.one);
    start_marks4<NM>(o.a + 4, ps.ne + 4, ps.pb + 4, nKbm, p, ps.one);
    return;
  }
#if DSE_LOCKSTEP
  if (!TAIL) {
    // all 8 planes in lockstep: one asm block marks hit h of every plane, so
    // the loop control is paid once per 8 marks (the plane starts take the
    // operand row's registers)
    uint32_t kk[8];
#pragma unroll
    for (uint32_t q = 0; q < 8; ++q) kk[q] = plane_start(o.a[q], nKbm, ps.ne[q], p);
#pragma unroll 1
    for (uint32_t h = 0; h < n_run; ++h) mark8(kk, ps.pb, p, ps.one);
    return;
  }
#endif
#pragma unroll
  for (uint32_t q = 0; q < 8; ++q) {
    const uint32_t kk = plane_start(o.a[q], nKbm, ps.ne[q], p);
    const uint32_t pb4 = ps.pb[q];
    const uint32_t k = mark_run(pb4, kk, p, n_run, ps.one);
    if (TAIL) mark_tail(pb4, k, p, ps.one);
  }
}

// BARRETT: the launch may hold Kb >= 2^38 (values above 8.2e12, only with
// bucketed primes: the ranges without them end below (2^20 + 1)^2 < 2^40, so
// Kb < 2^36 there and the instantiation keeps no Barrett factors in its
// operand registers)
template <bool BARRETT>
__device__ __forceinline__ void unit_L(const LargeOps& o, uint64_t Vs, uint64_t Vend, uint64_t Kb,
                                       const PlaneSteps& ps, uint32_t pl_rot, const uint64_t* rho_pack_p,
                                       uint32_t sqrt_vs) {
  const uint32_t p = o.p & kLPrimeMask;  // the prime (>= 2^31: a lane past the table end)
  const float invp = fast_rcp((float)p);
  const uint32_t kbm = kb_mod_p<BARRETT>(Kb, p, invp, o.m);
  const uint32_t nKbm = 0u - kbm;
  const uint32_t pmax = __builtin_amdgcn_readlane(p, 63);
  // some lane not live or with p^2 inside the segment: the set's primes
  // ascend (lanes past the table end hold 2^31 and up), so pmax decides, on
  // the scalar unit (a per-lane 64-bit p^2 and two compares: 1e12 +1.4%)
  const bool none = pmax > sqrt_vs;  // pmax^2 > Vs, sqrt_vs = isqrt(Vs)
  if (!none) {  // every lane live and past p^2: branch-free bodies chosen by the set's plan
    const uint32_t plan = (uint32_t)__builtin_amdgcn_readfirstlane(o.p) >> 20;  // lane 0: live
    const uint32_t n_run = plan >> 3;
    if ((plan & 3) == 2) unit_L_fast<2>(o, p, nKbm, ps, 0);
    else if ((plan & 3) == 1) unit_L_fast<1>(o, p, nKbm, ps, 0);
    else if (!(plan & 4)) unit_L_fast<0>(o, p, nKbm, ps, n_run);
    else unit_L_fast<0, true>(o, p, nKbm, ps, n_run);
    return;
  }
  const uint32_t pmin = __builtin_amdgcn_readfirstlane(p);
  const uint64_t p2 = (uint64_t)p * p;
  const bool live = p2 < Vend;
  const bool slow = p2 > Vs;
  const uint32_t D = slow && live ? (uint32_t)(p2 - Vs) : 0u;
  if (!live) return;
  // read here, not passed in: the compiler rematerialises a kernel-argument
  // value by a scalar load, and hoisted into the common path that load (with
  // the s_waitcnt lgkmcnt(0) before its register is reused) drained every
  // wave's outstanding marks once per set
  const uint64_t rho_pack = *(volatile const uint64_t*)rho_pack_p;
  // Primes above KP/2 mark branch-free: two marks, dropped past the segment.
#pragma unroll
  for (uint32_t q = 0; q < 8; ++q) {
    uint32_t kk = plane_start(o.a[q], nKbm, ps.ne[q], p);
    if (slow) {
      const uint32_t pl = (pl_rot >> (3 * q)) & 7u;
      const uint32_t rho = (uint32_t)(rho_pack >> (5 * pl)) & 31u;
      const uint32_t kmin = kmin_for(D, rho);
      if (kmin > kk) {
        const uint32_t d = kmin - kk;  // < 2^18
        uint32_t qd = (uint32_t)((float)d * invp);
        while (qd * p < d) ++qd;
        while (qd > 0 && (qd - 1) * p >= d) --qd;
        kk += qd * p;
      }
    }
    const uint32_t pb4 = ps.pb[q];
    if (pmin > KP / 2) {
      mark_k(pb4, kk, ps.one);
      mark_k(pb4, kk + p, ps.one);
    } else {
      for (; kk < KP; kk += p) mark_k(pb4, kk, ps.one);
    }
  }
}

// floor(sqrt(v)), v < 2^62: the double root is within one of it, and the two
// loops correct it with exact 64-bit products.
__device__ __forceinline__ uint32_t isqrt_u64(uint64_t v) {
  uint32_t r = (uint32_t)__builtin_sqrt((double)v);
  while ((uint64_t)r * r > v) --r;
  while ((uint64_t)(r + 1) * (r + 1) <= v) ++r;
  return r;
}

struct WheelLdsLow {
  uint64_t mid_m[kMidCap];         // Barrett factors of the staged mid primes
  uint32_t mid_p[kMidCap];         // p | (30^{-1} mod p) << 16
  uint32_t mid_x[kMidCap];         // Vs mod p of this workgroup's segment (MidRes)
  uint32_t mid_inc[kMidCap];       // G W mod p
  uint32_t x_seg;                  // the launch segment mid_x holds (~0: none)
  uint32_t sq[2];                  // isqrt(Vs), isqrt(Vend - 1) of the workgroup's segment (prepare_segment)
  uint4 itab[kGDW];                // init tables U_G, 4 copies shifted by 0..3 dwords (kGDW / 4 blocks each)
  uint32_t thr[5];
  uint32_t ctr;                    // unit counter
  unsigned long long rcnt[kMaxRanges];  // per range: primes counted by this workgroup
};
static_assert(sizeof(WheelLdsLow) <= kImgOff, "LDS below the image");
struct WheelLds : WheelLdsLow {
  uint8_t pad[kImgOff - sizeof(WheelLdsLow)];
  uint32_t img[IMG_WORDS];         // the segment image, at LDS byte kImgOff, the top of the allocation
};
static_assert(sizeof(WheelLds) == kImgOff + IMG_BYTES, "the image ends the allocation");

// BK: the range has bucketed primes (wa.bk_*). Two instantiations, so the
// ranges without (N up to 1.1e12) run a unit loop without the bucket code
// (with it, the loop's SGPR spills doubled and 1e11 ran 1.9% slower).
template <bool BK>
__global__ __launch_bounds__(NT) void wheel_segments_kernel(const void* __restrict__ table, WheelArgs wa) {
  // One static LDS object at LDS address 0, so the image sits at kImgOff,
  // the value every mark's ds_or adds in its offset field.
  __shared__ WheelLds lds;
  uint64_t* const s_mid_m = lds.mid_m;
  uint32_t* const s_mid_p = lds.mid_p;
  uint32_t* const s_thr = lds.thr;

  const TableHeader* th = reinterpret_cast<const TableHeader*>(table);
  const uint32_t np = th->count;
  const uint32_t* __restrict__ P = reinterpret_cast<const uint32_t*>(reinterpret_cast<const char*>(table) + 16);
  const uint64_t* __restrict__ M =
      reinterpret_cast<const uint64_t*>(reinterpret_cast<const char*>(table) + table_m_offset(th->cap));
  const uint32_t* __restrict__ A =
      reinterpret_cast<const uint32_t*>(reinterpret_cast<const char*>(table) + table_a_offset(th->cap));
  // the L list's words p | plan << 20 for this geometry (table pl[0] / pl[1])
  const uint32_t* __restrict__ PL = reinterpret_cast<const uint32_t*>(reinterpret_cast<const char*>(table) +
                                                                    table_l_offset(th->cap)) +
                                    (kWheelLogKP == 17 ? 0u : th->cap);

#if defined(DSE_PAD_NOPS) && DSE_PAD_NOPS > 0
  // code-placement A/B only: shifts the kernel's instruction stream by 4 B each
  asm volatile(".rept " DSE_STR(DSE_PAD_NOPS) "\n\ts_nop 0\n\t.endr");
#endif
  const uint32_t tid = threadIdx.x, lane_id = tid & 63, wave = tid >> 6;

  if (tid == 0) {
    // first index with p > kQMax, > TA, > TB1, > TB (capped by the LDS stage),
    // > kWheelMaxPrime (bucketed or absent): the table holds every odd prime
    // from 3 up, so these are the host's prime counts (wa.nthr), capped by
    // the table's size
    s_thr[0] = min(wa.nthr[0], np);
    s_thr[1] = min(wa.nthr[1], np);
    s_thr[2] = min(wa.nthr[2], np);
    s_thr[3] = min(min(wa.nthr[3], np), s_thr[0] + kMidCap);
    s_thr[2] = min(s_thr[2], s_thr[3]);
    s_thr[4] = max(s_thr[3], min(wa.nthr[4], np));
    if (BK) {  // the other instantiations: prepare_segment
      lds.ctr = 0;
      lds.x_seg = ~0u;
    }
  }
  if (tid < kMaxRanges) lds.rcnt[tid] = 0;
  for (uint32_t idx = tid; idx < 4 * kGDW; idx += NT) reinterpret_cast<uint32_t*>(lds.itab)[idx] = g_init_tables.w[idx];
  __syncthreads();
  const uint32_t i_mid0 = s_thr[0], i_midB = s_thr[1], i_midB2 = s_thr[2], i_mid1 = s_thr[3];
  for (uint32_t i = tid; i < i_mid1 - i_mid0; i += NT) {
    const uint32_t q = P[i_mid0 + i];
    s_mid_p[i] = q | ((uint32_t)inv30_of(q) << 16);  // p < 2^14, 30^{-1} mod p < p
    s_mid_m[i] = M[i_mid0 + i];
    lds.mid_inc[i] = (uint32_t)(((uint64_t)gridDim.x * kWheelSpan) % q);
  }
  // Work units: list 1 = nA single mid primes (A), nB1 units of two primes
  // (B1), nB2 units of 4 primes (B2); list 2 = nL large units (two sets of 64
  // primes each); handed out through one dynamic queue. Issue arbitration
  // favours older waves, so any static split finishes the youngest waves
  // last; the queue makes them take fewer units instead.
  const uint32_t nA = i_midB - i_mid0;
  const uint32_t n_mid = i_mid1 - i_mid0;
  const uint32_t n_b1 = i_midB2 - i_mid0;      // staged index where B2 starts
  const uint32_t nB1 = (i_midB2 - i_midB + 1) / 2;
  const uint32_t nB2 = (i_mid1 - i_midB2 + 3) / 4;
  const uint32_t i_big = s_thr[4];             // L units end here
  constexpr uint32_t kLU = 128;                // primes per L unit
  const uint32_t n1 = nA + nB1 + nB2;

  const uint32_t nseg = wa.nseg;
  const uint32_t grid = gridDim.x;
  const uint32_t T = blockIdx.x < nseg ? (nseg - 1 - blockIdx.x) / grid + 1 : 0u;  // rounds
  // launch segment g -> its range (uniform: a scan of <= kMaxRanges starts)
  auto range_of = [&](uint32_t g) -> uint32_t {
    uint32_t r = 0;
    for (uint32_t i = 1; i < wa.nranges; ++i) r = g >= wa.r[i].seg0 ? i : r;
    return r;
  };
  // Without bucket units (the bucket instantiation keeps the round-19 code:
  // every form of this one tried there raised its SGPR spills from 58 to 59 or
  // more, and it gained nothing on the 1e18 window, profiles/r20/INDEX.md).
  // What thread 0 leaves in LDS for the workgroup's segment g of round t,
  // behind a barrier: the unit counter at its first claimed position; whether
  // mid_x holds this segment's residues; and isqrt(Vs) and isqrt(Vend - 1),
  // which mark_segment's waves read as two wave-uniform words where every wave
  // took both roots itself (a double sqrt and two correction loops each, per
  // wave and segment). p^2 > Vs <=> p > sq[0]; p^2 < Vend <=> p <= sq[1].
  auto prepare_segment = [&](uint32_t g, uint32_t t) {
    const uint32_t r = range_of(g);
    const uint64_t Vs = wa.r[r].V0 + (uint64_t)(g - wa.r[r].seg0) * kWheelSpan;
    lds.ctr = kFirstClaim<BK>;
    // the mid units of the workgroup's previous segment left their residues
    // for this one: valid if that segment was of the same range and every mid
    // unit ran in it (p^2 < its Vs for p <= TB)
    const bool same = t > 0 && g - wa.r[r].seg0 >= grid;
    lds.x_seg = same && Vs - (uint64_t)grid * kWheelSpan >= (uint64_t)TB * TB ? g : ~0u;
    lds.sq[0] = isqrt_u64(Vs);
    lds.sq[1] = isqrt_u64(Vs + kWheelSpan - 1);
  };

  // ---- init: small-prime patterns (7..61) of segment s into the image. Lane
  // (plane L & 7, run q = 8 w + (L >> 3)) of wave w writes its plane's words
  // of a run of about kInitWords consecutive blocks inside the wave's
  // [kExpandBlocks w, +kExpandBlocks): the blocks this wave expands, so it
  // may init them right after expanding.
  auto init_segment = [&](uint32_t* __restrict__ img, uint32_t g_seg) {
    const WheelRange& rg = wa.r[range_of(g_seg)];
    const uint64_t s = g_seg - rg.seg0;  // the range's segment
    uint32_t lane = lane_id;
    asm volatile("" : "+v"(lane));
    const uint32_t pl = lane & 7, q = 8 * wave + (lane >> 3);
    const uint32_t rho = (uint32_t)(rg.rho_pack >> (5 * pl)) & 31u;
    constexpr uint32_t R = kInitWords;  // words per lane
    static_assert(R % 4 == 0, "staggered init runs");
    // a half-wave's four lanes of one plane (j = 0..3) cover a region of 4R
    // blocks with runs of R + 1, R + 1, R + 1 and R - 3 blocks starting at
    // (R + 1) j: at step r they write blocks j + r (mod 4) -- distinct banks
    // (runs of R from multiples of R put all four on one bank: 4-way, 1%
    // of the kernel, profiles/r04/ab_init_stagger_1e11.txt)
    const uint32_t j = q & 3;
    const uint32_t b0 = 4 * R * (q >> 2) + (R + 1) * j;
    const uint32_t k0 = 32 * b0;        // its first period
    constexpr uint32_t H = 16;          // words per pass (bounds the registers: 16 acc + 20 read)
    static_assert(R % H == 0 && H % 4 == 0, "init passes");
    uint32_t boff[kNG], bsh[kNG];       // per group: the lane's first aligned 16-byte block, bit shift
    // rho takes 8 values over the lanes: left visible, the compiler evaluates
    // the group offsets for all 8 on the scalar unit and selects per lane
    // (a 6.8x SALU blow-up, 33 ms kernels); opaque, it is one VALU chain.
    const uint32_t rho_o = opaque(rho), k0_o = opaque(k0);
#pragma unroll
    for (int g = 0; g < kNG; ++g) {
      const uint32_t Mg = gmod(g);
      const uint32_t wg = (uint32_t)(kWheelSpan % Mg);
      const uint32_t sg = (uint32_t)(s % Mg);
      const uint32_t x = ((uint32_t)rg.v0g[g] + sg * wg + rho_o) % Mg;  // (Vs + rho) mod M_G
      const uint32_t o = (k0_o + x * kGInv30[g]) % Mg;                  // bit offset of period k0
      const uint32_t d0 = o >> 5, kc = d0 & 3;
      boff[g] = (kc * kGDW + gbase(g) + d0 - kc) / 4;                    // 16-byte block index
#if DSE_FAKE_CF_INIT  // profiling knockout: a 16-lane read group on consecutive 16-byte blocks (wrong patterns)
      boff[g] = gbase(g) / 4 + (lane & 15u);
#endif
      bsh[g] = o & 31;
    }
    uint32_t* const wp = img + 8 * b0 + pl;
#pragma unroll
    for (uint32_t h = 0; h < R; h += H) {
      uint32_t acc[H];
#pragma unroll
      for (uint32_t r = 0; r < H; ++r) acc[r] = 0;
#pragma unroll
      for (int g = 0; g < kNG; ++g) {
        const uint4* bp = lds.itab + boff[g] + h / 4;
        uint32_t blk[H + 4];
#pragma unroll
        for (uint32_t b = 0; b < H / 4 + 1; ++b) {
          const uint4 v = bp[b];
          blk[4 * b] = v.x; blk[4 * b + 1] = v.y; blk[4 * b + 2] = v.z; blk[4 * b + 3] = v.w;
        }
#pragma unroll
        for (uint32_t r = 0; r < H; ++r) acc[r] |= __builtin_amdgcn_alignbit(blk[r + 1], blk[r], bsh[g]);
        asm volatile("" ::: "memory");  // keep the next group's reads after these (register pressure)
      }
#pragma unroll
      for (uint32_t r = 0; r < H; ++r) {
        if (h + r >= R - 3 && j == 3) continue;  // the short run
        wp[8 * (h + r)] = acc[r];
      }
    }
    if (j != 3) {  // word R of the long runs
      uint32_t acc = 0;
#pragma unroll
      for (int g = 0; g < kNG; ++g) {
        const uint4* bp = lds.itab + boff[g] + R / 4;
        const uint4 v = bp[0];
        acc |= __builtin_amdgcn_alignbit(v.y, v.x, bsh[g]);
      }
      wp[8 * R] = acc;
    }
  };

  // ---- expand segment s to odd-only bits, count, store: each lane reads one
  // block (all 8 planes of 32 periods: 32 contiguous bytes, two
  // ds_read_b128); wave w takes blocks [kExpandBlocks w, +kExpandBlocks), 64
  // per step. ds_read_b128 serves a wave in 4 lane groups of 16 ({0-3,12-15,
  // 20-27}, {4-11,16-19,28-31} and the same + 32, MI355X_MICROARCH.md section
  // LDS); lane m of group g takes block 16 g + m of the step, so a group's
  // read touches each of 32 banks twice (having lanes m >= 8 read their upper
  // 16 bytes first covered all 64 once, but cost 8 v_cndmask per block to
  // put the halves back: 1e11 +0.4%, profiles/r05/ab_expand_reads.txt).
  // Output words 15 R .. 15 R + 14 of block R: a wave stores 3,840
  // contiguous bytes per step.
  // The block loop for the range's variant VT (the slots its planes take in
  // a period, dse_expand_bits.h): one static body per variant.
  auto expand_blocks = [&](const uint32_t* __restrict__ img, uint32_t g_seg, uint32_t ri, auto vt) {
    constexpr int VT = decltype(vt)::value;
    const WheelRange& rg = wa.r[ri];
    const uint64_t s = g_seg - rg.seg0;  // the range's segment
    const uint64_t out_words = 2ull * ((rg.nbits + 63) / 64);  // 32-bit words of the caller's mask
    uint32_t* __restrict__ out = rg.out;
    uint32_t my_count = 0;
    uint32_t lane = lane_id;
    asm volatile("" : "+v"(lane));
    const uint32_t l = lane & 31;
    const uint32_t gsub = (l >= 4 && l < 12) || (l >= 16 && l < 20) || l >= 28;
    const uint32_t m = l < 4 ? l : l < 12 ? l - 4 : l < 20 ? l - 8 : l < 28 ? l - 12 : l - 16;
    const uint32_t bl = 16 * (2 * (lane >> 5) + gsub) + m;  // block within the step
    const uint64_t seg_word0 = s * (uint64_t)kOutWordsPerSeg;
    const ExpandMasks masks = expand_masks();  // in SGPRs for this segment's blocks only
#pragma unroll 1
    for (uint32_t t = 0; t < kExpandBlocks / 64; ++t) {
      const uint32_t blk = kExpandBlocks * wave + 64 * t + bl;
      const uint4* rp = reinterpret_cast<const uint4*>(img + 8 * blk);
      const uint4 lo = rp[0], hi = rp[1];
      uint32_t W[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};  // composite bits of planes 0..7
      // composite candidates of the block's 256 (8 planes x 32 periods), from
      // the raw words: 8 v_bcnt instead of 15 over the output words; the
      // range's first block (small primes put back by rg.fix) and its end
      // count the output instead
      uint32_t n_comp = 0;
#pragma unroll
      for (int j = 0; j < 8; ++j) n_comp += __popc(W[j]);
      // composite bits of 8 planes x 32 periods -> prime bits of 32 periods x
      // 15 odd slots, in registers
      uint32_t o[15];
      expand_block<VT>(W, o, masks);
      const uint64_t w0 = seg_word0 + 15ull * blk;  // caller's 32-bit word index
      if (s == 0 && blk == 0) {
        o[0] |= (uint32_t)rg.fix;
        o[1] |= (uint32_t)(rg.fix >> 32);
      }
      const uint64_t bit0 = 32ull * w0;
      if (bit0 + 480 <= rg.nbits) {  // whole block inside the range (a separate path: no phi copies of o[])
        uint32_t cnt = 0;
        if (s == 0 && blk == 0) {
#pragma unroll
          for (int w = 0; w < 15; ++w) cnt += __popc(o[w]);
        } else {
          cnt = 256u - n_comp;
        }
        my_count += cnt;
        if (out) {
#pragma unroll
          for (int w = 0; w < 15; ++w) out[w0 + w] = o[w];
        }
      } else {  // range end (last segment only): mask, count, store what is inside the caller's words
        const uint32_t rem = bit0 >= rg.nbits ? 0u : (uint32_t)(rg.nbits - bit0);  // < 480 valid bits
        uint32_t cnt = 0;
#pragma unroll
        for (int w = 0; w < 15; ++w) {
          const uint32_t b = 32u * w;
          o[w] = b >= rem ? 0u : (rem - b >= 32 ? o[w] : o[w] & ((1u << (rem - b)) - 1u));
          cnt += __popc(o[w]);
        }
        my_count += cnt;
        if (out) {
#pragma unroll
          for (int w = 0; w < 15; ++w)
            if (w0 + w < out_words) out[w0 + w] = o[w];
        }
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) my_count += __shfl_xor(my_count, o);
    if (lane == 0 && my_count) atomicAdd(&lds.rcnt[ri], (unsigned long long)my_count);
  };
  // one scalar branch per segment, around the block loop
  auto expand_segment = [&](const uint32_t* __restrict__ img, uint32_t g_seg) {
    const uint32_t ri = range_of(g_seg);
    switch (__builtin_amdgcn_readfirstlane(wa.r[ri].variant)) {
#define DSE_EXPAND_CASE(V) \
  case V: expand_blocks(img, g_seg, ri, std::integral_constant<int, V>{}); break;
      DSE_EXPAND_CASE(0) DSE_EXPAND_CASE(1) DSE_EXPAND_CASE(2) DSE_EXPAND_CASE(3) DSE_EXPAND_CASE(4)
      DSE_EXPAND_CASE(5) DSE_EXPAND_CASE(6) DSE_EXPAND_CASE(7) DSE_EXPAND_CASE(8) DSE_EXPAND_CASE(9)
      DSE_EXPAND_CASE(10) DSE_EXPAND_CASE(11) DSE_EXPAND_CASE(12) DSE_EXPAND_CASE(13) DSE_EXPAND_CASE(14)
#undef DSE_EXPAND_CASE
      default: break;  // make_wheel_range sets 0..14
    }
  };

  // ---- mark segment s into image img -------------------------------------
  auto mark_segment = [&](uint32_t* __restrict__ img, uint32_t g_seg) {
    const WheelRange& rg = wa.r[range_of(g_seg)];
    const uint64_t s = g_seg - rg.seg0;  // the range's segment
    const uint64_t Vs = rg.V0 + s * kWheelSpan;  // segment base value
    const uint64_t Vend = Vs + kWheelSpan;
    // Lane-derived values are segment-invariant; left visible, the compiler
    // hoists dozens of them out of the round loop and spills them. Recompute.
    uint32_t lane = lane_id;
    asm volatile("" : "+v"(lane));
    const uint32_t img0 = lds_addr(img) - kImgOff;  // 0: mark addresses are image-relative
    const uint32_t one = opaque(1u);
    // Bucketed hits of the primes > 2^kBucketLoLog as units of the queue,
    // interleaved with the marking units, so their global-load latency
    // overlaps other waves' marking instead of stalling every wave at the
    // segment start: n0u band-0 units (kBk0Lists columns each), then band-1
    // units of kBkUnit entries, then one unit over the spill list if it is
    // not empty.
    uint32_t bk_b0 = 0, bk_b1 = 0, n0u = 0, n1u = 0, n3 = 0;
    if (BK) {
      n0u = wa.bk_k0 ? kBkGrid0 / kBk0Lists : 0u;
      bk_b0 = wa.bk_start[s];
      bk_b1 = wa.bk_start[s + 1];
      n1u = (bk_b1 - bk_b0 + kBkUnit - 1) / kBkUnit;
      n3 = n0u + n1u + (wa.bk_k0 && *wa.bk_nspill ? 1u : 0u);
    }
    // the range's rho_pack in the kernel-argument segment (after the table
    // pointer), for unit_L's rare slow path: not &rg.rho_pack, which would
    // make the compiler copy the whole argument block to scratch
    const uint64_t* rho_pack_p = reinterpret_cast<const uint64_t*>(
        (const char*)__builtin_amdgcn_kernarg_segment_ptr() + kWaOffset +
        range_of(g_seg) * sizeof(WheelRange) + offsetof(WheelRange, rho_pack));
    // isqrt(Vs) and isqrt(Vend - 1) (p^2 < Vend <=> p <= isqrt(Vend - 1)): left
    // by thread 0 (prepare_segment), or per wave with bucket units
    const uint32_t sqrt_vs = __builtin_amdgcn_readfirstlane(BK ? isqrt_u64(Vs) : lds.sq[0]);
    const uint32_t sqrt_ve = __builtin_amdgcn_readfirstlane(BK ? isqrt_u64(Vend - 1) : lds.sq[1]);
    const uint32_t rot = (i_mid1 + lane) & 7;  // = table index & 7 of this lane's large primes
    // absolute residue (q + rot) & 7 at step q: its plane and e bit
    const uint32_t pl_rot = ((rg.pl_pack >> (3 * rot)) | (rg.pl_pack << (24 - 3 * rot))) & 0xFFFFFFu;
    const uint32_t e_rot = ((rg.e_iota >> rot) | (rg.e_iota << (8 - rot))) & 0xFFu;
    PlaneSteps ps;
    ps.one = one;
#pragma unroll
    for (uint32_t q = 0; q < 8; ++q) {
      ps.pb[q] = img0 + 4 * ((pl_rot >> (3 * q)) & 7u) + (DSE_FAKE_CF_L ? ((lane_id >> 3) & 3u) << 5 : 0u);
      ps.ne[q] = 0u - ((e_rot >> q) & 1u);
    }
    const uint64_t Kb = rg.KB0 + s * (uint64_t)KP;
    const bool need_m = BK && Kb >= (1ull << 38);  // unit_L's Barrett path (unit_L<BK>)
    MidRes mr;
    mr.x = lds.mid_x;
    mr.inc = lds.mid_inc;
    mr.have = __builtin_amdgcn_readfirstlane(lds.x_seg) == g_seg;
    // One dynamic queue over both lists, interleaved (list 1 at even, list 2
    // at odd positions while both last). Claims run two units ahead: the LDS
    // atomic for unit j+2 is issued when unit j starts and read when it ends
    // (by then this wave's marks of unit j have drained), and a large unit's
    // operands are loaded while the unit before it runs.
    // large units of this segment: up to its piece's bound (WheelRange::lcap)
    const uint32_t i_live = max(i_mid1, min(i_big, rg.lcap[min((uint32_t)(s >> rg.lsh), kLPieces - 1)]));
    const uint32_t n2 = (i_live - i_mid1 + kLU - 1) / kLU;
    const uint32_t n_int = min(n1, n2), n_all = n1 + n2;
    // The claim is an asm ds_add_rtn: written as a C++ atomic, the AMDGPU
    // atomic optimizer aggregates it over the wave and waits for its return
    // on the spot (draining the previous unit's marks with it), which
    // defeats the two-ahead issue. Read through claimed().
    const uint32_t ctr_addr = lds_addr(&lds.ctr);
    const uint32_t wave_u = __builtin_amdgcn_readfirstlane(wave);
    auto claim = [&]() -> uint32_t {
      uint32_t j = 0;
      if (lane == 0) asm volatile("ds_add_rtn_u32 %0, %1, %2" : "=v"(j) : "v"(ctr_addr), "v"(1u) : "memory");
      return j;  // per-lane value; lane 0 holds the claim
    };
    auto claimed = [&](uint32_t j) -> uint32_t {
      asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(j)::"memory");
      return __builtin_amdgcn_readlane(j, 0);
    };
    auto is_l = [&](uint32_t u) -> bool { return u < 2 * n_int ? (u & 1) != 0 : n2 > n1; };
    auto idx_of = [&](uint32_t u) -> uint32_t { return u < 2 * n_int ? u >> 1 : u - n_int; };
    // queue position -> marking unit (or ~0u: bucket unit bk_of(q)); the n3
    // bucket units interleave 1:1 with the marking units from the start
    const uint32_t mb = min(n3, n_all), n_q = n_all + n3;
    auto unit_of = [&](uint32_t q) -> uint32_t {
      if (q < 2 * mb) return (q & 1) ? ~0u : q >> 1;
      return n3 > n_all ? ~0u : q - mb;
    };
    auto bk_of = [&](uint32_t q) -> uint32_t { return q < 2 * mb ? q >> 1 : q - mb; };
    // a claimed queue position, decoded once: kind << 30 | index (kind 0: a mid
    // unit of list 1, 1: a large unit, 2: a bucket unit), ~0u past the end
    constexpr uint32_t kIdx = (1u << 30) - 1;
    auto decode = [&](uint32_t q) -> uint32_t {
      if (q >= n_q) return ~0u;
      const uint32_t u = unit_of(q);
      if (u == ~0u) return 2u << 30 | bk_of(q);
      return (is_l(u) ? 1u << 30 : 0u) | idx_of(u);
    };
    // Operands are only ever loaded into nxt and copied to cur at the top of
    // an iteration, after they have landed: had the first unit's loads gone
    // straight into cur, the compiler's wait analysis, merging that entry
    // with the loop's back edge, waited inside every unit for the next unit's
    // loads just issued (a vmcnt(4) and a vmcnt(0) per large unit).
    LargeOps cur, nxt;
    LargeOps cur1, nxt1;  // the unit's second 64 primes
    // without bucket units a wave's first two units are queue positions wave
    // and wave + NT / 64 of every segment (the counter starts at kFirstClaim):
    // no claim round trips before the first mark; positions past n_q decode to
    // ~0u as claimed ones do
    uint32_t d_nxt = decode(BK ? claimed(claim()) : wave_u);
    if ((d_nxt >> 30) == 1) {
      load_L(nxt, PL, M, A, i_mid1 + kLU * (d_nxt & kIdx) + lane, i_big, need_m);
      load_L(nxt1, PL, M, A, i_mid1 + kLU * (d_nxt & kIdx) + 64 + lane, i_big, need_m);
    }
    uint32_t d_after = decode(BK ? claimed(claim()) : wave_u + NT / 64);
    // the first unit's operands landed before the loop (an asm that reads
    // them makes the compiler wait here), so on no path into the loop does a
    // set's register still wait for a load
    asm volatile("" ::"v"(nxt.p), "v"(nxt.a[0]), "v"(nxt.a[1]), "v"(nxt.a[2]), "v"(nxt.a[3]), "v"(nxt.a[4]),
                 "v"(nxt.a[5]), "v"(nxt.a[6]), "v"(nxt.a[7]), "v"(nxt1.p), "v"(nxt1.a[0]), "v"(nxt1.a[1]),
                 "v"(nxt1.a[2]), "v"(nxt1.a[3]), "v"(nxt1.a[4]), "v"(nxt1.a[5]), "v"(nxt1.a[6]), "v"(nxt1.a[7]));
    for (;;) {
      cur = nxt;
      cur1 = nxt1;
      undef_ops(nxt);  // dead until the next unit's loads: cur and nxt are never one register
      undef_ops(nxt1);
      const uint32_t d_cur = d_nxt;
      d_nxt = d_after;
      if (d_cur == ~0u) break;
      // issued and read in the same iteration: the asm output is written when
      // the LDS returns it, so the value must not be live across a loop phi
      // (a register copy there reads it early; a claim carried from one
      // iteration into the next gave wrong counts)
      const uint32_t c2 = claim();  // unit after next, read at the end of this one
      if ((d_nxt >> 30) == 1) {
        load_L(nxt, PL, M, A, i_mid1 + kLU * (d_nxt & kIdx) + lane, i_big, need_m);
        load_L(nxt1, PL, M, A, i_mid1 + kLU * (d_nxt & kIdx) + 64 + lane, i_big, need_m);
      }
      if (BK && (d_cur >> 30) == 2) {  // a bucket unit, kBkBatchU loads in flight per lane
        const uint32_t bu = d_cur & kIdx;
        if (bu < n0u) {  // band 0: columns kBk0Lists bu .. +kBk0Lists, 4 at a time, each read by the whole wave
          const uint64_t li0 = s * (uint64_t)kBkGrid0 + bu * kBk0Lists;
          const uint32_t nl = lane < kBk0Lists ? wa.bk_n0[li0 + lane] : 0u;
#pragma unroll 1
          for (uint32_t g = 0; g < kBk0Lists; g += 4) {
            uint32_t n[4], nmax = 0;
            const uint32_t* __restrict__ r[4];
#pragma unroll
            for (uint32_t l = 0; l < 4; ++l) {
              n[l] = min((uint32_t)__builtin_amdgcn_readlane((int)nl, (int)(g + l)), wa.bk_k0);
              r[l] = wa.bk_reg0 + ((uint64_t)(bu * kBk0Lists + g + l) * wa.nseg + s) * wa.bk_k0;
              nmax = max(nmax, n[l]);
            }
            for (uint32_t o = lane; o < nmax + lane; o += 256) {  // contiguous 256-entry pieces of 4 lists
              uint32_t e[16];
#pragma unroll
              for (uint32_t l = 0; l < 4; ++l)
#pragma unroll
                for (uint32_t t = 0; t < 4; ++t)
                  e[4 * l + t] = o + 64 * t < n[l] ? __builtin_nontemporal_load(r[l] + o + 64 * t) : 0u;
#pragma unroll
              for (uint32_t l = 0; l < 4; ++l)
#pragma unroll
                for (uint32_t t = 0; t < 4; ++t)
                  if (o + 64 * t < n[l]) mark_entry(img0, e[4 * l + t], one);
            }
          }
        } else if (bu < n0u + n1u) {  // band 1: kBkUnit entries of the segment's list
          const uint32_t beg = bk_b0 + (bu - n0u) * kBkUnit, end = min(bk_b1, beg + kBkUnit);
          for (uint32_t j = beg + lane; j < end; j += 64 * kBkBatchU) {
            uint32_t e[kBkBatchU];
#pragma unroll
            for (uint32_t t = 0; t < kBkBatchU; ++t)
              e[t] = j + 64 * t < end ? __builtin_nontemporal_load(wa.bk_entries + j + 64 * t) : 0u;
#pragma unroll
            for (uint32_t t = 0; t < kBkBatchU; ++t)
              if (j + 64 * t < end) mark_entry(img0, e[t], one);
          }
        } else {  // the spill list (band-0 regions that overflowed): this segment's hits
          const uint32_t ns = (uint32_t)min((uint64_t)*wa.bk_nspill, wa.bk_spill_cap);
          for (uint32_t j = lane; j < ns; j += 64) {
            const unsigned long long v = wa.bk_spill[j];
            if ((uint32_t)(v >> 32) == (uint32_t)s) mark_entry(img0, (uint32_t)v, one);
          }
        }
        d_after = decode(claimed(c2));
        continue;
      }
      const uint32_t k = d_cur & kIdx;
      if ((d_cur >> 30) == 0) {
        if (k < nA) {
          const uint32_t pi = __builtin_amdgcn_readfirstlane(s_mid_p[k]);
          const uint32_t p = pi & 0xFFFFu;
          const uint64_t m = ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)(s_mid_m[k] >> 32)) << 32) |
                             (uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)s_mid_m[k]);
          if ((uint64_t)p * p < Vend) unit_A(img0, pi, m, mr, k, Vs, rg.rho_pack, lane, one);
        } else if (k < nA + nB1) {
          const uint32_t j0 = nA + (k - nA) * 2;
          const uint32_t pf = __builtin_amdgcn_readfirstlane(s_mid_p[j0]) & 0xFFFFu;
          if ((uint64_t)pf * pf < Vend)
            unit_B1(img0, s_mid_p, s_mid_m, mr, j0, min(2u, n_b1 - j0), Vs, rg.rho_pack, lane, one);
        } else {
          const uint32_t j0 = n_b1 + (k - nA - nB1) * 4;
          const uint32_t pf = __builtin_amdgcn_readfirstlane(s_mid_p[j0]) & 0xFFFFu;
          if ((uint64_t)pf * pf < Vend)
            unit_B2(img0, s_mid_p, s_mid_m, mr, j0, min(4u, n_mid - j0), Vs, rg.rho_pack, lane, one);
        }
      } else {
        // a set marks if its first prime's square is below the segment's end
        const uint32_t p0 = __builtin_amdgcn_readfirstlane(cur.p) & kLPrimeMask;
        if (p0 <= sqrt_ve) unit_L<BK>(cur, Vs, Vend, Kb, ps, pl_rot, rho_pack_p, sqrt_vs);
        const uint32_t p1 = __builtin_amdgcn_readfirstlane(cur1.p) & kLPrimeMask;
        if (p1 <= sqrt_ve) unit_L<BK>(cur1, Vs, Vend, Kb, ps, pl_rot, rho_pack_p, sqrt_vs);
      }
      d_after = decode(claimed(c2));
    }
  };

  if (T > 0) init_segment(lds.img, blockIdx.x);
  if (BK) __syncthreads();
  for (uint32_t t = 0; t < T; ++t) {
    const uint32_t s = blockIdx.x + t * grid;
    if (!BK) {
      // thread 0 prepares segment s; the waves still in the expand and init of
      // the segment before read none of these words
      if (tid == 0) prepare_segment(s, t);
      __syncthreads();
    }
    mark_segment(lds.img, s);
    lds_drain();
    __syncthreads();  // every claim of this segment has returned
    expand_segment(lds.img, s);
    // init of this workgroup's next segment, on the rows this wave just
    // expanded: no barrier in between, and waves drift into init while
    // others still expand
    if (t + 1 < T) init_segment(lds.img, s + grid);
    if (BK) {
      if (tid == 0) {
        lds.ctr = 0;
        // the mid units left their residues for segment s + grid: valid if it is
        // of the same range and every mid unit ran (p^2 < Vs for p <= TB)
        const uint32_t r0 = range_of(s), r1 = range_of(s + grid);
        const uint64_t Vs = wa.r[r0].V0 + (uint64_t)(s - wa.r[r0].seg0) * kWheelSpan;
        lds.x_seg = t + 1 < T && r1 == r0 && Vs >= (uint64_t)TB * TB ? s + grid : ~0u;
      }
      __syncthreads();
    }
  }
  if (!BK) __syncthreads();

  if (tid < wa.nranges && lds.rcnt[tid]) atomicAdd(wa.r[tid].count, lds.rcnt[tid]);
}

// One persistent launch of this unit's instantiation over wa's segments: a
// workgroup per CU, at most one per segment. Each unit wraps the one it emits
// in its public launcher (dse_internal.h).
template <bool BK>
hipError_t launch_wheel(const void* table, const WheelArgs& wa, int num_cus, hipStream_t stream) {
  if (wa.nseg == 0) return hipSuccess;
  const uint32_t grid = wheel_grid(wa.nseg, num_cus);
  hipLaunchKernelGGL(wheel_segments_kernel<BK>, dim3(grid), dim3(NT), 0, stream, table, wa);
  return hipGetLastError();
}

}  // namespace
}  // namespace dse
