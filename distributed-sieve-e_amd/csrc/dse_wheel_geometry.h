// dse_wheel_geometry.h -- mod-30 wheel segmented sieve for gfx950 (MI355X):
// the segment geometry, the init tables, the kernel's arguments and the bucket
// entry format. Everything here that depends on DSE_WHEEL_LOG_KP, DSE_TA,
// DSE_TB1 or DSE_TB has internal linkage: dse_wheel_half.hip compiles it with
// another geometry. The kernel itself is in dse_wheel_kernel.h, the host-side
// builders of its arguments in dse_wheel_args.h, the bucketed pass (which
// needs the geometry and the arguments, not the kernel) in dse_bucket.hip.
//
// Bit j of the caller's range stands for the odd value 3+2(g_start+j), the
// reference's element j of its chunk vector (sieve.clj:9-13); a set bit =
// prime. The marking loops replace sieve.clj:36-71's index walk; multiples of
// 3 and 5 are never stored in LDS, so they touch 8/15 of the words an odd-only
// image needs.
//
// Geometry. V0 = v_start - 1 (even); segment s covers the integers
// [Vs, Vs + W), W = 30*KP, Vs = V0 + s*W (KP = 2^17 periods), exactly output
// bits [s*15*KP, (s+1)*15*KP) -- a whole number of words, so no output word is
// shared by two segments. The 8 odd residues rho_0 < ... < rho_7 in [1,29]
// with gcd(V0 + rho, 30) = 1 define the planes: plane i bit k <-> the value
// Vs + rho_i + 30k, i.e. output bit 15k + (rho_i - 1)/2 of the segment.
//
// LDS image (128 KiB), word-interleaved: block R (periods 32R .. 32R+31)
// is 8 consecutive words, one per plane, so the word of (plane i, period k)
// is 8 (k >> 5) + i and its byte address (k & ~31) | 4i -- one v_and_or from
// a period index, and an image of 2^17 periods is 2^17 bytes. The bank of a
// ds_or_b32 (dword address mod 32) is 8 ((k >> 5) mod 4) + i, so a mark
// pattern is conflict-free when the lanes on one plane in a 32-lane group sit
// in distinct blocks mod 4; two lanes per bank cost nothing extra (the
// instruction's transfer takes 2 LDS cycles per group anyway).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <algorithm>

#include "dse_internal.h"

namespace dse {
namespace {

constexpr uint32_t KP = 1u << kWheelLogKP;  // periods per segment (per plane)
constexpr uint32_t BLOCKS = KP / 32;        // 32-period blocks (8 words each)
constexpr uint32_t IMG_WORDS = 8 * BLOCKS;  // one segment image
constexpr uint32_t IMG_BYTES = 4 * IMG_WORDS;
static_assert(IMG_BYTES == KP, "a period index is its block's byte address");
// The image sits at the top of the workgroup's LDS, bytes [kImgOff, kImgOff +
// IMG_BYTES) (WheelLds): mark addresses are image-relative (a period index |
// its plane's offset) and every ds_or adds kImgOff in its offset field. A
// mark at a period k >= KP (past the segment) thus lands at or beyond the end
// of the allocation, where the LDS drops it (microbench/lds_oor_bench.hip);
// nothing lives above the image. So marks that may fall past the segment's
// end are issued unconditionally, without a compare and exec masking.
#define DSE_IMG_OFF_S "32768"
constexpr uint32_t kImgOff = 32768;
#define DSE_STR2(x) #x
#define DSE_STR(x) DSE_STR2(x)
constexpr uint32_t NT = 1024;
constexpr uint32_t NW = NT / 64;            // waves; every wave marks, expands and inits
static_assert(BLOCKS % (64 * NW) == 0, "expansion blocks");
#ifndef DSE_TA
#define DSE_TA 96
#endif
constexpr uint32_t TA = DSE_TA;             // A/B1 threshold
#ifndef DSE_TB1
#define DSE_TB1 640
#endif
constexpr uint32_t TB1 = DSE_TB1;           // B1/B2 threshold
#ifndef DSE_TB
#define DSE_TB 1536
#endif
constexpr uint32_t TB = DSE_TB;             // B2/L threshold
static_assert(TA <= 256 && TA < TB1 && TB1 <= TB && TB <= KP / 8, "unit thresholds");
// Marks per hit class (class_marks_k). B1 and B2 mark every class to the
// segment end: a prime p has its hits at indices n <= floor((KP - 1) / p), and
// a B1 class holds every 128th, so T = floor(floor((KP - 1) / pmin) / 128) + 1
// <= floor((KP - 1) / (128 (TA + 1))) + 1 marks reach them all (pmin > TA: 11
// at p = 97 with KP = 2^17, 6 with 2^16); a B2 class holds every 64th, pmin >
// TB1 (4 and 2 at p = 641).
constexpr uint32_t kClassMarksMax = 11;
static_assert((KP - 1) / (128 * (TA + 1)) + 1 <= kClassMarksMax && (KP - 1) / (64 * (TB1 + 1)) + 1 <= kClassMarksMax,
              "class_marks_k covers K <= kClassMarksMax");
constexpr uint32_t kMidCap = TB >= 16384 ? 1920 : TB >= 8192 ? 1040 : TB >= 4096 ? 580 : 320;  // >= odd primes in (61, TB]
constexpr uint32_t kOutWordsPerSeg = (uint32_t)(kWheelOutBits / 32);  // 30720

constexpr uint32_t kQMax = 79;  // the pattern primes are 7..79

constexpr uint32_t inv30_const(uint32_t q) {
  for (uint32_t x = 1; x < q; ++x)
    if ((30 * x) % q == 1) return x;
  return 0;
}
// Init tables: the 15 small primes in 7 groups G with period M_G = prod(G).
// U_G[y] = 1 iff some q in G divides y. Plane i period k holds the value
// Vs + rho_i + 30k, and q | Vs + rho_i + 30k <=> q | k + c_G with
// c_G = (Vs + rho_i) * 30^{-1} mod M_G (gcd(30, M_G) = 1), so every plane
// reads the same bit string at its own offset. A lane inits kInitRun
// consecutive periods of one column: 33 dwords of each string from its bit
// offset o, read as 9 aligned ds_read_b128 from the copy of the string that
// is shifted by (o >> 5) & 3 dwords (4 copies), so every read is aligned
// whatever o is; word r = alignbit(U[d0 + r + 1], U[d0 + r], o & 31).
// 7..61 in 7 groups until round 4; 67..79 as two more groups (1e11 -0.3%, 1e12
// -0.7%: the init reads of two more strings cost less than A units for 4 primes)
constexpr int kNG = 9;
constexpr uint32_t kGQ[kNG][3] = {{7, 11, 13}, {17, 19, 1}, {23, 29, 1}, {31, 37, 1}, {41, 43, 1},
                                  {47, 53, 1}, {59, 61, 1}, {67, 71, 1}, {73, 79, 1}};
constexpr uint32_t gmod(int g) { return kGQ[g][0] * kGQ[g][1] * kGQ[g][2]; }
constexpr uint32_t kInitWords = IMG_WORDS / NT;  // words one lane inits per segment (one plane of a block run)
constexpr uint32_t kInitRun = 32 * kInitWords;    // their periods
constexpr uint32_t kExpandBlocks = BLOCKS / NW;   // blocks one wave expands (and inits) per segment
// ds_read_b128 per lane and group (+1: a staggered run's one word more, read as one more pass)
constexpr uint32_t kInitBlocks = kInitRun / 128 + 2;
// dwords per group string and copy: the reads reach dword d0 + 4 kInitBlocks - 1, d0 < M_G/32 + 1
constexpr uint32_t gdw(int g) { return ((gmod(g) + 32 * (4 * kInitBlocks + 1) + 127) / 128) * 4; }
constexpr uint32_t gbase(int g) { return g == 0 ? 0u : gbase(g - 1) + gdw(g - 1); }
constexpr uint32_t kGDW = gbase(kNG);  // dwords per copy (620)
constexpr uint32_t kGInv30[kNG] = {inv30_const(gmod(0)), inv30_const(gmod(1)), inv30_const(gmod(2)),
                                   inv30_const(gmod(3)), inv30_const(gmod(4)), inv30_const(gmod(5)),
                                   inv30_const(gmod(6)), inv30_const(gmod(7)), inv30_const(gmod(8))};

// The init tables, built at compile time (a launch copies them into LDS):
// copy k, group g, dword gbase(g) + j = bits [32 (j + k), 32 (j + k) + 32) of U_g.
struct InitTables {
  uint32_t w[4 * kGDW];
};
constexpr InitTables make_init_tables() {
  InitTables t{};
  for (int g = 0; g < kNG; ++g) {
    for (uint32_t j = 0; j < gdw(g) + 3; ++j) {  // dword j of U_g
      uint32_t v = 0;
      for (uint32_t b = 0; b < 32; ++b) {
        const uint32_t y = 32 * j + b;
        const bool hit = y % kGQ[g][0] == 0 || y % kGQ[g][1] == 0 || (kGQ[g][2] > 1 && y % kGQ[g][2] == 0);
        v |= (uint32_t)hit << b;
      }
      for (uint32_t k = 0; k < 4; ++k)
        if (j >= k && j - k < gdw(g)) t.w[k * kGDW + gbase(g) + (j - k)] = v;
    }
  }
  return t;
}
__device__ const InitTables g_init_tables = make_init_tables();

constexpr uint32_t kLPieces = 16;  // pieces of a range with their own large-prime bound
// Ranges per launch: several chunks of one device (dse_sieve_all with P >
// devices, and the dropped tail) go to one persistent launch, so no chunk's
// partial last round of segments leaves the CUs idle and no host launch
// latency sits between chunks.
constexpr uint32_t kMaxRanges = 9;

}  // namespace

// WheelRange and WheelArgs cross translation units (launch_wheel_plain,
// launch_wheel_bucketed; dse_internal.h forward-declares WheelArgs), so they
// are dse:: types with one layout in every unit: kNG, kLPieces and kMaxRanges
// do not depend on the geometry macros.

// One odd-index range of a launch: its segments are [seg0, seg0 + its
// segment count) of the launch's list (WheelArgs::nseg in all).
struct WheelRange {
  uint64_t V0;         // v_start - 1
  uint64_t nbits;      // odd candidates in the range
  uint64_t KB0;        // floor(V0 / 30)
  uint64_t rho_pack;   // rho_i in bits [5i, 5i+5)
  uint32_t* out;       // the range's mask (32-bit words), or null
  unsigned long long* count;  // incremented by the range's prime count (device)
  uint32_t pl_pack;    // plane of absolute residue R30[j] in bits [3j, 3j+3)
  uint32_t e_iota;     // bit j: floor((V0 + rho)/30) = KB0 + 1 for the plane of R30[j]
  uint64_t fix;        // output words 0, 1: bits of the primes 3..kQMax inside the range
  uint32_t seg0;       // first segment of the range in the launch
  uint16_t v0g[kNG];   // V0 mod M_G (init tables)
  // Large units past the live primes of a segment only load operands to skip
  // them: segment s of the range needs table indices below
  // lcap[min(s >> lsh, kLPieces - 1)] (>= the odd primes with p^2 < its end)
  uint32_t lsh;
  uint32_t lcap[kLPieces];
  uint32_t variant;    // (V0 mod 30) / 2: which slots the planes take in a period (dse_expand_bits.h)
};

struct WheelArgs {
  WheelRange r[kMaxRanges];
  uint32_t nranges;    // 1..kMaxRanges (1 with bucketed primes)
  uint32_t nseg;       // segments of all ranges
  uint32_t nthr[5];    // odd primes <= kQMax (79), TA, TB1, TB, kWheelMaxPrime (table indices of the unit lists)
  // Bucketed hits of the primes > 2^kBucketLoLog, or the bucket_lo_log2 option (bk_start null: none), as
  // entries (bucket_entry):
  const uint32_t* bk_entries;  // band 1: segment s owns [bk_start[s], bk_start[s+1])
  const uint32_t* bk_start;
  const uint32_t* bk_reg0;     // band 0: segment s, column b: bk_n0[s * kBucketGrid + b] entries
  const uint32_t* bk_n0;       //   from bk_reg0 + (b * nseg + s) * bk_k0
  const unsigned long long* bk_spill;  // band-0 hits past their region: segment << 32 | entry,
  const uint32_t* bk_nspill;           //   *bk_nspill of them (normally none)
  uint64_t bk_spill_cap;               //   (at most this many stored)
  uint32_t bk_k0;              // band-0 region capacity (0: no band 0 in the pass)
};
static_assert(sizeof(WheelArgs) <= 4096, "kernel arguments");
static_assert(alignof(WheelArgs) <= 8, "kernel argument layout");

namespace {

// wheel_segments_kernel(table, wa): wa follows the 8-byte table pointer in the
// kernel-argument segment
constexpr uint32_t kWaOffset = 8;

// The bucket units of the wheel kernel and the entry format they share with
// the fill kernels (dse_bucket.hip).
#ifndef DSE_BK_GRID
#define DSE_BK_GRID 1024  // band-0 fill workgroups (columns)
#endif
#ifndef DSE_BK_UNIT_BATCHES
#define DSE_BK_UNIT_BATCHES 4
#endif
constexpr uint32_t kBkBatchU = 16;                                // loads in flight per lane (bucket unit)
constexpr uint32_t kBkUnit = 64 * kBkBatchU * DSE_BK_UNIT_BATCHES;  // band-1 entries per bucket unit
constexpr uint32_t kBkGrid0 = DSE_BK_GRID;                         // band-0 columns (fill workgroups)
#ifndef DSE_BK0_LISTS
#define DSE_BK0_LISTS 16
#endif
constexpr uint32_t kBk0Lists = DSE_BK0_LISTS;                      // band-0 columns per bucket unit
static_assert(kBkGrid0 % kBk0Lists == 0 && 64 % kBk0Lists == 0, "band-0 bucket units");
constexpr uint32_t kKeyShift = 20;                                 // entry = LDS word index << 5 | bit < 2^20
static_assert(IMG_WORDS * 32 <= (1u << kKeyShift), "bucket entry layout");

}  // namespace
}  // namespace dse
