// Internal interface between the gfx950 kernel units (dse_base.hip, dse_wheel.hip,
// dse_wheel_plain.hip, dse_wheel_half.hip, dse_bucket.hip, dse_finish.hip,
// dse_primes.hip, dse_stats.hip, dse_query.hip, dse_goldbach.hip, dse_race.hip, dse_tuples.hip, dse_gaps.hip, dse_sums.hip, dse_consec.hip, and the test-only dse_arith_probe.hip)
// and the C-ABI host layer (dse_host.cpp,
// dse_finish_host.cpp, dse_primes_host.cpp, dse_stats_host.cpp, dse_query_host.cpp,
// dse_goldbach_host.cpp, dse_race_host.cpp, dse_tuples_host.cpp, dse_gaps_host.cpp, dse_sums_host.cpp, dse_consec_host.cpp). Not installed;
// include/dse.h is the ABI. The units that read a resident mask (finish,
// primes, stats, query, goldbach, race, tuples) share its range, tiles and clipped word load (dse_mask.h);
// every unit with a workgroup sum, scan or best-of takes it from dse_block.h; the two that reduce
// a range to one struct through per-workgroup slabs (stats, goldbach, race) share dse_slab.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dse_mask.h"

namespace dse {

// Base-prime table: one flat device buffer so ranks can broadcast it as bytes.
//   [0,16)            header {count, cap, limit}
//   [16, 16+4cap)     uint32 p[cap]      odd primes <= limit, ascending
//   [align8(...), +8cap) uint64 m[cap]  Barrett factors floor((2^64-1)/p) of the primes <= kWheelMaxPrime
//                                        (the bucketed primes' walks divide in double precision)
//   [align32(..), +32cap) uint32 a[8cap] wheel offsets, row i rotated by i mod 8:
//                                        a[8i+j] = first k >= 0 with p | R30[(j+i)&7] + 30k
//                                        (p >= 7; 0 for p = 3, 5)
//   [align32(..)+32cap, +8cap) uint32 pl[2][cap] the wheel kernel's large-prime words: p | plan << 20,
//                                        plan = the marking plan of the prime's set of 64 (unit_L;
//                                        pl[0] for 2^17-period segments, pl[1] for 2^16)
struct TableHeader {
  uint32_t count;
  uint32_t cap;
  uint64_t limit;
};

__host__ __device__ inline uint64_t table_m_offset(uint32_t cap) {
  return (16ull + 4ull * cap + 7ull) & ~7ull;
}
__host__ __device__ inline uint64_t table_a_offset(uint32_t cap) {
  return (table_m_offset(cap) + 8ull * cap + 31ull) & ~31ull;
}
__host__ __device__ inline uint64_t table_l_offset(uint32_t cap) { return table_a_offset(cap) + 32ull * cap; }
__host__ __device__ inline uint64_t table_bytes_for_cap(uint32_t cap) {
  return table_l_offset(cap) + 8ull * cap;
}

// The 8 residues mod 30 coprime to 30 (wheel planes, absolute numbering).
constexpr uint32_t kR30[8] = {1, 7, 11, 13, 17, 19, 23, 29};

// Mod-30 wheel segment geometry (dse_wheel_geometry.h): a segment is 2^17
// periods of 30 integers, 8 planes (one per coprime residue) x 8 columns of
// 2^14 periods (one 128 KiB LDS image). dse_wheel_half.hip compiles the same
// kernel (dse_wheel_kernel.h) with 2^16 periods per segment (range tails,
// DESIGN.md section 4.1.2).
#ifndef DSE_WHEEL_LOG_KP
#define DSE_WHEEL_LOG_KP 17
#endif
constexpr int kWheelLogKP = DSE_WHEEL_LOG_KP;
constexpr uint64_t kWheelSpan = 30ull << kWheelLogKP;   // integers per segment
constexpr uint64_t kWheelOutBits = kWheelSpan / 2;      // odd candidates per segment
// Ranges with base primes above this go through the bucketed pass
// (dse_bucket.hip), which then buckets every prime above 2^kBucketLoLog.
#ifndef DSE_WHEEL_MAX_LOG
// Builds support 19 and 20 only: the L list's table words carry the prime in
// 20 bits (dse_wheel_kernel.h kLPrimeMask), and the bucket threshold 2^19 must not
// exceed it. (r05 window A/B: 2^22 7.25 ms, 2^21 6.11, 2^20 5.62, 2^19 5.49)
#define DSE_WHEEL_MAX_LOG 20
#endif
constexpr uint64_t kWheelMaxPrime = 1ull << DSE_WHEEL_MAX_LOG;

// Largest limit the single-workgroup base-prime kernel handles (LDS bitmap).
constexpr uint64_t kBaseLimitMax = 2ull * 150u * 1024u * 8u + 1ull;  // 150 KiB of odd bits

// Big tables: odd primes < 2^31 (so p + SEG fits 32 bits in the kernel).
constexpr uint64_t kBigBaseLimitMax = (1ull << 31) - 1;

// floor(sqrt(x)) for any x < 2^63 (the double root is off by a few at most;
// (r + 1)^2 stays below 2^64).
inline uint64_t isqrt64(uint64_t x) {
  uint64_t r = (uint64_t)__builtin_sqrt((double)x);
  while (r * r > x) --r;
  while ((r + 1) * (r + 1) <= x) ++r;
  return r;
}

// Grow-only buffer of device memory (pinned: of page-locked host memory).
// grow_buf is a no-op while the buffer holds `bytes`; otherwise it frees the
// old allocation (the contents are lost) and allocates exactly `bytes`. The
// caller guarantees that nothing in flight still uses the old one.
// (dse_host.cpp)
struct Buf {
  void* ptr = nullptr;
  uint64_t bytes = 0;
  bool pinned = false;
  template <typename T>
  T* as() const {
    return static_cast<T*>(ptr);
  }
};
hipError_t grow_buf(Buf* b, uint64_t bytes);
hipError_t free_buf(Buf* b);

// A device scratch buffer shared by calls on any streams (the null stream
// included), ordered by an event. release_scratch records `done` on the
// stream of a user after its last kernel that touches the buffer;
// acquire_scratch makes the next user's stream wait on it (hipStreamWaitEvent,
// no host block), and a grow or free_scratch synchronises on it on the host
// before the buffer is freed. Every exit after an acquire must release.
// (dse_host.cpp)
struct StreamScratch {
  Buf buf;
  hipEvent_t done = nullptr;  // created on first use
  bool used = false;          // `done` has been recorded since the last grow
};
hipError_t acquire_scratch(StreamScratch* s, uint64_t bytes, hipStream_t stream);
// acquire_scratch for at least `need` bytes: a buffer that has to grow takes half as much again, 64 KiB at least
hipError_t acquire_scratch_roomy(StreamScratch* s, uint64_t need, hipStream_t stream);
hipError_t release_scratch(StreamScratch* s, hipStream_t stream);
hipError_t free_scratch(StreamScratch* s);

// Device scratch of one context's bucketed passes (high-offset ranges).
struct Scratch : StreamScratch {
  uint32_t* flag = nullptr;  // device {sticky overflow, this pass's overflow} (bucket capacity); freed by dse_destroy
};

// Test-only knobs, set through dse_debug_set_option (include/dse.h); the
// defaults are the production configuration. No environment variable is read.
struct SieveOpts {
  uint32_t bucket_pass_segs = 0;  // > 0: cap the segments per bucket pass (multi-pass coverage)
  uint32_t bucket_split_log2 = 0; // > 0: bucketed primes <= 2^k filled one level, above two levels (0: production)
  uint32_t bucket_cap_div = 0;    // > 1: divide the (rigorous) bucket entry capacities, to test the overflow flag
  uint32_t bucket_k0_div = 0;     // > 1: divide the band-0 region capacity, to test the spill list
  uint32_t wheel_geometry = 0;    // ranges without buckets: 0 auto (half-size tail), 1 full only, 2 half only
  uint32_t scratch_poison = 0;    // 1: fill the bucket scratch with 0xFF bytes before every pass (stale contents)
  uint32_t bucket_lo_log2 = 0;    // k in 17..kWheelMaxLog: bucketed ranges bucket the primes above 2^k (0: production)
  uint64_t table_bcast_max = 0;   // > 0: broadcast cap of share_table in bytes (0: DSE_TABLE_BROADCAST_MAX_BYTES)
};

// Test-only: what launch_sieve_ranges planned, as host-side counters read
// through dse_debug_get_stat ("plan_*", include/dse.h). The launchers add to
// the PlanStats they are given (null: nothing is recorded); a sieving entry
// point clears its context's before its first launch.
struct PlanStats {
  uint64_t wheel_launches = 0;          // launches of the wheel kernel, either geometry, with or without bucket units
  uint64_t full_segments = 0;           // full-size segments launched without bucket units
  uint64_t half_segments = 0;           // half-size segments launched
  uint64_t max_rounds = 0;              // largest ceil(segments / workgroups) of a wheel launch
  uint64_t bucket_passes = 0;           // bucketed passes
  uint64_t bucket_max_pass_segments = 0;  // segments of the largest one
  uint64_t bucket_max_lds_bytes = 0;      // largest dynamic LDS size given to bucket_fill_stage_kernel
  // one wheel launch of `nseg` segments over `grid` workgroups (wheel_grid)
  void add_wheel_launch(uint32_t nseg, uint32_t grid) {
    ++wheel_launches;
    max_rounds = max_rounds > (nseg + grid - 1) / grid ? max_rounds : (nseg + grid - 1) / grid;
  }
};

// Workgroups of a persistent launch of the wheel kernel over nseg >= 1
// segments: one per CU, at most one per segment.
inline uint32_t wheel_grid(uint32_t nseg, int num_cus) { return nseg < (uint32_t)num_cus ? nseg : (uint32_t)num_cus; }

// out[j] = sum_i in[i * n + j], i < nsrc (dse_debug_init_logical's count all-reduce)
hipError_t launch_sum_rows(const unsigned long long* in, uint32_t nsrc, uint32_t n, unsigned long long* out,
                           hipStream_t stream);
// Any limit <= kBigBaseLimitMax: the multi-workgroup kernel up to kBaseLimitMax,
// above it a sieve of [3, limit] by the wheel kernel + ordered compaction.
hipError_t launch_base_primes_big(uint64_t limit, void* table, uint32_t cap, int num_cus, hipStream_t stream);

// One odd-index range [g_start, g_start + nbits) of a launch: out (may be
// null) gets its mask as 32-bit words, *count (device) is incremented by its
// primes.
struct RangeSpec {
  uint64_t g_start;
  uint64_t nbits;
  uint32_t* out;
  unsigned long long* count;
};

// Sieve the ranges rs[0..n) on one stream: the ranges without bucketed primes
// share persistent launches of the wheel kernel (several chunks of one
// device: one launch, no idle partial rounds between them); ranges whose
// sqrt(max value) exceeds kWheelMaxPrime run their bucketed passes one by one
// (they need `scratch`). `opts` and `plan` may be null. Empty ranges are skipped.
hipError_t launch_sieve_ranges(const void* table, const RangeSpec* rs, size_t n, int num_cus, hipStream_t stream,
                               Scratch* scratch, const SieveOpts* opts, PlanStats* plan);
// Sieve odd indices [g_start, g_start+nbits) with the mod-30 wheel kernel: out
// (may be null) gets the mask as 32-bit words (2*ceil(nbits/64) of them, upper
// half of the last uint64 zeroed); *count (device) is incremented. Ranges whose
// sqrt(max value) exceeds kWheelMaxPrime need `scratch` (bucketed pass);
// `opts` and `plan` may be null.
hipError_t launch_sieve_range(const void* table, uint64_t g_start, uint64_t nbits, uint32_t* out,
                              unsigned long long* count, int num_cus, hipStream_t stream, Scratch* scratch,
                              const SieveOpts* opts, PlanStats* plan);
// A range whose primes reach above kWheelMaxPrime, as bucketed passes
// (dse_bucket.hip; launch_sieve_ranges routes such ranges here).
hipError_t launch_bucketed(const void* table, uint64_t g_start, uint64_t nbits, uint32_t* out,
                           unsigned long long* count, int num_cus, hipStream_t stream, Scratch* scratch,
                           const SieveOpts* opts, PlanStats* plan);
// The same sieve with the half-size segment geometry (2^16 periods,
// dse_wheel_half.hip): launch_sieve_ranges gives it the segments past the last
// full round of a launch when that finishes sooner. No bucketed primes.
hipError_t launch_wheel_ranges_half(const void* table, const RangeSpec* rs, size_t n, int num_cus,
                                    hipStream_t stream, PlanStats* plan);
// One persistent launch of the full-geometry wheel kernel over wa (built by
// make_wheel_args, dse_wheel_geometry.h, in a unit of the full geometry), one
// per instantiation, each in a unit with its own compile flags: without bucket
// units (dse_wheel_plain.hip; wa.bk_* unused) and with them (dse_wheel.hip;
// launch_bucketed's passes, wa.bk_* set).
struct WheelArgs;
hipError_t launch_wheel_plain(const void* table, const WheelArgs& wa, int num_cus, hipStream_t stream);
hipError_t launch_wheel_bucketed(const void* table, const WheelArgs& wa, int num_cus, hipStream_t stream);
// Fill the Barrett factors m[] and wheel offsets a[] of a table whose p[] is final.
// n_hint: table capacity when known (sizes the grid: about 4 primes per thread)
hipError_t launch_wheel_offsets(void* table, int num_cus, hipStream_t stream, uint64_t n_hint = 0);

// Test-only (dse_arith_probe.hip): out[i] = op(x[i], y[i]), i < n, by the wheel
// kernel's own integer helpers (dse_wheel_kernel.h); op = kArith*, the
// DSE_ARITH_* of include/dse.h. And the thresholds of the wheel kernel's units as the library was built.
enum : uint32_t {
  kArithKbModF32 = 0,
  kArithKbModF38,
  kArithKbModBarrett,
  kArithModBarrett,
  kArithBarrettFactor,
  kArithDivSmall,
  kArithDivCeilSmall,
  kArithMulmodSmall,
  kArithPlaneFirst,
  kArithFirstAtOrAfter,
  kArithOps
};
hipError_t launch_arith_probe(uint32_t op, const uint64_t* x, const uint64_t* y, uint64_t n, uint64_t* out,
                              int num_cus, hipStream_t stream);
struct WheelConsts {
  uint32_t ta, tb1, tb, log_kp;  // A/B1, B1/B2 and B2/L thresholds; log2 of a full segment's periods
  uint64_t max_prime;            // kWheelMaxPrime
};
WheelConsts wheel_consts();

// Device finish (dse_finish.hip): the set bits of mask (odd indices [g_start,
// g_start + nbits), 64-bit words) as the slice of a primes{k}.txt file whose
// first entry has rank first_rank; flags = DSE_FINISH_*. totals[0] = entries,
// totals[1] = text bytes; text is written only when they fit text_cap.
// tile_sums: finish_scratch_bytes(nbits) bytes of device scratch.
uint64_t finish_scratch_bytes(uint64_t nbits);
hipError_t launch_finish_text(uint32_t flags, uint64_t g_start, uint64_t nbits, const uint64_t* mask,
                              uint64_t first_rank, void* text, uint64_t text_cap, unsigned long long* totals,
                              void* tile_sums, hipStream_t stream);

// Primes as numbers (dse_primes.hip): the set bits of mask (odd indices
// [g_start, g_start + nbits), 64-bit words) as uint64 values 3 + 2 (g_start +
// bit), ranked in increasing order. A tile is kMaskTileBits candidates.
// launch_primes_scan: the size and scan launches. tile_sums
// (primes_scratch_bytes(nbits) bytes of device scratch) gets the tiles' first
// ranks, one uint64 per tile and the total behind them; totals[0] = entries,
// totals[1] = min(out_cap, max(0, entries - first)).
// launch_primes_emit: the emit launch over tiles [tile0, tile0 + tiles) of a
// scanned tile_sums: the entry of rank r is stored to out[r - first] exactly
// when first <= r < first + out_cap and one of those tiles holds it.
uint64_t primes_scratch_bytes(uint64_t nbits);
hipError_t launch_primes_scan(uint64_t g_start, uint64_t nbits, const uint64_t* mask, uint64_t first,
                              uint64_t out_cap, unsigned long long* totals, void* tile_sums, hipStream_t stream);
hipError_t launch_primes_emit(uint64_t g_start, uint64_t nbits, const uint64_t* mask, uint64_t first, uint64_t* out,
                              uint64_t out_cap, const void* tile_sums, uint64_t tile0, uint64_t tiles,
                              hipStream_t stream);
// The scan launch alone, on ntiles tile counts at tile_sums (ntiles + 1 uint64): what
// launch_primes_scan ends with, and the scan of every other compaction by rank window.
hipError_t launch_rank_scan(void* tile_sums, uint64_t ntiles, uint64_t first, uint64_t out_cap,
                            unsigned long long* totals, hipStream_t stream);

// Constellations as numbers (dse_tuples.hip): the positions of mask (odd indices [g_start,
// g_start + nbits)) at which the pattern (require, forbid) matches (dse_tuples_word.h), as uint64
// values 3 + 2 (g_start + position), ranked in increasing order. The above_bits <= 31 candidates
// behind the range are the bits of `above` from bit above_shift on. The launches, the scratch
// (primes_scratch_bytes(nbits)) and the totals are launch_primes_scan's and launch_primes_emit's.
struct TuplePattern {
  uint32_t require, forbid;
  const uint64_t* above;
  uint32_t above_shift, above_bits;
};
hipError_t launch_tuples_scan(uint64_t g_start, uint64_t nbits, const uint64_t* mask, const TuplePattern& p,
                              uint64_t first, uint64_t out_cap, unsigned long long* totals, void* tile_sums,
                              hipStream_t stream);
hipError_t launch_tuples_emit(uint64_t g_start, uint64_t nbits, const uint64_t* mask, const TuplePattern& p,
                              uint64_t first, uint64_t* out, uint64_t out_cap, const void* tile_sums, uint64_t tile0,
                              uint64_t tiles, hipStream_t stream);

// Statistics of a mask (dse_stats.hip): the two launches of a slab reduction (dse_slab.h), which
// write the dse_stats (kStatsWords uint64 words) at `stats`. grid = stats_grid(nbits, CUs of the
// device, cap or 0): slab_grid's rule. slabs: stats_scratch_bytes(grid) bytes of device scratch.
// patterns: npatterns <= 8 host values, passed by value.
constexpr uint32_t kStatsMaxGrid = 1024;
constexpr uint32_t kStatsWords = 27 + 1024;
uint32_t stats_grid(uint64_t nbits, int num_cus, uint32_t grid_cap);
uint64_t stats_scratch_bytes(uint32_t grid);
hipError_t launch_stats(uint64_t g_start, uint64_t nbits, const uint64_t* mask, const uint32_t* patterns,
                        uint32_t npatterns, uint64_t* stats, void* slabs, uint32_t grid, hipStream_t stream);

// Rank and select on a mask (dse_query.hip). The index of a range is the scanned
// tile sums of launch_primes_scan (first = 0, out_cap = 0): query_index_words(nbits)
// uint64 words, index[t] = entries in the tiles before t, index[tiles] = the total;
// the scan's two totals are written behind them. launch_query: out[i] = the answer
// to q[i] for kind = kQuery* (dse_query_word.h; the DSE_QUERY_* of include/dse.h),
// over `grid` workgroups = query_grid(kind, nq, CUs of the device, cap or 0): at
// most kQueryGridPerCu per CU, so a wave (a lane for kQueryTest) takes several
// queries of a large batch. kQueryTest reads no index.
constexpr uint32_t kQueryGridPerCu = 8;
constexpr uint32_t kQueryMaxGrid = 1024;  // of the test-only cap
uint64_t query_index_words(uint64_t nbits);
uint32_t query_grid(uint32_t kind, uint64_t nq, int num_cus, uint32_t grid_cap);
hipError_t launch_query(uint32_t kind, uint64_t g_start, uint64_t nbits, const uint64_t* mask, const void* index,
                        const uint64_t* q, uint64_t nq, uint64_t* out, uint32_t grid, hipStream_t stream);

// Minimal Goldbach partitions of a mask (dse_goldbach.hip): the two launches of a slab reduction
// (dse_slab.h), which write the dse_goldbach (kGbWords uint64 words) at `out`. The range's candidates
// are the bits of `mask` from bit mask_shift on (0 for a caller's mask; dse_goldbach_range's lies
// behind its `below` in one scratch mask), the below_bits candidates below it the bits of `below`
// from bit below_shift on; nprimes in 1..2048. grid = goldbach_grid(nbits, CUs of the device, cap
// or 0): slab_grid's rule. slabs: goldbach_scratch_bytes(grid) bytes of device scratch.
constexpr uint32_t kGbMaxGrid = 1024;
constexpr uint32_t kGbWords = 8 + 2048;
uint32_t goldbach_grid(uint64_t nbits, int num_cus, uint32_t grid_cap);
uint64_t goldbach_scratch_bytes(uint32_t grid);
hipError_t launch_goldbach(uint64_t g_start, uint64_t nbits, const uint64_t* mask, uint32_t mask_shift,
                           const uint64_t* below, uint32_t below_shift, uint64_t below_bits, uint32_t nprimes,
                           uint64_t* out, void* slabs, uint32_t grid, hipStream_t stream);

// Residue-class counts and a prime race of a mask (dse_race.hip): the launches of a slab reduction
// (dse_slab.h) with a count pass in front, which write the dse_race (kRaceWords uint64 words,
// dse_race_word.h) at `out`: the counts of the classes mod q (3..64) and, for a != b (both < q), the
// race of class a against class b from d_start; a == b (with d_start 0) runs the count and closing
// launches only. grid = race_grid(nbits, CUs of the device, cap or 0): slab_grid's rule. slabs:
// race_scratch_bytes(grid) bytes of device scratch.
constexpr uint32_t kRaceMaxGrid = 1024;
uint32_t race_grid(uint64_t nbits, int num_cus, uint32_t grid_cap);
uint64_t race_scratch_bytes(uint32_t grid);
hipError_t launch_race(uint64_t g_start, uint64_t nbits, const uint64_t* mask, uint32_t q, uint32_t a, uint32_t b,
                       int64_t d_start, uint64_t* out, void* slabs, uint32_t grid, hipStream_t stream);

// Where the prime gaps of a mask are (dse_gaps.hip): the two launches of a slab reduction
// (dse_slab.h), which write the dse_gaps (kGapsWords uint64 words) at `out`. grid = gaps_grid(nbits,
// CUs of the device, cap or 0): slab_grid's rule. slabs: gaps_scratch_bytes(grid) bytes of device
// scratch.
constexpr uint32_t kGapsMaxGrid = 1024;
constexpr uint32_t kGapsWords = 9 + 1024;
uint32_t gaps_grid(uint64_t nbits, int num_cus, uint32_t grid_cap);
uint64_t gaps_scratch_bytes(uint32_t grid);
hipError_t launch_gaps(uint64_t g_start, uint64_t nbits, const uint64_t* mask, uint64_t* out, void* slabs,
                       uint32_t grid, hipStream_t stream);

// The residue pairs of consecutive primes of a mask (dse_consec.hip): the two launches of a slab
// reduction (dse_slab.h), which write the dse_consec (kConsecWords uint64 words, dse_consec_word.h) at
// `out` for the modulus q (3..64). grid = consec_grid(nbits, CUs of the device, cap or 0): slab_grid's
// rule. slabs: consec_scratch_bytes(grid) bytes of device scratch. flush_tiles: the tiles after which
// a workgroup empties its 32-bit counters (0: kConsecFlushTiles, the most); body: 0 the in-word body
// of the measured threshold, 1 the bit-parallel one wherever it is built, 2 the per-entry one.
constexpr uint32_t kConsecMaxGrid = 1024;
// A 32-bit bin grows by at most 64 pairs per word and tile (every entry is the upper prime of at most
// one pair, counted by its word): emptied into 64 bits after at most this many tiles.
constexpr uint32_t kConsecFlushTiles = 0xFFFFFFFFu / (64u * kMaskTileWords);
uint32_t consec_grid(uint64_t nbits, int num_cus, uint32_t grid_cap);
uint64_t consec_scratch_bytes(uint32_t grid);
hipError_t launch_consec(uint64_t g_start, uint64_t nbits, const uint64_t* mask, uint32_t q, uint64_t* out,
                         void* slabs, uint32_t grid, uint32_t flush_tiles, uint32_t body, hipStream_t stream);

// Power and reciprocal sums over the matches of a pattern (dse_sums.hip): the two launches of a slab
// reduction (dse_slab.h), which write the dse_sums (kSumsWords uint64 words) at `out`. The pattern and
// the candidates above the range are launch_tuples_scan's; flags = DSE_SUMS_*. grid = sums_grid(nbits,
// CUs of the device, cap or 0): slab_grid's rule. slabs: sums_scratch_bytes(grid) bytes of device
// scratch.
constexpr uint32_t kSumsMaxGrid = 1024;
constexpr uint32_t kSumsWords = 17;
uint32_t sums_grid(uint64_t nbits, int num_cus, uint32_t grid_cap);
uint64_t sums_scratch_bytes(uint32_t grid);
hipError_t launch_sums(uint64_t g_start, uint64_t nbits, const uint64_t* mask, const TuplePattern& p, uint32_t flags,
                       uint64_t* out, void* slabs, uint32_t grid, hipStream_t stream);

}  // namespace dse
